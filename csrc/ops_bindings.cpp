// Bindings of the generic HIP ops (csrc/kernels/ops.hip).
#include <torch/extension.h>

#include <cstdlib>
#include <cstdio>
#include <limits>
#include <c10/hip/HIPStream.h>

#include "kernels/bn.h"
#include "kernels/conv.h"
#include "kernels/augment.h"
#include "kernels/dropout.h"
#include "kernels/gemm.h"
#include "kernels/gemm_f32.h"
#include "kernels/groupnorm.h"
#include "kernels/loss_head.h"
#include "kernels/ops.h"
#include "kernels/pool.h"
#include "kernels/stem.h"

namespace {
hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

// TDL_DEBUG_POISON=1: outputs and partial-sum buffers of the conv kernels start as NaN instead of
// uninitialised (a row or pixel a kernel fails to write then shows up in the results)
int poison() {  // 1: partial-sum buffers, 2: and the gradient outputs
  static const int on = [] {
    const char* e = std::getenv("TDL_DEBUG_POISON");
    return e != nullptr ? std::atoi(e) : 0;
  }();
  return on;
}
at::Tensor fresh(at::IntArrayRef shape, const at::TensorOptions& o, int level = 1) {
  const bool fp = o.dtype() == at::kFloat || o.dtype() == at::kBFloat16 || o.dtype() == at::kHalf;
  return (fp && poison() >= level) ? at::full(shape, std::numeric_limits<float>::quiet_NaN(), o) : at::empty(shape, o);
}

// (x [n, ...] f32, y [n]) = (X[idx], Y[idx]) in one launch; Y int64 or int32
std::vector<at::Tensor> gather_xy(at::Tensor X, at::Tensor Y, at::Tensor idx) {
  TORCH_CHECK(X.is_cuda() && Y.is_cuda() && idx.is_cuda(), "gather_xy: GPU tensors expected");
  TORCH_CHECK(X.is_contiguous() && Y.is_contiguous() && idx.is_contiguous(), "gather_xy: contiguous tensors expected");
  TORCH_CHECK(X.scalar_type() == at::kFloat && X.dim() >= 1, "gather_xy: X must be f32 [N, ...]");
  TORCH_CHECK((Y.scalar_type() == at::kLong || Y.scalar_type() == at::kInt) && Y.dim() == 1 && Y.size(0) == X.size(0),
              "gather_xy: Y must be int64 / int32 [N]");
  TORCH_CHECK(idx.scalar_type() == at::kInt && idx.dim() == 1, "gather_xy: idx must be int32 [n]");
  const int64_t rows = idx.numel();
  auto shape = X.sizes().vec();
  shape[0] = rows;
  auto x = at::empty(shape, X.options());
  auto y = at::empty({rows}, Y.options());
  const int64_t row_elems = X.size(0) > 0 ? X.numel() / X.size(0) : 0;
  TORCH_CHECK(reinterpret_cast<uintptr_t>(X.data_ptr()) % 16 == 0, "gather_xy: X must be 16-byte aligned");
  tdl::gather_xy(X.data_ptr<float>(), Y.data_ptr(), idx.data_ptr<int>(), x.data_ptr<float>(), y.data_ptr(), rows,
                 row_elems, (int)Y.element_size(), cur_stream());
  return {x, y};
}

// gather_xy with a third, f32 column W [N] (sample weights): (x, y, w) = (X[idx], Y[idx], W[idx]) in one launch.
// out_x / out_y / out_w: optional preallocated outputs (tests put guard words around them)
std::vector<at::Tensor> gather_xyw(at::Tensor X, at::Tensor Y, at::Tensor W, at::Tensor idx,
                                   c10::optional<at::Tensor> out_x, c10::optional<at::Tensor> out_y,
                                   c10::optional<at::Tensor> out_w) {
  TORCH_CHECK(X.is_cuda() && Y.is_cuda() && W.is_cuda() && idx.is_cuda(), "gather_xyw: GPU tensors expected");
  TORCH_CHECK(X.is_contiguous() && Y.is_contiguous() && W.is_contiguous() && idx.is_contiguous(),
              "gather_xyw: contiguous tensors expected");
  TORCH_CHECK(X.scalar_type() == at::kFloat && X.dim() >= 1, "gather_xyw: X must be f32 [N, ...]");
  TORCH_CHECK((Y.scalar_type() == at::kLong || Y.scalar_type() == at::kInt) && Y.dim() == 1 && Y.size(0) == X.size(0),
              "gather_xyw: Y must be int64 / int32 [N]");
  TORCH_CHECK(W.scalar_type() == at::kFloat && W.dim() == 1 && W.size(0) == X.size(0), "gather_xyw: W must be f32 [N]");
  TORCH_CHECK(idx.scalar_type() == at::kInt && idx.dim() == 1, "gather_xyw: idx must be int32 [n]");
  const int64_t rows = idx.numel();
  auto shape = X.sizes().vec();
  shape[0] = rows;
  const int64_t row_elems = X.size(0) > 0 ? X.numel() / X.size(0) : 0;
  auto given = [](const c10::optional<at::Tensor>& t) { return t.has_value() && t->defined(); };
  auto x = given(out_x) ? *out_x : at::empty(shape, X.options());
  auto y = given(out_y) ? *out_y : at::empty({rows}, Y.options());
  auto w = given(out_w) ? *out_w : at::empty({rows}, W.options());
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.scalar_type() == at::kFloat && x.numel() == rows * row_elems,
              "gather_xyw: out_x must be f32 with ", rows * row_elems, " elements");
  TORCH_CHECK(y.is_cuda() && y.is_contiguous() && y.scalar_type() == Y.scalar_type() && y.numel() == rows,
              "gather_xyw: out_y must have Y's dtype and ", rows, " elements");
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() && w.scalar_type() == at::kFloat && w.numel() == rows,
              "gather_xyw: out_w must be f32 with ", rows, " elements");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(X.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "gather_xyw: X and out_x must be 16-byte aligned");
  tdl::gather_xyw(X.data_ptr<float>(), Y.data_ptr(), W.data_ptr<float>(), idx.data_ptr<int>(), x.data_ptr<float>(),
                  y.data_ptr(), w.data_ptr<float>(), rows, row_elems, (int)Y.element_size(), cur_stream());
  return {x, y, w};
}

tdl::BnDType bn_dtype(const at::Tensor& x) {
  if (x.scalar_type() == at::kFloat) return tdl::BnDType::kF32;
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "batch_norm: float32 or bfloat16 activations expected");
  return tdl::BnDType::kBF16;
}

void bn_check(const at::Tensor& x) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() >= 2, "batch_norm: contiguous [..., C] GPU tensor expected");
  const int64_t C = x.size(-1);
  TORCH_CHECK(C >= 8 && C % 8 == 0 && C <= 2048, "batch_norm: C must be a multiple of 8, at least 8 and <= 2048");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, "batch_norm: 16-byte aligned data expected");
}

// the BN kernels divide by the row count: an empty batch is refused here (ops/batchnorm.py sends it to PyTorch)
void bn_check_rows(const at::Tensor& x) {
  bn_check(x);
  TORCH_CHECK(x.numel() > 0, "batch_norm: empty batch (no rows)");
}

const float* opt_f32(const c10::optional<at::Tensor>& t) {
  if (!t.has_value() || !t->defined()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous(), "batch_norm: f32 GPU params");
  return t->data_ptr<float>();
}

// partial rows P of a [P + ceil(P/64)][2][C] f32 workspace produced by a conv epilogue
int parts_rows(const at::Tensor& t, int64_t C) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kFloat && t.dim() == 3 && t.size(1) == 2 &&
                  t.size(2) == C,
              "batch_norm: part must be f32 [rows][2][C]");
  const int64_t rows = t.size(0);
  int64_t p = 1;
  while (p + (p + 63) / 64 < rows) ++p;  // invert rows = P + ceil(P / 64)
  TORCH_CHECK(p + (p + 63) / 64 == rows, "batch_norm: part rows must be P + ceil(P/64)");
  return (int)p;
}

// training forward: y = act(bn(x) [+ residual]); returns (y, stats[4][C] = mean, invstd, scale, shift);
// moving statistics updated in place (mean_off: folded conv bias, moving mean only)
static std::vector<at::Tensor> bn_forward_impl(at::Tensor x, c10::optional<at::Tensor> gamma,
                                               c10::optional<at::Tensor> beta, c10::optional<at::Tensor> moving_mean,
                                               c10::optional<at::Tensor> moving_var, double momentum, double eps,
                                               bool relu, c10::optional<at::Tensor> residual,
                                               c10::optional<at::Tensor> mean_off, c10::optional<at::Tensor> part_in,
                                               bool apply) {
  bn_check_rows(x);
  const int64_t C = x.size(-1), M = x.numel() / C;
  const void* res = nullptr;
  if (residual.has_value() && residual->defined()) {
    bn_check(*residual);
    TORCH_CHECK(residual->scalar_type() == x.scalar_type() && residual->numel() == x.numel(),
                "batch_norm: residual must match x");
    res = residual->data_ptr();
  }
  const tdl::BnPlan plan = tdl::bn_plan(M, (int)C);
  auto f = x.options().dtype(at::kFloat);
  int given = 0;
  at::Tensor part;
  if (part_in.has_value() && part_in->defined()) {
    // [rows + ceil(rows/64)][2][C] from conv_fwd_stats: the first `rows` rows are the partial sums
    TORCH_CHECK(part_in->is_cuda() && part_in->is_contiguous() && part_in->scalar_type() == at::kFloat &&
                    part_in->dim() == 3 && part_in->size(1) == 2 && part_in->size(2) == C,
                "batch_norm: part must be f32 [rows][2][C]");
    given = parts_rows(*part_in, C);
    part = *part_in;
  } else {
    part = fresh({(int64_t)plan.part_rows * 2 * C}, f);
  }
  auto st = fresh({4, C}, f);  // mean, invstd, scale, shift
  float* mm = const_cast<float*>(opt_f32(moving_mean));
  float* mv = const_cast<float*>(opt_f32(moving_var));
  TORCH_CHECK((mm == nullptr) == (mv == nullptr), "batch_norm: moving mean and variance go together");
  hipStream_t s = cur_stream();
  float* sp = st.data_ptr<float>();
  tdl::bn_forward_stats(x.data_ptr(), bn_dtype(x), M, (int)C, part.data_ptr<float>(), opt_f32(gamma), opt_f32(beta),
                        opt_f32(mean_off), sp, sp + C, sp + 2 * C, sp + 3 * C, mm, mv, (float)momentum, (float)eps, s,
                        given);
  if (!apply) return {st};
  auto y = fresh(x.sizes(), x.options());
  tdl::bn_apply(x.data_ptr(), res, y.data_ptr(), bn_dtype(x), M, (int)C, sp + 2 * C, sp + 3 * C, relu ? 1 : 0, s);
  return {y, st};
}

// backward (mode 0 plain, 1 relu, 2 add+relu using y); returns (dx, dgamma, dbeta[, dz])
// dgamma_out / dbeta_out: f32 [C] tensors the parameter gradients are ADDED into (a trainer's slab
// views); the returned dgamma / dbeta are then those tensors
std::vector<at::Tensor> bn_backward(at::Tensor dy, at::Tensor x, c10::optional<at::Tensor> y,
                                    c10::optional<at::Tensor> gamma, at::Tensor st, int64_t mode,
                                    c10::optional<at::Tensor> dgamma_out, c10::optional<at::Tensor> dbeta_out,
                                    c10::optional<at::Tensor> part_in) {
  bn_check_rows(x);
  bn_check(dy);
  TORCH_CHECK(dy.scalar_type() == x.scalar_type() && dy.numel() == x.numel(), "batch_norm backward: dy/x mismatch");
  TORCH_CHECK(mode >= 0 && mode <= 2, "batch_norm backward: bad mode");
  const int64_t C = x.size(-1), M = x.numel() / C;
  TORCH_CHECK(st.is_cuda() && st.is_contiguous() && st.numel() == 4 * C && st.scalar_type() == at::kFloat,
              "batch_norm: stats [4][C]");
  const void* yp = nullptr;
  at::Tensor dz;
  if (mode == 2 && !(part_in.has_value() && part_in->defined())) {
    TORCH_CHECK(y.has_value() && y->defined(), "batch_norm backward mode 2 needs y");
    bn_check(*y);
    TORCH_CHECK(y->scalar_type() == x.scalar_type() && y->numel() == x.numel(), "batch_norm backward: y/x mismatch");
    yp = y->data_ptr();
    dz = fresh(x.sizes(), x.options());
  } else if (mode == 2) {
    dz = dy;
  }
  const tdl::BnPlan plan = tdl::bn_plan(M, (int)C);
  auto f = x.options().dtype(at::kFloat);
  int given = 0;
  at::Tensor part;
  if (part_in.has_value() && part_in->defined()) {
    // (dz, part) from conv_dgrad_bn: dy IS the group's masked gradient dz (for an add+relu group
    // also returned as the residual's); mode 0: a plain BN whose output gradient is such a group's
    // dz (part2 of conv_dgrad_bn: sums of dz and dz * x)
    given = parts_rows(*part_in, C);
    part = *part_in;
  } else {
    part = fresh({(int64_t)plan.part_rows * 2 * C}, f);
  }
  auto out = fresh({5, C}, f);  // dgamma, dbeta, coef[3]
  auto dx = fresh(x.sizes(), x.options());
  float* o = out.data_ptr<float>();
  const float* sp = st.data_ptr<float>();
  auto check_out = [&](const c10::optional<at::Tensor>& t) {
    if (!t.has_value() || !t->defined()) return (float*)nullptr;
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->scalar_type() == at::kFloat && t->numel() == C,
                "batch_norm backward: gradient outputs must be contiguous f32 [C]");
    return t->data_ptr<float>();
  };
  float* pg = check_out(dgamma_out);
  float* pb = check_out(dbeta_out);
  const int acc = (pg ? 1 : 0) | (pb ? 2 : 0);
  tdl::bn_backward(dy.data_ptr(), x.data_ptr(), yp, mode == 2 ? dz.data_ptr() : nullptr, dx.data_ptr(), bn_dtype(x), M,
                   (int)C, part.data_ptr<float>(), opt_f32(gamma), sp, sp + C, sp + 2 * C, sp + 3 * C, pg ? pg : o,
                   pb ? pb : o + C, o + 2 * C, (int)mode, acc, cur_stream(), given);
  at::Tensor g = pg ? *dgamma_out : out[0], b = pb ? *dbeta_out : out[1];
  if (mode == 2) return {dx, g, b, dz};
  return {dx, g, b};
}
std::vector<at::Tensor> bn_forward_train(at::Tensor x, c10::optional<at::Tensor> gamma, c10::optional<at::Tensor> beta,
                                         c10::optional<at::Tensor> moving_mean, c10::optional<at::Tensor> moving_var,
                                         double momentum, double eps, bool relu, c10::optional<at::Tensor> residual,
                                         c10::optional<at::Tensor> mean_off, c10::optional<at::Tensor> part_in) {
  return bn_forward_impl(x, gamma, beta, moving_mean, moving_var, momentum, eps, relu, residual, mean_off, part_in,
                         true);
}

// the batch statistics only ([4][C]: mean, invstd, scale, shift; moving statistics updated): the
// normalisation is applied by the consumer (maxpool_fwd(bn_stats=...))
at::Tensor bn_stats_train(at::Tensor x, c10::optional<at::Tensor> gamma, c10::optional<at::Tensor> beta,
                          c10::optional<at::Tensor> moving_mean, c10::optional<at::Tensor> moving_var, double momentum,
                          double eps, c10::optional<at::Tensor> mean_off, c10::optional<at::Tensor> part_in) {
  return bn_forward_impl(x, gamma, beta, moving_mean, moving_var, momentum, eps, false, c10::nullopt, mean_off,
                         part_in, false)[0];
}

// ---- synchronized batch norm (kernels/bn.h): pack -> [the caller's SUM all-reduce of xbuf] -> finalize
static at::Tensor bn_sync_xbuf(const at::Tensor& x, int64_t C, int64_t rank, int64_t R, int64_t numel) {
  TORCH_CHECK(R >= 1 && rank >= 0 && rank < R, "sync batch_norm: rank must be in [0, R)");
  const int64_t need = tdl::bn_sync_xbuf_numel((int)C, (int)R);
  TORCH_CHECK(numel == 0 || numel >= need, "sync batch_norm: exchange buffer of ", numel, " elements, ", need, " needed");
  auto xbuf = fresh({numel > 0 ? numel : need}, x.options().dtype(at::kFloat));
  TORCH_CHECK(reinterpret_cast<uintptr_t>(xbuf.data_ptr()) % 16 == 0, "sync batch_norm: 16-byte aligned exchange buffer");
  return xbuf;
}

static void bn_sync_check_xbuf(const at::Tensor& xbuf, int64_t C, int64_t R) {
  TORCH_CHECK(xbuf.is_cuda() && xbuf.is_contiguous() && xbuf.scalar_type() == at::kFloat && R >= 1 &&
                  xbuf.numel() >= tdl::bn_sync_xbuf_numel((int)C, (int)R),
              "sync batch_norm: xbuf must be the f32 exchange buffer of bn_sync_*_pack");
}

static at::Tensor bn_sync_part(const c10::optional<at::Tensor>& part_in, const at::Tensor& x, int64_t M, int64_t C,
                               int& given) {
  given = 0;
  if (part_in.has_value() && part_in->defined()) {
    given = parts_rows(*part_in, C);
    return *part_in;
  }
  const tdl::BnPlan plan = tdl::bn_plan(M, (int)C);
  return fresh({(int64_t)plan.part_rows * 2 * C}, x.options().dtype(at::kFloat));
}

// this replica's sums of x and x*x (its own pass, or part_in from a conv epilogue) into rank `rank`'s
// slot of a fresh exchange buffer (numel > 0: that many elements, for a size no other collective uses)
at::Tensor bn_sync_forward_pack(at::Tensor x, int64_t rank, int64_t R, c10::optional<at::Tensor> part_in,
                                int64_t numel) {
  bn_check_rows(x);
  const int64_t C = x.size(-1), M = x.numel() / C;
  TORCH_CHECK(M > 0 && M < (int64_t(1) << 48), "sync batch_norm: row count out of range");
  int given = 0;
  at::Tensor part = bn_sync_part(part_in, x, M, C, given);
  at::Tensor xbuf = bn_sync_xbuf(x, C, rank, R, numel);
  tdl::bn_sync_forward_pack(x.data_ptr(), bn_dtype(x), M, (int)C, part.data_ptr<float>(), xbuf.data_ptr<float>(),
                            xbuf.numel(), (int)rank, cur_stream(), given);
  return xbuf;
}

// xbuf all-reduced: (y, stats[4][C]) or, apply = false, (stats) -- as bn_forward_train / bn_stats_train
std::vector<at::Tensor> bn_sync_forward_finalize(at::Tensor x, at::Tensor xbuf, int64_t R,
                                                 c10::optional<at::Tensor> gamma, c10::optional<at::Tensor> beta,
                                                 c10::optional<at::Tensor> moving_mean,
                                                 c10::optional<at::Tensor> moving_var, double momentum, double eps,
                                                 bool relu, c10::optional<at::Tensor> residual,
                                                 c10::optional<at::Tensor> mean_off, bool apply) {
  bn_check_rows(x);
  const int64_t C = x.size(-1), M = x.numel() / C;
  bn_sync_check_xbuf(xbuf, C, R);
  const void* res = nullptr;
  if (residual.has_value() && residual->defined()) {
    bn_check(*residual);
    TORCH_CHECK(residual->scalar_type() == x.scalar_type() && residual->numel() == x.numel(),
                "batch_norm: residual must match x");
    res = residual->data_ptr();
  }
  auto st = fresh({4, C}, x.options().dtype(at::kFloat));
  float* mm = const_cast<float*>(opt_f32(moving_mean));
  float* mv = const_cast<float*>(opt_f32(moving_var));
  TORCH_CHECK((mm == nullptr) == (mv == nullptr), "batch_norm: moving mean and variance go together");
  hipStream_t s = cur_stream();
  float* sp = st.data_ptr<float>();
  tdl::bn_sync_forward_finalize(xbuf.data_ptr<float>(), (int)R, (int)C, opt_f32(gamma), opt_f32(beta),
                                opt_f32(mean_off), sp, sp + C, sp + 2 * C, sp + 3 * C, mm, mv, (float)momentum,
                                (float)eps, s);
  if (!apply) return {st};
  auto y = fresh(x.sizes(), x.options());
  tdl::bn_apply(x.data_ptr(), res, y.data_ptr(), bn_dtype(x), M, (int)C, sp + 2 * C, sp + 3 * C, relu ? 1 : 0, s);
  return {y, st};
}

// returns (xbuf, dgamma, dbeta, dz): dgamma / dbeta from this replica's LOCAL sums (or added into
// dgamma_out / dbeta_out); dz: what bn_sync_backward_finalize takes (mode 2: the masked gradient, also
// the residual's; else dy)
std::vector<at::Tensor> bn_sync_backward_pack(at::Tensor dy, at::Tensor x, c10::optional<at::Tensor> y, at::Tensor st,
                                              int64_t mode, int64_t rank, int64_t R,
                                              c10::optional<at::Tensor> dgamma_out,
                                              c10::optional<at::Tensor> dbeta_out, c10::optional<at::Tensor> part_in,
                                              int64_t numel) {
  bn_check_rows(x);
  bn_check(dy);
  TORCH_CHECK(dy.scalar_type() == x.scalar_type() && dy.numel() == x.numel(), "batch_norm backward: dy/x mismatch");
  TORCH_CHECK(mode >= 0 && mode <= 2, "batch_norm backward: bad mode");
  const int64_t C = x.size(-1), M = x.numel() / C;
  TORCH_CHECK(M > 0 && M < (int64_t(1) << 48), "sync batch_norm: row count out of range");
  TORCH_CHECK(st.is_cuda() && st.is_contiguous() && st.numel() == 4 * C && st.scalar_type() == at::kFloat,
              "batch_norm: stats [4][C]");
  int given = 0;
  at::Tensor part = bn_sync_part(part_in, x, M, C, given);
  const void* yp = nullptr;
  at::Tensor dz = dy;
  if (mode == 2 && given == 0) {
    TORCH_CHECK(y.has_value() && y->defined(), "batch_norm backward mode 2 needs y");
    bn_check(*y);
    TORCH_CHECK(y->scalar_type() == x.scalar_type() && y->numel() == x.numel(), "batch_norm backward: y/x mismatch");
    yp = y->data_ptr();
    dz = fresh(x.sizes(), x.options());
  }
  auto out = fresh({2, C}, x.options().dtype(at::kFloat));
  auto check_out = [&](const c10::optional<at::Tensor>& t) {
    if (!t.has_value() || !t->defined()) return (float*)nullptr;
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->scalar_type() == at::kFloat && t->numel() == C,
                "batch_norm backward: gradient outputs must be contiguous f32 [C]");
    return t->data_ptr<float>();
  };
  float* pg = check_out(dgamma_out);
  float* pb = check_out(dbeta_out);
  const int acc = (pg ? 1 : 0) | (pb ? 2 : 0);
  at::Tensor xbuf = bn_sync_xbuf(x, C, rank, R, numel);
  float* o = out.data_ptr<float>();
  const float* sp = st.data_ptr<float>();
  tdl::bn_sync_backward_pack(dy.data_ptr(), x.data_ptr(), yp, yp ? dz.data_ptr() : nullptr, bn_dtype(x), M, (int)C,
                             part.data_ptr<float>(), sp, sp + C, sp + 2 * C, sp + 3 * C, pg ? pg : o, pb ? pb : o + C,
                             (int)mode, acc, xbuf.data_ptr<float>(), xbuf.numel(), (int)rank, cur_stream(), given);
  return {xbuf, pg ? *dgamma_out : out[0], pb ? *dbeta_out : out[1], dz};
}

// xbuf all-reduced: dx over this replica's rows (mask: dz is the unmasked dy of a BN -> ReLU group)
at::Tensor bn_sync_backward_finalize(at::Tensor dz, at::Tensor x, at::Tensor xbuf, int64_t R,
                                     c10::optional<at::Tensor> gamma, at::Tensor st, bool mask) {
  bn_check_rows(x);
  bn_check(dz);
  TORCH_CHECK(dz.scalar_type() == x.scalar_type() && dz.numel() == x.numel(), "batch_norm backward: dz/x mismatch");
  const int64_t C = x.size(-1), M = x.numel() / C;
  bn_sync_check_xbuf(xbuf, C, R);
  TORCH_CHECK(st.is_cuda() && st.is_contiguous() && st.numel() == 4 * C && st.scalar_type() == at::kFloat,
              "batch_norm: stats [4][C]");
  auto coef = fresh({3, C}, x.options().dtype(at::kFloat));
  auto dx = fresh(x.sizes(), x.options());
  const float* sp = st.data_ptr<float>();
  tdl::bn_sync_backward_finalize(xbuf.data_ptr<float>(), (int)R, dz.data_ptr(), x.data_ptr(), dx.data_ptr(), bn_dtype(x),
                                 M, (int)C, opt_f32(gamma), sp, sp + C, sp + 2 * C, sp + 3 * C, coef.data_ptr<float>(),
                                 mask, cur_stream());
  return dx;
}

static const float* bn_ss_of(const c10::optional<at::Tensor>& st, int64_t C) {
  if (!st.has_value() || !st->defined()) return nullptr;
  TORCH_CHECK(st->is_cuda() && st->is_contiguous() && st->scalar_type() == at::kFloat && st->numel() == 4 * C,
              "bn_stats must be the f32 [4][C] statistics of the batch norm");
  return st->data_ptr<float>() + 2 * C;  // scale[C], shift[C]
}

// max pool NHWC: returns (y, argmax bytes); pads = (top, left), output size given; bn_stats: x is a
// batch norm's input and the pool runs over relu(bn(x)) (the BN -> ReLU pass skipped)
std::vector<at::Tensor> maxpool_fwd(at::Tensor x, int64_t kh, int64_t kw, int64_t sh, int64_t sw, int64_t pt,
                                    int64_t pl, int64_t OH, int64_t OW, bool pad_zero,
                                    c10::optional<at::Tensor> bn_stats) {
  bn_check(x);
  TORCH_CHECK(x.dim() == 4, "maxpool: NHWC input expected");
  TORCH_CHECK(kh * kw < 255 && kh > 0 && kw > 0 && sh > 0 && sw > 0 && OH > 0 && OW > 0, "maxpool: bad geometry");
  tdl::PoolGeom g{(int)x.size(0), (int)x.size(1), (int)x.size(2), (int)x.size(3), (int)OH, (int)OW,
                  (int)kh, (int)kw, (int)sh, (int)sw, (int)pt, (int)pl, pad_zero ? 1 : 0};
  auto y = fresh({x.size(0), OH, OW, x.size(3)}, x.options());
  auto arg = fresh({x.size(0), OH, OW, x.size(3)}, x.options().dtype(at::kByte));
  if (bn_stats.has_value() && bn_stats->defined()) bn_ss_of(bn_stats, x.size(3));
  if (y.numel() == 0) return {y, arg};  // an empty batch: nothing to launch
  tdl::maxpool_forward(x.data_ptr(), y.data_ptr(), arg.data_ptr<uint8_t>(), bn_dtype(x) == tdl::BnDType::kBF16, g,
                       cur_stream(), bn_ss_of(bn_stats, x.size(3)));
  return {y, arg};
}

at::Tensor maxpool_bwd(at::Tensor dy, at::Tensor arg, std::vector<int64_t> in_shape, int64_t kh, int64_t kw,
                       int64_t sh, int64_t sw, int64_t pt, int64_t pl) {
  bn_check(dy);
  TORCH_CHECK(dy.dim() == 4 && arg.sizes() == dy.sizes() && arg.scalar_type() == at::kByte && arg.is_contiguous(),
              "maxpool backward: dy / argmax mismatch");
  TORCH_CHECK(in_shape.size() == 4 && in_shape[3] == dy.size(3) && in_shape[0] == dy.size(0), "maxpool: bad shape");
  tdl::PoolGeom g{(int)in_shape[0], (int)in_shape[1], (int)in_shape[2], (int)in_shape[3], (int)dy.size(1),
                  (int)dy.size(2), (int)kh, (int)kw, (int)sh, (int)sw, (int)pt, (int)pl, 0};
  auto dx = fresh(in_shape, dy.options());
  if (dx.numel() == 0) return dx;  // an empty batch: nothing to launch
  tdl::maxpool_backward(dy.data_ptr(), arg.data_ptr<uint8_t>(), dx.data_ptr(), bn_dtype(dy) == tdl::BnDType::kBF16, g,
                        cur_stream());
  return dx;
}

// ---- seeded dropout (csrc/kernels/dropout.hip; the stream and the ticket protocol: kernels/dropout.h) ----
// noise_strides: per dimension of x, the stride of that coordinate in the mask's index space (0 where the
// mask is broadcast); absent = the mask has x's shape.  Adjacent dimensions that form one run of the mask
// index are merged, and what remains must fit 4 dimensions.
at::Tensor dropout_run(const at::Tensor& x, int64_t* state, const int64_t* ticket_in, int64_t* ticket_out, int64_t k0,
                       int64_t k1, int64_t T, double scale, const c10::optional<std::vector<int64_t>>& noise_strides,
                       int64_t elem_offset) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "dropout: contiguous GPU tensor expected");
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16, "dropout: float32 or bfloat16 expected");
  TORCH_CHECK(k0 >= 0 && k0 <= 0xffffffffLL && k1 >= 0 && k1 <= 0xffffffffLL, "dropout: key words are 32-bit");
  TORCH_CHECK(T >= 0 && T <= (1LL << 32), "dropout: threshold must be in [0, 2^32]");
  TORCH_CHECK(elem_offset >= 0 && elem_offset % 4 == 0, "dropout: elem_offset must be a non-negative multiple of 4");
  auto y = at::empty_like(x);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(y.data_ptr()) % 16 == 0,
              "dropout: 16-byte aligned data expected");
  tdl::DropoutArgs a;
  a.x = x.data_ptr();
  a.y = y.data_ptr();
  a.n = x.numel();
  a.state = state;
  a.ticket_in = ticket_in;
  a.ticket_out = ticket_out;
  a.k0 = (uint32_t)k0;
  a.k1 = (uint32_t)k1;
  a.thr = (uint64_t)T;
  a.scale = (float)scale;
  a.elem_offset = elem_offset;
  a.bf16 = x.scalar_type() == at::kBFloat16;
  if (!noise_strides.has_value()) {
    tdl::dropout_apply(a, cur_stream());
    return y;
  }
  const auto& ns = *noise_strides;
  TORCH_CHECK((int64_t)ns.size() == x.dim(), "dropout: one noise stride per dimension expected");
  std::vector<int64_t> d, st;
  for (int64_t k = 0; k < x.dim(); ++k) {
    TORCH_CHECK(ns[k] >= 0, "dropout: negative noise stride");
    if (x.size(k) == 1) continue;
    if (!d.empty() && st.back() == ns[k] * x.size(k)) {  // one run of the mask index: merge
      d.back() *= x.size(k);
      st.back() = ns[k];
    } else {
      d.push_back(x.size(k));
      st.push_back(ns[k]);
    }
  }
  if (d.empty() || (d.size() == 1 && st[0] == 1)) {  // the mask index is the element index
    tdl::dropout_apply(a, cur_stream());
    return y;
  }
  TORCH_CHECK(d.size() <= 4, "dropout: noise_shape needs more than 4 dimensions after merging");
  int64_t dims[4] = {1, 1, 1, 1}, nst[4] = {0, 0, 0, 0};
  const size_t pad = 4 - d.size();
  for (size_t k = 0; k < d.size(); ++k) {
    dims[pad + k] = d[k];
    nst[pad + k] = st[k];
  }
  tdl::dropout_apply_bcast(a, dims, nst, cur_stream());
  return y;
}

std::vector<at::Tensor> dropout_fwd(at::Tensor x, at::Tensor state, int64_t k0, int64_t k1, int64_t T, double scale,
                                    c10::optional<std::vector<int64_t>> noise_strides, int64_t elem_offset) {
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == at::kLong && state.numel() == 2 && state.is_contiguous() &&
                  state.device() == x.device(),
              "dropout: state must be an int64 [calls, arrivals] tensor on x's device");
  auto ticket = at::empty({1}, state.options());
  auto y = dropout_run(x, state.data_ptr<int64_t>(), nullptr, ticket.data_ptr<int64_t>(), k0, k1, T, scale,
                       noise_strides, elem_offset);
  return {y, ticket};
}

at::Tensor dropout_bwd(at::Tensor dy, at::Tensor ticket, int64_t k0, int64_t k1, int64_t T, double scale,
                       c10::optional<std::vector<int64_t>> noise_strides, int64_t elem_offset) {
  TORCH_CHECK(ticket.is_cuda() && ticket.scalar_type() == at::kLong && ticket.numel() == 1 &&
                  ticket.device() == dy.device(),
              "dropout: ticket must be the forward's 1-element int64 tensor");
  return dropout_run(dy, nullptr, ticket.data_ptr<int64_t>(), nullptr, k0, k1, T, scale, noise_strides, elem_offset);
}

// ---- seeded image augmentation (csrc/kernels/augment.hip; the draws, the map and the fill modes: kernels/augment.h) ----
// spec = (flip_h, flip_w, off_h_lo, off_h_count, off_w_lo, off_w_count, out_h, out_w, fill_mode, fill_value):
// the offsets are drawn from [lo, lo + count), fill_mode is 0 constant, 1 nearest, 2 wrap, 3 reflect
tdl::AugmentArgs augment_args(const at::Tensor& src, int64_t H, int64_t W, int64_t k0, int64_t k1, bool flip_h,
                              bool flip_w, int64_t off_h_lo, int64_t off_h_count, int64_t off_w_lo,
                              int64_t off_w_count, int64_t out_h, int64_t out_w, int64_t fill_mode,
                              double fill_value) {
  TORCH_CHECK(src.is_cuda() && src.is_contiguous() && src.dim() == 4, "augment: contiguous NHWC GPU tensor expected");
  TORCH_CHECK(src.scalar_type() == at::kFloat || src.scalar_type() == at::kBFloat16,
              "augment: float32 or bfloat16 expected");
  TORCH_CHECK(k0 >= 0 && k0 <= 0xffffffffLL && k1 >= 0 && k1 <= 0xffffffffLL, "augment: key words are 32-bit");
  TORCH_CHECK(fill_mode >= 0 && fill_mode <= 3,
              "augment: fill_mode must be 0 (constant), 1 (nearest), 2 (wrap) or 3 (reflect)");
  const int64_t lim = (1LL << 31) - 1;
  TORCH_CHECK(H >= 1 && W >= 1 && H <= lim && W <= lim && src.size(3) >= 1 && src.size(3) <= lim / 4 && src.size(0) <= lim,
              "augment: sizes out of range");
  TORCH_CHECK(out_h >= 1 && out_h <= H && out_w >= 1 && out_w <= W, "augment: the output must be no larger than the input");
  TORCH_CHECK(off_h_count >= 1 && off_w_count >= 1, "augment: an offset range needs at least one value");
  TORCH_CHECK(off_h_lo >= -H && off_h_lo + off_h_count - 1 <= H && off_w_lo >= -W && off_w_lo + off_w_count - 1 <= W,
              "augment: offsets must stay within [-size, size]");
  const bool bf16 = src.scalar_type() == at::kBFloat16;
  tdl::AugmentArgs a;
  a.src = src.data_ptr();
  a.dst = nullptr;
  a.N = src.size(0);
  a.H = (int)H;
  a.W = (int)W;
  a.Ho = (int)out_h;
  a.Wo = (int)out_w;
  a.C = (int)src.size(3);
  a.state = nullptr;
  a.ticket_in = nullptr;
  a.ticket_out = nullptr;
  a.k0 = (uint32_t)k0;
  a.k1 = (uint32_t)k1;
  a.spec.flip_h = flip_h;
  a.spec.flip_w = flip_w;
  a.spec.off_h_lo = (int)off_h_lo;
  a.spec.off_h_count = (int)off_h_count;
  a.spec.off_w_lo = (int)off_w_lo;
  a.spec.off_w_count = (int)off_w_count;
  a.spec.fill_mode = (int)fill_mode;
  // the fill value rounded ONCE to the tensor's dtype (bf16: to nearest even), as bits
  if (bf16) {
    a.spec.fill_bits = (uint32_t)c10::BFloat16((float)fill_value).x;
  } else {
    const float f = (float)fill_value;
    memcpy(&a.spec.fill_bits, &f, 4);
  }
  a.bf16 = bf16;
  return a;
}

std::vector<at::Tensor> augment_fwd(at::Tensor x, at::Tensor state, int64_t k0, int64_t k1, bool flip_h, bool flip_w,
                                    int64_t off_h_lo, int64_t off_h_count, int64_t off_w_lo, int64_t off_w_count,
                                    int64_t out_h, int64_t out_w, int64_t fill_mode, double fill_value) {
  TORCH_CHECK(x.dim() == 4, "augment: NHWC tensor expected");
  auto a = augment_args(x, x.size(1), x.size(2), k0, k1, flip_h, flip_w, off_h_lo, off_h_count, off_w_lo, off_w_count,
                        out_h, out_w, fill_mode, fill_value);
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == at::kLong && state.numel() == 2 && state.is_contiguous() &&
                  state.device() == x.device(),
              "augment: state must be an int64 [calls, arrivals] tensor on x's device");
  auto ticket = at::empty({1}, state.options());
  auto y = at::empty({x.size(0), out_h, out_w, x.size(3)}, x.options());
  a.dst = y.data_ptr();
  a.state = state.data_ptr<int64_t>();
  a.ticket_out = ticket.data_ptr<int64_t>();
  tdl::augment_forward(a, cur_stream());
  return {y, ticket};
}

at::Tensor augment_bwd(at::Tensor dy, at::Tensor ticket, int64_t k0, int64_t k1, bool flip_h, bool flip_w,
                       int64_t off_h_lo, int64_t off_h_count, int64_t off_w_lo, int64_t off_w_count, int64_t out_h,
                       int64_t out_w, int64_t fill_mode, double fill_value, int64_t H, int64_t W) {
  auto a = augment_args(dy, H, W, k0, k1, flip_h, flip_w, off_h_lo, off_h_count, off_w_lo, off_w_count, out_h, out_w,
                        fill_mode, fill_value);
  TORCH_CHECK(dy.size(1) == out_h && dy.size(2) == out_w, "augment: dy must be [N, out_h, out_w, C]");
  TORCH_CHECK(ticket.is_cuda() && ticket.scalar_type() == at::kLong && ticket.numel() == 1 &&
                  ticket.device() == dy.device(),
              "augment: ticket must be the forward's 1-element int64 tensor");
  auto dx = at::empty({dy.size(0), H, W, dy.size(3)}, dy.options());
  a.dst = dx.data_ptr();
  a.ticket_in = ticket.data_ptr<int64_t>();
  tdl::augment_backward(a, cur_stream());
  return dx;
}

// backward of maxpool_fwd(bn_stats=...): (dz, part) -- dz the BN -> ReLU group's masked input gradient,
// part [P + ceil(P/64)][2][C] its BN backward sums (bn_backward(part=...))
std::vector<at::Tensor> maxpool_bwd_bn(at::Tensor dy, at::Tensor arg, std::vector<int64_t> in_shape, int64_t kh,
                                       int64_t kw, int64_t sh, int64_t sw, int64_t pt, int64_t pl, at::Tensor bn_x,
                                       at::Tensor bn_stats) {
  bn_check(dy);
  bn_check(bn_x);
  TORCH_CHECK(dy.dim() == 4 && arg.sizes() == dy.sizes() && arg.scalar_type() == at::kByte && arg.is_contiguous(),
              "maxpool backward: dy / argmax mismatch");
  TORCH_CHECK(in_shape.size() == 4 && in_shape[3] == dy.size(3) && in_shape[0] == dy.size(0), "maxpool: bad shape");
  TORCH_CHECK(bn_x.sizes() == at::IntArrayRef(in_shape) && bn_x.scalar_type() == dy.scalar_type(),
              "maxpool backward: bn_x must be the pool input's batch-norm input");
  const int64_t C = in_shape[3];
  TORCH_CHECK(C <= 2048 && ((C / 8) & (C / 8 - 1)) == 0, "maxpool backward (BN-fused): C / 8 must be a power of two");
  tdl::PoolGeom g{(int)in_shape[0], (int)in_shape[1], (int)in_shape[2], (int)in_shape[3], (int)dy.size(1),
                  (int)dy.size(2), (int)kh, (int)kw, (int)sh, (int)sw, (int)pt, (int)pl, 0};
  auto dx = fresh(in_shape, dy.options());
  const int64_t P = tdl::maxpool_backward_blocks(g);
  auto part = fresh({P + (P + 63) / 64, 2, C}, dy.options().dtype(at::kFloat));
  bn_ss_of(bn_stats, C);
  if (dx.numel() == 0) return {dx, part};  // an empty batch: nothing to launch (and no partial rows)
  tdl::maxpool_backward(dy.data_ptr(), arg.data_ptr<uint8_t>(), dx.data_ptr(), bn_dtype(dy) == tdl::BnDType::kBF16, g,
                        cur_stream(), bn_x.data_ptr(), bn_ss_of(bn_stats, C), part.data_ptr<float>());
  return {dx, part};
}

// The output size must be one the input, filter, stride and top / left padding can produce: the bottom /
// right padding (OH-1)*SH + KH - H - PT that (OH, OW) imply is below the filter size (a larger output
// would read rows no padding explains; the kernels' range checks would hand it zeros, silently).  It may
// be negative: the last rows / columns of the input are then unused (stride 2 on an even size).
// exact (the stride-1 input gradient): the implied padding is also >= 0, every input row is reached.
void conv_geom_consistent(const tdl::ConvGeom& g, const char* what, bool exact = false) {
  TORCH_CHECK(g.SH >= 1 && g.SW >= 1 && g.H >= 1 && g.W >= 1, what, ": strides and image sizes must be positive");
  const int64_t pb = (int64_t)(g.OH - 1) * g.SH + g.KH - g.H - g.PT, pr = (int64_t)(g.OW - 1) * g.SW + g.KW - g.W - g.PL;
  TORCH_CHECK(pb < g.KH && pr < g.KW, what, ": output ", g.OH, "x", g.OW, " is larger than input ", g.H, "x", g.W,
              ", filter ", g.KH, "x", g.KW, ", stride ", g.SH, "x", g.SW, " and padding (", g.PT, ", ", g.PL,
              ") allow (implied bottom / right padding ", pb, ", ", pr, ")");
  TORCH_CHECK(!exact || (pb >= 0 && pr >= 0), what, ": (h, w) = (", g.H, ", ", g.W, ") does not give dy's ", g.OH, "x",
              g.OW, " (implied bottom / right padding ", pb, ", ", pr, ")");
}

tdl::ConvGeom conv_geom(const at::Tensor& x, int64_t oh, int64_t ow, int64_t k, int64_t kh, int64_t kw, int64_t sh,
                        int64_t sw, int64_t pt, int64_t pl) {
  TORCH_CHECK(x.dim() == 4, "conv: NHWC activations expected");
  tdl::ConvGeom g{(int)x.size(0), (int)x.size(1), (int)x.size(2), (int)x.size(3), (int)oh, (int)ow, (int)k,
                  (int)kh, (int)kw, (int)sh, (int)sw, (int)pt, (int)pl};
  TORCH_CHECK(tdl::conv_bf16_supported(g), "conv: unsupported geometry (C and K must be multiples of 64)");
  conv_geom_consistent(g, "conv");
  return g;
}

void conv_check(const at::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kBFloat16, "conv: ", what,
              " must be a contiguous bf16 GPU tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "conv: ", what, " must be 16-byte aligned");
}

// y[N,OH,OW,K] = conv(x[N,H,W,C], w_ohwi[K,KH,KW,C]); top/left padding pt/pl, bottom/right implied by OH/OW
// in_bn: x is the input of a BN -> ReLU (its [4][C] batch statistics); the conv runs over relu(bn(x))
static const float* conv_in_bn(const c10::optional<at::Tensor>& in_bn, const tdl::ConvGeom& g) {
  const float* ss = bn_ss_of(in_bn, g.C);
  TORCH_CHECK(!ss || tdl::conv_in_bn_supported(g),
              "conv: the input-side batch norm takes 1x1 stride-1 unpadded convolutions of <= 512 channels");
  return ss;
}

at::Tensor conv_fwd(at::Tensor x, at::Tensor w_ohwi, int64_t oh, int64_t ow, int64_t sh, int64_t sw, int64_t pt,
                    int64_t pl, c10::optional<at::Tensor> in_bn) {
  conv_check(x, "x");
  conv_check(w_ohwi, "w");
  TORCH_CHECK(w_ohwi.dim() == 4 && w_ohwi.size(3) == x.size(3), "conv_fwd: weights must be OHWI [K,KH,KW,C]");
  auto g = conv_geom(x, oh, ow, w_ohwi.size(0), w_ohwi.size(1), w_ohwi.size(2), sh, sw, pt, pl);
  const float* ss = conv_in_bn(in_bn, g);
  auto y = fresh({x.size(0), oh, ow, w_ohwi.size(0)}, x.options());
  tdl::conv_fwd_bf16(x.data_ptr(), w_ohwi.data_ptr(), y.data_ptr(), g, cur_stream(), nullptr, ss);
  return y;
}

// forward + batch-norm partial sums of y: returns (y, part[P + ceil(P/64)][2][K]) with P row tiles
std::vector<at::Tensor> conv_fwd_stats(at::Tensor x, at::Tensor w_ohwi, int64_t oh, int64_t ow, int64_t sh,
                                       int64_t sw, int64_t pt, int64_t pl, c10::optional<at::Tensor> in_bn) {
  conv_check(x, "x");
  conv_check(w_ohwi, "w");
  TORCH_CHECK(w_ohwi.dim() == 4 && w_ohwi.size(3) == x.size(3), "conv_fwd: weights must be OHWI [K,KH,KW,C]");
  auto g = conv_geom(x, oh, ow, w_ohwi.size(0), w_ohwi.size(1), w_ohwi.size(2), sh, sw, pt, pl);
  const float* ss = conv_in_bn(in_bn, g);
  auto y = fresh({x.size(0), oh, ow, w_ohwi.size(0)}, x.options());
  const int64_t M = (int64_t)g.N * g.OH * g.OW, bm = tdl::conv_fwd_row_tile(g, ss != nullptr);
  const int64_t P = (M + bm - 1) / bm;
  auto part = fresh({P + (P + 63) / 64, 2, (int64_t)g.K}, x.options().dtype(at::kFloat));
  tdl::conv_fwd_bf16(x.data_ptr(), w_ohwi.data_ptr(), y.data_ptr(), g, cur_stream(), part.data_ptr<float>(), ss);
  return {y, part};
}

// stride-1 input gradient: dx[N,H,W,C] from dy[N,OH,OW,K] and w_hwio[KH,KW,C,K]
const void* opt_residual(const c10::optional<at::Tensor>& r, const at::Tensor& like_dy, int64_t n, int64_t h,
                         int64_t w, int64_t c) {
  if (!r.has_value() || !r->defined()) return nullptr;
  conv_check(*r, "residual");
  TORCH_CHECK(r->dim() == 4 && r->size(0) == n && r->size(1) == h && r->size(2) == w && r->size(3) == c,
              "conv dgrad: residual must be shaped like dx");
  (void)like_dy;
  return r->data_ptr();
}

std::vector<at::Tensor> conv_dgrad_impl(at::Tensor dy, at::Tensor w_hwio, int64_t h, int64_t w, int64_t pt,
                                        int64_t pl, c10::optional<at::Tensor> residual,
                                        c10::optional<at::Tensor> bn_y, c10::optional<at::Tensor> bn_x,
                                        c10::optional<at::Tensor> bn_x2, c10::optional<at::Tensor> bn_stats);

// BN-group fusion operands of an input gradient (see conv.h): (bn_y, bn_x[, bn_x2]) tensors shaped
// like dx, and the part buffers [P + ceil(P/64)][2][C] for P row tiles
// bn_stats: the [4][C] statistics (mean, invstd, scale, shift) of a plain BN -> ReLU group's forward:
// the mask is recomputed from bn_x (bn_y may then be absent)
struct DgradBn {
  const void *by = nullptr, *bx = nullptr, *bx2 = nullptr;
  const float* ss = nullptr;
  at::Tensor part, part2;
  DgradBn(const c10::optional<at::Tensor>& bn_y, const c10::optional<at::Tensor>& bn_x,
          const c10::optional<at::Tensor>& bn_x2, const c10::optional<at::Tensor>& bn_stats, const at::Tensor& dy,
          int64_t h, int64_t w, int64_t c, int64_t P) {
    by = opt_residual(bn_y, dy, dy.size(0), h, w, c);
    bx = opt_residual(bn_x, dy, dy.size(0), h, w, c);
    bx2 = opt_residual(bn_x2, dy, dy.size(0), h, w, c);
    if (bn_stats.has_value() && bn_stats->defined()) {
      TORCH_CHECK(bn_stats->is_cuda() && bn_stats->is_contiguous() && bn_stats->scalar_type() == at::kFloat &&
                      bn_stats->numel() == 4 * c,
                  "conv_dgrad: bn_stats must be the f32 [4][C] statistics of the group's BN");
      ss = bn_stats->data_ptr<float>() + 2 * c;  // scale[C], shift[C]
    }
    TORCH_CHECK((by != nullptr || ss != nullptr) == (bx != nullptr), "conv_dgrad: bn_y (or bn_stats) and bn_x go together");
    TORCH_CHECK(bx2 == nullptr || bx != nullptr, "conv_dgrad: bn_x2 needs bn_x");
    auto f = dy.options().dtype(at::kFloat);
    if (bx) part = fresh({P + (P + 63) / 64, 2, c}, f);
    if (bx2) part2 = fresh({P + (P + 63) / 64, 2, c}, f);
  }
  float* p() { return bx ? part.data_ptr<float>() : nullptr; }
  float* p2() { return bx2 ? part2.data_ptr<float>() : nullptr; }
  std::vector<at::Tensor> out(const at::Tensor& dx) {
    if (bx2) return {dx, part, part2};
    if (bx) return {dx, part};
    return {dx};
  }
};

at::Tensor conv_dgrad(at::Tensor dy, at::Tensor w_hwio, int64_t h, int64_t w, int64_t pt, int64_t pl,
                      c10::optional<at::Tensor> residual) {
  return conv_dgrad_impl(dy, w_hwio, h, w, pt, pl, residual, c10::nullopt, c10::nullopt, c10::nullopt, c10::nullopt)[0];
}

// input gradient with the fused backward of the BN -> Add -> ReLU group that produced the conv's
// input bn_y from bn_x: returns (dz, part[P + ceil(P/64)][2][C][, part2]); bn_x2: the input of the
// plain BN whose output is the group's residual (part2: its backward sums); bn_stats instead of bn_y:
// a plain BN -> ReLU group, mask recomputed from bn_x
std::vector<at::Tensor> conv_dgrad_bn(at::Tensor dy, at::Tensor w_hwio, int64_t h, int64_t w, int64_t pt, int64_t pl,
                                      c10::optional<at::Tensor> residual, c10::optional<at::Tensor> bn_y,
                                      at::Tensor bn_x, c10::optional<at::Tensor> bn_x2,
                                      c10::optional<at::Tensor> bn_stats) {
  return conv_dgrad_impl(dy, w_hwio, h, w, pt, pl, residual, bn_y, bn_x, bn_x2, bn_stats);
}

std::vector<at::Tensor> conv_dgrad_impl(at::Tensor dy, at::Tensor w_hwio, int64_t h, int64_t w, int64_t pt,
                                        int64_t pl, c10::optional<at::Tensor> residual,
                                        c10::optional<at::Tensor> bn_y, c10::optional<at::Tensor> bn_x,
                                        c10::optional<at::Tensor> bn_x2, c10::optional<at::Tensor> bn_stats) {
  conv_check(dy, "dy");
  conv_check(w_hwio, "w");
  TORCH_CHECK(dy.dim() == 4, "conv_dgrad: dy must be NHWC [N,OH,OW,K]");
  TORCH_CHECK(w_hwio.dim() == 4 && w_hwio.size(3) == dy.size(3), "conv_dgrad: weights must be HWIO [KH,KW,C,K]");
  tdl::ConvGeom g{(int)dy.size(0), (int)h, (int)w, (int)w_hwio.size(2), (int)dy.size(1), (int)dy.size(2),
                  (int)dy.size(3), (int)w_hwio.size(0), (int)w_hwio.size(1), 1, 1, (int)pt, (int)pl};
  TORCH_CHECK(tdl::conv_bf16_supported(g), "conv_dgrad: unsupported geometry (C and K must be multiples of 64)");
  conv_geom_consistent(g, "conv_dgrad", true);
  auto dx = fresh({dy.size(0), h, w, w_hwio.size(2)}, dy.options(), 2);
  const int64_t M = (int64_t)g.N * g.H * g.W, bm = tdl::conv_dgrad_row_tile(g);
  DgradBn bn(bn_y, bn_x, bn_x2, bn_stats, dy, h, w, w_hwio.size(2), (M + bm - 1) / bm);
  tdl::conv_dgrad_bf16(dy.data_ptr(), w_hwio.data_ptr(), dx.data_ptr(), g, cur_stream(),
                       opt_residual(residual, dy, dy.size(0), h, w, w_hwio.size(2)), bn.by, bn.bx, bn.p(), bn.bx2,
                       bn.p2(), bn.ss);
  return bn.out(dx);
}
// input gradient of a 1x1 stride-2 unpadded conv: dx[N,H,W,C] from dy[N,OH,OW,K] and w_hwio[1,1,C,K];
// with bn_y / bn_x[ / bn_x2] the fused BN-group backward as in conv_dgrad_bn: (dz, part[, part2])
std::vector<at::Tensor> conv_dgrad_s2_impl(at::Tensor dy, at::Tensor w_hwio, int64_t h, int64_t w,
                                           c10::optional<at::Tensor> residual, c10::optional<at::Tensor> bn_y,
                                           c10::optional<at::Tensor> bn_x, c10::optional<at::Tensor> bn_x2,
                                           c10::optional<at::Tensor> bn_stats) {
  conv_check(dy, "dy");
  conv_check(w_hwio, "w");
  TORCH_CHECK(dy.dim() == 4, "conv_dgrad_s2: dy must be NHWC [N,OH,OW,K]");
  TORCH_CHECK(w_hwio.dim() == 4 && w_hwio.size(0) == 1 && w_hwio.size(1) == 1 && w_hwio.size(3) == dy.size(3),
              "conv_dgrad_s2: weights must be HWIO [1,1,C,K]");
  TORCH_CHECK(h <= 2 * dy.size(1) && w <= 2 * dy.size(2) && h > 2 * (dy.size(1) - 1) && w > 2 * (dy.size(2) - 1),
              "conv_dgrad_s2: (h, w) inconsistent with a stride-2 1x1 conv");
  tdl::ConvGeom g{(int)dy.size(0), (int)h, (int)w, (int)w_hwio.size(2), (int)dy.size(1), (int)dy.size(2),
                  (int)dy.size(3), 1, 1, 2, 2, 0, 0};
  TORCH_CHECK(tdl::conv_bf16_supported(g), "conv_dgrad_s2: unsupported geometry (C and K must be multiples of 64)");
  auto dx = fresh({dy.size(0), h, w, w_hwio.size(2)}, dy.options(), 2);
  const int64_t M = (int64_t)g.N * g.OH * g.OW, bm = tdl::conv_dgrad_s2_row_tile(g);
  DgradBn bn(bn_y, bn_x, bn_x2, bn_stats, dy, h, w, w_hwio.size(2), (M + bm - 1) / bm);
  tdl::conv_dgrad_s2_1x1_bf16(dy.data_ptr(), w_hwio.data_ptr(), dx.data_ptr(), g, cur_stream(),
                              opt_residual(residual, dy, dy.size(0), h, w, w_hwio.size(2)), bn.by, bn.bx, bn.p(),
                              bn.bx2, bn.p2(), bn.ss);
  return bn.out(dx);
}

at::Tensor conv_dgrad_s2(at::Tensor dy, at::Tensor w_hwio, int64_t h, int64_t w, c10::optional<at::Tensor> residual) {
  return conv_dgrad_s2_impl(dy, w_hwio, h, w, residual, c10::nullopt, c10::nullopt, c10::nullopt, c10::nullopt)[0];
}

std::vector<at::Tensor> conv_dgrad_s2_bn(at::Tensor dy, at::Tensor w_hwio, int64_t h, int64_t w,
                                         c10::optional<at::Tensor> residual, c10::optional<at::Tensor> bn_y,
                                         at::Tensor bn_x, c10::optional<at::Tensor> bn_x2,
                                         c10::optional<at::Tensor> bn_stats) {
  return conv_dgrad_s2_impl(dy, w_hwio, h, w, residual, bn_y, bn_x, bn_x2, bn_stats);
}

// weight gradient: dw[KH,KW,C,K] (bf16, or added into the f32 `out` when given) from x[N,H,W,C] and
// dy[N,OH,OW,K]; deterministic split-K.  plan = [wmw, wnw, nsplit] (empty: the model's first choice)
at::Tensor conv_wgrad(at::Tensor x, at::Tensor dy, int64_t kh, int64_t kw, int64_t sh, int64_t sw, int64_t pt,
                      int64_t pl, c10::optional<at::Tensor> out, bool accumulate, std::vector<int64_t> plan,
                      c10::optional<at::Tensor> in_bn) {
  conv_check(x, "x");
  conv_check(dy, "dy");
  TORCH_CHECK(dy.dim() == 4 && dy.size(0) == x.size(0), "conv_wgrad: dy must be NHWC [N,OH,OW,K]");
  auto g = conv_geom(x, dy.size(1), dy.size(2), dy.size(3), kh, kw, sh, sw, pt, pl);
  const float* ss = conv_in_bn(in_bn, g);
  TORCH_CHECK(!ss || plan.empty() || (plan[0] != 0 && plan[0] * plan[1] <= 4 && (plan.size() == 3 || plan[3] == 0)),
              "conv_wgrad: the input-side batch norm runs on the register-staged plans (<= 4 waves, kind 0)");
  // (a smaller output is a legal 1x1 geometry, but the input-side BN staging reads pixel m of x for row m of dy)
  TORCH_CHECK(!ss || (g.H == g.OH && g.W == g.OW), "conv_wgrad: the input-side batch norm needs dy as large as x");
  TORCH_CHECK(tdl::conv_wgrad_supported(g), "conv_wgrad: N*OH*OW must be < 2^24");
  TORCH_CHECK(plan.empty() || plan.size() == 3 || plan.size() == 4, "conv_wgrad: plan = [wmw, wnw, nsplit(, kind)]");
  if (!plan.empty() && plan[0] == 0) {  // [0, 0, 0]: the row kernel of 3x3 / C = 64 convs (wgrad3x3.hip)
    TORCH_CHECK(tdl::conv_wgrad3x3_c64_supported(g), "conv_wgrad: the 3x3 row kernel does not take this shape");
    auto ws = fresh({tdl::conv_wgrad3x3_c64_ws_elems(g)}, x.options().dtype(at::kFloat));
    if (out.has_value()) {
      auto& o = *out;
      TORCH_CHECK(o.is_cuda() && o.is_contiguous() && o.scalar_type() == at::kFloat &&
                      o.numel() == kh * kw * x.size(3) * dy.size(3),
                  "conv_wgrad: out must be a contiguous f32 tensor of KH*KW*C*K elements");
      tdl::conv_wgrad3x3_c64(x.data_ptr(), dy.data_ptr(), ws.data_ptr<float>(), nullptr, o.data_ptr<float>(), accumulate,
                             g, cur_stream());
      return o;
    }
    auto dw = fresh({kh, kw, x.size(3), dy.size(3)}, x.options());
    tdl::conv_wgrad3x3_c64(x.data_ptr(), dy.data_ptr(), ws.data_ptr<float>(), dw.data_ptr(), nullptr, false, g,
                           cur_stream());
    return dw;
  }
  tdl::WgradPlan p;
  if (plan.empty()) {
    p = tdl::conv_wgrad_plans(g, 1, ss != nullptr).at(0);
  } else {
    const int wmw = (int)plan[0], wnw = (int)plan[1];
    TORCH_CHECK((wmw == 1 || wmw == 2 || wmw == 4) && (wnw == 1 || wnw == 2 || wnw == 4) &&
                    (wmw * wnw <= 4 || (wmw * wnw == 8 && wmw != wnw)) &&
                    g.K % (64 * wmw) == 0 && plan[2] >= 1 &&
                    (plan.size() == 3 || plan[3] == 0 || (plan[3] == 1 && wmw == 2 && wnw == 2)),
                "conv_wgrad: bad plan");
    p = tdl::conv_wgrad_make_plan(g, wmw, wnw, (int)plan[2], plan.size() == 4 ? (int)plan[3] : 0);
  }
  auto ws = fresh({p.ws_elems}, x.options().dtype(at::kFloat));
  if (out.has_value()) {
    auto& o = *out;
    TORCH_CHECK(o.is_cuda() && o.is_contiguous() && o.scalar_type() == at::kFloat &&
                    o.numel() == kh * kw * x.size(3) * dy.size(3),
                "conv_wgrad: out must be a contiguous f32 tensor of KH*KW*C*K elements");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(o.data_ptr()) % 16 == 0, "conv_wgrad: out must be 16-byte aligned");
    tdl::conv_wgrad_bf16(x.data_ptr(), dy.data_ptr(), ws.data_ptr<float>(), p, nullptr, o.data_ptr<float>(),
                         accumulate, g, cur_stream(), ss);
    return o;
  }
  auto dw = fresh({kh, kw, x.size(3), dy.size(3)}, x.options());
  tdl::conv_wgrad_bf16(x.data_ptr(), dy.data_ptr(), ws.data_ptr<float>(), p, dw.data_ptr(), nullptr, false, g,
                       cur_stream(), ss);
  return dw;
}

// small-channel stride-2 conv (ResNet stem, csrc/kernels/stem.hip).  x [N,H,W,C] (bf16 or f32,
// C <= 4), w_hwio [KH,KW,C,K] bf16, zero padding (pt, pb, pl, pr) folded into the packed copy.
// Returns (y [N,OH,OW,K] bf16, xp packed image for the backward[, part [P + ceil(P/64)][2][K]])
std::vector<at::Tensor> stem_fwd(at::Tensor x, at::Tensor w_hwio, int64_t pt, int64_t pb, int64_t pl, int64_t pr,
                                 int64_t sh, int64_t sw, bool stats) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 4 &&
                  (x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat),
              "stem: x must be a contiguous NHWC bf16/f32 GPU tensor");
  conv_check(w_hwio, "w");
  TORCH_CHECK(w_hwio.dim() == 4 && w_hwio.size(2) == x.size(3), "stem: weights must be HWIO [KH,KW,C,K]");
  const int N = (int)x.size(0), H = (int)x.size(1), W = (int)x.size(2), C = (int)x.size(3);
  const int KH = (int)w_hwio.size(0), KW = (int)w_hwio.size(1), K = (int)w_hwio.size(3);
  TORCH_CHECK(tdl::stem_supported(C, KH, KW, (int)sw, K) && sh >= 1 && pt >= 0 && pb >= 0 && pl >= 0 && pr >= 0,
              "stem: unsupported geometry");
  const int HP = H + (int)(pt + pb), WPv = W + (int)(pl + pr);
  // (a padded image smaller than the filter has no output: the division below truncates toward zero
  // and would count one)
  TORCH_CHECK(N > 0 && HP >= KH && WPv >= KW, "stem: empty output");
  const int OH = (HP - KH) / (int)sh + 1, OW = (WPv - KW) / 2 + 1;
  // packed width: every receptive field reads 8 columns (taps past KW are zero-weighted): 2(OW-1)+8
  const int WP = std::max(WPv, 2 * (OW - 1) + 8);
  const int HPp = std::max(HP, (OH - 1) * (int)sh + KH);
  TORCH_CHECK((long long)N * HPp * WP * 4 < (1LL << 31), "stem: packed image too large");
  auto xp = fresh({N, HPp, WP, 4}, x.options().dtype(at::kBFloat16));
  tdl::stem_pack(x.data_ptr(), x.scalar_type() == at::kBFloat16, xp.data_ptr(), N, H, W, C, HPp, WP, (int)pt, (int)pl,
                 cur_stream());
  auto wp = fresh({K, KH, 32}, w_hwio.options());
  tdl::stem_wpack(w_hwio.data_ptr(), wp.data_ptr(), KH, KW, C, K, cur_stream());
  auto y = fresh({N, OH, OW, K}, x.options().dtype(at::kBFloat16));
  const int64_t M = (int64_t)N * OH * OW, bm = tdl::stem_fwd_row_tile(), P = (M + bm - 1) / bm;
  at::Tensor part;
  if (stats) part = fresh({P + (P + 63) / 64, 2, (int64_t)K}, x.options().dtype(at::kFloat));
  tdl::stem_fwd(xp.data_ptr(), wp.data_ptr(), y.data_ptr(), stats ? part.data_ptr<float>() : nullptr, N, HPp, WP, OH,
                OW, K, KH, (int)sh, cur_stream());
  if (stats) return {y, xp, part};
  return {y, xp};
}

// weight gradient of stem_fwd from its packed image: dW HWIO [KH,KW,C,K] bf16, or added into the f32
// `out` (accumulate) / written to it
at::Tensor stem_wgrad(at::Tensor xp, at::Tensor dy, int64_t kh, int64_t kw, int64_t c, int64_t sh,
                      c10::optional<at::Tensor> out, bool accumulate) {
  conv_check(xp, "xp");
  conv_check(dy, "dy");
  TORCH_CHECK(xp.dim() == 4 && xp.size(3) == 4 && dy.dim() == 4 && dy.size(0) == xp.size(0), "stem_wgrad: shapes");
  const int N = (int)xp.size(0), HP = (int)xp.size(1), WP = (int)xp.size(2);
  const int OH = (int)dy.size(1), OW = (int)dy.size(2), K = (int)dy.size(3);
  TORCH_CHECK(tdl::stem_supported((int)c, (int)kh, (int)kw, 2, K) && sh >= 1 && N > 0 && OH > 0 && OW > 0 &&
                  (OH - 1) * sh + kh <= HP &&
                  2 * (OW - 1) + 8 <= WP,
              "stem_wgrad: geometry inconsistent with the packed image");
  const int M = N * OH * OW;
  auto ws = fresh({tdl::stem_wgrad_ws_elems(M, K, (int)kh)}, dy.options().dtype(at::kFloat));
  if (out.has_value()) {
    auto& o = *out;
    TORCH_CHECK(o.is_cuda() && o.is_contiguous() && o.scalar_type() == at::kFloat && o.numel() == kh * kw * c * K,
                "stem_wgrad: out must be a contiguous f32 tensor of KH*KW*C*K elements");
    tdl::stem_wgrad(xp.data_ptr(), dy.data_ptr(), ws.data_ptr<float>(), N, HP, WP, OH, OW, K, (int)kh, (int)kw, (int)c,
                    (int)sh, o.data_ptr<float>(), nullptr, accumulate, cur_stream());
    return o;
  }
  auto dw = fresh({kh, kw, c, (int64_t)K}, dy.options());
  tdl::stem_wgrad(xp.data_ptr(), dy.data_ptr(), ws.data_ptr<float>(), N, HP, WP, OH, OW, K, (int)kh, (int)kw, (int)c,
                  (int)sh, nullptr, dw.data_ptr(), false, cur_stream());
  return dw;
}

// the model's best candidate plans: [[wmw, wnw, chunk, nsplit, kind], ...]
std::vector<std::vector<int64_t>> conv_wgrad_plans(std::vector<int64_t> x_shape, std::vector<int64_t> dy_shape,
                                                   int64_t kh, int64_t kw, int64_t sh, int64_t sw, int64_t pt,
                                                   int64_t pl, int64_t max_plans, bool in_bn) {
  tdl::ConvGeom g{(int)x_shape[0], (int)x_shape[1], (int)x_shape[2], (int)x_shape[3], (int)dy_shape[1],
                  (int)dy_shape[2], (int)dy_shape[3], (int)kh, (int)kw, (int)sh, (int)sw, (int)pt, (int)pl};
  std::vector<std::vector<int64_t>> out;
  // the 3x3 / C = 64 row kernel first where it applies (it beats the split-K tiles on these shapes)
  if (!in_bn && tdl::conv_wgrad3x3_c64_supported(g)) out.push_back({0, 0, 0, 0, 0});
  for (const auto& p : tdl::conv_wgrad_plans(g, (int)max_plans, in_bn))
    out.push_back({p.wmw, p.wnw, p.chunk, p.nsplit, p.kind});
  return out;
}
// (kernel name, row tile) the launch of one conv geometry takes under the current A/B hooks (conv.h
// conv_selected; no GPU needed).  direction "fwd" | "dgrad" | "dgrad_s2"; x_shape [N,H,W,C] the conv's
// input (dx of a gradient), w_shape the direction's own weight layout (OHWI forward, HWIO gradients),
// (oh, ow) the conv's output size, strides and top / left padding the conv's.  flags: "stats", "residual"
// (neither moves the selection), "bn" (BN-group backward), "bn_ss" (its mask from bn_stats), "in_bn".
std::tuple<std::string, int64_t> conv_selected(const std::string& direction, std::vector<int64_t> x_shape,
                                               std::vector<int64_t> w_shape, int64_t oh, int64_t ow, int64_t sh,
                                               int64_t sw, int64_t pt, int64_t pl, std::vector<std::string> flags) {
  const int dir = direction == "fwd" ? 0 : (direction == "dgrad" ? 1 : (direction == "dgrad_s2" ? 2 : -1));
  TORCH_CHECK(dir >= 0, "conv_selected: direction must be fwd, dgrad or dgrad_s2");
  TORCH_CHECK(x_shape.size() == 4 && w_shape.size() == 4, "conv_selected: x_shape [N,H,W,C] and a 4-D w_shape expected");
  bool bn = false, bn_ss = false, in_bn = false;
  for (const auto& f : flags) {
    TORCH_CHECK(f == "stats" || f == "residual" || f == "bn" || f == "bn_ss" || f == "in_bn",
                "conv_selected: unknown flag ", f);
    bn = bn || f == "bn";
    bn_ss = bn_ss || f == "bn_ss";
    in_bn = in_bn || f == "in_bn";
  }
  const int64_t k = dir == 0 ? w_shape[0] : w_shape[3], kh = dir == 0 ? w_shape[1] : w_shape[0],
                kw = dir == 0 ? w_shape[2] : w_shape[1], c = dir == 0 ? w_shape[3] : w_shape[2];
  TORCH_CHECK(c == x_shape[3], "conv_selected: the weights' input channels must match x_shape");
  TORCH_CHECK(dir == 0 || !in_bn, "conv_selected: in_bn is a forward flag");
  TORCH_CHECK(dir != 0 || !(bn || bn_ss), "conv_selected: bn / bn_ss are input-gradient flags");
  tdl::ConvGeom g{(int)x_shape[0], (int)x_shape[1], (int)x_shape[2], (int)c, (int)oh, (int)ow, (int)k,
                  (int)kh, (int)kw, (int)sh, (int)sw, (int)pt, (int)pl};
  TORCH_CHECK(dir != 1 || (sh == 1 && sw == 1), "conv_selected: dgrad is the stride-1 input gradient");
  TORCH_CHECK(dir != 2 || (sh == 2 && sw == 2 && kh == 1 && kw == 1 && pt == 0 && pl == 0),
              "conv_selected: dgrad_s2 is the input gradient of a 1x1 stride-2 unpadded conv");
  TORCH_CHECK(tdl::conv_bf16_supported(g), "conv_selected: unsupported geometry (C and K must be multiples of 64)");
  conv_geom_consistent(g, "conv_selected", dir == 1);
  TORCH_CHECK(!in_bn || tdl::conv_in_bn_supported(g),
              "conv_selected: the input-side batch norm takes 1x1 stride-1 unpadded convolutions of <= 512 channels");
  const auto r = tdl::conv_selected(dir, g, bn || bn_ss, bn_ss, in_bn);
  return {r.name, (int64_t)r.row_tile};
}

// dst (bf16 slab) <- transposed copies of the HWIO f32 conv kernels in src (f32 slab); entries
// [E][4] (src off, dst off, R, K) and tiles [T][4] (entry, row tile, col tile, 0) int32 on the GPU
void slab_transpose_bf16(at::Tensor src, at::Tensor dst, at::Tensor entries, at::Tensor tiles) {
  TORCH_CHECK(src.is_cuda() && src.is_contiguous() && src.scalar_type() == at::kFloat, "slab_transpose: f32 src");
  TORCH_CHECK(dst.is_cuda() && dst.is_contiguous() && dst.scalar_type() == at::kBFloat16, "slab_transpose: bf16 dst");
  TORCH_CHECK(entries.is_cuda() && entries.scalar_type() == at::kInt && entries.dim() == 2 && entries.size(1) == 4,
              "slab_transpose: entries [E][4] int32");
  TORCH_CHECK(tiles.is_cuda() && tiles.scalar_type() == at::kInt && tiles.dim() == 2 && tiles.size(1) == 4,
              "slab_transpose: tiles [T][4] int32");
  tdl::slab_transpose_bf16(src.data_ptr<float>(), reinterpret_cast<uint16_t*>(dst.data_ptr()),
                           entries.data_ptr<int>(), tiles.data_ptr<int>(), (int)tiles.size(0), cur_stream());
}
void slab_cast_bf16(at::Tensor src, at::Tensor dst) {
  TORCH_CHECK(src.is_cuda() && src.is_contiguous() && src.scalar_type() == at::kFloat, "slab_cast: f32 src");
  TORCH_CHECK(dst.is_cuda() && dst.is_contiguous() && dst.scalar_type() == at::kBFloat16, "slab_cast: bf16 dst");
  TORCH_CHECK(src.numel() == dst.numel() && src.numel() % 8 == 0, "slab_cast: sizes (multiple of 8)");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(src.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(dst.data_ptr()) % 16 == 0,
              "slab_cast: 16-byte aligned buffers");
  tdl::cast_bf16(src.data_ptr<float>(), reinterpret_cast<uint16_t*>(dst.data_ptr()), src.numel(), cur_stream());
}
void bf16_check(const at::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.dim() == 2 && t.stride(1) == 1, what,
              " must be a 2-D row-major bf16 GPU tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0 && t.stride(0) % 8 == 0, what,
              " must be 16-byte aligned (rows too)");
}

// C = alpha * op(A) op(B) (+ bias), see kernels/gemm.h; A/B given in their STORED [rows][cols] form:
// ta = 0: a is [M][K], ta = 1: a is [K][M]; tb = 0: b is [N][K], tb = 1: b is [K][N].
// out: f32 [M][N] (+= when accumulate) or None -> a new bf16 [M][N]
at::Tensor gemm_bf16(at::Tensor a, int64_t ta, at::Tensor b, int64_t tb, c10::optional<at::Tensor> bias,
                     c10::optional<at::Tensor> out, bool accumulate, double alpha) {
  bf16_check(a, "gemm: a");
  bf16_check(b, "gemm: b");
  const int64_t M = ta ? a.size(1) : a.size(0), K = ta ? a.size(0) : a.size(1);
  const int64_t N = tb ? b.size(1) : b.size(0), Kb = tb ? b.size(0) : b.size(1);
  TORCH_CHECK(K == Kb, "gemm: inner dimensions differ");
  TORCH_CHECK(tdl::gemm_bf16_supported((int)M, (int)N, (int)K), "gemm: M, N, K must be multiples of 8");
  const float* bp = nullptr;
  if (bias.has_value() && bias->defined()) {
    TORCH_CHECK(bias->is_cuda() && bias->scalar_type() == at::kFloat && bias->is_contiguous() && bias->numel() == N &&
                    reinterpret_cast<uintptr_t>(bias->data_ptr()) % 16 == 0,
                "gemm: bias must be a 16-byte aligned contiguous f32 [N]");
    bp = bias->data_ptr<float>();
  }
  if (out.has_value() && out->defined()) {
    auto& o = *out;
    TORCH_CHECK(o.is_cuda() && o.scalar_type() == at::kFloat && o.dim() == 2 && o.size(0) == M && o.size(1) == N &&
                    o.stride(1) == 1 && o.stride(0) % 4 == 0 && reinterpret_cast<uintptr_t>(o.data_ptr()) % 16 == 0,
                "gemm: out must be a 16-byte aligned row-major f32 [M][N]");
    tdl::gemm_bf16((int)ta, (int)tb, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), (int)M, (int)N, (int)K,
                   o.data_ptr<float>(), nullptr, o.stride(0), bp, (float)alpha, accumulate, cur_stream());
    return o;
  }
  auto c = fresh({M, N}, a.options());
  tdl::gemm_bf16((int)ta, (int)tb, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), (int)M, (int)N, (int)K,
                 nullptr, c.data_ptr(), N, bp, (float)alpha, false, cur_stream());
  return c;
}

// ---- generic f32 GEMM / convolution (kernels/gemm_f32.hip) ----
void f32_check(const at::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous(), what,
              " must be a contiguous f32 GPU tensor");
}
bool al16(const at::Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; }

// TDL_F32_SPLIT="kmin,cap" (A/B of the split plan; default 64,1024)
const std::pair<int, int>& f32_split_plan() {
  static const std::pair<int, int> plan = [] {
    int kmin = 64, cap = 1024;
    if (const char* e = std::getenv("TDL_F32_SPLIT")) std::sscanf(e, "%d,%d", &kmin, &cap);
    return std::make_pair(kmin < 16 ? 16 : kmin, cap < 1 ? 1 : cap);
  }();
  return plan;
}

tdl::F32Selected g_f32_last;  // what the most recent f32 launch of this process took (f32_last_selected)

void f32_run(int mode, tdl::F32GemmArgs& a, const at::TensorOptions& o) {
  TORCH_CHECK(a.Kred > 0, "f32 gemm: empty reduction");
  const auto& plan = f32_split_plan();
  tdl::f32_gemm_plan(a, plan.first, plan.second);
  at::Tensor ws;
  if (a.splits > 1) {
    ws = at::empty({(int64_t)a.splits * a.M * a.N}, o);
    a.ws = ws.data_ptr<float>();
  }
  g_f32_last = tdl::f32_gemm_launch(mode, a, cur_stream());
}

// (splits, kchunk, unfused_splits) of an M x N x Kred problem (pool: the pooled conv, whose plan is the
// unfused conv's over plan_m rows unless that has 16 or more slices); no device needed
std::tuple<int64_t, int64_t, int64_t> f32_plan(int64_t M, int64_t N, int64_t Kred, bool pool, int64_t plan_m) {
  TORCH_CHECK(M > 0 && N > 0 && Kred > 0, "f32_plan: positive sizes");
  const auto& plan = f32_split_plan();
  tdl::F32GemmArgs a{}, u{};
  a.M = (int)M, a.N = (int)N, a.Kred = (int)Kred, a.pool = pool ? 1 : 0, a.plan_m = (int)plan_m;
  u.M = (int)(plan_m > 0 ? plan_m : M), u.N = (int)N, u.Kred = (int)Kred;
  tdl::f32_gemm_plan(a, plan.first, plan.second);
  tdl::f32_gemm_plan(u, plan.first, plan.second);
  return std::make_tuple((int64_t)a.splits, (int64_t)a.kchunk, (int64_t)u.splits);
}

const float* f32_bias(const c10::optional<at::Tensor>& bias, int64_t n) {
  if (!bias.has_value() || !bias->defined()) return nullptr;
  f32_check(*bias, "f32 gemm: bias");
  TORCH_CHECK(bias->numel() == n, "f32 gemm: bias must have N elements");
  return bias->data_ptr<float>();
}

// out: f32 [rows][cols] given (accumulate: +=) or a new tensor
at::Tensor f32_out(c10::optional<at::Tensor>& out, at::IntArrayRef shape, const at::TensorOptions& o) {
  if (out.has_value() && out->defined()) {
    f32_check(*out, "f32 gemm: out");
    TORCH_CHECK(out->sizes() == shape, "f32 gemm: out has the wrong shape");
    return *out;
  }
  return fresh(shape, o);
}

// ReLU mask of an operand (the layer's output, same layout as the operand): nullptr when absent
const float* f32_mask(const c10::optional<at::Tensor>& mask, const at::Tensor& like, const char* what) {
  if (!mask.has_value() || !mask->defined()) return nullptr;
  f32_check(*mask, what);
  TORCH_CHECK(mask->numel() == like.numel(), what, " must have the operand's shape");
  return mask->data_ptr<float>();
}
bool mask_al16(const c10::optional<at::Tensor>& mask) {
  return !mask.has_value() || !mask->defined() || al16(*mask);
}
// bias gradient target [n] (written, or += when accumulating)
float* f32_dbias(c10::optional<at::Tensor>& dbias, int64_t n) {
  if (!dbias.has_value() || !dbias->defined()) return nullptr;
  f32_check(*dbias, "f32 gemm: dbias");
  TORCH_CHECK(dbias->numel() == n, "f32 gemm: dbias must have ", n, " elements");
  return dbias->data_ptr<float>();
}

// C = op(A) op(B) (+ bias) in f32; ta = 0: a is [M][K], 1: [K][M]; tb = 0: b is [N][K], 1: [K][N].
// act = 1: ReLU epilogue.  amask / bmask: operand * (mask > 0) (ReLU backward).  dbias: a row of ones
// appended to A, its output row (the column sums of op(B): a bias gradient) written to dbias.
at::Tensor gemm_f32(at::Tensor a, int64_t ta, at::Tensor b, int64_t tb, c10::optional<at::Tensor> bias,
                    c10::optional<at::Tensor> out, bool accumulate, int64_t act, c10::optional<at::Tensor> amask,
                    c10::optional<at::Tensor> bmask, c10::optional<at::Tensor> dbias) {
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2, "gemm_f32: 2-D operands");
  f32_check(a, "gemm_f32: a");
  f32_check(b, "gemm_f32: b");
  const int64_t M = ta ? a.size(1) : a.size(0), K = ta ? a.size(0) : a.size(1);
  const int64_t N = tb ? b.size(1) : b.size(0), Kb = tb ? b.size(0) : b.size(1);
  TORCH_CHECK(K == Kb, "gemm_f32: inner dimensions differ");
  auto c = f32_out(out, {M, N}, a.options());
  tdl::F32GemmArgs g{};
  g.a = a.data_ptr<float>();
  g.b = b.data_ptr<float>();
  g.na = a.numel();
  g.nb = b.numel();
  g.out = c.data_ptr<float>();
  g.bias = f32_bias(bias, N);
  g.sam = ta ? 1 : a.stride(0);
  g.sak = ta ? a.stride(0) : 1;
  g.sbk = tb ? b.stride(0) : 1;
  g.sbn = tb ? 1 : b.stride(0);
  g.M = (int)M;
  g.N = (int)N;
  g.Kred = (int)K;
  g.ldo = N;
  g.accumulate = accumulate && out.has_value() && out->defined();
  g.act = (int)act;
  g.amask = f32_mask(amask, a, "gemm_f32: amask");
  g.bmask = f32_mask(bmask, b, "gemm_f32: bmask");
  g.vec_a = g.sak == 1 && g.sam % 4 == 0 && K % 4 == 0 && al16(a) && mask_al16(amask);
  g.vec_b = g.sbn == 1 && g.sbk % 4 == 0 && N % 4 == 0 && al16(b) && mask_al16(bmask);
  g.dbias = f32_dbias(dbias, N);
  if (g.dbias != nullptr) {
    TORCH_CHECK(act == 0, "gemm_f32: dbias with an activation epilogue");
    g.ones_m = g.M++;  // the appended row of ones
  }
  f32_run(tdl::kF32Gemm, g, a.options());
  return c;
}

tdl::F32ConvGeom f32_geom(const at::Tensor& x_like, int64_t k, int64_t r, int64_t s, int64_t oh, int64_t ow, int64_t sh,
                          int64_t sw, int64_t pt, int64_t pl, int64_t dh, int64_t dw) {
  tdl::F32ConvGeom g{};
  g.n = (int)x_like.size(0);
  g.h = (int)x_like.size(1);
  g.w = (int)x_like.size(2);
  g.c = (int)x_like.size(3);
  g.k = (int)k;
  g.r = (int)r;
  g.s = (int)s;
  g.oh = (int)oh;
  g.ow = (int)ow;
  g.sh = (int)sh;
  g.sw = (int)sw;
  g.pt = (int)pt;
  g.pl = (int)pl;
  g.dh = (int)dh;
  g.dw = (int)dw;
  TORCH_CHECK(sh > 0 && sw > 0 && dh > 0 && dw > 0, "f32 conv: strides and dilations must be positive");
  return g;
}

// y[N][OH][OW][K] = conv(x NHWC, w HWIO) (+ bias); padding (pt, pl) top / left, the rest implied by OH / OW
at::Tensor conv_f32_fwd(at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias, int64_t oh, int64_t ow, int64_t sh,
                        int64_t sw, int64_t pt, int64_t pl, int64_t dh, int64_t dw, int64_t act) {
  f32_check(x, "conv_f32_fwd: x");
  f32_check(w, "conv_f32_fwd: w");
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4 && w.size(2) == x.size(3), "conv_f32_fwd: x NHWC, w [R][S][C][K]");
  const int64_t K = w.size(3);
  auto y = fresh({x.size(0), oh, ow, K}, x.options());
  tdl::F32GemmArgs g{};
  g.g = f32_geom(x, K, w.size(0), w.size(1), oh, ow, sh, sw, pt, pl, dh, dw);
  g.a = x.data_ptr<float>();
  g.b = w.data_ptr<float>();
  g.na = x.numel();
  g.nb = w.numel();
  g.out = y.data_ptr<float>();
  g.bias = f32_bias(bias, K);
  g.M = (int)(x.size(0) * oh * ow);
  g.N = (int)K;
  g.Kred = (int)(w.size(0) * w.size(1) * x.size(3));
  g.ldo = K;
  g.vec_a = x.size(3) % 4 == 0 && al16(x);
  g.vec_b = K % 4 == 0 && al16(w);
  g.act = (int)act;
  f32_run(tdl::kF32ConvFwd, g, x.options());
  return y;
}

// conv_f32_fwd followed by a 2x2 / stride-2 'valid' max pool, in one launch (the pool in the GEMM's
// epilogue, rows ordered by pool window): returns [y [N][OH][OW][K], pooled [N][OH/2][OW/2][K], argmax
// (uint8 window positions, the maxpool_fwd format, for maxpool_bwd)].  With odd OH / OW the last output
// row / column belongs to no window and is not computed (its y entries are left unset: their gradient
// is zero, and the backward only selects on them).
std::vector<at::Tensor> conv_f32_fwd_pool(at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias, int64_t oh,
                                          int64_t ow, int64_t sh, int64_t sw, int64_t pt, int64_t pl, int64_t dh,
                                          int64_t dw, int64_t act) {
  f32_check(x, "conv_f32_fwd_pool: x");
  f32_check(w, "conv_f32_fwd_pool: w");
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4 && w.size(2) == x.size(3), "conv_f32_fwd_pool: x NHWC, w [R][S][C][K]");
  TORCH_CHECK(oh >= 2 && ow >= 2, "conv_f32_fwd_pool: the output must hold at least one 2x2 window");
  const int64_t K = w.size(3), PH = oh / 2, PW = ow / 2;
  auto y = at::empty({x.size(0), oh, ow, K}, x.options());
  auto p = at::empty({x.size(0), PH, PW, K}, x.options());
  auto arg = at::empty({x.size(0), PH, PW, K}, x.options().dtype(at::kByte));
  tdl::F32GemmArgs g{};
  g.g = f32_geom(x, K, w.size(0), w.size(1), oh, ow, sh, sw, pt, pl, dh, dw);
  g.a = x.data_ptr<float>();
  g.b = w.data_ptr<float>();
  g.na = x.numel();
  g.nb = w.numel();
  g.out = y.data_ptr<float>();
  g.bias = f32_bias(bias, K);
  g.M = (int)(x.size(0) * PH * PW * 4);
  g.N = (int)K;
  g.Kred = (int)(w.size(0) * w.size(1) * x.size(3));
  g.ldo = K;
  g.vec_a = x.size(3) % 4 == 0 && al16(x);
  g.vec_b = K % 4 == 0 && al16(w);
  g.act = (int)act;
  g.pool = 1;
  g.pool_h = (int)PH;
  g.pool_w = (int)PW;
  g.plan_m = (int)(x.size(0) * oh * ow);  // the unfused conv's split: the same partial sums
  g.pout = p.data_ptr<float>();
  g.parg = arg.data_ptr<uint8_t>();
  f32_run(tdl::kF32ConvFwd, g, x.options());
  return {y, p, arg};
}

// dx[N][H][W][C] of a conv with dy [N][OH][OW][K] and wt = w as [R][S][K][C]
// pooled output gradient (pin_arg given: the backward of conv_f32_fwd_pool): dy = the pool's output gradient
// [N][PH][PW][K], dy_mask = the pooled maximum, pin_arg = its argmax, (out_h, out_w) = the conv's output size
static void f32_pin(tdl::F32GemmArgs& g, const at::Tensor& dy, const c10::optional<at::Tensor>& pin_arg,
                    const c10::optional<at::Tensor>& dy_mask, int64_t out_h, int64_t out_w, const char* what) {
  if (!pin_arg.has_value() || !pin_arg->defined()) return;
  TORCH_CHECK(pin_arg->is_cuda() && pin_arg->scalar_type() == at::kByte && pin_arg->is_contiguous() &&
                  pin_arg->sizes() == dy.sizes(), what, ": pin_arg must be a contiguous uint8 tensor shaped like dy");
  TORCH_CHECK(dy_mask.has_value() && dy_mask->defined(), what, ": pin_arg needs dy_mask (the pooled maximum)");
  TORCH_CHECK(out_h >= 2 * dy.size(1) && out_w >= 2 * dy.size(2) && out_h <= 2 * dy.size(1) + 1 &&
                  out_w <= 2 * dy.size(2) + 1, what, ": (out_h, out_w) must be the pooled conv's output size");
  g.pin_arg = pin_arg->data_ptr<uint8_t>();
  g.pool_h = (int)dy.size(1);
  g.pool_w = (int)dy.size(2);
}

at::Tensor conv_f32_dgrad(at::Tensor dy, at::Tensor wt, int64_t h, int64_t wd, int64_t sh, int64_t sw, int64_t pt,
                          int64_t pl, int64_t dh, int64_t dw, c10::optional<at::Tensor> dy_mask, bool w_hwio,
                          c10::optional<at::Tensor> pin_arg, int64_t out_h, int64_t out_w) {
  f32_check(dy, "conv_f32_dgrad: dy");
  f32_check(wt, "conv_f32_dgrad: wt");
  // wt: [R][S][K][C], or (w_hwio) the forward kernel [R][S][C][K] read transposed in the kernel
  TORCH_CHECK(dy.dim() == 4 && wt.dim() == 4 && wt.size(w_hwio ? 3 : 2) == dy.size(3),
              "conv_f32_dgrad: dy NHWC, wt [R][S][K][C] (or w [R][S][C][K] with w_hwio)");
  const int64_t C = wt.size(w_hwio ? 2 : 3), K = dy.size(3);
  auto dx = fresh({dy.size(0), h, wd, C}, dy.options());
  tdl::F32GemmArgs g{};
  const bool pin = pin_arg.has_value() && pin_arg->defined();
  g.g = f32_geom(dx, K, wt.size(0), wt.size(1), pin ? out_h : dy.size(1), pin ? out_w : dy.size(2), sh, sw, pt, pl,
                 dh, dw);
  f32_pin(g, dy, pin_arg, dy_mask, out_h, out_w, "conv_f32_dgrad");
  g.a = dy.data_ptr<float>();
  g.b = wt.data_ptr<float>();
  g.na = dy.numel();
  g.nb = wt.numel();
  g.out = dx.data_ptr<float>();
  g.M = (int)(dy.size(0) * h * wd);
  g.N = (int)C;
  g.Kred = (int)(wt.size(0) * wt.size(1) * K);
  g.ldo = C;
  g.amask = f32_mask(dy_mask, dy, "conv_f32_dgrad: dy_mask");
  g.vec_a = K % 4 == 0 && al16(dy) && mask_al16(dy_mask);
  g.vec_b = !w_hwio && C % 4 == 0 && al16(wt);
  g.b_hwio = w_hwio ? 1 : 0;
  f32_run(tdl::kF32ConvDgrad, g, dy.options());
  return dx;
}

// dW HWIO [R][S][C][K] of a conv with x NHWC and dy [N][OH][OW][K] (into / += out when given)
at::Tensor conv_f32_wgrad(at::Tensor x, at::Tensor dy, int64_t r, int64_t s, int64_t sh, int64_t sw, int64_t pt,
                          int64_t pl, int64_t dh, int64_t dw, c10::optional<at::Tensor> out, bool accumulate,
                          c10::optional<at::Tensor> dy_mask, c10::optional<at::Tensor> dbias,
                          c10::optional<at::Tensor> pin_arg, int64_t out_h, int64_t out_w) {
  f32_check(x, "conv_f32_wgrad: x");
  f32_check(dy, "conv_f32_wgrad: dy");
  TORCH_CHECK(x.dim() == 4 && dy.dim() == 4 && x.size(0) == dy.size(0), "conv_f32_wgrad: x, dy NHWC");
  const int64_t C = x.size(3), K = dy.size(3);
  auto dW = f32_out(out, {r, s, C, K}, x.options());
  tdl::F32GemmArgs g{};
  const bool pin = pin_arg.has_value() && pin_arg->defined();
  const int64_t oh = pin ? out_h : dy.size(1), ow = pin ? out_w : dy.size(2);
  g.g = f32_geom(x, K, r, s, oh, ow, sh, sw, pt, pl, dh, dw);
  f32_pin(g, dy, pin_arg, dy_mask, out_h, out_w, "conv_f32_wgrad");
  g.a = dy.data_ptr<float>();
  g.b = x.data_ptr<float>();
  g.na = dy.numel();
  g.nb = x.numel();
  g.out = dW.data_ptr<float>();
  g.M = (int)K;
  g.N = (int)(r * s * C);
  TORCH_CHECK(dy.size(0) * oh * ow < (int64_t)1 << 31, "conv_f32_wgrad: reduction too long");
  g.Kred = (int)(dy.size(0) * oh * ow);
  g.ldo = K;
  g.trans_out = 1;
  g.accumulate = accumulate && out.has_value() && out->defined();
  g.vec_b = C % 4 == 0 && al16(x);
  g.amask = f32_mask(dy_mask, dy, "conv_f32_wgrad: dy_mask");
  g.dbias = f32_dbias(dbias, K);
  if (g.dbias != nullptr) g.ones_n = g.N++;  // the appended column of ones: sum over pixels of dy
  f32_run(tdl::kF32ConvWgrad, g, x.options());
  return dW;
}

at::Tensor gap_fwd(at::Tensor x) {
  conv_check(x, "gap: x");
  TORCH_CHECK(x.dim() == 4 && x.size(3) % 8 == 0, "gap: NHWC with C % 8 == 0");
  auto y = fresh({x.size(0), x.size(3)}, x.options());
  tdl::gap_fwd_bf16(x.data_ptr(), y.data_ptr(), (int)x.size(0), (int)(x.size(1) * x.size(2)), (int)x.size(3),
                    cur_stream());
  return y;
}

at::Tensor gap_bwd(at::Tensor dy, int64_t h, int64_t w) {
  conv_check(dy, "gap: dy");
  TORCH_CHECK(dy.dim() == 2 && dy.size(1) % 8 == 0, "gap: dy [N][C], C % 8 == 0");
  auto dx = fresh({dy.size(0), h, w, dy.size(1)}, dy.options());
  tdl::gap_bwd_bf16(dy.data_ptr(), dx.data_ptr(), (int)dy.size(0), (int)(h * w), (int)dy.size(1), cur_stream());
  return dx;
}
// Sparse softmax cross-entropy (xent_fwd / xent_bwd / xent_head).  A label outside [0, K) is not an error:
// its row contributes no loss, its dz is the plain softmax (no one-hot term), and xent_head counts the row
// in `count` but never as correct.  (Parity of this case with TF is not pinned and not claimed.)
std::vector<at::Tensor> xent_fwd(at::Tensor z, at::Tensor labels) {
  TORCH_CHECK(z.is_cuda() && z.is_contiguous() && z.scalar_type() == at::kFloat && z.dim() == 2, "xent: f32 [N][K] logits");
  TORCH_CHECK(labels.is_cuda() && labels.is_contiguous() && labels.scalar_type() == at::kLong &&
                  labels.numel() == z.size(0), "xent: int64 [N] labels");
  auto loss = fresh({z.size(0)}, z.options());
  auto lse = fresh({z.size(0)}, z.options());
  tdl::softmax_xent_fwd(z.data_ptr<float>(), reinterpret_cast<const long long*>(labels.data_ptr<int64_t>()), (int)z.size(0), (int)z.size(1),
                        loss.data_ptr<float>(), lse.data_ptr<float>(), cur_stream());
  return {loss, lse};
}

double* f64_scalar(const c10::optional<at::Tensor>& t, const char* what) {
  if (!t.has_value() || !t->defined()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kDouble && t->numel() == 1, what, ": f64 GPU scalar expected");
  return t->data_ptr<double>();
}

// the generic engine's fused loss head: (loss [] = sum / gn, dz [N][K] = (softmax - onehot) / gn), metric
// accumulators advanced in place
std::vector<at::Tensor> xent_head(at::Tensor z, at::Tensor labels, double gn, c10::optional<at::Tensor> lt_total,
                                  c10::optional<at::Tensor> lt_count, c10::optional<at::Tensor> acc_total,
                                  c10::optional<at::Tensor> acc_count) {
  TORCH_CHECK(z.is_cuda() && z.is_contiguous() && z.scalar_type() == at::kFloat && z.dim() == 2, "xent_head: f32 [N][K] logits");
  TORCH_CHECK(labels.is_cuda() && labels.is_contiguous() && labels.scalar_type() == at::kLong &&
                  labels.numel() == z.size(0), "xent_head: int64 [N] labels");
  TORCH_CHECK(gn > 0, "xent_head: global batch must be positive");
  auto loss = at::empty({}, z.options());
  auto dz = fresh(z.sizes(), z.options());
  // one workgroup up to 64K logits (the reference CNN's 64 x 10), else per-row waves + a finishing sum
  at::Tensor ws;
  if (z.numel() > 65536) ws = at::empty({2 * z.size(0)}, z.options());
  tdl::xent_head(z.data_ptr<float>(), reinterpret_cast<const long long*>(labels.data_ptr<int64_t>()), (int)z.size(0),
                 (int)z.size(1), gn, loss.data_ptr<float>(), dz.data_ptr<float>(), f64_scalar(lt_total, "lt_total"),
                 f64_scalar(lt_count, "lt_count"), f64_scalar(acc_total, "acc_total"), f64_scalar(acc_count, "acc_count"),
                 ws.defined() ? ws.data_ptr<float>() : nullptr, cur_stream());
  return {loss, dz};
}

const float* f32_vec(const c10::optional<at::Tensor>& t, int64_t n, const char* what) {
  if (!t.has_value() || !t->defined()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->scalar_type() == at::kFloat && t->dim() == 1 && t->size(0) == n,
              what, ": f32 GPU vector of ", n, " elements expected");
  return t->data_ptr<float>();
}

// xent_head with sample weights sw [N], class weights cw [K], label smoothing eps, and sparse (int64 [N]) or
// dense (f32 [N][K]) targets (kernels/loss_head.h).  dz_out / rows_ws: optional preallocated dz and row
// workspace ([3N] f32, used above 64K logits); tests put guard words around them
std::vector<at::Tensor> xent_head_w(at::Tensor z, at::Tensor target, double gn, c10::optional<at::Tensor> sw,
                                    c10::optional<at::Tensor> cw, double eps, c10::optional<at::Tensor> lt_total,
                                    c10::optional<at::Tensor> lt_count, c10::optional<at::Tensor> acc_total,
                                    c10::optional<at::Tensor> acc_count, c10::optional<at::Tensor> dz_out,
                                    c10::optional<at::Tensor> rows_ws) {
  TORCH_CHECK(z.is_cuda() && z.is_contiguous() && z.scalar_type() == at::kFloat && z.dim() == 2 && z.size(1) >= 1,
              "xent_head_w: f32 [N][K >= 1] logits");
  TORCH_CHECK(target.is_cuda() && target.is_contiguous(), "xent_head_w: contiguous GPU target");
  const bool dense = target.scalar_type() == at::kFloat;
  if (dense) {
    TORCH_CHECK(target.sizes() == z.sizes(), "xent_head_w: dense f32 targets must have the logits' shape");
  } else {
    TORCH_CHECK(target.scalar_type() == at::kLong && target.dim() == 1 && target.size(0) == z.size(0),
                "xent_head_w: int64 [N] labels or f32 [N][K] targets");
  }
  TORCH_CHECK(gn > 0, "xent_head_w: global batch must be positive");
  TORCH_CHECK(eps >= 0.0 && eps <= 1.0, "xent_head_w: label smoothing must be in [0, 1]");
  const int64_t N = z.size(0), K = z.size(1);
  TORCH_CHECK(z.numel() < (int64_t(1) << 31), "xent_head_w: too many logits");
  const float* swp = f32_vec(sw, N, "xent_head_w sw");
  const float* cwp = f32_vec(cw, K, "xent_head_w cw");
  auto loss = at::empty({}, z.options());
  auto given = [](const c10::optional<at::Tensor>& t) { return t.has_value() && t->defined(); };
  auto dz = given(dz_out) ? *dz_out : fresh(z.sizes(), z.options());
  TORCH_CHECK(dz.is_cuda() && dz.is_contiguous() && dz.scalar_type() == at::kFloat && dz.numel() == z.numel(),
              "xent_head_w: dz_out must be f32 with the logits' element count");
  // the form switches where xent_head's does: one workgroup up to 64K logits, else rows + finish
  at::Tensor ws;
  if (z.numel() > 65536) {
    ws = given(rows_ws) ? *rows_ws : at::empty({3 * N}, z.options());
    TORCH_CHECK(ws.is_cuda() && ws.is_contiguous() && ws.scalar_type() == at::kFloat && ws.numel() >= 3 * N,
                "xent_head_w: rows_ws must be f32 with at least 3 N elements");
  }
  tdl::xent_head_w(z.data_ptr<float>(),
                   dense ? nullptr : reinterpret_cast<const long long*>(target.data_ptr<int64_t>()),
                   dense ? target.data_ptr<float>() : nullptr, swp, cwp, (int)N, (int)K, gn, (float)eps,
                   loss.data_ptr<float>(), dz.data_ptr<float>(), f64_scalar(lt_total, "lt_total"),
                   f64_scalar(lt_count, "lt_count"), f64_scalar(acc_total, "acc_total"),
                   f64_scalar(acc_count, "acc_count"), ws.defined() ? ws.data_ptr<float>() : nullptr, cur_stream());
  return {loss, dz};
}

at::Tensor xent_bwd(at::Tensor z, at::Tensor labels, at::Tensor g) {
  TORCH_CHECK(z.is_cuda() && z.is_contiguous() && z.scalar_type() == at::kFloat && z.dim() == 2, "xent: f32 [N][K] logits");
  TORCH_CHECK(labels.is_cuda() && labels.is_contiguous() && labels.scalar_type() == at::kLong &&
                  labels.numel() == z.size(0), "xent: int64 [N] GPU labels");
  TORCH_CHECK(g.is_cuda() && g.is_contiguous() && g.scalar_type() == at::kFloat && g.numel() == z.size(0), "xent: g");
  auto dz = fresh(z.sizes(), z.options());
  tdl::softmax_xent_bwd(z.data_ptr<float>(), reinterpret_cast<const long long*>(labels.data_ptr<int64_t>()), (int)z.size(0), (int)z.size(1),
                        g.data_ptr<float>(), dz.data_ptr<float>(), cur_stream());
  return dz;
}

// ---- group normalisation (kernels/groupnorm.h) over a channels-last [N, ..., C] tensor
struct GnShape {
  int64_t N, P, C;
  tdl::GnDType dt;
  tdl::GnPlan plan;
};
GnShape gn_check(const at::Tensor& x, int64_t G, const char* what) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() >= 2, what, ": contiguous [N, ..., C] GPU tensor expected");
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16, what, ": float32 or bfloat16 expected");
  TORCH_CHECK(x.numel() > 0, what, ": empty tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, what, ": 16-byte aligned data expected");
  GnShape sh;
  sh.N = x.size(0);
  sh.C = x.size(-1);
  sh.P = x.numel() / (sh.N * sh.C);
  TORCH_CHECK(G >= 1 && sh.C % G == 0, what, ": groups must divide the channel count");
  TORCH_CHECK(sh.C <= 16384 && sh.N * sh.C <= (int64_t(1) << 24), what, ": C <= 16384 and N * C <= 2^24 expected");
  sh.dt = x.scalar_type() == at::kFloat ? tdl::GnDType::kF32 : tdl::GnDType::kBF16;
  sh.plan = tdl::gn_plan(sh.P, (int)sh.C, sh.dt);
  // 256 threads each: a grid of 2^32 threads and more does not launch
  TORCH_CHECK(sh.N * sh.plan.colblocks * sh.plan.chunks < (int64_t(1) << 24), what, ": 2^24 workgroups or more");
  return sh;
}
const float* gn_param(const c10::optional<at::Tensor>& t, int64_t C, const char* what) {
  if (!t.has_value() || !t->defined()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->numel() == C, what,
              ": f32 [C] GPU parameters expected");
  return t->data_ptr<float>();
}
at::Tensor gn_ws(const c10::optional<std::vector<at::Tensor>>& ws, size_t i, at::IntArrayRef shape,
                 const at::TensorOptions& o) {
  if (!ws.has_value()) return fresh(shape, o);
  TORCH_CHECK(i < ws->size(), "group_norm: workspace list too short");
  const at::Tensor& t = (*ws)[i];
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == o.dtype().toScalarType() &&
                  t.numel() == c10::multiply_integers(shape),
              "group_norm: workspace tensor ", i, " has the wrong dtype or size");
  return t;
}

// (y, stats f64 [N][G][2] = mean, 1/sqrt(var + eps), part, coef).  phases / ws: run a subset of the three
// launches on the buffers (y, stats, part, coef) of an earlier call (timing each launch alone)
std::vector<at::Tensor> gn_forward(at::Tensor x, int64_t G, c10::optional<at::Tensor> gamma,
                                   c10::optional<at::Tensor> beta, double eps, int64_t phases,
                                   c10::optional<std::vector<at::Tensor>> ws) {
  const GnShape sh = gn_check(x, G, "group_norm");
  auto d = x.options().dtype(at::kDouble);
  auto y = gn_ws(ws, 0, x.sizes(), x.options());
  auto stats = gn_ws(ws, 1, {sh.N, G, 2}, d);
  auto part = gn_ws(ws, 2, {sh.N, sh.plan.chunks, 2, sh.C}, d);
  auto coef = gn_ws(ws, 3, {2, sh.N, sh.C}, x.options().dtype(at::kFloat));
  tdl::gn_forward(x.data_ptr(), y.data_ptr(), sh.dt, sh.N, sh.P, (int)sh.C, (int)G, gn_param(gamma, sh.C, "group_norm"),
                  gn_param(beta, sh.C, "group_norm"), eps, part.data_ptr<double>(), stats.data_ptr<double>(),
                  coef.data_ptr<float>(), cur_stream(), (int)phases);
  return {y, stats, part, coef};
}

// (dx, dgamma, dbeta, part, coef).  dgamma_out / dbeta_out: f32 [C] tensors the parameter gradients are
// ADDED into (a trainer's slab views); the returned dgamma / dbeta are then those tensors
std::vector<at::Tensor> gn_backward(at::Tensor dy, at::Tensor x, int64_t G, c10::optional<at::Tensor> gamma,
                                    at::Tensor stats, c10::optional<at::Tensor> dgamma_out,
                                    c10::optional<at::Tensor> dbeta_out, int64_t phases,
                                    c10::optional<std::vector<at::Tensor>> ws) {
  const GnShape sh = gn_check(x, G, "group_norm backward");
  gn_check(dy, G, "group_norm backward");
  TORCH_CHECK(dy.scalar_type() == x.scalar_type() && dy.sizes() == x.sizes(), "group_norm backward: dy/x mismatch");
  TORCH_CHECK(stats.is_cuda() && stats.is_contiguous() && stats.scalar_type() == at::kDouble &&
                  stats.numel() == sh.N * G * 2,
              "group_norm backward: stats must be f64 [N][G][2]");
  auto f = x.options().dtype(at::kFloat);
  auto dx = gn_ws(ws, 0, x.sizes(), x.options());
  auto part = gn_ws(ws, 1, {sh.N, sh.plan.chunks, 2, sh.C}, x.options().dtype(at::kDouble));
  auto coef = gn_ws(ws, 2, {3, sh.N, sh.C}, f);
  auto check_out = [&](const c10::optional<at::Tensor>& t) {
    if (!t.has_value() || !t->defined()) return (float*)nullptr;
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->scalar_type() == at::kFloat && t->numel() == sh.C,
                "group_norm backward: gradient outputs must be contiguous f32 [C]");
    return t->data_ptr<float>();
  };
  float* pg = check_out(dgamma_out);
  float* pb = check_out(dbeta_out);
  auto out = fresh({2, sh.C}, f);
  float* o = out.data_ptr<float>();
  const int acc = (pg ? 1 : 0) | (pb ? 2 : 0);
  tdl::gn_backward(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), sh.dt, sh.N, sh.P, (int)sh.C, (int)G,
                   gn_param(gamma, sh.C, "group_norm backward"), stats.data_ptr<double>(), part.data_ptr<double>(),
                   coef.data_ptr<float>(), pg ? pg : o, pb ? pb : o + sh.C, acc, cur_stream(), (int)phases);
  return {dx, pg ? *dgamma_out : out[0], pb ? *dbeta_out : out[1], part, coef};
}
}  // namespace

void register_ops(pybind11::module& m) {
  m.def("gn_forward", &gn_forward, "channels-last group normalisation forward: (y, stats, part, coef)",
        pybind11::arg("x"), pybind11::arg("groups"), pybind11::arg("gamma"), pybind11::arg("beta"),
        pybind11::arg("eps"), pybind11::arg("phases") = 7, pybind11::arg("ws") = pybind11::none());
  m.def("gn_backward", &gn_backward, "channels-last group normalisation backward: (dx, dgamma, dbeta, part, coef)",
        pybind11::arg("dy"), pybind11::arg("x"), pybind11::arg("groups"), pybind11::arg("gamma"),
        pybind11::arg("stats"), pybind11::arg("dgamma_out") = pybind11::none(),
        pybind11::arg("dbeta_out") = pybind11::none(), pybind11::arg("phases") = 7,
        pybind11::arg("ws") = pybind11::none());
  m.def("gn_plan", [](int64_t P, int64_t C, bool bf16) {
    const tdl::GnPlan p = tdl::gn_plan(P, (int)C, bf16 ? tdl::GnDType::kBF16 : tdl::GnDType::kF32);
    return std::vector<int64_t>{p.vec, p.cols, p.tc, p.rl, p.colblocks, p.rows_wg, p.chunks};
  }, "group normalisation plan for (P, C, dtype): vec, cols, tc, rl, colblocks, rows_wg, chunks");
  m.def("xent_fwd", &xent_fwd, "sparse softmax cross-entropy forward: (loss, logsumexp)");
  m.def("xent_bwd", &xent_bwd, "sparse softmax cross-entropy backward: (softmax - onehot) * g");
  m.def("xent_head", &xent_head, "fused loss head: mean-reduced sparse softmax cross-entropy, its dlogits and "
        "the loss / accuracy metric accumulators", pybind11::arg("z"), pybind11::arg("labels"), pybind11::arg("gn"),
        pybind11::arg("lt_total") = pybind11::none(), pybind11::arg("lt_count") = pybind11::none(),
        pybind11::arg("acc_total") = pybind11::none(), pybind11::arg("acc_count") = pybind11::none());
  m.def("xent_head_w", &xent_head_w, "fused loss head with sample weights, class weights, label smoothing and "
        "sparse or dense targets", pybind11::arg("z"), pybind11::arg("target"), pybind11::arg("gn"),
        pybind11::arg("sw") = pybind11::none(), pybind11::arg("cw") = pybind11::none(), pybind11::arg("eps") = 0.0,
        pybind11::arg("lt_total") = pybind11::none(), pybind11::arg("lt_count") = pybind11::none(),
        pybind11::arg("acc_total") = pybind11::none(), pybind11::arg("acc_count") = pybind11::none(),
        pybind11::arg("dz_out") = pybind11::none(), pybind11::arg("rows_ws") = pybind11::none());
  m.def("gemm_bf16", &gemm_bf16, "bf16 MFMA GEMM with either storage per operand (Dense fwd / dgrad / wgrad)",
        pybind11::arg("a"), pybind11::arg("ta"), pybind11::arg("b"), pybind11::arg("tb"),
        pybind11::arg("bias") = pybind11::none(), pybind11::arg("out") = pybind11::none(),
        pybind11::arg("accumulate") = false, pybind11::arg("alpha") = 1.0);
  m.def("gemm_f32", &gemm_f32, "f32 MFMA GEMM (v_mfma_f32_16x16x4_f32) with either storage per operand; "
        "ReLU epilogue, ReLU-masked operands, bias gradient as an appended row of ones",
        pybind11::arg("a"), pybind11::arg("ta"), pybind11::arg("b"), pybind11::arg("tb"),
        pybind11::arg("bias") = pybind11::none(), pybind11::arg("out") = pybind11::none(),
        pybind11::arg("accumulate") = false, pybind11::arg("act") = 0, pybind11::arg("amask") = pybind11::none(),
        pybind11::arg("bmask") = pybind11::none(), pybind11::arg("dbias") = pybind11::none());
  m.def("conv_f32_fwd_pool", &conv_f32_fwd_pool,
        "conv_f32_fwd + 2x2/2 'valid' max pool in the epilogue: [y, pooled, argmax]", pybind11::arg("x"),
        pybind11::arg("w"), pybind11::arg("bias"), pybind11::arg("oh"), pybind11::arg("ow"), pybind11::arg("sh"),
        pybind11::arg("sw"), pybind11::arg("pt"), pybind11::arg("pl"), pybind11::arg("dh") = 1,
        pybind11::arg("dw") = 1, pybind11::arg("act") = 0);
  m.def("conv_f32_fwd", &conv_f32_fwd, "NHWC f32 implicit-GEMM convolution forward, any geometry (act 1: + ReLU)",
        pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("bias"), pybind11::arg("oh"), pybind11::arg("ow"),
        pybind11::arg("sh"), pybind11::arg("sw"), pybind11::arg("pt"), pybind11::arg("pl"), pybind11::arg("dh") = 1,
        pybind11::arg("dw") = 1, pybind11::arg("act") = 0);
  m.def("conv_f32_dgrad", &conv_f32_dgrad, "NHWC f32 convolution input gradient, any geometry (wt: [R][S][K][C]); "
        "dy_mask: dy * (mask > 0)",
        pybind11::arg("dy"), pybind11::arg("wt"), pybind11::arg("h"), pybind11::arg("w"), pybind11::arg("sh"),
        pybind11::arg("sw"), pybind11::arg("pt"), pybind11::arg("pl"), pybind11::arg("dh") = 1, pybind11::arg("dw") = 1,
        pybind11::arg("dy_mask") = pybind11::none(), pybind11::arg("w_hwio") = false,
        pybind11::arg("pin_arg") = pybind11::none(), pybind11::arg("out_h") = 0, pybind11::arg("out_w") = 0);
  m.def("conv_f32_wgrad", &conv_f32_wgrad, "NHWC f32 convolution weight gradient (HWIO), deterministic split-K; "
        "dy_mask: dy * (mask > 0); dbias: the bias gradient from an appended column of ones",
        pybind11::arg("x"), pybind11::arg("dy"), pybind11::arg("r"), pybind11::arg("s"), pybind11::arg("sh"),
        pybind11::arg("sw"), pybind11::arg("pt"), pybind11::arg("pl"), pybind11::arg("dh") = 1, pybind11::arg("dw") = 1,
        pybind11::arg("out") = pybind11::none(), pybind11::arg("accumulate") = false,
        pybind11::arg("dy_mask") = pybind11::none(), pybind11::arg("dbias") = pybind11::none(),
        pybind11::arg("pin_arg") = pybind11::none(), pybind11::arg("out_h") = 0, pybind11::arg("out_w") = 0);
  m.def("gap_fwd", &gap_fwd, "NHWC bf16 global average pooling");
  m.def("gap_bwd", &gap_bwd, "NHWC bf16 global average pooling backward");
  m.def("slab_cast_bf16", &slab_cast_bf16, "f32 -> bf16 copy of a whole weight slab (one launch)");
  m.def("bn_set_tuning", &tdl::bn_set_tuning,
        "BN kernel sweep hooks (max_parts, elem_blocks: grid cap of the grid-stride elementwise kernels, elem_unroll, "
        "blk_blocks: grid cap of the blocked elementwise kernels; 0 = keep)",
        pybind11::arg("max_parts"), pybind11::arg("elem_blocks"), pybind11::arg("elem_unroll"),
        pybind11::arg("blk_blocks") = 0);
  m.def("bn_get_tuning", [] {
    int v[4];
    tdl::bn_get_tuning(v);
    return std::make_tuple(v[0], v[1], v[2], v[3]);
  }, "(max_parts, elem_blocks, elem_unroll, blk_blocks) as bn_set_tuning set them");
  m.def("bn_set_elementwise", &tdl::bn_set_elementwise,
        "BN elementwise kernel family A/B hook (kind 0 grid-stride / 1 blocked, vectors per thread 2/4/8)");
  m.def("slab_transpose_bf16", &slab_transpose_bf16, "HWIO f32 conv kernels -> OHWI bf16, all in one launch");
  m.def("conv_dgrad_bn", &conv_dgrad_bn, "stride-1 conv input gradient + fused BN->Add->ReLU backward (dz, part[, part2])",
        pybind11::arg("dy"), pybind11::arg("w"), pybind11::arg("h"), pybind11::arg("wd"), pybind11::arg("pt"),
        pybind11::arg("pl"), pybind11::arg("residual"), pybind11::arg("bn_y"), pybind11::arg("bn_x"),
        pybind11::arg("bn_x2") = pybind11::none(), pybind11::arg("bn_stats") = pybind11::none());
  m.def("conv_dgrad_s2_bn", &conv_dgrad_s2_bn,
        "1x1 stride-2 conv input gradient + fused BN->Add->ReLU backward (dz, part[, part2])", pybind11::arg("dy"),
        pybind11::arg("w"), pybind11::arg("h"), pybind11::arg("wd"), pybind11::arg("residual"), pybind11::arg("bn_y"),
        pybind11::arg("bn_x"), pybind11::arg("bn_x2") = pybind11::none(), pybind11::arg("bn_stats") = pybind11::none());
  m.def("conv_dgrad_s2", &conv_dgrad_s2, "NHWC bf16 1x1 stride-2 convolution input gradient (MFMA)",
        pybind11::arg("dy"), pybind11::arg("w"), pybind11::arg("h"), pybind11::arg("wd"),
        pybind11::arg("residual") = pybind11::none());
  m.def("conv_wgrad", &conv_wgrad, "NHWC bf16 convolution weight gradient (MFMA, transposed LDS reads, split-K)",
        pybind11::arg("x"), pybind11::arg("dy"), pybind11::arg("kh"), pybind11::arg("kw"), pybind11::arg("sh"),
        pybind11::arg("sw"), pybind11::arg("pt"), pybind11::arg("pl"), pybind11::arg("out") = pybind11::none(),
        pybind11::arg("accumulate") = false, pybind11::arg("plan") = std::vector<int64_t>{},
        pybind11::arg("in_bn") = pybind11::none());
  m.def("conv_wgrad_plans", &conv_wgrad_plans, "weight-gradient candidate plans, best first: [[wmw, wnw, chunk, nsplit, kind]]",
        pybind11::arg("x_shape"), pybind11::arg("dy_shape"), pybind11::arg("kh"), pybind11::arg("kw"),
        pybind11::arg("sh"), pybind11::arg("sw"), pybind11::arg("pt"), pybind11::arg("pl"), pybind11::arg("max_plans"),
        pybind11::arg("in_bn") = false);
  m.def("conv_selected", &conv_selected,
        "(kernel name, row tile) a conv launch of this geometry takes under the current hooks; no GPU needed",
        pybind11::arg("direction"), pybind11::arg("x_shape"), pybind11::arg("w_shape"), pybind11::arg("oh"),
        pybind11::arg("ow"), pybind11::arg("sh") = 1, pybind11::arg("sw") = 1, pybind11::arg("pt") = 0,
        pybind11::arg("pl") = 0, pybind11::arg("flags") = std::vector<std::string>{});
  m.def("conv_kernel_names", &tdl::conv_kernel_names, "every kernel name conv_selected can return");
  m.def("conv_force_tile", &tdl::conv_force_tile, "conv tile sweep hook (0 = heuristic)");
  m.def("conv_force_impl", &tdl::conv_force_impl,
        "conv main loop A/B hook: 1 v1 register staged, 2 default selection, 3 LDS-DMA ring, 4/5 dma1 at 4/3 waves "
        "per SIMD on 16x16x32 MFMAs, 6 dma1 on 32x32x16 MFMAs everywhere");
  m.def("f32_reduce16", &tdl::f32_reduce16,
        "f32 split-K reduce A/B hook: 16 outputs per wave over many slices (True, default) or one output per wave; returns the previous setting");
  m.def("f32_buf", &tdl::f32_buf,
        "f32 operand loader A/B hook: buffer resources where the operands fit (True, default) or 64-bit addresses; returns the previous setting");
  m.def("f32_reduce_narrow", &tdl::f32_reduce_narrow,
        "f32 few-slice reduce A/B hook: only the loads 4 / 8 slices need (True, default) or always 16; returns the previous setting");
  m.def("f32_pool_hoist", &tdl::f32_pool_hoist,
        "f32 pooled reduce A/B hook: a window's partial sums loaded before any store (True, default) or row by row; returns the previous setting");
  m.def("f32_last_selected", [] {
    return std::make_tuple(g_f32_last.main_name(), std::string(g_f32_last.reduce_name()), g_f32_last.splits,
                           g_f32_last.kchunk);
  }, "(main kernel, reduce kernel, splits, kchunk) of the most recent f32 GEMM / conv launch of this process");
  m.def("f32_kernel_names", &tdl::f32_kernel_names, "every main and reduce kernel name f32_last_selected can return");
  m.def("f32_plan", &f32_plan, "(splits, kchunk, unfused_splits) of the f32 split plan; no GPU needed",
        pybind11::arg("M"), pybind11::arg("N"), pybind11::arg("Kred"), pybind11::arg("pool") = false,
        pybind11::arg("plan_m") = 0);
  m.def("conv_force_halo", &tdl::conv_force_halo, "halo (input-reuse) main loop for stride-1 multi-tap convs: 1 on, 0 off");
  m.def("conv_force_mfma", &tdl::conv_force_mfma, "dma1 MFMA form: 32 (32x32x16, default) or 16 (16x16x32)");
  m.def("conv_wgrad3x3_set_rows", &tdl::conv_wgrad3x3_set_rows, "3x3 row-kernel wgrad: output rows per slice (0 = auto)");
  m.def("conv_wgrad_force_single", &tdl::conv_wgrad_force_single,
        "weight-gradient A/B hook: single LDS stage at 3 waves/SIMD (True) or double-buffered (False, default)");
  m.attr("AUGMENT_WG_ELEMS") = (int64_t)tdl::kAugmentWgElems;  // work items (16-B vectors / elements) per workgroup and trip
  m.attr("AUGMENT_MAX_GRID") = (int64_t)tdl::kAugmentMaxGrid;  // grid cap of the augmentation kernels
  m.attr("AUGMENT_FWD_MAX_GRID") = (int64_t)tdl::kAugmentFwdMaxGrid;  // ... of the forward (it arrives at the counter)
  m.def("augment_force_max_grid", &tdl::augment_force_max_grid,
        "augment test hook: grid cap (0 = AUGMENT_FWD_MAX_GRID / AUGMENT_MAX_GRID)");
  m.def("augment_fwd", &augment_fwd,
        "seeded flip / crop / translation forward: (y, ticket); advances state = [calls, arrivals]", py::arg("x"),
        py::arg("state"), py::arg("k0"), py::arg("k1"), py::arg("flip_h"), py::arg("flip_w"), py::arg("off_h_lo"),
        py::arg("off_h_count"), py::arg("off_w_lo"), py::arg("off_w_count"), py::arg("out_h"), py::arg("out_w"),
        py::arg("fill_mode") = 0, py::arg("fill_value") = 0.0);
  m.def("augment_bwd", &augment_bwd,
        "seeded flip / crop / translation backward: dx [N, H, W, C] from dy and the forward's ticket (draws recomputed)",
        py::arg("dy"), py::arg("ticket"), py::arg("k0"), py::arg("k1"), py::arg("flip_h"), py::arg("flip_w"),
        py::arg("off_h_lo"), py::arg("off_h_count"), py::arg("off_w_lo"), py::arg("off_w_count"), py::arg("out_h"),
        py::arg("out_w"), py::arg("fill_mode"), py::arg("fill_value"), py::arg("H"), py::arg("W"));
  m.attr("DROPOUT_WG_ELEMS") = (int64_t)tdl::kDropoutWgElems;  // elements per workgroup and grid-stride trip
  m.attr("DROPOUT_MAX_GRID") = (int64_t)tdl::kDropoutMaxGrid;  // grid cap of the dropout kernels
  m.attr("DROPOUT_SMALL_N") = (int64_t)tdl::kDropoutSmallN;    // up to this many elements: ...
  m.attr("DROPOUT_SMALL_WG_ELEMS") = (int64_t)tdl::kDropoutSmallWgElems;  // ... this many per workgroup and trip
  m.def("dropout_force_max_grid", &tdl::dropout_force_max_grid, "dropout test hook: grid cap (0 = DROPOUT_MAX_GRID)");
  m.def("dropout_fwd", &dropout_fwd, "seeded dropout forward: (y, ticket); advances state = [calls, arrivals]",
        pybind11::arg("x"), pybind11::arg("state"), pybind11::arg("k0"), pybind11::arg("k1"), pybind11::arg("T"),
        pybind11::arg("scale"), pybind11::arg("noise_strides") = pybind11::none(), pybind11::arg("elem_offset") = 0);
  m.def("dropout_bwd", &dropout_bwd, "seeded dropout backward: dx from dy and the forward's ticket (mask recomputed)",
        pybind11::arg("dy"), pybind11::arg("ticket"), pybind11::arg("k0"), pybind11::arg("k1"), pybind11::arg("T"),
        pybind11::arg("scale"), pybind11::arg("noise_strides") = pybind11::none(), pybind11::arg("elem_offset") = 0);
  m.def("maxpool_force_generic", &tdl::maxpool_force_generic,
        "max-pool A/B hook: generic window loops (True, default) or the unrolled 3x3 stride-2 kernels (False)");
  m.def("maxpool_w2", &tdl::maxpool_w2,
        "max-pool backward A/B hook: 2x2 stride-2 unpadded windows in scatter form (True, default) or the gather form");
  m.def("conv_force_depth", &tdl::conv_force_depth, "conv main-loop A/B hook: 0 single stage, 1/2 prefetch depth, 3 depth 2 without the short-reduction single-stage variant");
  m.def("stem_fwd", &stem_fwd, "small-channel stride-2 conv (ResNet stem): (y, packed x[, BN part])",
        pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("pt"), pybind11::arg("pb"), pybind11::arg("pl"),
        pybind11::arg("pr"), pybind11::arg("sh"), pybind11::arg("sw"), pybind11::arg("stats") = false);
  m.def("stem_wgrad", &stem_wgrad, "stem conv weight gradient from the packed image", pybind11::arg("xp"),
        pybind11::arg("dy"), pybind11::arg("kh"), pybind11::arg("kw"), pybind11::arg("c"), pybind11::arg("sh"),
        pybind11::arg("out") = pybind11::none(), pybind11::arg("accumulate") = false);
  m.def("conv_fwd", &conv_fwd, "NHWC bf16 implicit-GEMM convolution forward (MFMA); in_bn: over relu(bn(x))",
        pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("oh"), pybind11::arg("ow"), pybind11::arg("sh"),
        pybind11::arg("sw"), pybind11::arg("pt"), pybind11::arg("pl"), pybind11::arg("in_bn") = pybind11::none());
  m.def("conv_fwd_stats", &conv_fwd_stats, "conv forward + batch-norm partial channel sums of its output",
        pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("oh"), pybind11::arg("ow"), pybind11::arg("sh"),
        pybind11::arg("sw"), pybind11::arg("pt"), pybind11::arg("pl"), pybind11::arg("in_bn") = pybind11::none());
  m.def("conv_dgrad", &conv_dgrad, "NHWC bf16 implicit-GEMM stride-1 convolution input gradient (MFMA)",
        pybind11::arg("dy"), pybind11::arg("w"), pybind11::arg("h"), pybind11::arg("wd"), pybind11::arg("pt"),
        pybind11::arg("pl"), pybind11::arg("residual") = pybind11::none());
  m.def("gather_xy", &gather_xy, "a batch of (feature row, label) pairs of a device-resident dataset, one launch");
  m.def("gather_xyw", &gather_xyw, "a batch of (feature row, label, f32 weight) triples of a device-resident "
        "dataset, one launch", pybind11::arg("X"), pybind11::arg("Y"), pybind11::arg("W"), pybind11::arg("idx"),
        pybind11::arg("out_x") = pybind11::none(), pybind11::arg("out_y") = pybind11::none(),
        pybind11::arg("out_w") = pybind11::none());
  m.def("bn_forward_train", &bn_forward_train, "NHWC batch-norm training forward (+relu)", pybind11::arg("x"),
        pybind11::arg("gamma"), pybind11::arg("beta"), pybind11::arg("moving_mean"), pybind11::arg("moving_var"),
        pybind11::arg("momentum"), pybind11::arg("eps"), pybind11::arg("relu") = false,
        pybind11::arg("residual") = pybind11::none(), pybind11::arg("mean_off") = pybind11::none(),
        pybind11::arg("part") = pybind11::none());
  m.def("maxpool_fwd", &maxpool_fwd, "NHWC max pool forward (+argmax)", pybind11::arg("x"), pybind11::arg("kh"),
        pybind11::arg("kw"), pybind11::arg("sh"), pybind11::arg("sw"), pybind11::arg("pt"), pybind11::arg("pl"),
        pybind11::arg("OH"), pybind11::arg("OW"), pybind11::arg("pad_zero"), pybind11::arg("bn_stats") = pybind11::none());
  m.def("maxpool_bwd_bn", &maxpool_bwd_bn, "NHWC max pool backward fused with the BN -> ReLU group's mask and sums");
  m.def("bn_stats_train", &bn_stats_train, "NHWC batch-norm training statistics only ([4][C])", pybind11::arg("x"),
        pybind11::arg("gamma"), pybind11::arg("beta"), pybind11::arg("moving_mean"), pybind11::arg("moving_var"),
        pybind11::arg("momentum"), pybind11::arg("eps"), pybind11::arg("mean_off") = pybind11::none(),
        pybind11::arg("part") = pybind11::none());
  m.def("maxpool_bwd", &maxpool_bwd, "NHWC max pool backward (gather form)");
  m.def("bn_backward", &bn_backward, "NHWC batch-norm training backward", pybind11::arg("dy"), pybind11::arg("x"),
        pybind11::arg("y"), pybind11::arg("gamma"), pybind11::arg("stats"), pybind11::arg("mode"),
        pybind11::arg("dgamma_out") = pybind11::none(), pybind11::arg("dbeta_out") = pybind11::none(),
        pybind11::arg("part") = pybind11::none());
  m.def("bn_sync_xbuf_numel", [](int64_t C, int64_t R) { return tdl::bn_sync_xbuf_numel((int)C, (int)R); },
        "elements of the exchange buffer of a synchronized batch norm over C channels and R replicas");
  m.def("bn_sync_forward_pack", &bn_sync_forward_pack, "synchronized batch norm: local sums -> exchange buffer",
        pybind11::arg("x"), pybind11::arg("rank"), pybind11::arg("R"), pybind11::arg("part") = pybind11::none(),
        pybind11::arg("numel") = 0);
  m.def("bn_sync_forward_finalize", &bn_sync_forward_finalize,
        "synchronized batch norm: all-reduced exchange buffer -> statistics (+ apply)", pybind11::arg("x"),
        pybind11::arg("xbuf"), pybind11::arg("R"), pybind11::arg("gamma"), pybind11::arg("beta"),
        pybind11::arg("moving_mean"), pybind11::arg("moving_var"), pybind11::arg("momentum"), pybind11::arg("eps"),
        pybind11::arg("relu") = false, pybind11::arg("residual") = pybind11::none(),
        pybind11::arg("mean_off") = pybind11::none(), pybind11::arg("apply") = true);
  m.def("bn_sync_backward_pack", &bn_sync_backward_pack,
        "synchronized batch norm backward: local sums -> exchange buffer, local dgamma / dbeta", pybind11::arg("dy"),
        pybind11::arg("x"), pybind11::arg("y"), pybind11::arg("stats"), pybind11::arg("mode"), pybind11::arg("rank"),
        pybind11::arg("R"), pybind11::arg("dgamma_out") = pybind11::none(),
        pybind11::arg("dbeta_out") = pybind11::none(), pybind11::arg("part") = pybind11::none(),
        pybind11::arg("numel") = 0);
  m.def("bn_sync_backward_finalize", &bn_sync_backward_finalize,
        "synchronized batch norm backward: all-reduced exchange buffer -> dx", pybind11::arg("dz"), pybind11::arg("x"),
        pybind11::arg("xbuf"), pybind11::arg("R"), pybind11::arg("gamma"), pybind11::arg("stats"),
        pybind11::arg("mask") = false);
}
