// Python bindings of the HIP kernel library (module `tensorflow_distributed_learning_amd._C`).
//
// Kernels launch on the caller's current HIP stream, so every entry point here is capturable
// into a hipGraph by torch.cuda.graph (the engine captures whole train steps).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <cmath>
#include <vector>

#include "kernels/accum.h"
#include "kernels/ema.h"
#include "kernels/mnist_cnn.h"
#include "kernels/ops.h"
#include "kernels/optim.h"
#include "xgmi_channel.h"

namespace {

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check_cuda_f32(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32");
}

// an optimizer kernel's slab operand: read and written with 16-byte vector accesses
void check_slab_f32(const at::Tensor& t, const char* name) {
  check_cuda_f32(t, name);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}

// Owns the scratch buffers and the argument block of one replica's fused MNIST step.
class MnistStep {
 public:
  MnistStep(at::Tensor X, at::Tensor Y, at::Tensor idx_buf, at::Tensor W, at::Tensor G,
            std::vector<int64_t> offsets, int64_t b, double scale, at::Tensor lr, at::Tensor metrics)
      : X_(X), Y_(Y), idx_(idx_buf), W_(W), G_(G), lr_(lr), metrics_(metrics) {
    check_cuda_f32(X, "X");
    check_cuda_f32(W, "W");
    check_cuda_f32(G, "G");
    check_cuda_f32(lr, "lr");
    check_cuda_f32(metrics, "metrics");
    TORCH_CHECK(Y.is_cuda() && Y.scalar_type() == at::kInt, "Y must be int32 on GPU");
    TORCH_CHECK(idx_buf.is_cuda() && idx_buf.scalar_type() == at::kInt, "idx must be int32 on GPU");
    TORCH_CHECK(X.numel() % 784 == 0, "X must be [N,28,28,1]");
    TORCH_CHECK(offsets.size() == 8, "8 variable offsets expected");
    TORCH_CHECK(b >= 1 && b <= 256, "fused MNIST step supports 1 <= per-replica batch <= 256");
    TORCH_CHECK(W.numel() == G.numel(), "slab size mismatch");
    for (auto o : offsets) TORCH_CHECK(o % 4 == 0 && o >= 0 && o < W.numel(), "offsets must be 16B aligned");
    auto f = W.options();
    auto u8 = f.dtype(at::kByte);
    P1_ = at::empty({b * 169 * 32}, f);
    A1_ = at::empty({b * 169 * 32}, u8);
    P2_ = at::empty({b * 1600}, f);
    A2_ = at::empty({b * 1600}, u8);
    H_ = at::empty({b * 128}, f);
    dH_ = at::empty({b * 128}, f);
    dL_ = at::zeros({b * tdl::kDLStride}, f);
    cnt_ = at::zeros({b}, f.dtype(at::kInt));
    dHt_ = at::zeros({b * 128}, f.dtype(at::kLong));  // tag 0 never matches (tags start at 1)
    ep_ = at::zeros({1}, f.dtype(at::kInt));
    part3t_ = at::zeros({(int64_t)tdl::kDense1Chunks * b * 128}, f.dtype(at::kLong));
    dP2_ = at::empty({b * 1600}, f);
    part2_ = at::zeros({b * std::max(tdl::kMnistPart2Rows * 64, tdl::kP2QuadFloats)}, f);
    part1_ = at::zeros({(int64_t)tdl::mnist_part1_rows((int)b, true) * tdl::kMnistPart1Cols}, f);
    err_ = at::zeros({1}, f.dtype(at::kInt));
    part3_ = at::zeros({(int64_t)tdl::kDense1Chunks * b * 128}, f);
    a_ = tdl::MnistArgs{};
    a_.X = X_.data_ptr<float>();
    a_.Y = Y_.data_ptr<int>();
    a_.idx = idx_.data_ptr<int>();
    a_.W = W_.data_ptr<float>();
    a_.G = G_.data_ptr<float>();
    a_.ow1 = (int)offsets[0]; a_.ob1 = (int)offsets[1]; a_.ow2 = (int)offsets[2]; a_.ob2 = (int)offsets[3];
    a_.ow3 = (int)offsets[4]; a_.ob3 = (int)offsets[5]; a_.ow4 = (int)offsets[6]; a_.ob4 = (int)offsets[7];
    a_.P1 = P1_.data_ptr<float>();
    a_.A1 = A1_.data_ptr<uint8_t>();
    a_.P2 = P2_.data_ptr<float>();
    a_.A2 = A2_.data_ptr<uint8_t>();
    a_.H = H_.data_ptr<float>();
    a_.dH = dH_.data_ptr<float>();
    a_.dL = dL_.data_ptr<float>();
    a_.cnt = reinterpret_cast<unsigned*>(cnt_.data_ptr<int>());
    a_.dHt = reinterpret_cast<unsigned long long*>(dHt_.data_ptr<int64_t>());
    a_.ep = reinterpret_cast<unsigned*>(ep_.data_ptr<int>());
    a_.part3t = reinterpret_cast<unsigned long long*>(part3t_.data_ptr<int64_t>());
    a_.head = 1;
    {  // A/B switches of the fused kernel (diagnostics; see mnist_cnn.hip)
      const char* v = std::getenv("TDL_MNIST_VARIANT");
      a_.variant = v != nullptr ? std::atoi(v) : tdl::kDefaultMnistVariant;
      const char* g = std::getenv("TDL_FX_GRID");
      a_.fx_grid = g != nullptr ? std::max(0, std::atoi(g)) : 0;
    }
    a_.dp2_fwd = 0;
    a_.fused_bwd = 0;
    a_.err = reinterpret_cast<unsigned*>(err_.data_ptr<int>());
    a_.xchg = 0;
    a_.xtwo = 0;
    a_.dP2 = dP2_.data_ptr<float>();
    a_.part2 = part2_.data_ptr<float>();
    a_.part1 = part1_.data_ptr<float>();
    a_.part3 = part3_.data_ptr<float>();
    a_.metrics = metrics_.data_ptr<float>();
    a_.lr = lr_.data_ptr<float>();
    a_.b = (int)b;
    a_.scale = (float)scale;
    a_.nslab = (int)W.numel();
  }

  // accumulate metrics into another [>= 3] f32 tensor from now on (evaluation reuses step objects)
  void set_metrics(at::Tensor m) {
    check_cuda_f32(m, "metrics");
    TORCH_CHECK(m.numel() >= 3, "metrics needs >= 3 elements");
    metrics_ = m;
    a_.metrics = metrics_.data_ptr<float>();
  }

  void set_idx_offset(int64_t off) {
    TORCH_CHECK(off >= 0 && off + a_.b <= idx_.numel(), "idx offset out of range");
    a_.idx = idx_.data_ptr<int>() + off;
  }

  // Individual stages (tests / profiling): 5 dense weight grads, 6 conv bwd,
  // 8 fwd conv (+dense1, +head), 9 finalize.
  void stage(int64_t k, bool apply_sgd) {
    hipStream_t s = cur_stream();
    switch (k) {
      case 5: tdl::mnist_dense1_bwd(a_, !a_.dp2_fwd, false, s); break;
      case 6: tdl::mnist_conv_bwd(a_, s); break;
      case 8:
        a_.fused_bwd = (fused_bwd_ && a_.dp2_fwd) ? 1 : 0;
        tdl::mnist_fwd_conv(a_, s);
        break;
      case 9: finalize(apply_sgd, false); break;
      default: TORCH_CHECK(false, "unknown stage");
    }
  }

  // forward + loss + backward: leaves the complete gradient in G after finalize(), which also
  // computes the dense weight gradients.
  void forward_backward(int64_t idx_off) {
    set_idx_offset(idx_off);
    hipStream_t s = cur_stream();
    if (fused_bwd_ && a_.dp2_fwd) {  // ONE launch: forward, loss head, dP2 and the conv backward
      a_.fused_bwd = 1;
      tdl::mnist_fwd_conv(a_, s);
    } else {
      a_.fused_bwd = 0;
      tdl::mnist_fwd_conv(a_, s);
      if (!a_.dp2_fwd) tdl::mnist_dense1_bwd(a_, true, false, s);
      tdl::mnist_conv_bwd(a_, s);
    }
    dense_pending_ = true;
  }

  // dP2 inside k_fwd_conv (its workgroups wait for their image's head) or in a K5 launch; the
  // caller enables it only when the step's launches have the GPU to themselves and all 4b
  // workgroups of k_fwd_conv fit on the device at once
  void set_dp2_in_forward(bool on) { a_.dp2_fwd = on ? 1 : 0; }
  bool dp2_in_forward() const { return a_.dp2_fwd != 0; }
  // with dP2 in the forward kernel, also run the conv backward there (forward_backward only)
  void set_fused_bwd(bool on) { fused_bwd_ = on; }
  // keep_grad = false: a single replica's finalize with fused SGD does not write the gradient slab
  // G (nothing reads it on that path; fewer dirty lines for the kernel-end write-back)
  void set_keep_grad(bool on) {
    a_.variant = on ? (a_.variant & ~tdl::kMnistVariantNoG) : (a_.variant | tdl::kMnistVariantNoG);
  }
  bool keep_grad() const { return (a_.variant & tdl::kMnistVariantNoG) == 0; }
  bool fused_bwd() const { return fused_bwd_ && a_.dp2_fwd; }
  // k_finalize_x grid cap (0: one workgroup per range; see MnistArgs::fx_grid)
  void set_fx_grid(int64_t n) { a_.fx_grid = (int)std::max<int64_t>(0, n); }
  int64_t fx_grid() const { return a_.fx_grid; }

  // error word of the in-kernel hand-offs (bit 1: a wait timed out; host sync); reset=true clears it
  int64_t error(bool reset) {
    int64_t v = err_.item<int>();
    if (reset) err_.zero_();
    return v;
  }

  // the same step split at the point where the dense-layer gradients are final in G (after K5):
  // the engine all-reduces that bucket while backward_conv() runs
  void forward_dense(int64_t idx_off) {
    set_idx_offset(idx_off);
    hipStream_t s = cur_stream();
    a_.fused_bwd = 0;
    tdl::mnist_fwd_conv(a_, s);
    tdl::mnist_dense1_bwd(a_, !a_.dp2_fwd, true, s);
    dense_pending_ = false;
  }
  void backward_conv() { tdl::mnist_conv_bwd(a_, cur_stream()); }

  // partial reductions + dense weight gradients (+ SGD).  After a fused forward_backward the
  // fused finalize runs; with `exchange` (fused, apply_sgd, a channel set) it also all-reduces the
  // gradient across the replicas over xGMI before the update (one launch, see k_finalize_x)
  void finalize(bool apply_sgd, bool exchange) {
    if (a_.fused_bwd) {
      TORCH_CHECK(!exchange || (apply_sgd && xchg_ready_), "finalize: the exchange needs apply_sgd and set_exchange()");
      tdl::MnistArgs f = a_;
      f.xchg = exchange ? 1 : 0;
      tdl::mnist_finalize_x(f, apply_sgd, cur_stream());
      return;
    }
    TORCH_CHECK(!exchange, "finalize: the exchange needs the fused backward (forward_backward with fused_bwd)");
    tdl::mnist_finalize(a_, apply_sgd, dense_pending_, cur_stream());
  }

  // the xGMI channel finalize(exchange=true) all-reduces through: exchange slots at slab offsets
  // (capacity >= slab), one signal / epoch slot per finalize workgroup
  void set_exchange(const tdl_host::XgmiChannel& ch) {
    TORCH_CHECK(ch.device() == W_.get_device(), "set_exchange: channel on another device");
    TORCH_CHECK(ch.cap() >= W_.numel(), "set_exchange: channel smaller than the slab");
    TORCH_CHECK(ch.sig_blocks() >= tdl::kFxBlocks, "set_exchange: channel needs >= ", tdl::kFxBlocks, " signal slots");
    TORCH_CHECK(a_.ow4 == a_.ob3 + 128 && a_.ob4 == a_.ow4 + 1280, "set_exchange: dense bias/kernel ranges not contiguous");
    ch.fill_args(a_.xa);
    xchg_ready_ = true;
  }
  bool has_exchange() const { return xchg_ready_; }
  // 0: one-shot exchange in finalize (every rank sums every range); 1: two-shot (reduce-scatter of
  // 1/R of every range + copy of the owners' updated weights: 2 (R-1)/R of the slab over the fabric)
  void set_exchange_algo(int algo) { a_.xtwo = algo != 0; }
  int exchange_algo() const { return a_.xtwo; }

  // forward-only evaluation / inference of the b rows at idx_off: loss, correct count and sample
  // count accumulate into the metrics tensor; logits ([>= b*10] f32, optional) receive the logits
  void forward_eval(int64_t idx_off, c10::optional<at::Tensor> logits) {
    set_idx_offset(idx_off);
    tdl::MnistArgs f = a_;
    f.head = 2;
    f.fused_bwd = 0;
    f.logits = nullptr;
    if (logits.has_value()) {
      check_cuda_f32(*logits, "logits");
      TORCH_CHECK(logits->numel() >= (int64_t)a_.b * 10, "logits buffer too small");
      f.logits = logits->data_ptr<float>();
    }
    tdl::mnist_fwd_conv(f, cur_stream());
  }

  // forward features only (dense1 partials, no loss head / metrics)
  void forward_features(int64_t idx_off) {
    set_idx_offset(idx_off);
    tdl::MnistArgs f = a_;
    f.head = 0;
    f.fused_bwd = 0;
    tdl::mnist_fwd_conv(f, cur_stream());
  }

  // diagnostics: per-workgroup phase timestamps of the next launches (None to disable)
  void set_stamps(c10::optional<at::Tensor> t) {
    if (t.has_value()) {
      TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kLong, "stamps must be int64 on GPU");
      stamps_ = *t;
      a_.stamps = reinterpret_cast<unsigned long long*>(stamps_.data_ptr<int64_t>());
    } else {
      a_.stamps = nullptr;
    }
  }

  std::vector<at::Tensor> buffers() { return {P1_, A1_, P2_, A2_, H_, dH_, dP2_, part2_, part1_, part3_, dL_}; }

 private:
  at::Tensor X_, Y_, idx_, W_, G_, lr_, metrics_;
  at::Tensor P1_, A1_, P2_, A2_, H_, dH_, dP2_, part2_, part1_, part3_, dL_, cnt_, dHt_, ep_, part3t_, err_;
  bool fused_bwd_ = false;
  bool xchg_ready_ = false;
  bool dense_pending_ = true;  // finalize computes the dense weight gradients (forward_backward)
  at::Tensor stamps_;
  tdl::MnistArgs a_;
};

// The clip operands of an update kernel (keras/optimizers.py): gscale = the [scale, norm] buffer that
// clip_norm wrote (the kernel reads word 0), clipvalue = the clamp bound; both optional.
using OptTensor = c10::optional<at::Tensor>;
using OptDouble = c10::optional<double>;

const float* gscale_ptr(const OptTensor& gscale) {
  if (!gscale.has_value()) return nullptr;
  check_slab_f32(*gscale, "gscale");
  TORCH_CHECK(gscale->numel() >= 1, "gscale must hold the scale word");
  return gscale->data_ptr<float>();
}

void set_clip(tdl::OptimArgs& a, const OptTensor& gscale, const OptDouble& clipvalue) {
  a.gscale = gscale_ptr(gscale);
  a.clip = clipvalue.has_value() ? 1 : 0;
  a.clipvalue = clipvalue.has_value() ? (float)*clipvalue : 0.f;
}

// The weight-EMA operands of an update kernel (keras/optimizers.py device_ema): ema = the average slab E of
// w's size, momentum = ema_momentum (E = f32(m) * E + f32(1 - m) * W_new, the subtraction in f64 here),
// mode 0 none / 1 update E / 2 update E and store W = E.
tdl::WeightEma ema_operands(const at::Tensor& w, const OptTensor& ema, double momentum, int64_t mode) {
  TORCH_CHECK(mode >= 0 && mode <= 2, "ema_mode must be 0 (off), 1 (update E) or 2 (update E, W = E), got ", mode);
  if (mode == 0) {
    TORCH_CHECK(!ema.has_value(), "ema given with ema_mode 0");
    return tdl::WeightEma{nullptr, 0.f, 0.f, 0};
  }
  TORCH_CHECK(ema.has_value(), "ema_mode ", mode, " needs the ema slab");
  check_slab_f32(*ema, "ema");
  TORCH_CHECK(ema->device() == w.device(), "ema and w must be on the same device");
  TORCH_CHECK(ema->numel() == w.numel(), "slab size mismatch: w has ", w.numel(), " elements, ema has ", ema->numel());
  TORCH_CHECK(momentum >= 0.0 && momentum <= 1.0, "ema_momentum must lie in [0, 1], got ", momentum);
  const int64_t n = w.numel();
  const char* pw = reinterpret_cast<const char*>(w.data_ptr());
  const char* pe = reinterpret_cast<const char*>(ema->data_ptr());
  TORCH_CHECK(n == 0 || pw + n * 4 <= pe || pe + n * 4 <= pw, "w and ema must be different, non-overlapping slabs");
  return tdl::WeightEma{ema->data_ptr<float>(), (float)momentum, (float)(1.0 - momentum), (int)mode};
}

// The moving average of the weights as a launch of its own (csrc/kernels/ema.hip): mode 1 E = m E + c W, mode 2
// also W = E.  max_blocks lowers the grid cap (tests and scripts/bench_ema.py only).  Empty slabs launch nothing.
void weight_ema(at::Tensor w, at::Tensor e, double m, int64_t mode, c10::optional<int64_t> max_blocks) {
  check_slab_f32(w, "w");
  TORCH_CHECK(mode == 1 || mode == 2, "mode must be 1 (update E) or 2 (update E, W = E), got ", mode);
  const tdl::WeightEma x = ema_operands(w, e, m, mode);
  const int64_t mb = max_blocks.value_or(tdl::kEmaMaxBlocks);
  TORCH_CHECK(mb >= 1 && mb <= tdl::kEmaMaxBlocks, "max_blocks must lie in [1, ", tdl::kEmaMaxBlocks, "]");
  tdl::weight_ema_apply(w.data_ptr<float>(), x.e, w.numel(), x.m, x.c, x.mode, cur_stream(), (int)mb);
}

// Global gradient norm of a flat f32 slab and the clip scale (csrc/kernels/clip.hip, two launches):
// out[0] = scale = min(1, clipnorm / (norm + 1e-12)), out[1] = norm = |clamp(g, +-clipvalue)|_2 (f32 words;
// the sum in f64, in an order that depends on g.numel() alone).  partials: f64 scratch of
// >= clip_partials(g.numel()) elements.  An empty g launches no partial sums and writes norm 0, scale 1.
void clip_norm_chunk(at::Tensor g, at::Tensor partials, at::Tensor out, double clipnorm, OptDouble clipvalue,
                     int64_t chunk) {
  check_slab_f32(g, "g");
  check_slab_f32(out, "out");
  TORCH_CHECK(partials.is_cuda() && partials.is_contiguous() && partials.scalar_type() == at::kDouble,
              "partials must be a contiguous float64 GPU tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(partials.data_ptr()) % 16 == 0, "partials must be 16-byte aligned");
  TORCH_CHECK(out.numel() >= 2, "out must hold [scale, norm]");
  TORCH_CHECK(chunk == 2048 || chunk == 4096 || chunk == tdl::kClipChunk || chunk == 16384, "unknown chunk size");
  TORCH_CHECK(partials.numel() >= tdl::clip_partials_count(g.numel(), chunk), "partials too small: ",
              partials.numel(), " < ", tdl::clip_partials_count(g.numel(), chunk));
  tdl::clip_norm_apply(g.data_ptr<float>(), partials.data_ptr<double>(), out.data_ptr<float>(), g.numel(),
                       (float)clipnorm, clipvalue.has_value(), clipvalue.has_value() ? (float)*clipvalue : 0.f,
                       cur_stream(), (int)chunk);
}

void clip_norm(at::Tensor g, at::Tensor partials, at::Tensor out, double clipnorm, OptDouble clipvalue) {
  clip_norm_chunk(g, partials, out, clipnorm, clipvalue, tdl::kClipChunk);
}

// One micro-step of gradient accumulation over whole slabs (csrc/kernels/accum.hip, one launch):
// mode 0: A = G, mode 1: A = A + G, mode 2: G = (A + G) * c; zero_grad (modes 0, 1): G = 0 once it is read.
// max_blocks lowers the grid cap (tests and scripts/bench_accum.py only).  Empty slabs launch nothing.
void grad_accum(at::Tensor g, at::Tensor a, int64_t mode, double c, bool zero_grad, c10::optional<int64_t> max_blocks) {
  check_slab_f32(g, "g");
  check_slab_f32(a, "a");
  TORCH_CHECK(g.numel() == a.numel(), "slab size mismatch: g has ", g.numel(), " elements, a has ", a.numel());
  TORCH_CHECK(mode >= 0 && mode <= 2, "mode must be 0 (A = G), 1 (A += G) or 2 (G = (A + G) * c), got ", mode);
  TORCH_CHECK(!(zero_grad && mode == 2), "zero_grad only with modes 0 and 1 (mode 2 writes its result to g)");
  const int64_t n = g.numel();
  const char* pg = reinterpret_cast<const char*>(g.data_ptr());
  const char* pa = reinterpret_cast<const char*>(a.data_ptr());
  TORCH_CHECK(n == 0 || pg + n * 4 <= pa || pa + n * 4 <= pg, "g and a must be different, non-overlapping slabs");
  const int64_t mb = max_blocks.value_or(tdl::kAccumMaxBlocks);
  TORCH_CHECK(mb >= 1 && mb <= tdl::kAccumMaxBlocks, "max_blocks must lie in [1, ", tdl::kAccumMaxBlocks, "]");
  TORCH_CHECK(g.device() == a.device(), "g and a must be on the same device");
  tdl::grad_accum_apply(g.data_ptr<float>(), a.data_ptr<float>(), n, (int)mode, (float)c, zero_grad, cur_stream(),
                        (int)mb);
}

void sgd(at::Tensor w, at::Tensor g, at::Tensor lr, bool zero_grad, OptTensor gscale, OptDouble clipvalue,
         OptTensor ema, double ema_momentum, int64_t ema_mode) {
  check_slab_f32(w, "w");
  check_slab_f32(g, "g");
  check_cuda_f32(lr, "lr");
  TORCH_CHECK(w.numel() == g.numel());
  const float cv = clipvalue.has_value() ? (float)*clipvalue : 0.f;
  const tdl::WeightEma x = ema_operands(w, ema, ema_momentum, ema_mode);
  tdl::sgd_apply(w.data_ptr<float>(), g.data_ptr<float>(), lr.data_ptr<float>(), w.numel(), cur_stream(), zero_grad,
                 gscale_ptr(gscale), clipvalue.has_value() ? &cv : nullptr, &x);
}

void sgd_momentum(at::Tensor w, at::Tensor g, at::Tensor v, at::Tensor lr, double m, bool nesterov, bool zero_grad,
                  OptTensor gscale, OptDouble clipvalue, OptTensor ema, double ema_momentum, int64_t ema_mode) {
  check_slab_f32(w, "w");
  check_slab_f32(g, "g");
  check_slab_f32(v, "v");
  check_cuda_f32(lr, "lr");
  TORCH_CHECK(w.numel() == g.numel() && v.numel() == w.numel());
  const float cv = clipvalue.has_value() ? (float)*clipvalue : 0.f;
  const tdl::WeightEma x = ema_operands(w, ema, ema_momentum, ema_mode);
  tdl::sgd_momentum_apply(w.data_ptr<float>(), g.data_ptr<float>(), v.data_ptr<float>(), lr.data_ptr<float>(),
                          (float)m, nesterov, w.numel(), cur_stream(), zero_grad, gscale_ptr(gscale),
                          clipvalue.has_value() ? &cv : nullptr, &x);
}

// Flat-slab Adam / AdamW (+AMSGrad): state m, v (vhat), device lr and execution-start step t0
void adam(at::Tensor w, at::Tensor g, at::Tensor m, at::Tensor v, c10::optional<at::Tensor> vhat, at::Tensor lr,
          at::Tensor t0, int64_t t_add, double b1, double b2, double eps, double wd, OptTensor gscale,
          OptDouble clipvalue, OptTensor ema, double ema_momentum, int64_t ema_mode) {
  for (auto* t : {&w, &g, &m, &v}) check_slab_f32(*t, "adam operand");
  for (auto* t : {&lr, &t0}) check_cuda_f32(*t, "adam operand");
  TORCH_CHECK(g.numel() == w.numel() && m.numel() == w.numel() && v.numel() == w.numel());
  tdl::OptimArgs a{};
  a.w = w.data_ptr<float>(); a.g = g.data_ptr<float>(); a.s0 = m.data_ptr<float>(); a.s1 = v.data_ptr<float>();
  if (vhat.has_value()) {
    check_slab_f32(*vhat, "vhat");
    TORCH_CHECK(vhat->numel() == w.numel());
    a.s2 = vhat->data_ptr<float>();
    a.flags = 1;
  }
  a.lr = lr.data_ptr<float>(); a.t0 = t0.data_ptr<float>(); a.t_add = (int)t_add; a.n = w.numel();
  a.b1 = (float)b1; a.b2 = (float)b2; a.eps = (float)eps; a.wd = (float)wd;
  set_clip(a, gscale, clipvalue);
  a.ema = ema_operands(w, ema, ema_momentum, ema_mode);
  tdl::adam_apply(a, cur_stream());
}

// Flat-slab RMSprop (+momentum, centered)
void rmsprop(at::Tensor w, at::Tensor g, at::Tensor rms, c10::optional<at::Tensor> mom, c10::optional<at::Tensor> mg,
             at::Tensor lr, double rho, double momentum, double eps, OptTensor gscale, OptDouble clipvalue,
             OptTensor ema, double ema_momentum, int64_t ema_mode) {
  for (auto* t : {&w, &g, &rms}) check_slab_f32(*t, "rmsprop operand");
  check_cuda_f32(lr, "lr");
  TORCH_CHECK(g.numel() == w.numel() && rms.numel() == w.numel());
  tdl::OptimArgs a{};
  a.w = w.data_ptr<float>(); a.g = g.data_ptr<float>(); a.s0 = rms.data_ptr<float>();
  if (mom.has_value()) { check_slab_f32(*mom, "mom"); TORCH_CHECK(mom->numel() == w.numel()); a.s1 = mom->data_ptr<float>(); a.flags |= 1; }
  if (mg.has_value()) { check_slab_f32(*mg, "mg"); TORCH_CHECK(mg->numel() == w.numel()); a.s2 = mg->data_ptr<float>(); a.flags |= 2; }
  a.lr = lr.data_ptr<float>(); a.n = w.numel(); a.b1 = (float)rho; a.b2 = (float)momentum; a.eps = (float)eps;
  set_clip(a, gscale, clipvalue);
  a.ema = ema_operands(w, ema, ema_momentum, ema_mode);
  tdl::rmsprop_apply(a, cur_stream());
}

// Flat-slab Adagrad
void adagrad(at::Tensor w, at::Tensor g, at::Tensor acc, at::Tensor lr, double eps, OptTensor gscale,
             OptDouble clipvalue, OptTensor ema, double ema_momentum, int64_t ema_mode) {
  for (auto* t : {&w, &g, &acc}) check_slab_f32(*t, "adagrad operand");
  check_cuda_f32(lr, "lr");
  TORCH_CHECK(g.numel() == w.numel() && acc.numel() == w.numel());
  tdl::OptimArgs a{};
  a.w = w.data_ptr<float>(); a.g = g.data_ptr<float>(); a.s0 = acc.data_ptr<float>();
  a.lr = lr.data_ptr<float>(); a.n = w.numel(); a.eps = (float)eps;
  set_clip(a, gscale, clipvalue);
  a.ema = ema_operands(w, ema, ema_momentum, ema_mode);
  tdl::adagrad_apply(a, cur_stream());
}

// Layer tables of the layer-wise optimizers (csrc/kernels/layerwise.hip, optim.h): the only source of the
// indices those kernels use, validated here on the host.  The launchers accept nothing else.
struct LayerTables {
  at::Tensor chunks, first_chunk, wd, adapt;
  int64_t V = 0, C = 0, n = 0, chunk = tdl::kLayerChunk;
};

// chunk: kLayerChunk, or one of the measured candidates 4096 / 8192 (scripts/bench_layerwise.py)
LayerTables layer_tables_chunk(std::vector<int64_t> offsets, std::vector<int64_t> sizes, int64_t n,
                               std::vector<double> wd, std::vector<bool> adapt, int64_t chunk) {
  TORCH_CHECK(chunk == tdl::kLayerChunk || chunk == 4096 || chunk == 8192, "unknown chunk size");
  const size_t V = offsets.size();
  TORCH_CHECK(sizes.size() == V && wd.size() == V && adapt.size() == V,
              "layer_tables: offsets, sizes, wd and adapt must have one entry per variable");
  TORCH_CHECK(n >= 0 && n < (int64_t(1) << 31), "layer_tables: slab size ", n, " out of the int32 range");
  std::vector<int32_t> chunks, first;
  int64_t end = 0;
  for (size_t i = 0; i < V; ++i) {
    const int64_t o = offsets[i], sz = sizes[i];
    TORCH_CHECK(o >= 0 && sz >= 1, "layer_tables: variable ", i, " has offset ", o, ", size ", sz);
    TORCH_CHECK(o % 4 == 0, "layer_tables: variable ", i, " starts at ", o, ", not a multiple of 4 floats");
    if (i > 0) {
      TORCH_CHECK(o >= offsets[i - 1], "layer_tables: variables are not sorted by offset (variable ", i, ")");
      TORCH_CHECK(o >= end, "layer_tables: variable ", i, " at ", o, " overlaps its predecessor, which ends at ", end);
    }
    TORCH_CHECK(sz <= n && o <= n - sz, "layer_tables: variable ", i, " [", o, ", ", o + sz, ") ends past the slab's ",
                n, " elements");
    end = o + sz;
    first.push_back((int32_t)(chunks.size() / 4));
    for (int64_t p = 0; p < sz; p += chunk) {
      chunks.push_back((int32_t)(o + p));
      chunks.push_back((int32_t)std::min<int64_t>(chunk, sz - p));
      chunks.push_back((int32_t)i);
      chunks.push_back(0);
    }
  }
  first.push_back((int32_t)(chunks.size() / 4));
  LayerTables t;
  t.V = (int64_t)V;
  t.C = (int64_t)chunks.size() / 4;
  t.n = n;
  t.chunk = chunk;
  std::vector<float> wdf(wd.begin(), wd.end());
  std::vector<int32_t> ad(adapt.begin(), adapt.end());
  const auto i32 = at::TensorOptions().dtype(at::kInt);
  const auto dev = at::Device(at::kCUDA, c10::hip::current_device());
  const auto f32 = at::TensorOptions().dtype(at::kFloat);
  auto upload = [&](void* p, at::IntArrayRef shape, const at::TensorOptions& o) {
    return p == nullptr ? at::empty(shape, o.device(dev)) : at::from_blob(p, shape, o).clone().to(dev);
  };
  t.chunks = upload(t.C ? chunks.data() : nullptr, {t.C, 4}, i32);
  t.first_chunk = upload(first.data(), {t.V + 1}, i32);
  t.wd = upload(t.V ? wdf.data() : nullptr, {t.V}, f32);
  t.adapt = upload(t.V ? ad.data() : nullptr, {t.V}, i32);
  return t;
}

LayerTables layer_tables(std::vector<int64_t> offsets, std::vector<int64_t> sizes, int64_t n, std::vector<double> wd,
                         std::vector<bool> adapt) {
  return layer_tables_chunk(std::move(offsets), std::move(sizes), n, std::move(wd), std::move(adapt), tdl::kLayerChunk);
}

// an n-element slab operand of a layer-wise launch
float* layer_slab(const at::Tensor& t, const LayerTables& T, const char* name) {
  check_slab_f32(t, name);
  TORCH_CHECK(t.get_device() == T.chunks.get_device(), name, " is not on the layer tables' device");
  TORCH_CHECK(t.numel() >= T.n, name, " is too short: ", t.numel(), " < ", T.n, " elements");
  TORCH_CHECK(t.numel() == T.n, "the layer tables were built for n = ", T.n, ", ", name, " has ", t.numel());
  return t.data_ptr<float>();
}

double* layer_partials(const at::Tensor& p, const LayerTables& T) {
  TORCH_CHECK(p.is_cuda() && p.is_contiguous() && p.scalar_type() == at::kDouble,
              "partials must be a contiguous float64 GPU tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(p.data_ptr()) % 16 == 0, "partials must be 16-byte aligned");
  TORCH_CHECK(p.numel() >= 2 * T.C, "partials too small: ", p.numel(), " < ", 2 * T.C);
  return p.data_ptr<double>();
}

float* layer_words(const at::Tensor& t, int64_t need, const char* name) {
  check_slab_f32(t, name);
  TORCH_CHECK(t.numel() >= need, name, " too small: ", t.numel(), " < ", need);
  return t.data_ptr<float>();
}

tdl::LayerArgs layer_args(const LayerTables& T) {
  tdl::LayerArgs a{};
  a.chunks = T.chunks.data_ptr<int>();
  a.first_chunk = T.first_chunk.data_ptr<int>();
  a.wd = T.wd.data_ptr<float>();
  a.adapt = T.adapt.data_ptr<int>();
  a.V = (int)T.V;
  a.C = (int)T.C;
  a.chunk = (int)T.chunk;
  return a;
}

void set_layer_clip(tdl::LayerArgs& a, const OptTensor& gscale, const OptDouble& clipvalue) {
  a.gscale = gscale_ptr(gscale);
  a.clip = clipvalue.has_value() ? 1 : 0;
  a.clipvalue = clipvalue.has_value() ? (float)*clipvalue : 0.f;
}

void set_lamb(tdl::LayerArgs& a, const at::Tensor& t0, int64_t t_add, double b1, double b2, double eps) {
  check_cuda_f32(t0, "t0");
  TORCH_CHECK(t0.numel() >= 1, "t0 must hold the step count");
  a.t0 = t0.data_ptr<float>();
  a.t_add = (int)t_add;
  a.b1 = (float)b1;
  a.b2 = (float)b2;
  a.eps = (float)eps;
  TORCH_CHECK(a.b1 > 0.f && a.b1 < 1.f && a.b2 > 0.f && a.b2 < 1.f, "LAMB: beta_1 and beta_2 must lie in (0, 1)");
  a.lb1 = (float)std::log((double)a.b1);
  a.lb2 = (float)std::log((double)a.b2);
}

// launch 1: partials[c] = (sum w^2, sum g'^2) of chunk c
void lars_sums(const LayerTables& T, at::Tensor w, at::Tensor g, at::Tensor partials, OptTensor gscale,
               OptDouble clipvalue) {
  tdl::LayerArgs a = layer_args(T);
  a.w = layer_slab(w, T, "w");
  a.g = layer_slab(g, T, "g");
  a.partials = layer_partials(partials, T);
  set_layer_clip(a, gscale, clipvalue);
  tdl::layer_sums_apply(a, false, cur_stream());
}

// launch 1: m, v updated in place; partials[c] = (sum w^2, sum u^2) of chunk c
void lamb_sums(const LayerTables& T, at::Tensor w, at::Tensor g, at::Tensor m, at::Tensor v, at::Tensor partials,
               at::Tensor t0, int64_t t_add, double b1, double b2, double eps, OptTensor gscale,
               OptDouble clipvalue) {
  tdl::LayerArgs a = layer_args(T);
  a.w = layer_slab(w, T, "w");
  a.g = layer_slab(g, T, "g");
  a.s0 = layer_slab(m, T, "m");
  a.s1 = layer_slab(v, T, "v");
  a.partials = layer_partials(partials, T);
  set_lamb(a, t0, t_add, b1, b2, eps);
  set_layer_clip(a, gscale, clipvalue);
  tdl::layer_sums_apply(a, true, cur_stream());
}

// launch 2: ratio[v], norms[v] = (|w_v|, |g'_v| or |u_v|) from the chunk sums
void layer_ratio(const LayerTables& T, at::Tensor partials, at::Tensor ratio, at::Tensor norms, bool lamb,
                 double eeta, double eps) {
  tdl::LayerArgs a = layer_args(T);
  a.partials = layer_partials(partials, T);
  a.ratio = layer_words(ratio, T.V, "ratio");
  a.norms = layer_words(norms, 2 * T.V, "norms");
  TORCH_CHECK(ratio.get_device() == T.chunks.get_device() && norms.get_device() == T.chunks.get_device() &&
                  partials.get_device() == T.chunks.get_device(), "operands are not on the layer tables' device");
  a.eeta = (float)eeta;
  a.eps = (float)eps;
  tdl::layer_ratio_apply(a, lamb, cur_stream());
}

void lars_ratio(const LayerTables& T, at::Tensor partials, at::Tensor ratio, at::Tensor norms, double eeta,
                double eps) {
  layer_ratio(T, partials, ratio, norms, false, eeta, eps);
}

void lamb_ratio(const LayerTables& T, at::Tensor partials, at::Tensor ratio, at::Tensor norms) {
  layer_ratio(T, partials, ratio, norms, true, 0.0, 0.0);
}

// launch 3
void lars_update(const LayerTables& T, at::Tensor w, at::Tensor g, at::Tensor v, at::Tensor ratio, at::Tensor lr,
                 double momentum, bool nesterov, OptTensor gscale, OptDouble clipvalue, OptTensor ema,
                 double ema_momentum, int64_t ema_mode) {
  tdl::LayerArgs a = layer_args(T);
  a.w = layer_slab(w, T, "w");
  a.g = layer_slab(g, T, "g");
  a.s0 = layer_slab(v, T, "v");
  a.ratio = layer_words(ratio, T.V, "ratio");
  check_cuda_f32(lr, "lr");
  TORCH_CHECK(lr.numel() >= 1, "lr must hold the learning rate");
  a.lr = lr.data_ptr<float>();
  a.b1 = (float)momentum;
  a.nesterov = nesterov ? 1 : 0;
  set_layer_clip(a, gscale, clipvalue);
  a.ema = ema_operands(w, ema, ema_momentum, ema_mode);
  tdl::lars_apply(a, cur_stream());
}

void lamb_update(const LayerTables& T, at::Tensor w, at::Tensor m, at::Tensor v, at::Tensor ratio, at::Tensor lr,
                 at::Tensor t0, int64_t t_add, double b1, double b2, double eps, OptTensor ema, double ema_momentum,
                 int64_t ema_mode) {
  tdl::LayerArgs a = layer_args(T);
  a.w = layer_slab(w, T, "w");
  a.s0 = layer_slab(m, T, "m");
  a.s1 = layer_slab(v, T, "v");
  a.ratio = layer_words(ratio, T.V, "ratio");
  check_cuda_f32(lr, "lr");
  TORCH_CHECK(lr.numel() >= 1, "lr must hold the learning rate");
  a.lr = lr.data_ptr<float>();
  set_lamb(a, t0, t_add, b1, b2, eps);
  a.ema = ema_operands(w, ema, ema_momentum, ema_mode);
  tdl::lamb_apply(a, cur_stream());
}

}  // namespace

void register_ops(pybind11::module& m);
void register_comm(pybind11::module& m);
void register_rccl(pybind11::module& m);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 HIP kernels of tensorflow_distributed_learning_amd";
  pybind11::class_<MnistStep>(m, "MnistStep")
      .def(pybind11::init<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, std::vector<int64_t>, int64_t,
                          double, at::Tensor, at::Tensor>())
      .def("set_idx_offset", &MnistStep::set_idx_offset)
      .def("set_metrics", &MnistStep::set_metrics)
      .def("stage", &MnistStep::stage, pybind11::arg("k"), pybind11::arg("apply_sgd") = false)
      .def("forward_backward", &MnistStep::forward_backward)
      .def("forward_features", &MnistStep::forward_features)
      .def("forward_eval", &MnistStep::forward_eval, pybind11::arg("idx_off"), pybind11::arg("logits") = pybind11::none())
      .def("forward_dense", &MnistStep::forward_dense)
      .def("backward_conv", &MnistStep::backward_conv)
      .def("set_fx_grid", &MnistStep::set_fx_grid)
      .def("fx_grid", &MnistStep::fx_grid)
      .def("finalize", &MnistStep::finalize, pybind11::arg("apply_sgd"), pybind11::arg("exchange") = false)
      .def("set_exchange", &MnistStep::set_exchange)
      .def("has_exchange", &MnistStep::has_exchange)
      .def("set_exchange_algo", &MnistStep::set_exchange_algo)
      .def("exchange_algo", &MnistStep::exchange_algo)
      .def("set_dp2_in_forward", &MnistStep::set_dp2_in_forward)
      .def("dp2_in_forward", &MnistStep::dp2_in_forward)
      .def("set_fused_bwd", &MnistStep::set_fused_bwd)
      .def("fused_bwd", &MnistStep::fused_bwd)
      .def("set_keep_grad", &MnistStep::set_keep_grad)
      .def("keep_grad", &MnistStep::keep_grad)
      .def("error", &MnistStep::error, pybind11::arg("reset") = false)
      .def("buffers", &MnistStep::buffers)
      .def("set_stamps", &MnistStep::set_stamps);
  const auto none = pybind11::none();
  m.attr("CLIP_CHUNK") = (int64_t)tdl::kClipChunk;           // elements per k_clip_partials workgroup
  m.attr("CLIP_SCALE_THREADS") = (int64_t)tdl::kClipScaleThreads;  // threads of k_clip_scale
  m.def("clip_partials", [](int64_t n) { return tdl::clip_partials_count(n); },
        "f64 partial sums clip_norm needs for an n-element slab");
  m.def("clip_norm", &clip_norm,
        "out[0] = min(1, clipnorm / (|clamp(g)|_2 + 1e-12)), out[1] = the norm; deterministic f64 sum",
        pybind11::arg("g"), pybind11::arg("partials"), pybind11::arg("out"), pybind11::arg("clipnorm"),
        pybind11::arg("clipvalue") = none);
  m.def("clip_norm_chunk", &clip_norm_chunk, "clip_norm at another chunk size (measurement only)",
        pybind11::arg("g"), pybind11::arg("partials"), pybind11::arg("out"), pybind11::arg("clipnorm"),
        pybind11::arg("clipvalue"), pybind11::arg("chunk"));
  m.attr("ACCUM_MAX_BLOCKS") = (int64_t)tdl::kAccumMaxBlocks;    // grid cap of k_grad_accum
  m.attr("ACCUM_BLOCK_ELEMS") = (int64_t)tdl::kAccumBlockElems;  // elements a workgroup handles per grid pass
  m.def("grad_accum", &grad_accum,
        "gradient accumulation micro-step: mode 0 a = g, 1 a += g, 2 g = (a + g) * c (zero_grad: g := 0, modes 0/1)",
        pybind11::arg("g"), pybind11::arg("a"), pybind11::arg("mode"), pybind11::arg("c"),
        pybind11::arg("zero_grad") = false, pybind11::arg("max_blocks") = none);
  m.attr("EMA_MAX_BLOCKS") = (int64_t)tdl::kEmaMaxBlocks;    // grid cap of k_weight_ema
  m.attr("EMA_BLOCK_ELEMS") = (int64_t)tdl::kEmaBlockElems;  // elements a workgroup handles per grid pass
  m.def("weight_ema", &weight_ema,
        "moving average of the weights: mode 1 e = f32(m) e + f32(1 - m) w, mode 2 also w = e (three f32 roundings)",
        pybind11::arg("w"), pybind11::arg("e"), pybind11::arg("m"), pybind11::arg("mode"),
        pybind11::arg("max_blocks") = none);
  m.def("sgd", &sgd, "w -= lr * g over a flat slab (zero_grad: g := 0 afterwards)", pybind11::arg("w"),
        pybind11::arg("g"), pybind11::arg("lr"), pybind11::arg("zero_grad") = false,
        pybind11::arg("gscale") = none, pybind11::arg("clipvalue") = none, pybind11::arg("ema") = none,
        pybind11::arg("ema_momentum") = 0.0, pybind11::arg("ema_mode") = 0);
  m.def("sgd_momentum", &sgd_momentum, "Keras momentum SGD over a flat slab (zero_grad: g := 0 afterwards)",
        pybind11::arg("w"), pybind11::arg("g"), pybind11::arg("v"), pybind11::arg("lr"), pybind11::arg("m"),
        pybind11::arg("nesterov"), pybind11::arg("zero_grad") = false, pybind11::arg("gscale") = none,
        pybind11::arg("clipvalue") = none, pybind11::arg("ema") = none,
        pybind11::arg("ema_momentum") = 0.0, pybind11::arg("ema_mode") = 0);
  m.def("adam", &adam, pybind11::arg("w"), pybind11::arg("g"), pybind11::arg("m"), pybind11::arg("v"),
        pybind11::arg("vhat"), pybind11::arg("lr"), pybind11::arg("t0"), pybind11::arg("t_add"), pybind11::arg("b1"),
        pybind11::arg("b2"), pybind11::arg("eps"), pybind11::arg("wd") = 0.0, pybind11::arg("gscale") = none,
        pybind11::arg("clipvalue") = none, pybind11::arg("ema") = none,
        pybind11::arg("ema_momentum") = 0.0, pybind11::arg("ema_mode") = 0);
  m.def("rmsprop", &rmsprop, pybind11::arg("w"), pybind11::arg("g"), pybind11::arg("rms"), pybind11::arg("mom"),
        pybind11::arg("mg"), pybind11::arg("lr"), pybind11::arg("rho"), pybind11::arg("momentum"), pybind11::arg("eps"),
        pybind11::arg("gscale") = none, pybind11::arg("clipvalue") = none, pybind11::arg("ema") = none,
        pybind11::arg("ema_momentum") = 0.0, pybind11::arg("ema_mode") = 0);
  m.def("adagrad", &adagrad, pybind11::arg("w"), pybind11::arg("g"), pybind11::arg("acc"), pybind11::arg("lr"),
        pybind11::arg("eps"), pybind11::arg("gscale") = none, pybind11::arg("clipvalue") = none, pybind11::arg("ema") = none,
        pybind11::arg("ema_momentum") = 0.0, pybind11::arg("ema_mode") = 0);
  // layer-wise optimizers (csrc/kernels/layerwise.hip): host-validated tables, then three launches per step
  m.attr("LAYER_CHUNK") = (int64_t)tdl::kLayerChunk;  // largest chunk of a variable (one workgroup)
  pybind11::class_<LayerTables>(m, "LayerTables")
      .def_readonly("chunks", &LayerTables::chunks)
      .def_readonly("first_chunk", &LayerTables::first_chunk)
      .def_readonly("wd", &LayerTables::wd)
      .def_readonly("adapt", &LayerTables::adapt)
      .def_readonly("V", &LayerTables::V)
      .def_readonly("C", &LayerTables::C)
      .def_readonly("n", &LayerTables::n)
      .def_readonly("chunk", &LayerTables::chunk);
  m.def("layer_tables", &layer_tables,
        "validated chunk tables of the variables [offsets[i], offsets[i] + sizes[i]) of an n-element slab, on the "
        "current device",
        pybind11::arg("offsets"), pybind11::arg("sizes"), pybind11::arg("n"), pybind11::arg("wd"),
        pybind11::arg("adapt"));
  m.def("layer_tables_chunk", &layer_tables_chunk, "layer_tables at another chunk size (measurement only)",
        pybind11::arg("offsets"), pybind11::arg("sizes"), pybind11::arg("n"), pybind11::arg("wd"),
        pybind11::arg("adapt"), pybind11::arg("chunk"));
  m.def("lars_sums", &lars_sums, pybind11::arg("tables"), pybind11::arg("w"), pybind11::arg("g"),
        pybind11::arg("partials"), pybind11::arg("gscale") = none, pybind11::arg("clipvalue") = none);
  m.def("lamb_sums", &lamb_sums, pybind11::arg("tables"), pybind11::arg("w"), pybind11::arg("g"), pybind11::arg("m"),
        pybind11::arg("v"), pybind11::arg("partials"), pybind11::arg("t0"), pybind11::arg("t_add"),
        pybind11::arg("b1"), pybind11::arg("b2"), pybind11::arg("eps"), pybind11::arg("gscale") = none,
        pybind11::arg("clipvalue") = none);
  m.def("lars_ratio", &lars_ratio, pybind11::arg("tables"), pybind11::arg("partials"), pybind11::arg("ratio"),
        pybind11::arg("norms"), pybind11::arg("eeta"), pybind11::arg("eps"));
  m.def("lamb_ratio", &lamb_ratio, pybind11::arg("tables"), pybind11::arg("partials"), pybind11::arg("ratio"),
        pybind11::arg("norms"));
  m.def("lars_update", &lars_update, pybind11::arg("tables"), pybind11::arg("w"), pybind11::arg("g"),
        pybind11::arg("v"), pybind11::arg("ratio"), pybind11::arg("lr"), pybind11::arg("momentum"),
        pybind11::arg("nesterov"), pybind11::arg("gscale") = none, pybind11::arg("clipvalue") = none, pybind11::arg("ema") = none,
        pybind11::arg("ema_momentum") = 0.0, pybind11::arg("ema_mode") = 0);
  m.def("lamb_update", &lamb_update, pybind11::arg("tables"), pybind11::arg("w"), pybind11::arg("m"),
        pybind11::arg("v"), pybind11::arg("ratio"), pybind11::arg("lr"), pybind11::arg("t0"), pybind11::arg("t_add"),
        pybind11::arg("b1"), pybind11::arg("b2"), pybind11::arg("eps"), pybind11::arg("ema") = none,
        pybind11::arg("ema_momentum") = 0.0, pybind11::arg("ema_mode") = 0);
  register_ops(m);
  register_comm(m);
  register_rccl(m);
}
