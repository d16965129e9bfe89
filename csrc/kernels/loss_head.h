// Weighted / smoothed softmax cross-entropy loss head of the generic engine, and the three-column batch
// gather of a weighted device-resident dataset (csrc/kernels/loss_head.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdl {

// The fused loss head (gemm.h xent_head) with sample weights, class weights, label smoothing and dense
// targets.  Per row r of the f32 logits z [N][K], with m = max z, u_k = z_k - m, se = sum exp(u_k),
// p_k = exp(u_k) / se:
//   sparse (labels int64 [N]), label y in [0, K):  q_k = (1 - eps) [k == y] + eps / K,  S = 1,
//       loss = log(se) - (1 - eps) u_y - (eps / K) sum_k u_k
//   sparse, y outside [0, K):  q = 0, loss = 0, class weight 1 (cw is not read)
//   dense (targets f32 [N][K]):  q_k = (1 - eps) t_k + eps / K,  S = sum q_k,
//       loss = S log(se) - sum q_k u_k,  class = argmax_k t_k (first index on ties)
//   w = sw[r] * cw[class] (an absent factor is 1),  dz_k = (p_k S - q_k) * f32(w * f32(1 / gn)).
// loss_out[0] = f32(sum w loss / gn); the f64 accumulators (any may be null) advance by
//   lt_total += sum w loss, lt_count += N, acc_total += sum w [argmax z == class], acc_count += sum w
// (exactly N without weights).  Rows are added in f64 in an order that depends only on (N, K).
// eps == 0, a sparse target and no (or all-ones) weights give xent_head's bits.
// rows_ws: null for the one-workgroup form, else [3N] f32 scratch of the rows + finish form.
void xent_head_w(const float* z, const long long* labels, const float* targets, const float* sw, const float* cw,
                 int N, int K, double gn, float eps, float* loss_out, float* dz, double* lt_total, double* lt_count,
                 double* acc_total, double* acc_count, float* rows_ws, hipStream_t s);

// (out[r, :], out_lab[r], out_w[r]) = (src[idx[r], :], lab[idx[r]], w[idx[r]]): gather_xy (ops.h) with a
// third, f32 column (the sample weights of a weighted device-resident dataset), one launch
void gather_xyw(const float* src, const void* lab, const float* w, const int* idx, float* out, void* out_lab,
                float* out_w, int64_t rows, int64_t row_elems, int lab_bytes, hipStream_t s);

}  // namespace tdl
