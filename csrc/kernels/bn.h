// Training-mode batch normalisation over channels-innermost activations [M, C] (NHWC flattened:
// M = N*H*W), bf16 or f32 data, f32 statistics.  Used by keras.layers.BatchNormalization on the
// GPU (ResNet-50, BASELINE configs 4/5).
// Accuracy: the variance is Q/M - mean^2 with the per-workgroup sums of x and x^2 in f32, so invstd loses
// relative accuracy with (mean/std)^2: supported is |mean|/std up to about 16 (measured relative error of
// invstd on f32 data, 3000 rows: 8e-5 at mean 8 / std 0.5, 3e-3 at 30 / 0.25; at 100 / 0.1 it is 0.24,
// i.e. only finite and bounded by 1/sqrt(eps); tests/test_bn_edges_gpu.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdl {

enum class BnDType { kF32 = 0, kBF16 = 1 };

// rows per workgroup and workgroup count of the partial-sum passes for [M, C]
struct BnPlan {
  int groups;       // C / 8 channel groups (8 channels per thread)
  int rows_iter;    // rows per workgroup iteration = 256 / groups
  int64_t rows_wg;  // rows per workgroup
  int parts;        // workgroups (partial rows in the workspace)
  int part_rows;    // workspace rows ([part_rows][2][C] f32): partials + their first-level reduction
};
BnPlan bn_plan(int64_t M, int C);
// sweep hooks (0 = keep): partial-pass workgroup cap, grid cap of the grid-stride elementwise kernels
// (default 4096), their vectors per thread (1 or 2), grid cap of the blocked elementwise kernels
// (default 8192)
void bn_set_tuning(int max_parts, int elem_blocks, int elem_unroll, int blk_blocks = 0);
// the four values bn_set_tuning sets, in its argument order
void bn_get_tuning(int out[4]);
// elementwise kernel family (A/B hook): 0 grid-stride, 1 blocked with 2 / 4 / 8 vectors per thread
void bn_set_elementwise(int kind, int vectors_per_thread);

// forward: part [parts][2][C] scratch; mean/invstd [C] out; scale/shift [C] out (x*scale+shift);
// moving stats updated in place (momentum m: moving = moving*m + batch*(1-m), variance unbiased);
// mean_off (nullable): per-channel bias of a preceding conv folded into this BN (moving mean only).
// given_parts > 0: `part` already holds that many partial rows ([rows][2][C]; space for
// ceil(rows / 64) more behind them), the partial pass is skipped
void bn_forward_stats(const void* x, BnDType dt, int64_t M, int C, float* part, const float* gamma,
                      const float* beta, const float* mean_off, float* mean, float* invstd, float* scale, float* shift,
                      float* moving_mean, float* moving_var, float momentum, float eps, hipStream_t s,
                      int given_parts = 0);
// y = act(x*scale + shift [+ residual])  (relu when relu != 0; residual nullable).  The ReLU is fmaxf(., 0):
// a NaN pre-activation is stored as 0 (and masks its gradient); the channel's statistics, moving variance,
// dgamma and dx keep the NaN
void bn_apply(const void* x, const void* residual, void* y, BnDType dt, int64_t M, int C, const float* scale,
              const float* shift, int relu, hipStream_t s);
// backward; dgamma/dbeta [C] out (acc bit 0/1: added into them), coef [3][C] scratch, dx = A*dz + B*x + D where
//   mode 0: dz = dy                         (plain BN)
//   mode 1: dz = dy * (x*scale+shift > 0)   (BN + ReLU, mask recomputed from x)
//   mode 2: dz = dy * (y > 0), written to dz (BN + Add + ReLU: dz is also the residual's gradient)
void bn_backward(const void* dy, const void* x, const void* y, void* dz, void* dx, BnDType dt, int64_t M, int C,
                 float* part, const float* gamma, const float* mean, const float* invstd, const float* scale,
                 const float* shift, float* dgamma, float* dbeta, float* coef, int mode, int acc, hipStream_t s,
                 int given_parts = 0);  // > 0: dy is the masked dz and part holds its reduction

// Synchronized (cross-replica) batch norm: the finalize of either direction split around an
// all-reduce.  `*_pack` reduces this replica's partial rows (its own pass over the tensor, or
// given_parts rows as above) and writes them into rank `rank`'s slot of the exchange buffer xbuf
// (f32, xnumel >= bn_sync_xbuf_numel(C, R) elements, 16-byte aligned), zeroing the rest of it; the
// caller SUM-all-reduces xbuf across the R replicas; `*_finalize` adds the replicas' sums in rank
// order and finishes as bn_forward_stats / bn_backward do, with the global sums and row count.
int64_t bn_sync_xbuf_numel(int C, int R);
void bn_sync_forward_pack(const void* x, BnDType dt, int64_t M, int C, float* part, float* xbuf, int64_t xnumel,
                          int rank, hipStream_t s, int given_parts = 0);
void bn_sync_forward_finalize(const float* xbuf, int R, int C, const float* gamma, const float* beta,
                              const float* mean_off, float* mean, float* invstd, float* scale, float* shift,
                              float* moving_mean, float* moving_var, float momentum, float eps, hipStream_t s);
// dgamma / dbeta: from this replica's LOCAL sums (the gradient all-reduce adds the replicas');
// mode 2 without given_parts writes dz as bn_backward does
void bn_sync_backward_pack(const void* dy, const void* x, const void* y, void* dz, BnDType dt, int64_t M, int C,
                           float* part, const float* mean, const float* invstd, const float* scale,
                           const float* shift, float* dgamma, float* dbeta, int mode, int acc, float* xbuf,
                           int64_t xnumel, int rank, hipStream_t s, int given_parts = 0);
// coef [3][C] from the global sums, then dx = A*dz + B*x + D over this replica's rows (mask: dz is
// dy, masked by x*scale+shift > 0 as in mode 1)
void bn_sync_backward_finalize(const float* xbuf, int R, const void* dz, const void* x, void* dx, BnDType dt, int64_t M,
                               int C, const float* gamma, const float* mean, const float* invstd, const float* scale,
                               const float* shift, float* coef, bool mask, hipStream_t s);

}  // namespace tdl
