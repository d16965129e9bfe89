// The moving average of the weights as a launch of its own (see ema.h): a pure streaming kernel, laid out
// as k_grad_accum (accum.hip) is.
//
// Every element depends on its own two operands only -- no atomics, no reductions -- so the result has the
// same bits at every grid size, buffer address and replica.  A workgroup handles kEmaBlockElems contiguous
// elements per grid pass: every thread issues its kEmaVecs 16-B loads of each tensor before its first
// store, then computes and stores.  The grid is capped at kEmaMaxBlocks and strides over larger slabs.
// Only the one tile that holds the slab's end takes the guarded path: whole vectors while they fit, then
// a scalar tail of n % 4 elements.  Plain stores: the next step's forward reads W, and its update E, soon.
#include "ema.h"

#include "common.h"
#include "optim.h"

namespace tdl {
namespace {

constexpr int kT = kEmaThreads;
constexpr int kU = kEmaVecs;

// MODE 1: w is only read.  MODE 2: the new average is stored as w too.
template <int MODE>
__global__ __launch_bounds__(kT) void k_weight_ema(float* __restrict__ w, float* __restrict__ e, int64_t n,
                                                   WeightEma x) {
  static_assert(MODE == 1 || MODE == 2, "mode 0 launches nothing");
  constexpr int64_t BE = kEmaBlockElems;
  const int tid = threadIdx.x;
  for (int64_t base = (int64_t)blockIdx.x * BE; base < n; base += (int64_t)gridDim.x * BE) {
    if (base + BE <= n) {
      f4 vw[kU], ve[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) vw[u] = ld4(w + base + ((int64_t)u * kT + tid) * 4);
#pragma unroll
      for (int u = 0; u < kU; ++u) ve[u] = ld4(e + base + ((int64_t)u * kT + tid) * 4);
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int64_t i4 = base + ((int64_t)u * kT + tid) * 4;
        const f4 r = ema_fold(x, ve[u], vw[u]);
        st4(e + i4, r);
        if (MODE == 2) st4(w + i4, r);
      }
    } else {  // the tile that holds the slab's end: whole vectors while they fit, then a scalar tail
#pragma unroll 1
      for (int u = 0; u < kU; ++u) {
        const int64_t i4 = base + ((int64_t)u * kT + tid) * 4;
        if (i4 + 3 < n) {
          const f4 r = ema_fold(x, ld4(e + i4), ld4(w + i4));
          st4(e + i4, r);
          if (MODE == 2) st4(w + i4, r);
        } else {
          for (int k = 0; k < 4 && i4 + k < n; ++k) {
            const float r = ema_fold(x, e[i4 + k], w[i4 + k]);
            e[i4 + k] = r;
            if (MODE == 2) w[i4 + k] = r;
          }
        }
      }
    }
  }
}

}  // namespace

void weight_ema_apply(float* w, float* e, int64_t n, float m, float c, int mode, hipStream_t s, int max_blocks) {
  if (n <= 0 || mode == 0) return;
  const int64_t tiles = (n + kEmaBlockElems - 1) / kEmaBlockElems;
  const int cap = max_blocks < 1 ? 1 : (max_blocks > kEmaMaxBlocks ? kEmaMaxBlocks : max_blocks);
  const dim3 grid((unsigned)(tiles < cap ? tiles : cap)), block(kT);
  const WeightEma x{e, m, c, mode};
  if (mode == 2) hipLaunchKernelGGL(k_weight_ema<2>, grid, block, 0, s, w, e, n, x);
  else hipLaunchKernelGGL(k_weight_ema<1>, grid, block, 0, s, w, e, n, x);
}

}  // namespace tdl
