// Gradient accumulation over the flat gradient slab (see accum.h): a pure streaming kernel.
//
// Every element depends on its own two operands only -- no atomics, no reductions -- so the result has the
// same bits at every grid size, buffer address and replica.  A workgroup handles kAccumBlockElems
// contiguous elements per grid pass: every thread issues its kAccumVecs 16-B loads of each tensor before
// its first store (the loads of a pass are all in flight together, as in the blocked BN passes), then
// computes and stores.  The grid is capped at kAccumMaxBlocks and strides over larger slabs.  Only the
// one tile that holds the slab's end takes the guarded path: whole vectors while they fit, then a scalar
// tail of n % 4 elements.  Plain stores: the next kernel (the following micro-step's accumulate, the
// all-reduce or the update) reads A and G again soon, and a plain store keeps the line in the XCD's L2.
#include "accum.h"
#include "common.h"

namespace tdl {
namespace {

constexpr int kT = kAccumThreads;
constexpr int kU = kAccumVecs;

#pragma clang fp contract(off)  // (a + g) * c is two roundings wherever the compiler sees it

template <int MODE>
__device__ __forceinline__ float accum1(float a, float g, float c) {
  if (MODE == 0) return g;
  if (MODE == 1) return a + g;
  return (a + g) * c;
}

template <int MODE>
__device__ __forceinline__ f4 accum4(f4 a, f4 g, float c) {
  f4 r;
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k] = accum1<MODE>(a[k], g[k], c);
  return r;
}

template <int MODE, bool ZERO_G>
__global__ __launch_bounds__(kT) void k_grad_accum(float* __restrict__ g, float* __restrict__ a, int64_t n, float c) {
  static_assert(MODE != 2 || !ZERO_G, "mode 2 writes its result to G");
  constexpr int64_t BE = kAccumBlockElems;
  float* const dst = MODE == 2 ? g : a;
  const int tid = threadIdx.x;
  for (int64_t base = (int64_t)blockIdx.x * BE; base < n; base += (int64_t)gridDim.x * BE) {
    if (base + BE <= n) {
      f4 vg[kU], va[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) vg[u] = ld4(g + base + ((int64_t)u * kT + tid) * 4);
      if (MODE != 0) {
#pragma unroll
        for (int u = 0; u < kU; ++u) va[u] = ld4(a + base + ((int64_t)u * kT + tid) * 4);
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int64_t i4 = base + ((int64_t)u * kT + tid) * 4;
        st4(dst + i4, accum4<MODE>(MODE != 0 ? va[u] : vg[u], vg[u], c));
        if (ZERO_G) st4(g + i4, zero4());
      }
    } else {  // the tile that holds the slab's end: whole vectors while they fit, then a scalar tail
#pragma unroll 1
      for (int u = 0; u < kU; ++u) {
        const int64_t i4 = base + ((int64_t)u * kT + tid) * 4;
        if (i4 + 3 < n) {
          const f4 vg = ld4(g + i4);
          const f4 va = MODE != 0 ? ld4(a + i4) : vg;
          st4(dst + i4, accum4<MODE>(va, vg, c));
          if (ZERO_G) st4(g + i4, zero4());
        } else {
          for (int k = 0; k < 4 && i4 + k < n; ++k) {
            const float xg = g[i4 + k];
            const float xa = MODE != 0 ? a[i4 + k] : xg;
            dst[i4 + k] = accum1<MODE>(xa, xg, c);
            if (ZERO_G) g[i4 + k] = 0.f;
          }
        }
      }
    }
  }
}

}  // namespace

void grad_accum_apply(float* g, float* a, int64_t n, int mode, float c, bool zero_g, hipStream_t s, int max_blocks) {
  if (n <= 0) return;
  const int64_t tiles = (n + kAccumBlockElems - 1) / kAccumBlockElems;
  const int cap = max_blocks < 1 ? 1 : (max_blocks > kAccumMaxBlocks ? kAccumMaxBlocks : max_blocks);
  const dim3 grid((unsigned)(tiles < cap ? tiles : cap)), block(kT);
  if (mode == 0) {
    if (zero_g) hipLaunchKernelGGL((k_grad_accum<0, true>), grid, block, 0, s, g, a, n, c);
    else hipLaunchKernelGGL((k_grad_accum<0, false>), grid, block, 0, s, g, a, n, c);
  } else if (mode == 1) {
    if (zero_g) hipLaunchKernelGGL((k_grad_accum<1, true>), grid, block, 0, s, g, a, n, c);
    else hipLaunchKernelGGL((k_grad_accum<1, false>), grid, block, 0, s, g, a, n, c);
  } else {
    hipLaunchKernelGGL((k_grad_accum<2, false>), grid, block, 0, s, g, a, n, c);
  }
}

}  // namespace tdl
