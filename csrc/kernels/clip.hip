// Global-norm gradient clipping over the flat gradient slab (see optim.h): the norm in two launches,
// the clip itself inside the optimizer kernels (GradClip), so G is read once more and never rewritten.
//
// The sum of squares is taken in f64: an f32 x f32 product is exact in f64, and the accumulation of up
// to 2^25 such terms has a relative error below 2^-28, far under the f32 rounding of the result.  It is
// also taken in a FIXED order that depends on n alone -- workgroup p owns elements [p CH, (p + 1) CH),
// a thread adds its elements in index order, lanes / waves / partials combine in fixed trees -- so the
// norm has the same bits on every run, at every buffer address and on every replica (the replicas hold
// bit-identical all-reduced gradients), like the BN sums and the split-K reductions of this library.
//
// CH (kClipChunk) is a compile-time constant, never derived from the device or the grid: changing it
// changes the order.  Measured candidates (profiles/clip_cost.txt, us for both launches): at the reference
// CNN's slab (225 k floats) 2048 / 4096 / 8192 tie at 5.6 (launch latency; 16384 leaves 14 workgroups and
// takes 6.9); at ResNet-50's (25.6 M floats) 29.4 / 23.7 / 21.0 / 21.2 for 2048 / 4096 / 8192 / 16384
// against a floor of 16.5-19.7 (one read of G at the 5.2-6.2 TB/s of the BN passes).  8192 = 8 16-B loads
// in flight per thread and 3125 workgroups for the 256 CUs; 16384 gains nothing more and costs registers
// (72 VGPRs, 7 waves/SIMD instead of 8).
#include "common.h"
#include "optim.h"

namespace tdl {
namespace {

constexpr int kT = 256;  // threads of a k_clip_partials workgroup

__device__ __forceinline__ double wave_sum_f64(double v) {
  // xor butterfly: both partners add the same two values, so every lane ends with the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float clampf_keep_nan(float g, float cv) { return g > cv ? cv : (g < -cv ? -cv : g); }

template <int CH>
__global__ __launch_bounds__(kT) void k_clip_partials(const float* __restrict__ g, double* __restrict__ partials,
                                                       int64_t n, float cv) {
  static_assert(CH % (kT * 4) == 0, "a workgroup sweeps its range in whole rows of 16-B loads");
  constexpr int U = CH / (kT * 4);  // 16-B loads per thread, all issued before the first use
  const int64_t base = (int64_t)blockIdx.x * CH;
  const int tid = threadIdx.x;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (base + CH <= n) {
    f4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = ld4(g + base + ((int64_t)u * kT + tid) * 4);
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double x = (double)clampf_keep_nan(v[u][k], cv);
        acc[k] += x * x;
      }
    }
  } else {  // the slab's last workgroup: whole vectors while they fit, then a scalar tail
#pragma unroll 1
    for (int u = 0; u < U; ++u) {
      const int64_t i4 = base + ((int64_t)u * kT + tid) * 4;
      if (i4 + 3 < n) {
        const f4 v = ld4(g + i4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double x = (double)clampf_keep_nan(v[k], cv);
          acc[k] += x * x;
        }
      } else {
        for (int k = 0; k < 4 && i4 + k < n; ++k) {
          const double x = (double)clampf_keep_nan(g[i4 + k], cv);
          acc[k] += x * x;
        }
      }
    }
  }
  const double lane = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  const double wave = wave_sum_f64(lane);
  __shared__ double sw[kT / 64];
  if ((tid & 63) == 0) sw[tid >> 6] = wave;
  __syncthreads();
  if (tid == 0) partials[blockIdx.x] = (sw[0] + sw[1]) + (sw[2] + sw[3]);
}

__global__ __launch_bounds__(kClipScaleThreads) void k_clip_scale(const double* __restrict__ partials, int64_t P,
                                                                  float clipnorm, float* __restrict__ out) {
  constexpr int T = kClipScaleThreads;
  __shared__ double s[T];
  const int t = threadIdx.x;
  double a = 0.0;
  for (int64_t i = t; i < P; i += T) a += partials[i];
  s[t] = a;
  __syncthreads();
#pragma unroll
  for (int h = T / 2; h > 0; h >>= 1) {
    if (t < h) s[t] += s[t + h];
    __syncthreads();
  }
  if (t == 0) {
    const float norm = (float)sqrt(s[0]);
    const float r = clipnorm / (norm + 1e-12f);
    // min(r, 1) that keeps a NaN (a NaN norm must poison the update: TerminateOnNaN sees it);
    // an infinite norm gives r = 0
    out[0] = r >= 1.f ? 1.f : r;
    out[1] = norm;
  }
}

}  // namespace

void clip_norm_apply(const float* g, double* partials, float* out, int64_t n, float clipnorm, bool clamp,
                     float clipvalue, hipStream_t s, int chunk) {
  const float cv = clamp ? clipvalue : __builtin_inff();
  const int64_t P = n > 0 ? clip_partials_count(n, chunk) : 0;
  if (P > 0) {
    const dim3 grid((unsigned)P);
    switch (chunk) {
      case 2048: hipLaunchKernelGGL(k_clip_partials<2048>, grid, dim3(kT), 0, s, g, partials, n, cv); break;
      case 4096: hipLaunchKernelGGL(k_clip_partials<4096>, grid, dim3(kT), 0, s, g, partials, n, cv); break;
      case 16384: hipLaunchKernelGGL(k_clip_partials<16384>, grid, dim3(kT), 0, s, g, partials, n, cv); break;
      default: hipLaunchKernelGGL(k_clip_partials<kClipChunk>, grid, dim3(kT), 0, s, g, partials, n, cv); break;
    }
  }
  hipLaunchKernelGGL(k_clip_scale, dim3(1), dim3(kClipScaleThreads), 0, s, partials, P, clipnorm, out);
}

}  // namespace tdl
