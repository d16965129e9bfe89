// Layer-wise adaptive optimizers over the flat slab (see optim.h): LARS and LAMB in three launches per step,
// whatever the number of variables.  The step of every element depends on two norms of its own variable
// (|w_i| and |g'_i| for LARS, |w_i| and |u_i| for LAMB), so the slab is cut into CHUNKS that never cross a
// variable (layer tables, built and validated once on the host: optim.h) and
//
//   1. k_layer_sums   one workgroup per chunk: the f64 sums of squares of the chunk (LAMB also updates m, v
//                     in place and sums the update u it evaluates from them) -> partials[c][0..1]
//   2. k_layer_ratio  one wave per variable: adds the variable's chunk sums, takes the square roots and forms
//                     the trust ratio in f64, rounds once -> ratio[v], norms[v][0..1]
//   3. k_*_apply      one workgroup per chunk: the update with s = lr * ratio[var]
//
// No workgroup waits on another and there are no atomics: a kernel boundary costs 1.6 us here, a grid
// barrier 4.8-7.2 us, and co-residency is not guaranteed on a shared GPU.
//
// Order.  As in clip.hip the sums are f64 sums of exact products (LARS) taken in a FIXED order: a thread adds
// its elements in index order, lanes combine by the xor butterfly, waves and then a variable's chunks by
// fixed trees.  Every one of these depends on the layout alone (kLayerChunk is a compile-time constant), so
// partials, ratios and norms have the same bits on every run, at every buffer address and on every replica.
//
// LAMB's u is ONE function (lamb_u, contraction off) used by launch 1 (for the norm) and launch 3 (for the
// step, from the m and v that launch 1 wrote): the recomputation has the same bits, and g is not loaded again.
//
// Only variable elements are read or written: the alignment padding between variables is never touched.
// Traffic per element: LAMB 24 B + 16 B = 40 B (Adam: 28 B), LARS 8 B + 20 B = 28 B (momentum SGD: 20 B).
#include <type_traits>

#include "common.h"
#include "optim.h"

namespace tdl {
namespace {

constexpr int kT = 256;  // threads of a per-chunk workgroup
// (the per-chunk kernels are templates on the chunk size CH only so that scripts/bench_layerwise.py can measure
// the candidates behind kLayerChunk; the optimizers always run CH = kLayerChunk)

__device__ __forceinline__ double wave_sum_f64(double v) {
  // xor butterfly: both partners add the same two values, so every lane ends with the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the chunk's two sums: lanes, then waves, in fixed trees; thread 0 writes them
__device__ __forceinline__ void block_sums_to(double a, double b, double* __restrict__ out) {
  a = wave_sum_f64(a);
  b = wave_sum_f64(b);
  __shared__ double sw[2][kT / 64];
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) {
    sw[0][tid >> 6] = a;
    sw[1][tid >> 6] = b;
  }
  __syncthreads();
  if (tid == 0) {
    out[0] = (sw[0][0] + sw[0][1]) + (sw[0][2] + sw[0][3]);
    out[1] = (sw[1][0] + sw[1][1]) + (sw[1][2] + sw[1][3]);
  }
}

// Adam's bias corrections at step t = *t0 + t_add + 1 (the step as k_adam takes it), as -expm1(t log beta)
// with log beta taken in f64 on the host: the plain f32 form 1 - beta^t cancels (1 - 0.999^2 keeps 9 of its 24
// bits), and that error would go straight into |u_i| and the trust ratio of every variable; an f64 pow per
// thread costs about a microsecond of latency at the reference CNN's size.  Once per thread, not per element.
struct LambCorr {
  float c1, c2;
  __device__ __forceinline__ LambCorr(const LayerArgs& a) {
    const float t = *a.t0 + (float)(a.t_add + 1);
    c1 = -expm1f(t * a.lb1);
    c2 = -expm1f(t * a.lb2);
  }
};

// u = m^ / (sqrt(v^) + eps) + wd w: every operation rounded on its own (no contraction), so launch 3
// recomputes the bits that launch 1 summed
__device__ __forceinline__ float lamb_u(float m, float v, float w, const LambCorr& c, float eps, float wd) {
#pragma clang fp contract(off)
  const float q = (m / c.c1) / (sqrtf(v / c.c2) + eps);
  const float dw = wd * w;
  return q + dw;
}

// (contraction off here too: the vector body and the scalar tail of a chunk must round alike)
__device__ __forceinline__ void lamb_moments(float& m, float& v, float g, float b1, float b2) {
#pragma clang fp contract(off)
  const float mg = g * (1.f - b1), vg = g * g * (1.f - b2);
  m = m * b1 + mg;
  v = v * b2 + vg;
}

__device__ __forceinline__ float lamb_step(float w, float s, float u) { return __builtin_fmaf(-s, u, w); }

// One element of LARS: k_sgd_momentum's roundings (the fused forms hipcc gives its 16-B body: s d rounded,
// then fma(mu, v, -s d), for Nesterov once more on the new v) with lr -> s and g -> d = g' + wd w, written
// out so that the body and the tail of a chunk, and any later compiler, round alike.
__device__ __forceinline__ void lars_one(float& w, float& v, float g, float wd, float mu, float s, int nesterov) {
#pragma clang fp contract(off)
  float d = g;
  if (wd != 0.f) {
    const float dw = wd * w;
    d = g + dw;
  }
  const float sd = s * d;
  v = __builtin_fmaf(mu, v, -sd);
  w = w + (nesterov ? __builtin_fmaf(mu, v, -sd) : v);
}

struct Chunk {
  int64_t start;
  int len, var;
  __device__ __forceinline__ Chunk(const int* __restrict__ chunks) {
    const int4 c = *reinterpret_cast<const int4*>(chunks + (int64_t)blockIdx.x * 4);
    start = c.x;
    len = c.y;
    var = c.z;
  }
};

// ---------------------------------------------------------------------------------------- launch 1
template <int CH, bool CLIP>
__global__ __launch_bounds__(kT) void k_layer_sums_lars(LayerArgs a) {
  static_assert(CH % (kT * 4) == 0, "a workgroup sweeps a full chunk in whole rows of 16-B accesses");
  constexpr int kU = CH / (kT * 4);  // 16-B accesses per thread and operand in a full chunk
  const GradClip gc(CLIP ? a.gscale : nullptr, a.clipvalue, CLIP ? a.clip : 0);
  const Chunk c(a.chunks);
  const float* __restrict__ w = a.w + c.start;
  const float* __restrict__ g = a.g + c.start;
  const int tid = threadIdx.x;
  double aw[4] = {0.0, 0.0, 0.0, 0.0}, ag[4] = {0.0, 0.0, 0.0, 0.0};
  if (c.len == CH) {
    f4 wv[kU], gv[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) wv[u] = ld4(w + (u * kT + tid) * 4);
#pragma unroll
    for (int u = 0; u < kU; ++u) gv[u] = ld4(g + (u * kT + tid) * 4);
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const f4 gg = grad_of<CLIP>(gc, gv[u]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double x = (double)wv[u][k], y = (double)gg[k];
        aw[k] += x * x;
        ag[k] += y * y;
      }
    }
  } else {  // a variable's last chunk: whole vectors while they fit, then a scalar tail
#pragma unroll 1
    for (int u = 0; u < kU; ++u) {
      const int i4 = (u * kT + tid) * 4;
      if (i4 + 3 < c.len) {
        const f4 wv = ld4(w + i4);
        const f4 gg = grad_of<CLIP>(gc, ld4(g + i4));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double x = (double)wv[k], y = (double)gg[k];
          aw[k] += x * x;
          ag[k] += y * y;
        }
      } else {
        for (int k = 0; k < 4 && i4 + k < c.len; ++k) {
          const double x = (double)w[i4 + k], y = (double)grad_of<CLIP>(gc, g[i4 + k]);
          aw[k] += x * x;
          ag[k] += y * y;
        }
      }
    }
  }
  block_sums_to((aw[0] + aw[1]) + (aw[2] + aw[3]), (ag[0] + ag[1]) + (ag[2] + ag[3]),
                a.partials + (int64_t)blockIdx.x * 2);
}

template <int CH, bool CLIP>
__global__ __launch_bounds__(kT) void k_layer_sums_lamb(LayerArgs a) {
  static_assert(CH % (kT * 4) == 0, "whole rows of 16-B accesses");
  constexpr int kU = CH / (kT * 4);
  const GradClip gc(CLIP ? a.gscale : nullptr, a.clipvalue, CLIP ? a.clip : 0);
  const Chunk c(a.chunks);
  const LambCorr corr(a);
  const float wd = a.wd[c.var];
  const float* __restrict__ w = a.w + c.start;
  const float* __restrict__ g = a.g + c.start;
  float* __restrict__ m = a.s0 + c.start;
  float* __restrict__ v = a.s1 + c.start;
  const int tid = threadIdx.x;
  double aw[4] = {0.0, 0.0, 0.0, 0.0}, au[4] = {0.0, 0.0, 0.0, 0.0};
  auto one = [&](float wk, float gk, float& mk, float& vk, int k) {
    lamb_moments(mk, vk, gk, a.b1, a.b2);
    const double x = (double)wk, y = (double)lamb_u(mk, vk, wk, corr, a.eps, wd);
    aw[k] += x * x;
    au[k] += y * y;
  };
  if (c.len == CH) {
    // four operands: two halves of kU / 2 rows, every load of a half issued before its first use
    constexpr int NH = kU >= 2 ? 2 : 1, H = kU / NH;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      f4 wv[H], gv[H], mv[H], vv[H];
#pragma unroll
      for (int u = 0; u < H; ++u) wv[u] = ld4(w + ((h * H + u) * kT + tid) * 4);
#pragma unroll
      for (int u = 0; u < H; ++u) gv[u] = ld4(g + ((h * H + u) * kT + tid) * 4);
#pragma unroll
      for (int u = 0; u < H; ++u) mv[u] = ld4(m + ((h * H + u) * kT + tid) * 4);
#pragma unroll
      for (int u = 0; u < H; ++u) vv[u] = ld4(v + ((h * H + u) * kT + tid) * 4);
#pragma unroll
      for (int u = 0; u < H; ++u) {
        const f4 gg = grad_of<CLIP>(gc, gv[u]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float mk = mv[u][k], vk = vv[u][k];
          one(wv[u][k], gg[k], mk, vk, k);
          mv[u][k] = mk;
          vv[u][k] = vk;
        }
        st4(m + ((h * H + u) * kT + tid) * 4, mv[u]);
        st4(v + ((h * H + u) * kT + tid) * 4, vv[u]);
      }
    }
  } else {
#pragma unroll 1
    for (int u = 0; u < kU; ++u) {
      const int i4 = (u * kT + tid) * 4;
      if (i4 + 3 < c.len) {
        const f4 wv = ld4(w + i4);
        const f4 gg = grad_of<CLIP>(gc, ld4(g + i4));
        f4 mv = ld4(m + i4), vv = ld4(v + i4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float mk = mv[k], vk = vv[k];
          one(wv[k], gg[k], mk, vk, k);
          mv[k] = mk;
          vv[k] = vk;
        }
        st4(m + i4, mv);
        st4(v + i4, vv);
      } else {
        for (int k = 0; k < 4 && i4 + k < c.len; ++k) {
          float mk = m[i4 + k], vk = v[i4 + k];
          one(w[i4 + k], grad_of<CLIP>(gc, g[i4 + k]), mk, vk, k);
          m[i4 + k] = mk;
          v[i4 + k] = vk;
        }
      }
    }
  }
  block_sums_to((aw[0] + aw[1]) + (aw[2] + aw[3]), (au[0] + au[1]) + (au[2] + au[3]),
                a.partials + (int64_t)blockIdx.x * 2);
}

// ---------------------------------------------------------------------------------------- launch 2
// One wave per variable: lane l adds chunk sums l, l + 64, ... of the variable in that order, the lanes
// combine by the xor butterfly.  Square roots and the ratio in f64 from the f64 sums, the constants as
// the f32 values passed, widened; one rounding to f32.  A comparison with a NaN norm is false: ratio 1.
template <bool LAMB>
__global__ __launch_bounds__(64) void k_layer_ratio(LayerArgs a) {
  const int var = blockIdx.x;
  const int c0 = a.first_chunk[var], c1 = a.first_chunk[var + 1];
  double s0 = 0.0, s1 = 0.0;
  for (int c = c0 + (int)threadIdx.x; c < c1; c += 64) {
    s0 += a.partials[(int64_t)c * 2];
    s1 += a.partials[(int64_t)c * 2 + 1];
  }
  s0 = wave_sum_f64(s0);
  s1 = wave_sum_f64(s1);
  if (threadIdx.x == 0) {
    const double nw = sqrt(s0), nx = sqrt(s1);
    double r = 1.0;
    if (a.adapt[var] != 0 && nw > 0.0 && nx > 0.0) {
      if constexpr (LAMB)
        r = nw / nx;
      else
        r = (double)a.eeta * nw / (nx + (double)a.wd[var] * nw + (double)a.eps);
    }
    a.ratio[var] = (float)r;
    a.norms[var * 2] = (float)nw;
    a.norms[var * 2 + 1] = (float)nx;
  }
}

// ---------------------------------------------------------------------------------------- launch 3
// LARS: momentum SGD (lars_one) with lr -> s = lr * ratio[var], g -> d = g' + wd w
// EMA (both apply kernels): the moving average of the weights (WeightEma, optim.h) is loaded with the other
// operands and stored where w is; on an overwrite step it is what is stored as w.  Elements between two
// variables (the layout's alignment gaps) belong to no chunk: neither w nor e of them is touched.
template <int CH, bool CLIP, bool EMA>
__global__ __launch_bounds__(kT) void k_lars_apply(LayerArgs a) {
  constexpr int kU = CH / (kT * 4);
  const GradClip gc(CLIP ? a.gscale : nullptr, a.clipvalue, CLIP ? a.clip : 0);
  const Chunk c(a.chunks);
  const float lr = *a.lr;
  const float s = lr * a.ratio[c.var];
  const float wd = a.wd[c.var];
  const float mu = a.b1;
  const int nesterov = a.nesterov;
  float* __restrict__ w = a.w + c.start;
  const float* __restrict__ g = a.g + c.start;
  float* __restrict__ v = a.s0 + c.start;
  float* __restrict__ e = EMA ? a.ema.e + c.start : nullptr;
  const int tid = threadIdx.x;
  if (c.len == CH) {
    f4 wv[kU], gv[kU], vv[kU], ev[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) wv[u] = ld4(w + (u * kT + tid) * 4);
#pragma unroll
    for (int u = 0; u < kU; ++u) gv[u] = ld4(g + (u * kT + tid) * 4);
#pragma unroll
    for (int u = 0; u < kU; ++u) vv[u] = ld4(v + (u * kT + tid) * 4);
    if constexpr (EMA) {
#pragma unroll
      for (int u = 0; u < kU; ++u) ev[u] = ld4(e + (u * kT + tid) * 4);
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const f4 gg = grad_of<CLIP>(gc, gv[u]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float wk = wv[u][k], vk = vv[u][k];
        lars_one(wk, vk, gg[k], wd, mu, s, nesterov);
        wv[u][k] = wk;
        vv[u][k] = vk;
      }
      if constexpr (EMA) wv[u] = ema_store(a.ema, e + (u * kT + tid) * 4, ev[u], wv[u]);
      st4(w + (u * kT + tid) * 4, wv[u]);
      st4(v + (u * kT + tid) * 4, vv[u]);
    }
  } else {
#pragma unroll 1
    for (int u = 0; u < kU; ++u) {
      const int i4 = (u * kT + tid) * 4;
      if (i4 + 3 < c.len) {
        f4 wv = ld4(w + i4), vv = ld4(v + i4);
        const f4 gg = grad_of<CLIP>(gc, ld4(g + i4));
        f4 ev = zero4();
        if constexpr (EMA) ev = ld4(e + i4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float wk = wv[k], vk = vv[k];
          lars_one(wk, vk, gg[k], wd, mu, s, nesterov);
          wv[k] = wk;
          vv[k] = vk;
        }
        if constexpr (EMA) wv = ema_store(a.ema, e + i4, ev, wv);
        st4(w + i4, wv);
        st4(v + i4, vv);
      } else {
        for (int j = i4; j < c.len; ++j) {
          float wj = w[j], vj = v[j];
          float ej = 0.f;
          if constexpr (EMA) ej = e[j];
          lars_one(wj, vj, grad_of<CLIP>(gc, g[j]), wd, mu, s, nesterov);
          v[j] = vj;
          if constexpr (EMA) wj = ema_store(a.ema, e + j, ej, wj);
          w[j] = wj;
        }
      }
    }
  }
}

// LAMB: w -= s u, u re-evaluated from the m, v of launch 1 (g is not loaded)
template <int CH, bool EMA>
__global__ __launch_bounds__(kT) void k_lamb_apply(LayerArgs a) {
  constexpr int kU = CH / (kT * 4);
  const Chunk c(a.chunks);
  const LambCorr corr(a);
  const float lr = *a.lr;
  const float s = lr * a.ratio[c.var];
  const float wd = a.wd[c.var];
  float* __restrict__ w = a.w + c.start;
  const float* __restrict__ m = a.s0 + c.start;
  const float* __restrict__ v = a.s1 + c.start;
  float* __restrict__ e = EMA ? a.ema.e + c.start : nullptr;
  const int tid = threadIdx.x;
  if (c.len == CH) {
    f4 wv[kU], mv[kU], vv[kU], ev[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) wv[u] = ld4(w + (u * kT + tid) * 4);
#pragma unroll
    for (int u = 0; u < kU; ++u) mv[u] = ld4(m + (u * kT + tid) * 4);
#pragma unroll
    for (int u = 0; u < kU; ++u) vv[u] = ld4(v + (u * kT + tid) * 4);
    if constexpr (EMA) {
#pragma unroll
      for (int u = 0; u < kU; ++u) ev[u] = ld4(e + (u * kT + tid) * 4);
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
#pragma unroll
      for (int k = 0; k < 4; ++k) wv[u][k] = lamb_step(wv[u][k], s, lamb_u(mv[u][k], vv[u][k], wv[u][k], corr, a.eps, wd));
      if constexpr (EMA) wv[u] = ema_store(a.ema, e + (u * kT + tid) * 4, ev[u], wv[u]);
      st4(w + (u * kT + tid) * 4, wv[u]);
    }
  } else {
#pragma unroll 1
    for (int u = 0; u < kU; ++u) {
      const int i4 = (u * kT + tid) * 4;
      if (i4 + 3 < c.len) {
        f4 wv = ld4(w + i4);
        const f4 mv = ld4(m + i4), vv = ld4(v + i4);
        f4 ev = zero4();
        if constexpr (EMA) ev = ld4(e + i4);
#pragma unroll
        for (int k = 0; k < 4; ++k) wv[k] = lamb_step(wv[k], s, lamb_u(mv[k], vv[k], wv[k], corr, a.eps, wd));
        if constexpr (EMA) wv = ema_store(a.ema, e + i4, ev, wv);
        st4(w + i4, wv);
      } else {
        for (int j = i4; j < c.len; ++j) {
          float ej = 0.f;
          if constexpr (EMA) ej = e[j];
          float wj = lamb_step(w[j], s, lamb_u(m[j], v[j], w[j], corr, a.eps, wd));
          if constexpr (EMA) wj = ema_store(a.ema, e + j, ej, wj);
          w[j] = wj;
        }
      }
    }
  }
}

inline bool clipped(const LayerArgs& a) { return a.gscale != nullptr || a.clip != 0; }

// k(std::integral_constant<int, CH>) for the tables' chunk size
template <class F>
void with_chunk(int chunk, F f) {
  switch (chunk) {
    case 4096: f(std::integral_constant<int, 4096>{}); break;
    case 8192: f(std::integral_constant<int, 8192>{}); break;
    default: f(std::integral_constant<int, kLayerChunk>{}); break;
  }
}

}  // namespace

void layer_sums_apply(const LayerArgs& a, bool lamb, hipStream_t s) {
  if (a.C <= 0) return;
  const dim3 grid((unsigned)a.C), block(kT);
  with_chunk(a.chunk, [&](auto ch) {
    constexpr int CH = decltype(ch)::value;
    if (lamb) {
      if (clipped(a)) hipLaunchKernelGGL((k_layer_sums_lamb<CH, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((k_layer_sums_lamb<CH, false>), grid, block, 0, s, a);
    } else {
      if (clipped(a)) hipLaunchKernelGGL((k_layer_sums_lars<CH, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((k_layer_sums_lars<CH, false>), grid, block, 0, s, a);
    }
  });
}

void layer_ratio_apply(const LayerArgs& a, bool lamb, hipStream_t s) {
  if (a.V <= 0) return;
  if (lamb)
    hipLaunchKernelGGL(k_layer_ratio<true>, dim3((unsigned)a.V), dim3(64), 0, s, a);
  else
    hipLaunchKernelGGL(k_layer_ratio<false>, dim3((unsigned)a.V), dim3(64), 0, s, a);
}

void lars_apply(const LayerArgs& a, hipStream_t s) {
  if (a.C <= 0) return;
  const dim3 grid((unsigned)a.C), block(kT);
  with_chunk(a.chunk, [&](auto ch) {
    constexpr int CH = decltype(ch)::value;
    if (a.ema.mode != 0) {
      if (clipped(a)) hipLaunchKernelGGL((k_lars_apply<CH, true, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((k_lars_apply<CH, false, true>), grid, block, 0, s, a);
    } else {
      if (clipped(a)) hipLaunchKernelGGL((k_lars_apply<CH, true, false>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((k_lars_apply<CH, false, false>), grid, block, 0, s, a);
    }
  });
}

void lamb_apply(const LayerArgs& a, hipStream_t s) {
  if (a.C <= 0) return;
  const dim3 grid((unsigned)a.C), block(kT);
  with_chunk(a.chunk, [&](auto ch) {
    constexpr int CH = decltype(ch)::value;
    if (a.ema.mode != 0) hipLaunchKernelGGL((k_lamb_apply<CH, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_lamb_apply<CH, false>), grid, block, 0, s, a);
  });
}

}  // namespace tdl
