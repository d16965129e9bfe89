// Flat-slab optimizer updates for gfx950 (see optim.hip): Keras Adam / AdamW (+AMSGrad), RMSprop
// (+momentum, centered) and Adagrad over a whole parameter slab in ONE launch, learning rate and step
// counter read from device memory so a captured execution graph replays them correctly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include "common.h"
#endif

namespace tdl {

// The moving average of the weights (use_ema, keras/optimizers.py), kept by the kernel that stores the new
// weight: E = m * E + c * W_new, two products and a sum, three f32 roundings, never contracted (ema_fold).
// mode 0: off (e is null); 1: update E; 2: update E and store W = E_new (an overwrite step).  The mode of a
// step is known to the host at launch and at capture time: a launch argument, never a device counter.
struct WeightEma {
  float* e;
  float m, c;  // float32(ema_momentum), float32(1 - ema_momentum) with the subtraction done in f64 on the host
  int mode;
};

struct OptimArgs {
  float* w;
  const float* g;
  float* s0;          // Adam m / RMSprop rms / Adagrad accumulator
  float* s1;          // Adam v / RMSprop momentum (or null)
  float* s2;          // Adam vhat (AMSGrad) / RMSprop mean gradient (centered) (or null)
  const float* lr;    // device learning rate
  const float* t0;    // Adam: device step count of the execution's first step (float, exact to 2^24)
  int64_t n;
  float b1, b2, eps;  // Adam beta_1 / beta_2 / epsilon; RMSprop rho / momentum / epsilon
  float wd;           // AdamW decoupled weight decay (0: none)
  int t_add;          // Adam: this step's offset from t0 (the step's index inside a captured execution)
  int flags;          // Adam: 1 AMSGrad; RMSprop: 1 momentum, 2 centered
  // gradient clipping, applied where the kernel loads g: g' = clamp(g, +-clipvalue) * *gscale.  Either
  // operand may be absent (null / clip = 0); with both absent the kernel is the unclipped instantiation
  const float* gscale;  // device scale word written by clip_norm (or null)
  float clipvalue;      // clamp bound (read only when clip != 0)
  int clip;             // 1: clamp by clipvalue
  WeightEma ema;        // mode 0: none, and the kernel is the instantiation without it
};

#if defined(__HIPCC__)  // device code (the bindings include this header with the host compiler)
// The clip operands of one update kernel, resolved once per thread (see OptimArgs).  The clamp keeps a
// NaN (both comparisons are false), as Tensor.clamp_ does; min / max / med3 instructions would drop it.
struct GradClip {
  float cv, sc;
  __device__ __forceinline__ GradClip(const float* gscale, float clipvalue, int clip)
      : cv(clip ? clipvalue : __builtin_inff()), sc(gscale != nullptr ? *gscale : 1.f) {}
  __device__ __forceinline__ float operator()(float g) const {
    const float c = g > cv ? cv : (g < -cv ? -cv : g);
    return c * sc;
  }
};
// g as the update sees it (CLIP = false: g itself, no instruction added)
template <bool CLIP>
__device__ __forceinline__ float grad_of(const GradClip& c, float g) {
  if constexpr (CLIP) return c(g);
  return g;
}
template <bool CLIP>
__device__ __forceinline__ f4 grad_of(const GradClip& c, f4 g) {
  if constexpr (CLIP) return f4{c(g[0]), c(g[1]), c(g[2]), c(g[3])};
  return g;
}
// The new average of one element.  Contraction is off for exactly this expression: the update formulas
// around a call keep the fused forms hipcc gives them.
__device__ __forceinline__ float ema_fold(const WeightEma& x, float e, float w) {
#pragma clang fp contract(off)
  const float me = x.m * e, cw = x.c * w;
  return me + cw;
}
__device__ __forceinline__ f4 ema_fold(const WeightEma& x, f4 e, f4 w) {
  return f4{ema_fold(x, e[0], w[0]), ema_fold(x, e[1], w[1]), ema_fold(x, e[2], w[2]), ema_fold(x, e[3], w[3])};
}
// Where an EMA instantiation stores w: e becomes the new average and is stored at pe; on an overwrite step
// the caller then stores the returned value, e's, as the weight.
__device__ __forceinline__ f4 ema_store(const WeightEma& x, float* pe, f4 e, f4 w) {
  e = ema_fold(x, e, w);
  st4(pe, e);
  return x.mode == 2 ? e : w;
}
__device__ __forceinline__ float ema_store(const WeightEma& x, float* pe, float e, float w) {
  e = ema_fold(x, e, w);
  *pe = e;
  return x.mode == 2 ? e : w;
}
#endif

void adam_apply(const OptimArgs& a, hipStream_t s);
void rmsprop_apply(const OptimArgs& a, hipStream_t s);
void adagrad_apply(const OptimArgs& a, hipStream_t s);

// Global-norm clip over a flat f32 slab in two launches (clip.hip): k_clip_partials leaves the f64 sum
// of clamp(g)^2 of each kClipChunk-element range in partials[p]; k_clip_scale adds them in a fixed order
// and writes out[0] = scale = min(1, clipnorm / (norm + 1e-12)) and out[1] = norm, both f32.  The order
// of every addition depends on n alone: the words are bit-identical from run to run, at any buffer
// address and on every replica.  A NaN norm gives a NaN scale, an infinite norm scale 0.  n == 0: only
// k_clip_scale runs and writes norm 0, scale 1.
constexpr int kClipChunk = 8192;       // elements per k_clip_partials workgroup (why: see clip.hip)
constexpr int kClipScaleThreads = 256;  // k_clip_scale's single workgroup
inline int64_t clip_partials_count(int64_t n, int64_t chunk = kClipChunk) { return (n + chunk - 1) / chunk; }
// clamp: the norm is that of clamp(g, +-clipvalue).  chunk: kClipChunk, or one of the measured
// candidates 2048 / 4096 / 16384 (scripts/bench_clip.py; partials then needs clip_partials_count(n, chunk))
void clip_norm_apply(const float* g, double* partials, float* out, int64_t n, float clipnorm, bool clamp,
                     float clipvalue, hipStream_t s, int chunk = kClipChunk);

// Layer-wise adaptive updates (layerwise.hip): LARS and LAMB, whose step depends on two norms of each
// element's own variable, in three launches over the slab -- chunk sums, per-variable trust ratios, update.
//
// Layer tables (built and validated on the host, bindings.cpp layer_tables): chunks[C][4] = (start, len,
// var, 0) with every chunk inside one variable, 1 <= len <= kLayerChunk, start % 4 == 0, a variable's
// chunks consecutive and ascending; first_chunk[V + 1]; per variable wd[V] (f32) and adapt[V] (int32).
// kLayerChunk is a compile-time constant, never derived from the device or the grid: the order of the
// sums hangs on it.  Measured candidates (profiles/layerwise_cost.txt, us for the three launches): at
// ResNet-50's 25.6 M parameters 2048 / 4096 / 8192 tie (LARS 112 / 111 / 112, LAMB 185 / 190 / 187: the bytes
// decide); at the reference CNN's 225 k LARS ties at 9.9 (three launch latencies) and LAMB takes 10.2 / 12.0 /
// 15.7: 8192 leaves 34 workgroups of one wave per SIMD, each with 32 elements of divide / sqrt latency per
// thread and nothing to hide it behind.  kClipChunk's 8192 suits a kernel that only squares and adds.
constexpr int kLayerChunk = 2048;
struct LayerArgs {
  float* w;
  const float* g;       // (k_lamb_apply does not read it)
  float* s0;            // LARS momentum / LAMB m
  float* s1;            // LAMB v
  const int* chunks;
  const int* first_chunk;
  const float* wd;
  const int* adapt;
  double* partials;     // [C][2]: chunk sums of w^2 and of g'^2 (LARS) / u^2 (LAMB)
  float* ratio;         // [V]
  float* norms;         // [V][2]: |w_i| and |g'_i| / |u_i|
  const float* lr;      // device learning rate
  const float* t0;      // LAMB: device step count of the execution's first step (see OptimArgs)
  int t_add;
  int V, C;
  int chunk;            // the tables' chunk size: kLayerChunk, or a measured candidate (4096 / 8192)
  float b1, b2, eps;    // LAMB beta_1 / beta_2 / epsilon; LARS momentum / - / epsilon
  float lb1, lb2;       // LAMB: log beta_1, log beta_2 (taken in f64 on the host)
  float eeta;           // LARS trust coefficient
  int nesterov;
  const float* gscale;  // gradient clipping, as in OptimArgs
  float clipvalue;
  int clip;
  WeightEma ema;        // the moving average, as in OptimArgs (read by the apply kernels, launch 3)
};
void layer_sums_apply(const LayerArgs& a, bool lamb, hipStream_t s);   // launch 1
void layer_ratio_apply(const LayerArgs& a, bool lamb, hipStream_t s);  // launch 2
void lars_apply(const LayerArgs& a, hipStream_t s);                    // launch 3
void lamb_apply(const LayerArgs& a, hipStream_t s);

}  // namespace tdl
