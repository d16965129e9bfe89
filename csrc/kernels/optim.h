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

}  // namespace tdl
