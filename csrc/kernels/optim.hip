// Flat-slab optimizer updates (see optim.h).  The formulas are those of keras/optimizers.py (Keras
// semantics, the ones the eager torch fallback applies), element for element in f32: one pass over
// the slab, 16-B vector accesses, every state tensor read and written once.  Adam's bias correction
// uses the step t = *t0 + t_add + 1: the host refreshes t0 before each execution and a captured
// graph bakes each step's offset t_add in, so no host sync per step and no device counter race.
#include <type_traits>

#include "common.h"
#include "optim.h"

// Gradient clipping (CLIP instantiations): every kernel applies GradClip (optim.h) to g where it loads it;
// the unclipped instantiations contain none of it and compute the bits they always did.
//
// Weight EMA (EMA instantiations, WeightEma in optim.h): the kernel loads e with its other operands and,
// where it stores w, stores the new average too (ema_store); on an overwrite step the average is what it
// stores as w.  The update itself is the same expression in both instantiations, so w (mode 1) and every
// slot carry the bits of the instantiation without EMA, which contains none of this.
namespace tdl {
namespace {

template <bool AMS, bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void k_adam(OptimArgs a) {
  const GradClip gc(CLIP ? a.gscale : nullptr, a.clipvalue, CLIP ? a.clip : 0);
  const int64_t i4 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const float lr = *a.lr;
  const float t = *a.t0 + (float)(a.t_add + 1);
  const float lr_t = lr * sqrtf(1.f - powf(a.b2, t)) / (1.f - powf(a.b1, t));
  const float decay = 1.f - lr * a.wd;
  auto one = [&](float& w, float g, float& m, float& v, float* vh) {
    if (a.wd != 0.f) w *= decay;
    m = m * a.b1 + g * (1.f - a.b1);
    v = v * a.b2 + g * g * (1.f - a.b2);
    float vv = v;
    if constexpr (AMS) {
      *vh = fmaxf(*vh, v);
      vv = *vh;
    }
    w = w - lr_t * m / (sqrtf(vv) + a.eps);
  };
  if (i4 + 3 < a.n) {
    f4 w = ld4(a.w + i4), m = ld4(a.s0 + i4), v = ld4(a.s1 + i4);
    const f4 g = grad_of<CLIP>(gc, ld4(a.g + i4));
    f4 vh = AMS ? ld4(a.s2 + i4) : zero4();
    f4 e = zero4();
    if constexpr (EMA) e = ld4(a.ema.e + i4);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float wk = w[k], mk = m[k], vk = v[k], hk = vh[k];
      one(wk, g[k], mk, vk, &hk);
      w[k] = wk;
      m[k] = mk;
      v[k] = vk;
      vh[k] = hk;
    }
    if constexpr (EMA) w = ema_store(a.ema, a.ema.e + i4, e, w);
    st4(a.w + i4, w);
    st4(a.s0 + i4, m);
    st4(a.s1 + i4, v);
    if constexpr (AMS) st4(a.s2 + i4, vh);
  } else {
    for (int64_t j = i4; j < a.n; ++j) {
      if constexpr (EMA) {
        const float e = a.ema.e[j];
        float w = a.w[j];
        one(w, grad_of<CLIP>(gc, a.g[j]), a.s0[j], a.s1[j], AMS ? a.s2 + j : nullptr);
        a.w[j] = ema_store(a.ema, a.ema.e + j, e, w);
      } else {
        one(a.w[j], grad_of<CLIP>(gc, a.g[j]), a.s0[j], a.s1[j], AMS ? a.s2 + j : nullptr);
      }
    }
  }
}

// One element of RMSprop with the roundings written out: the fused forms hipcc gives the kernel without EMA
// (rms = fma(rms, rho, g g (1 - rho)), denom = fma(-mg, mg, rms), every other product rounded on its own).
// In a sum of two products the compiler is free to fuse either one, and with the average's extra uses in the
// EMA instantiation it fused the other one: that instantiation calls this, and tests/test_ema_kernels_gpu.py
// holds it to the bits of the instantiation without EMA.
__device__ __forceinline__ float rmsprop_one(float w, float g, float& rms, float* mom, float* mg, float lr, float rho,
                                             float momentum, float eps) {
#pragma clang fp contract(off)
  const float gg = g * g, t = gg * (1.f - rho);
  rms = __builtin_fmaf(rms, rho, t);
  float denom = rms;
  if (mg != nullptr) {
    const float a = *mg * rho, b = g * (1.f - rho);
    *mg = a + b;
    denom = __builtin_fmaf(-*mg, *mg, rms);
  }
  const float step = g / (sqrtf(denom) + eps);
  const float ls = lr * step;
  if (mom != nullptr) {
    const float a = *mom * momentum;
    *mom = a + ls;
    return w - *mom;
  }
  return w - ls;
}

template <bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void k_rmsprop(OptimArgs a) {
  const GradClip gc(CLIP ? a.gscale : nullptr, a.clipvalue, CLIP ? a.clip : 0);
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const float lr = *a.lr;
  const bool mom = a.flags & 1, centered = a.flags & 2;
  for (int64_t j = i0; j < i0 + 4 && j < a.n; ++j) {
    const float g = grad_of<CLIP>(gc, a.g[j]);
    if constexpr (EMA) {
      const float e = a.ema.e[j];
      float rms = a.s0[j];
      const float w = rmsprop_one(a.w[j], g, rms, mom ? a.s1 + j : nullptr, centered ? a.s2 + j : nullptr, lr, a.b1,
                                  a.b2, a.eps);
      a.s0[j] = rms;
      a.w[j] = ema_store(a.ema, a.ema.e + j, e, w);
    } else {
      const float rms = a.s0[j] * a.b1 + g * g * (1.f - a.b1);
      a.s0[j] = rms;
      float denom = rms;
      if (centered) {
        const float mg = a.s2[j] * a.b1 + g * (1.f - a.b1);
        a.s2[j] = mg;
        denom = rms - mg * mg;
      }
      const float step = g / (sqrtf(denom) + a.eps);
      if (mom) {
        const float m = a.s1[j] * a.b2 + lr * step;
        a.s1[j] = m;
        a.w[j] -= m;
      } else {
        a.w[j] -= lr * step;
      }
    }
  }
}

template <bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void k_adagrad(OptimArgs a) {
  const GradClip gc(CLIP ? a.gscale : nullptr, a.clipvalue, CLIP ? a.clip : 0);
  const int64_t i4 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const float lr = *a.lr;
  if (i4 + 3 < a.n) {
    const f4 g = grad_of<CLIP>(gc, ld4(a.g + i4));
    const f4 acc = ld4(a.s0 + i4) + g * g;
    f4 w = ld4(a.w + i4);
    f4 e = zero4();
    if constexpr (EMA) e = ld4(a.ema.e + i4);
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = w[k] - lr * g[k] / (sqrtf(acc[k]) + a.eps);
    st4(a.s0 + i4, acc);
    if constexpr (EMA) w = ema_store(a.ema, a.ema.e + i4, e, w);
    st4(a.w + i4, w);
  } else {
    for (int64_t j = i4; j < a.n; ++j) {
      const float g = grad_of<CLIP>(gc, a.g[j]);
      const float acc = a.s0[j] + g * g;
      a.s0[j] = acc;
      if constexpr (EMA) {
        const float e = a.ema.e[j];
        const float w = a.w[j] - lr * g / (sqrtf(acc) + a.eps);
        a.w[j] = ema_store(a.ema, a.ema.e + j, e, w);
      } else {
        a.w[j] -= lr * g / (sqrtf(acc) + a.eps);
      }
    }
  }
}

inline dim3 grid_of(int64_t n) { return dim3((unsigned)(((n + 3) / 4 + 255) / 256)); }
inline bool clipped(const OptimArgs& a) { return a.gscale != nullptr || a.clip != 0; }

// k(std::bool_constant<CLIP>, std::bool_constant<EMA>) for the operands present
template <class F>
void with_clip_ema(const OptimArgs& a, F f) {
  const bool ema = a.ema.mode != 0;
  if (clipped(a))
    ema ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
  else
    ema ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

}  // namespace

void adam_apply(const OptimArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  with_clip_ema(a, [&](auto clip, auto ema) {
    constexpr bool C = decltype(clip)::value, E = decltype(ema)::value;
    if (a.flags & 1)
      hipLaunchKernelGGL((k_adam<true, C, E>), grid_of(a.n), dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL((k_adam<false, C, E>), grid_of(a.n), dim3(256), 0, s, a);
  });
}
void rmsprop_apply(const OptimArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  with_clip_ema(a, [&](auto clip, auto ema) {
    hipLaunchKernelGGL((k_rmsprop<decltype(clip)::value, decltype(ema)::value>), grid_of(a.n), dim3(256), 0, s, a);
  });
}
void adagrad_apply(const OptimArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  with_clip_ema(a, [&](auto clip, auto ema) {
    hipLaunchKernelGGL((k_adagrad<decltype(clip)::value, decltype(ema)::value>), grid_of(a.n), dim3(256), 0, s, a);
  });
}

}  // namespace tdl
