// Layer / RMS normalisation kernels (layernorm.h): a row lives in the registers of its L lanes, every sum
// is f64 and taken in the order layernorm.h describes.
#include "common.h"
#include "layernorm.h"

namespace tdl {
namespace {

constexpr int kT = kLnThreads;

typedef unsigned u4 __attribute__((ext_vector_type(4)));

// one access of V elements of T: a 16-byte vector (V = 4 f32 / 8 bf16) or a single element
template <typename T, int V>
struct Io;
template <>
struct Io<float, 4> {
  static __device__ __forceinline__ void ld(const float* p, float* v) {
    const f4 r = ld4(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = r[k];
  }
  static __device__ __forceinline__ void st(float* p, const float* v) { st4(p, f4{v[0], v[1], v[2], v[3]}); }
};
template <>
struct Io<float, 1> {
  static __device__ __forceinline__ void ld(const float* p, float* v) { v[0] = *p; }
  static __device__ __forceinline__ void st(float* p, const float* v) { *p = v[0]; }
};
template <>
struct Io<uint16_t, 8> {
  static __device__ __forceinline__ void ld(const uint16_t* p, float* v) {
    const u4 r = *reinterpret_cast<const u4*>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[2 * k] = __uint_as_float(r[k] << 16);
      v[2 * k + 1] = __uint_as_float(r[k] & 0xffff0000u);
    }
  }
  static __device__ __forceinline__ void st(uint16_t* p, const float* v) {
    *reinterpret_cast<u4*>(p) = u4{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                                   pack_bf16x2(v[6], v[7])};
  }
};
template <>
struct Io<uint16_t, 1> {
  static __device__ __forceinline__ void ld(const uint16_t* p, float* v) {
    v[0] = __uint_as_float((unsigned)*p << 16);
  }
  static __device__ __forceinline__ void st(uint16_t* p, const float* v) {
    *p = (uint16_t)(pack_bf16x2(v[0], 0.f) & 0xffffu);
  }
};

// V consecutive f32 parameters (gamma / beta; 16-byte aligned at a vector column when V > 1)
template <int V>
__device__ __forceinline__ void ld_param(const float* p, float* v) {
  if constexpr (V == 1) {
    v[0] = *p;
  } else {
#pragma unroll
    for (int q = 0; q < V / 4; ++q) {
      const f4 r = ld4(p + 4 * q);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[4 * q + k] = r[k];
    }
  }
}

template <int PLAN>
struct Geo {
  static constexpr int EPT = PLAN == kLnSub ? kLnEptSub : kLnEpt;
  static constexpr bool WG = PLAN == kLnGroup;
};

// where a thread works: lane lr of row group rg; a row group is L consecutive lanes (the workgroup in kLnGroup)
struct Lane {
  int lr, rg;
};
template <bool WG>
__device__ __forceinline__ Lane lane_of(int L) {
  const int tid = threadIdx.x;
  return WG ? Lane{tid, 0} : Lane{tid & (L - 1), tid / L};
}

// the sum of s over the lanes of a row, the same bits in every lane of the row: an xor butterfly over the
// row's lanes of a wave, then (WG) the four waves in wave order through sm[4]
template <bool WG>
__device__ __forceinline__ double row_sum(double s, int L, double* sm) {
  const int n = WG ? kWave : L;
  for (int o = 1; o < n; o <<= 1) s += __shfl_xor(s, o, kWave);
  if constexpr (WG) {
    if ((threadIdx.x & (kWave - 1)) == 0) sm[threadIdx.x / kWave] = s;
    __syncthreads();
    s = ((sm[0] + sm[1]) + sm[2]) + sm[3];
  }
  return s;
}

template <typename T, int VEC, int PLAN, bool RMS>
__global__ __launch_bounds__(kT) void k_ln_fwd(const T* __restrict__ x, T* __restrict__ y,
                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                               double* __restrict__ stats, int64_t R, int C, int cols, int L,
                                               double eps) {
  using IO = Io<T, VEC>;
  constexpr int EPT = Geo<PLAN>::EPT, NV = EPT / VEC;
  constexpr bool WG = Geo<PLAN>::WG;
  __shared__ double sm[2][4];
  const Lane ln = lane_of<WG>(L);
  const int64_t row = (int64_t)blockIdx.x * (kT / L) + ln.rg;
  const bool ok = row < R;
  const int64_t base = row * C;
  float v[EPT];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int cv = ln.lr + j * L;
    if (ok && cv < cols) {
      IO::ld((x + base) + (unsigned)(cv * VEC), &v[j * VEC]);
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[j * VEC + k] = 0.f;
    }
  }
  double mean = 0.0;
  if constexpr (!RMS) {
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) s += (double)v[e];  // (the columns past the row hold 0)
    mean = row_sum<WG>(s, L, sm[0]) / (double)C;
  }
  double q = 0.0;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    if (ln.lr + j * L < cols) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const double d = (double)v[j * VEC + k] - mean;
        q = fma(d, d, q);
      }
    }
  }
  q = row_sum<WG>(q, L, sm[1]);
  const double r = 1.0 / sqrt(q / (double)C + eps);
  if (ok && ln.lr == 0) {
    stats[row * 2] = mean;
    stats[row * 2 + 1] = r;
  }
  const float a = (float)r, b = (float)(-mean * r);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int cv = ln.lr + j * L;
    if (ok && cv < cols) {
      float g[VEC], bt[VEC], o[VEC];
      if (gamma) ld_param<VEC>(gamma + (unsigned)(cv * VEC), g);
      if (!RMS && beta) ld_param<VEC>(beta + (unsigned)(cv * VEC), bt);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float xv = v[j * VEC + k];
        const float xh = RMS ? xv * a : fmaf(xv, a, b);
        if (!RMS && beta)
          o[k] = gamma ? fmaf(xh, g[k], bt[k]) : xh + bt[k];
        else
          o[k] = gamma ? xh * g[k] : xh;
      }
      IO::st((y + base) + (unsigned)(cv * VEC), o);
    }
  }
}

// The backward holds x, dy and two f64 column accumulators per element, so a lane takes kLnEptSub elements in
// every plan and a wider row spreads over more lanes.  SPREAD = false: L = 4 ... 64 lanes per row, 256 / L rows
// per iteration of a 256-thread workgroup (the forward's kLnSub).  SPREAD = true: the workgroup is the L = 128
// ... 1024 lanes of one row; its L / 64 waves meet in LDS and are added in wave order.
template <bool SPREAD>
constexpr int acc_lds() {
  return SPREAD ? 1 : 2 * kLnSubMaxC;
}

template <typename T, int VEC, bool SPREAD, bool RMS>
__global__ __launch_bounds__(SPREAD ? (VEC == 1 ? kLnMaxThreads / 2 : kLnMaxThreads) : kT) void k_ln_bwd(const T* __restrict__ x, const T* __restrict__ dy,
                                               T* __restrict__ dx, const float* __restrict__ gamma,
                                               const double* __restrict__ stats, double* __restrict__ part,
                                               int64_t R, int C, int cols, int L, int64_t rows_wg, int want) {
  using IO = Io<T, VEC>;
  constexpr int EPT = kLnEptSub, NV = EPT / VEC;
  constexpr bool WG = SPREAD;
  constexpr int MAXW = kLnMaxThreads / kWave;
  __shared__ double sm[2][2][MAXW];
  __shared__ double sacc[acc_lds<SPREAD>()];
  const Lane ln = lane_of<WG>(L);
  const int rpi = SPREAD ? 1 : kT / L;
  const int64_t r0 = (int64_t)blockIdx.x * rows_wg;
  const int64_t rend = r0 + rows_wg < R ? r0 + rows_wg : R;
  double ag[EPT], ab[RMS ? 1 : EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) ag[e] = 0.0;
#pragma unroll
  for (int e = 0; e < (RMS ? 1 : EPT); ++e) ab[e] = 0.0;

  int it = 0;
  for (int64_t rb = r0; rb < rend; rb += rpi, ++it) {
    const int64_t row = rb + ln.rg;
    const bool ok = row < rend;
    const int64_t base = row * C;
    float xh[EPT], d[EPT];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int cv = ln.lr + j * L;
      if (ok && cv < cols) {
        IO::ld((x + base) + (unsigned)(cv * VEC), &xh[j * VEC]);
        IO::ld((dy + base) + (unsigned)(cv * VEC), &d[j * VEC]);
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) xh[j * VEC + k] = d[j * VEC + k] = 0.f;
      }
    }
    const double mean = ok ? stats[row * 2] : 0.0;
    const double r = ok ? stats[row * 2 + 1] : 0.0;
    const float a = (float)r, b = (float)(-mean * r);
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int cv = ln.lr + j * L;
      const bool in = ok && cv < cols;
      float g[VEC];
      if (gamma && in) ld_param<VEC>(gamma + (unsigned)(cv * VEC), g);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const int e = j * VEC + k;
        // (outside the row x = dy = 0 and xhat = b: 0 in the sums, unless b is non-finite -- and then the row's
        // own xhat, hence its S2 and dx, are non-finite already; the accumulators there are never written out)
        const float h = RMS ? xh[e] * a : fmaf(xh[e], a, b);
        xh[e] = h;
        const double dd = (double)d[e], hd = (double)h;
        ag[e] = fma(dd, hd, ag[e]);
        if constexpr (!RMS) ab[e] += dd;
        const float gg = (gamma && in) ? d[e] * g[k] : d[e];
        d[e] = gg;
        if constexpr (!RMS) s1 += (double)gg;
        s2 = fma((double)gg, hd, s2);
      }
    }
    // both row sums: the butterfly, then (SPREAD) one LDS round for the two, in the slot of this iteration's
    // parity (the barrier of the next iteration separates this one's reads from the writes of the one after)
    {
      const int n = WG ? kWave : L;
      for (int o = 1; o < n; o <<= 1) {
        if constexpr (!RMS) s1 += __shfl_xor(s1, o, kWave);
        s2 += __shfl_xor(s2, o, kWave);
      }
      if constexpr (WG) {
        double(*slot)[MAXW] = sm[it & 1];
        if ((threadIdx.x & (kWave - 1)) == 0) {
          slot[0][threadIdx.x / kWave] = s1;
          slot[1][threadIdx.x / kWave] = s2;
        }
        __syncthreads();
        s1 = slot[0][0];
        s2 = slot[1][0];
        for (int w = 1; w < L / kWave; ++w) {
          s1 += slot[0][w];
          s2 += slot[1][w];
        }
      }
    }
    const float m1 = (float)(s1 / (double)C), m2 = (float)(s2 / (double)C);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int cv = ln.lr + j * L;
      if (ok && cv < cols) {
        float o[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const int e = j * VEC + k;
          const float u = RMS ? d[e] : d[e] - m1;
          o[k] = a * fmaf(-xh[e], m2, u);
        }
        IO::st((dx + base) + (unsigned)(cv * VEC), o);
      }
    }
  }
  if (!want) return;

  // dgamma / dbeta partials of the block
  double* pg = part + (int64_t)blockIdx.x * 2 * C;
  double* pb = pg + C;
  if constexpr (WG) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int cv = ln.lr + j * L;
      if (cv < cols) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          pg[cv * VEC + k] = ag[j * VEC + k];
          if constexpr (!RMS) pb[cv * VEC + k] = ab[j * VEC + k];
        }
      }
    }
  } else {
    // the row groups of a wave, then the waves into wave 0 in wave order
    for (int o = L; o < kWave; o <<= 1) {
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        ag[e] += __shfl_xor(ag[e], o, kWave);
        if constexpr (!RMS) ab[e] += __shfl_xor(ab[e], o, kWave);
      }
    }
    const int wave = threadIdx.x / kWave;
    const bool first = (threadIdx.x & (kWave - 1)) < L;  // the wave's first row group holds its columns
    constexpr int HALF = acc_lds<SPREAD>() / 2;
    for (int w = 1; w < kT / kWave; ++w) {
      if (wave == w && first) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          const int cv = ln.lr + j * L;
          if (cv < cols) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
              sacc[cv * VEC + k] = ag[j * VEC + k];
              if constexpr (!RMS) sacc[HALF + cv * VEC + k] = ab[j * VEC + k];
            }
          }
        }
      }
      __syncthreads();
      if (wave == 0 && first) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          const int cv = ln.lr + j * L;
          if (cv < cols) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
              ag[j * VEC + k] += sacc[cv * VEC + k];
              if constexpr (!RMS) ab[j * VEC + k] += sacc[HALF + cv * VEC + k];
            }
          }
        }
      }
      __syncthreads();
    }
    if (wave == 0 && first) {
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const int cv = ln.lr + j * L;
        if (cv < cols) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            pg[cv * VEC + k] = ag[j * VEC + k];
            if constexpr (!RMS) pb[cv * VEC + k] = ab[j * VEC + k];
          }
        }
      }
    }
  }
}

// out_q[c] (+)= f32(sum over the blocks of part[block][q][c]): 32 columns x kLnDgbRanges sub-ranges per
// workgroup, blockIdx.y = q (0 dgamma, 1 dbeta)
__global__ __launch_bounds__(kT) void k_ln_dgb(const double* __restrict__ part, int64_t blocks, int C,
                                               float* __restrict__ dgamma, float* __restrict__ dbeta, int acc) {
  __shared__ double sm[kLnDgbRanges][32];
  const int q = blockIdx.y;
  float* out = q == 0 ? dgamma : dbeta;
  if (!out) return;
  const int cl = threadIdx.x & 31, s = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  const int64_t per = (blocks + kLnDgbRanges - 1) / kLnDgbRanges;
  const int64_t b0 = s * per, b1 = b0 + per < blocks ? b0 + per : blocks;
  double t = 0.0;
  if (c < C)
    for (int64_t bl = b0; bl < b1; ++bl) t += part[(bl * 2 + q) * C + c];
  sm[s][cl] = t;
  __syncthreads();
  if (s == 0 && c < C) {
    t = sm[0][cl];
#pragma unroll
    for (int i = 1; i < kLnDgbRanges; ++i) t += sm[i][cl];
    const float v = (float)t;
    out[c] = ((acc >> q) & 1) ? out[c] + v : v;
  }
}

template <typename T, int VEC, int PLAN>
void launch_fwd(const LnPlan& p, const void* x, void* y, int64_t R, int C, const float* gamma, const float* beta,
                double eps, bool rms, double* stats, hipStream_t s) {
  const dim3 grid((unsigned)p.fwd_blocks), block(kT);
  if (rms)
    hipLaunchKernelGGL((k_ln_fwd<T, VEC, PLAN, true>), grid, block, 0, s, (const T*)x, (T*)y, gamma, beta, stats, R, C,
                       p.cols, p.L, eps);
  else
    hipLaunchKernelGGL((k_ln_fwd<T, VEC, PLAN, false>), grid, block, 0, s, (const T*)x, (T*)y, gamma, beta, stats, R,
                       C, p.cols, p.L, eps);
}

template <typename T, int VEC, int PLAN>
void launch_bwd(const LnPlan& p, const void* dy, const void* x, void* dx, int64_t R, int C, const float* gamma,
                const double* stats, bool rms, double* part, int want, hipStream_t s) {
  constexpr bool SPREAD = PLAN != kLnSub;
  const dim3 grid((unsigned)p.blocks), block(SPREAD ? p.Lb : kT);
  if (rms)
    hipLaunchKernelGGL((k_ln_bwd<T, VEC, SPREAD, true>), grid, block, 0, s, (const T*)x, (const T*)dy, (T*)dx, gamma,
                       stats, part, R, C, p.cols, p.Lb, p.rows_wg, want);
  else
    hipLaunchKernelGGL((k_ln_bwd<T, VEC, SPREAD, false>), grid, block, 0, s, (const T*)x, (const T*)dy, (T*)dx, gamma,
                       stats, part, R, C, p.cols, p.Lb, p.rows_wg, want);
}

// calls F<T, VEC, PLAN>(args...) for the plan's (dtype, vec, plan)
#define TDL_LN_DISPATCH(F, dt, p, ...)                                                       \
  do {                                                                                       \
    const int key_ = ((dt) == LnDType::kBF16 ? 6 : 0) + ((p).vec > 1 ? 3 : 0) + (p).plan;    \
    switch (key_) {                                                                          \
      case 0: F<float, 1, kLnSub>(__VA_ARGS__); break;                                       \
      case 1: F<float, 1, kLnWave>(__VA_ARGS__); break;                                      \
      case 2: F<float, 1, kLnGroup>(__VA_ARGS__); break;                                     \
      case 3: F<float, 4, kLnSub>(__VA_ARGS__); break;                                       \
      case 4: F<float, 4, kLnWave>(__VA_ARGS__); break;                                      \
      case 5: F<float, 4, kLnGroup>(__VA_ARGS__); break;                                     \
      case 6: F<uint16_t, 1, kLnSub>(__VA_ARGS__); break;                                    \
      case 7: F<uint16_t, 1, kLnWave>(__VA_ARGS__); break;                                   \
      case 8: F<uint16_t, 1, kLnGroup>(__VA_ARGS__); break;                                  \
      case 9: F<uint16_t, 8, kLnSub>(__VA_ARGS__); break;                                    \
      case 10: F<uint16_t, 8, kLnWave>(__VA_ARGS__); break;                                  \
      default: F<uint16_t, 8, kLnGroup>(__VA_ARGS__); break;                                 \
    }                                                                                        \
  } while (0)

}  // namespace

LnPlan ln_plan(int64_t R, int C, LnDType dt) {
  LnPlan p;
  const int esz = dt == LnDType::kF32 ? 4 : 2;
  p.vec = ((int64_t)C * esz) % 16 == 0 ? 16 / esz : 1;
  p.cols = C / p.vec;
  if (C <= kLnSubMaxC) {
    p.plan = kLnSub;
    const int nv = kLnEptSub / p.vec;
    const int need = (p.cols + nv - 1) / nv;
    p.L = 4;
    while (p.L < need) p.L <<= 1;
  } else if (C <= kLnWaveMaxC) {
    p.plan = kLnWave;
    p.L = kWave;
  } else {
    p.plan = kLnGroup;
    p.L = kLnThreads;
  }
  p.rpi = kLnThreads / p.L;
  p.Lb = p.L;
  if (p.plan != kLnSub) {
    const int nv = kLnEptSub / p.vec;
    const int need = (p.cols + nv - 1) / nv;
    p.Lb = 2 * kWave;
    while (p.Lb < need) p.Lb <<= 1;
  }
  const int rpb = p.plan == kLnSub ? p.rpi : 1;  // rows per iteration of a backward workgroup
  const int64_t per = (R + kLnTargetBlocks - 1) / kLnTargetBlocks;
  p.rows_wg = (per + rpb - 1) / rpb * rpb;
  if (p.rows_wg < 4 * rpb) p.rows_wg = 4 * rpb;
  p.blocks = (R + p.rows_wg - 1) / p.rows_wg;
  p.fwd_blocks = (R + p.rpi - 1) / p.rpi;
  return p;
}

void ln_forward(const void* x, void* y, LnDType dt, int64_t R, int C, const float* gamma, const float* beta,
                double eps, bool rms, double* stats, hipStream_t s) {
  const LnPlan p = ln_plan(R, C, dt);
  TDL_LN_DISPATCH(launch_fwd, dt, p, p, x, y, R, C, gamma, beta, eps, rms, stats, s);
}

void ln_backward(const void* dy, const void* x, void* dx, LnDType dt, int64_t R, int C, const float* gamma,
                 const double* stats, bool rms, double* part, float* dgamma, float* dbeta, int acc, hipStream_t s) {
  const LnPlan p = ln_plan(R, C, dt);
  if (rms) dbeta = nullptr;
  const int want = (dgamma || dbeta) ? 1 : 0;
  TDL_LN_DISPATCH(launch_bwd, dt, p, p, dy, x, dx, R, C, gamma, stats, rms, part, want, s);
  if (want)
    hipLaunchKernelGGL(k_ln_dgb, dim3((unsigned)((C + 31) / 32), 2), dim3(kT), 0, s, (const double*)part, p.blocks, C,
                       dgamma, dbeta, acc);
}

}  // namespace tdl
