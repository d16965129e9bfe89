// Group normalisation kernels (groupnorm.h): per-(sample, channel) f64 sums in a fixed order, a finalize
// that folds them into groups and writes per-(sample, channel) f32 coefficient tables, and elementwise
// passes that read the tables.  The order of every add is described in groupnorm.h.
#include "common.h"
#include "groupnorm.h"

namespace tdl {
namespace {

constexpr int kT = kGnThreads;
constexpr int kU = kGnUnroll;

typedef unsigned u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

// one access of V elements of T: a 16-byte vector (V = 4 f32 / 8 bf16) or a single element
template <typename T, int V>
struct Io;
template <>
struct Io<float, 4> {
  using Raw = f4;
  static __device__ __forceinline__ Raw ld(const float* p) { return ld4(p); }
  static __device__ __forceinline__ void unpack(const Raw& r, float (&v)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = r[k];
  }
  static __device__ __forceinline__ void st(float* p, const float (&v)[4]) { st4(p, f4{v[0], v[1], v[2], v[3]}); }
};
template <>
struct Io<float, 1> {
  using Raw = float;
  static __device__ __forceinline__ Raw ld(const float* p) { return *p; }
  static __device__ __forceinline__ void unpack(const Raw& r, float (&v)[1]) { v[0] = r; }
  static __device__ __forceinline__ void st(float* p, const float (&v)[1]) { *p = v[0]; }
};
template <>
struct Io<uint16_t, 8> {
  using Raw = u4;
  static __device__ __forceinline__ Raw ld(const uint16_t* p) { return *reinterpret_cast<const u4*>(p); }
  static __device__ __forceinline__ void unpack(const Raw& r, float (&v)[8]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[2 * k] = bf16_lo(r[k]);
      v[2 * k + 1] = bf16_hi(r[k]);
    }
  }
  static __device__ __forceinline__ void st(uint16_t* p, const float (&v)[8]) {
    *reinterpret_cast<u4*>(p) = u4{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                                   pack_bf16x2(v[6], v[7])};
  }
};
template <>
struct Io<uint16_t, 1> {
  using Raw = uint16_t;
  static __device__ __forceinline__ Raw ld(const uint16_t* p) { return *p; }
  static __device__ __forceinline__ void unpack(const Raw& r, float (&v)[1]) { v[0] = bf16_lo(r); }
  static __device__ __forceinline__ void st(uint16_t* p, const float (&v)[1]) {
    *p = (uint16_t)(pack_bf16x2(v[0], 0.f) & 0xffffu);
  }
};

// where a thread of workgroup blockIdx.x works: sample n, pixels [p0 + rl, pend) in steps of RL, column cv
struct Where {
  int64_t n, chunk, p, pend;
  int rl, cv;
  bool active;
};
__device__ __forceinline__ Where where(const GnPlan& pl, int64_t P) {
  Where w;
  const int64_t b = blockIdx.x;
  w.chunk = b % pl.chunks;
  const int64_t r = b / pl.chunks;
  const int cb = (int)(r % pl.colblocks);
  w.n = r / pl.colblocks;
  const int tid = threadIdx.x;
  w.rl = tid / pl.tc;
  w.cv = cb * pl.tc + (tid - w.rl * pl.tc);
  w.active = w.rl < pl.rl && w.cv < pl.cols;
  const int64_t p0 = w.chunk * pl.rows_wg;
  w.pend = p0 + pl.rows_wg < P ? p0 + pl.rows_wg : P;
  w.p = p0 + w.rl;
  return w;
}

// part[n][chunk][0][c] = sum_p u, part[n][chunk][1][c] = sum_p u x over the chunk's pixels, where
// forward: u = x (sums of x and x^2); backward: u = dy (sums of dy and dy x)
template <typename T, int V, bool BWD>
__global__ __launch_bounds__(kT) void k_gn_sums(const T* __restrict__ x, const T* __restrict__ dy,
                                                double* __restrict__ part, int64_t P, int C, GnPlan pl) {
  using IO = Io<T, V>;
  const Where w = where(pl, P);
  const int tid = threadIdx.x;
  double s1[V], s2[V];
#pragma unroll
  for (int k = 0; k < V; ++k) s1[k] = s2[k] = 0.0;
  if (w.active) {
    const int64_t row0 = w.n * P;
    const int64_t col = (int64_t)w.cv * V;
    const int RL = pl.rl;
    int64_t p = w.p;
    for (; p + (int64_t)(kU - 1) * RL < w.pend; p += (int64_t)kU * RL) {
      typename IO::Raw rx[kU], rd[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int64_t off = (row0 + p + (int64_t)u * RL) * C + col;
        rx[u] = IO::ld(x + off);
        if (BWD) rd[u] = IO::ld(dy + off);
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        float vx[V], vd[V];
        IO::unpack(rx[u], vx);
        if (BWD) IO::unpack(rd[u], vd);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const double xd = (double)vx[k];
          const double ud = BWD ? (double)vd[k] : xd;
          s1[k] += ud;
          s2[k] = fma(ud, xd, s2[k]);  // the product is exact in f64: one rounding, that of the add
        }
      }
    }
    for (; p < w.pend; p += RL) {
      const int64_t off = (row0 + p) * C + col;
      float vx[V], vd[V];
      IO::unpack(IO::ld(x + off), vx);
      if (BWD) IO::unpack(IO::ld(dy + off), vd);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const double xd = (double)vx[k];
        const double ud = BWD ? (double)vd[k] : xd;
        s1[k] += ud;
        s2[k] = fma(ud, xd, s2[k]);
      }
    }
  }
  // the row lanes of a column combine in a fixed tree: lane rl takes lane rl + h for h = RLP2 / 2 ... 1
  __shared__ double sm[2 * V * kT];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    sm[k * kT + tid] = s1[k];
    sm[(V + k) * kT + tid] = s2[k];
  }
  __syncthreads();
  int h = 1;
  while (h < pl.rl) h <<= 1;
  for (h >>= 1; h > 0; h >>= 1) {
    if (w.active && w.rl < h && w.rl + h < pl.rl) {
#pragma unroll
      for (int k = 0; k < 2 * V; ++k) sm[k * kT + tid] += sm[k * kT + tid + h * pl.tc];
    }
    __syncthreads();
  }
  if (w.active && w.rl == 0) {
    double* o = part + ((w.n * pl.chunks + w.chunk) * 2) * C + (int64_t)w.cv * V;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      o[k] = sm[k * kT + tid];
      o[C + k] = sm[(V + k) * kT + tid];
    }
  }
}

// forward: out = fmaf(x, t0, t1); backward: out = fmaf(t0, dy, fmaf(t1, x, t2)); tables [N][C] f32
template <typename T, int V, bool BWD>
__global__ __launch_bounds__(kT) void k_gn_apply(const T* __restrict__ x, const T* __restrict__ dy,
                                                 T* __restrict__ out, const float* __restrict__ t0,
                                                 const float* __restrict__ t1, const float* __restrict__ t2,
                                                 int64_t P, int C, GnPlan pl) {
  using IO = Io<T, V>;
  const Where w = where(pl, P);
  if (!w.active) return;
  const int64_t col = (int64_t)w.cv * V;
  const int64_t tb = w.n * C + col;
  float c0[V], c1[V], c2[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    c0[k] = t0[tb + k];
    c1[k] = t1[tb + k];
    c2[k] = BWD ? t2[tb + k] : 0.f;
  }
  const int64_t row0 = w.n * P;
  const int RL = pl.rl;
  int64_t p = w.p;
  for (; p + (int64_t)(kU - 1) * RL < w.pend; p += (int64_t)kU * RL) {
    typename IO::Raw rx[kU], rd[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int64_t off = (row0 + p + (int64_t)u * RL) * C + col;
      rx[u] = IO::ld(x + off);
      if (BWD) rd[u] = IO::ld(dy + off);
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      float vx[V], vd[V], vo[V];
      IO::unpack(rx[u], vx);
      if (BWD) IO::unpack(rd[u], vd);
#pragma unroll
      for (int k = 0; k < V; ++k)
        vo[k] = BWD ? fmaf(c0[k], vd[k], fmaf(c1[k], vx[k], c2[k])) : fmaf(vx[k], c0[k], c1[k]);
      IO::st(out + (row0 + p + (int64_t)u * RL) * C + col, vo);
    }
  }
  for (; p < w.pend; p += RL) {
    const int64_t off = (row0 + p) * C + col;
    float vx[V], vd[V], vo[V];
    IO::unpack(IO::ld(x + off), vx);
    if (BWD) IO::unpack(IO::ld(dy + off), vd);
#pragma unroll
    for (int k = 0; k < V; ++k)
      vo[k] = BWD ? fmaf(c0[k], vd[k], fmaf(c1[k], vx[k], c2[k])) : fmaf(vx[k], c0[k], c1[k]);
    IO::st(out + off, vo);
  }
}

// Sum across the L = 2^k <= 64 adjacent lanes of a group's slot, in every one of them: an xor butterfly (both
// partners add the same two values, so every lane ends with the same bits) over the offsets below L.  The
// offsets of L and above of a whole-wave butterfly would only add the zeros of lanes that hold no channel
// of the group, so the bits do not depend on how many groups share a wave.
__device__ __forceinline__ double slot_sum_f64(double v, int L) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double t = __shfl_xor(v, o, 64);
    if (o < L) v += t;
  }
  return v;
}

// a, b = sums over the chunks, ascending, of rows 0 and 1 of channel c of sample n (four chunks' loads
// are issued before their adds; the adds stay in chunk order)
__device__ __forceinline__ void chunk_sums(const double* __restrict__ part, int64_t n, int64_t chunks, int C, int c,
                                           double& a, double& b) {
  const double* p = part + (n * chunks * 2) * C + c;
  const int64_t st = 2 * (int64_t)C;
  a = 0.0;
  b = 0.0;
  int64_t k = 0;
  for (; k + 4 <= chunks; k += 4, p += 4 * st) {
    double va[4], vb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      va[u] = p[u * st];
      vb[u] = p[u * st + C];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a += va[u];
      b += vb[u];
    }
  }
  for (; k < chunks; ++k, p += st) {
    a += p[0];
    b += p[C];
  }
}

// L adjacent lanes per (n, g) -- L = group_lanes(C / G): a whole wave for 33 channels and more, 64 / L groups
// per wave below that (one lane each for instance normalisation): group statistics, then the scale / shift
// of the group's channels
__global__ __launch_bounds__(kT) void k_gn_fwd_finalize(const double* __restrict__ part,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, double* __restrict__ stats,
                                                        float* __restrict__ scale, float* __restrict__ shift,
                                                        int64_t N, int C, int G, int64_t chunks, double m,
                                                        double eps, int L) {
  const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
  const int64_t w = t / L;
  const int lane = (int)(t - w * L);
  const bool live = w < N * G;  // (a slot past the end takes part in the shuffles and stores nothing)
  const int64_t n = live ? w / G : 0;
  const int g = live ? (int)(w - n * G) : 0;
  const int cpg = live ? C / G : 0;
  double t1 = 0.0, t2 = 0.0;
  for (int c = lane; c < cpg; c += L) {
    double a, b;
    chunk_sums(part, n, chunks, C, g * cpg + c, a, b);
    t1 += a;
    t2 += b;
  }
  t1 = slot_sum_f64(t1, L);
  t2 = slot_sum_f64(t2, L);
  const double mean = t1 / m;
  const double v = t2 / m - mean * mean;
  const double var = v < 0.0 ? 0.0 : v;  // (keeps a NaN, which fmax would drop)
  const double r = 1.0 / sqrt(var + eps);
  if (live && lane == 0) {
    stats[2 * w] = mean;
    stats[2 * w + 1] = r;
  }
  for (int c = lane; c < cpg; c += L) {
    const int ch = g * cpg + c;
    const double sc = (gamma != nullptr ? (double)gamma[ch] : 1.0) * r;
    const double bt = beta != nullptr ? (double)beta[ch] : 0.0;
    scale[n * C + ch] = (float)sc;
    shift[n * C + ch] = (float)(bt - mean * sc);
  }
}

// workgroups [0, nb1): L lanes per (n, g) as in the forward, the dx coefficients; workgroups [nb1, ...): kBwdCh channels
// each, dgamma / dbeta over the samples in ascending order
constexpr int kBwdCh = 4, kBwdNl = kT / kBwdCh;
__global__ __launch_bounds__(kT) void k_gn_bwd_finalize(const double* __restrict__ part,
                                                        const float* __restrict__ gamma,
                                                        const double* __restrict__ stats, float* __restrict__ A,
                                                        float* __restrict__ B, float* __restrict__ D,
                                                        float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                        int acc, int64_t N, int C, int G, int64_t chunks, double m,
                                                        int64_t nb1, int L) {
  if ((int64_t)blockIdx.x >= nb1) {
    const int cpg = C / G;
    // kBwdCh channels x kBwdNl sample lanes: the lanes form the terms of kBwdNl consecutive samples, lane 0
    // of a channel adds them in ascending order; blocks of samples ascend, so the whole sum does
    __shared__ double tg[kBwdNl][kBwdCh], tb[kBwdNl][kBwdCh];
    const int cl = threadIdx.x % kBwdCh, nl = threadIdx.x / kBwdCh;
    const int64_t c64 = ((int64_t)blockIdx.x - nb1) * kBwdCh + cl;
    const bool live = c64 < C;
    const int c = live ? (int)c64 : 0;
    const int g = c / cpg;
    double dg = 0.0, db = 0.0;
    for (int64_t n0 = 0; n0 < N; n0 += kBwdNl) {
      const int64_t n = n0 + nl;
      double ta = 0.0, tgm = 0.0;
      if (live && n < N) {
        double a, b;
        chunk_sums(part, n, chunks, C, c, a, b);
        const double mean = stats[2 * (n * G + g)], r = stats[2 * (n * G + g) + 1];
        ta = a;
        tgm = r * (b - mean * a);
      }
      tb[nl][cl] = ta;
      tg[nl][cl] = tgm;
      __syncthreads();
      if (nl == 0) {
        const int cnt = N - n0 < kBwdNl ? (int)(N - n0) : kBwdNl;
        for (int i = 0; i < cnt; ++i) {
          db += tb[i][cl];
          dg += tg[i][cl];
        }
      }
      __syncthreads();
    }
    if (live && nl == 0) {
      if (dgamma != nullptr) dgamma[c] = (acc & 1) ? dgamma[c] + (float)dg : (float)dg;
      if (dbeta != nullptr) dbeta[c] = (acc & 2) ? dbeta[c] + (float)db : (float)db;
    }
    return;
  }
  const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
  const int64_t w = t / L;
  const int lane = (int)(t - w * L);
  const bool live = w < N * G;
  const int64_t n = live ? w / G : 0;
  const int g = live ? (int)(w - n * G) : 0;
  const int cpg = live ? C / G : 0;
  const double mean = live ? stats[2 * w] : 0.0, r = live ? stats[2 * w + 1] : 0.0;
  double s1 = 0.0, s2 = 0.0;
  for (int c = lane; c < cpg; c += L) {
    const int ch = g * cpg + c;
    const double gm = gamma != nullptr ? (double)gamma[ch] : 1.0;
    double a, b;
    chunk_sums(part, n, chunks, C, ch, a, b);
    s1 += gm * a;
    s2 += gm * (b - mean * a);
  }
  s1 = slot_sum_f64(s1, L);
  s2 = r * slot_sum_f64(s2, L);
  const float Bf = (float)(-(r * r) * s2 / m);
  const float Df = (float)((r * r) * mean * s2 / m - r * s1 / m);
  for (int c = lane; c < cpg; c += L) {
    const int ch = g * cpg + c;
    const double gm = gamma != nullptr ? (double)gamma[ch] : 1.0;
    A[n * C + ch] = (float)(gm * r);
    B[n * C + ch] = Bf;
    D[n * C + ch] = Df;
  }
}

template <typename T, int V, bool BWD>
void launch_sums(const void* x, const void* dy, double* part, int64_t N, int64_t P, int C, const GnPlan& pl,
                 hipStream_t s) {
  const dim3 grid((unsigned)(N * pl.colblocks * pl.chunks));
  hipLaunchKernelGGL((k_gn_sums<T, V, BWD>), grid, dim3(kT), 0, s, (const T*)x, (const T*)dy, part, P, C, pl);
}
template <typename T, int V, bool BWD>
void launch_apply(const void* x, const void* dy, void* out, const float* t0, const float* t1, const float* t2,
                  int64_t N, int64_t P, int C, const GnPlan& pl, hipStream_t s) {
  const dim3 grid((unsigned)(N * pl.colblocks * pl.chunks));
  hipLaunchKernelGGL((k_gn_apply<T, V, BWD>), grid, dim3(kT), 0, s, (const T*)x, (const T*)dy, (T*)out, t0, t1, t2, P,
                     C, pl);
}

template <bool BWD>
void sums(const void* x, const void* dy, double* part, GnDType dt, int64_t N, int64_t P, int C, const GnPlan& pl,
          hipStream_t s) {
  if (dt == GnDType::kF32) {
    if (pl.vec == 4) launch_sums<float, 4, BWD>(x, dy, part, N, P, C, pl, s);
    else launch_sums<float, 1, BWD>(x, dy, part, N, P, C, pl, s);
  } else {
    if (pl.vec == 8) launch_sums<uint16_t, 8, BWD>(x, dy, part, N, P, C, pl, s);
    else launch_sums<uint16_t, 1, BWD>(x, dy, part, N, P, C, pl, s);
  }
}
template <bool BWD>
void apply(const void* x, const void* dy, void* out, const float* t0, const float* t1, const float* t2, GnDType dt,
           int64_t N, int64_t P, int C, const GnPlan& pl, hipStream_t s) {
  if (dt == GnDType::kF32) {
    if (pl.vec == 4) launch_apply<float, 4, BWD>(x, dy, out, t0, t1, t2, N, P, C, pl, s);
    else launch_apply<float, 1, BWD>(x, dy, out, t0, t1, t2, N, P, C, pl, s);
  } else {
    if (pl.vec == 8) launch_apply<uint16_t, 8, BWD>(x, dy, out, t0, t1, t2, N, P, C, pl, s);
    else launch_apply<uint16_t, 1, BWD>(x, dy, out, t0, t1, t2, N, P, C, pl, s);
  }
}

// lanes per (sample, group) slot of the finalize kernels: the power of two that holds the group's channels, 64 at most
int group_lanes(int cpg) {
  int L = 1;
  while (L < cpg && L < 64) L <<= 1;
  return L;
}

}  // namespace

GnPlan gn_plan(int64_t P, int C, GnDType dt) {
  const int es = dt == GnDType::kF32 ? 4 : 2;
  GnPlan pl;
  pl.vec = ((int64_t)C * es) % 16 == 0 ? 16 / es : 1;
  pl.cols = C / pl.vec;
  pl.tc = pl.cols < kGnMaxCols ? pl.cols : kGnMaxCols;
  pl.rl = kT / pl.tc;
  pl.colblocks = (pl.cols + pl.tc - 1) / pl.tc;
  const int64_t row_bytes = (int64_t)pl.tc * pl.vec * es;
  const int64_t fit = kGnChunkBytes / row_bytes;
  const int64_t rows = fit < kGnMaxRows ? fit : kGnMaxRows;
  const int64_t step = (int64_t)pl.rl * kU;
  pl.rows_wg = (rows + step - 1) / step * step;
  pl.chunks = P > pl.rows_wg ? (P + pl.rows_wg - 1) / pl.rows_wg : 1;
  return pl;
}

void gn_forward(const void* x, void* y, GnDType dt, int64_t N, int64_t P, int C, int G, const float* gamma,
                const float* beta, double eps, double* part, double* stats, float* coef, hipStream_t s, int phases) {
  const GnPlan pl = gn_plan(P, C, dt);
  float* scale = coef;
  float* shift = coef + N * C;
  if (phases & kGnSums) sums<false>(x, nullptr, part, dt, N, P, C, pl, s);
  if (phases & kGnFinalize) {
    const int L = group_lanes(C / G);
    const int64_t nb = (N * G + kT / L - 1) / (kT / L);
    hipLaunchKernelGGL(k_gn_fwd_finalize, dim3((unsigned)nb), dim3(kT), 0, s, part, gamma, beta, stats, scale, shift, N,
                       C, G, pl.chunks, (double)P * (double)(C / G), eps, L);
  }
  if (phases & kGnApply) apply<false>(x, nullptr, y, scale, shift, nullptr, dt, N, P, C, pl, s);
}

void gn_backward(const void* dy, const void* x, void* dx, GnDType dt, int64_t N, int64_t P, int C, int G,
                 const float* gamma, const double* stats, double* part, float* coef, float* dgamma, float* dbeta,
                 int acc, hipStream_t s, int phases) {
  const GnPlan pl = gn_plan(P, C, dt);
  float* A = coef;
  float* B = coef + N * C;
  float* D = coef + 2 * N * C;
  if (phases & kGnSums) sums<true>(x, dy, part, dt, N, P, C, pl, s);
  if (phases & kGnFinalize) {
    const int L = group_lanes(C / G);
    const int64_t nb1 = (N * G + kT / L - 1) / (kT / L);
    const int64_t nb2 = (C + kBwdCh - 1) / kBwdCh;
    hipLaunchKernelGGL(k_gn_bwd_finalize, dim3((unsigned)(nb1 + nb2)), dim3(kT), 0, s, part, gamma, stats, A, B, D,
                       dgamma, dbeta, acc, N, C, G, pl.chunks, (double)P * (double)(C / G), nb1, L);
  }
  if (phases & kGnApply) apply<true>(x, dy, dx, A, B, D, dt, N, P, C, pl, s);
}

}  // namespace tdl
