// Depthwise convolution kernels (depthwise.h): LDS-staged stencils for the forward and the input gradient,
// a two-launch f64 reduction for the weight / bias gradient.  The order of every add is described in depthwise.h.
#include "common.h"
#include "depthwise.h"

namespace tdl {
namespace {

constexpr int kT = kDwThreads;
constexpr int kS = kDwStrip;

typedef unsigned u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

// one access of V elements of T: a 16-byte vector (V = 4 f32 / 8 bf16) or a single element
template <typename T, int V>
struct Io;
template <>
struct Io<float, 4> {
  using Raw = f4;
  static __device__ __forceinline__ Raw zero() { return zero4(); }
  static __device__ __forceinline__ void unpack(const Raw& r, float (&v)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = r[k];
  }
  static __device__ __forceinline__ Raw pack(const float (&v)[4]) { return f4{v[0], v[1], v[2], v[3]}; }
};
template <>
struct Io<float, 1> {
  using Raw = float;
  static __device__ __forceinline__ Raw zero() { return 0.f; }
  static __device__ __forceinline__ void unpack(const Raw& r, float (&v)[1]) { v[0] = r; }
  static __device__ __forceinline__ Raw pack(const float (&v)[1]) { return v[0]; }
};
template <>
struct Io<uint16_t, 8> {
  using Raw = u4;
  static __device__ __forceinline__ Raw zero() { return u4{0u, 0u, 0u, 0u}; }
  static __device__ __forceinline__ void unpack(const Raw& r, float (&v)[8]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[2 * k] = bf16_lo(r[k]);
      v[2 * k + 1] = bf16_hi(r[k]);
    }
  }
  static __device__ __forceinline__ Raw pack(const float (&v)[8]) {
    return u4{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
  }
};
template <>
struct Io<uint16_t, 1> {
  using Raw = uint16_t;
  static __device__ __forceinline__ Raw zero() { return 0; }
  static __device__ __forceinline__ void unpack(const Raw& r, float (&v)[1]) { v[0] = bf16_lo(r); }
  static __device__ __forceinline__ Raw pack(const float (&v)[1]) { return (uint16_t)(pack_bf16x2(v[0], 0.f) & 0xffffu); }
};

// V consecutive f32 weights (16-byte loads on the vector path: C % V == 0 there and w is 16-byte aligned)
template <int V>
__device__ __forceinline__ void ldw(const float* __restrict__ p, float (&v)[V]) {
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

__device__ __forceinline__ int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// Stage rows [r0, r0 + RH) x columns [c0, c0 + RW) of sample n of src [.][Hs][Ws][Cs], channels
// [ch0, ch0 + kE * V), into tile[(r * RW + c) * kE + k] (k: the V-element item of the channel run; consecutive
// lanes take consecutive items).  Positions outside the image or past Cs are zeros; with mask (the forward's
// ReLU output, same shape as src) an element counts where mask > 0.
template <typename T, int V>
__device__ __forceinline__ void dw_stage(typename Io<T, V>::Raw* tile, const T* __restrict__ src,
                                         const T* __restrict__ mask, int64_t n, int r0, int c0, int RH, int RW, int Hs,
                                         int Ws, int Cs, int ch0, int kE) {
  using IO = Io<T, V>;
  using Raw = typename IO::Raw;
  const int total = RH * RW * kE;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int k = idx % kE;
    const int pix = idx / kE;
    const int c = pix % RW, r = pix / RW;
    const int gr = r0 + r, gc = c0 + c, ch = ch0 + k * V;
    Raw v = IO::zero();
    if (gr >= 0 && gr < Hs && gc >= 0 && gc < Ws && ch < Cs) {
      const int64_t off = ((n * Hs + gr) * Ws + gc) * (int64_t)Cs + ch;
      v = *reinterpret_cast<const Raw*>(src + off);
      if (mask != nullptr) {
        float a[V], m[V];
        IO::unpack(v, a);
        IO::unpack(*reinterpret_cast<const Raw*>(mask + off), m);
#pragma unroll
        for (int q = 0; q < V; ++q) a[q] = m[q] > 0.f ? a[q] : 0.f;
        v = IO::pack(a);  // (a bf16 value packs back to itself)
      }
    }
    tile[idx] = v;
  }
}

struct Block {
  int64_t n;
  int cb, th, tw;
};
__device__ __forceinline__ Block decode(const DwPlan& p, int tiles_h, int tiles_w) {
  Block b;
  int64_t r = blockIdx.x;
  b.tw = (int)(r % tiles_w);
  r /= tiles_w;
  b.th = (int)(r % tiles_h);
  r /= tiles_h;
  b.cb = (int)(r % p.colblocks);
  b.n = r / p.colblocks;
  return b;
}

// Forward (FLIP = false: tiles over [OH, OW], source x) and input gradient (FLIP = true: tiles over [H, W],
// source dy with dm elements per column).  KW > 0: a kernel row of KW taps at stride SW along W without
// dilation along W, dm == 1 (FLIP: both strides 1): the row's weights and the strip's window sit in registers.
// KW == 0: every shape, each tap read from LDS.
template <typename T, int V, int KW, int SW, bool FLIP>
__global__ __launch_bounds__(kT) void k_dw_conv(const T* __restrict__ src, const T* __restrict__ mask,
                                                const float* __restrict__ w, const float* __restrict__ bias,
                                                T* __restrict__ out, DwGeom g, DwPlan p, int act, int tiles_h,
                                                int tiles_w, int per_h, int per_w) {
  using IO = Io<T, V>;
  using Raw = typename IO::Raw;
  extern __shared__ u4 smem[];
  Raw* tile = reinterpret_cast<Raw*>(smem);
  const Block b = decode(p, tiles_h, tiles_w);
  const int TH = FLIP ? g.H : g.OH, TW = FLIP ? g.W : g.OW;
  const int E = FLIP ? g.dm : 1;
  const int kE = p.tc * E;
  const int rt0 = b.th * p.toh, ct0 = b.tw * p.tow;
  int r0, c0, RH, RW;
  if (!FLIP) {
    r0 = rt0 * g.sh - g.pt;
    c0 = ct0 * g.sw - g.pl;
    RH = p.hh;
    RW = p.hw;
    dw_stage<T, V>(tile, src, nullptr, b.n, r0, c0, RH, RW, g.H, g.W, g.C, b.cb * p.tc * V, kE);
  } else {
    r0 = floor_div(rt0 + g.pt - (g.kh - 1) * g.dh, g.sh);
    c0 = floor_div(ct0 + g.pl - (g.kw - 1) * g.dw, g.sw);
    RH = floor_div(rt0 + p.toh - 1 + g.pt, g.sh) - r0 + 1;
    RW = floor_div(ct0 + p.tow - 1 + g.pl, g.sw) - c0 + 1;
    dw_stage<T, V>(tile, src, mask, b.n, r0, c0, RH, RW, g.OH, g.OW, g.C * g.dm, b.cb * p.tc * V * E, kE);
  }
  __syncthreads();
  const int tid = threadIdx.x;
  const int cl = tid % p.tc, strip = tid / p.tc;
  const int orow = strip / p.nsw, ocol0 = (strip - orow * p.nsw) * kS;
  const int cv = b.cb * p.tc + cl;
  const int row = rt0 + orow, col = ct0 + ocol0;
  if (cv >= p.cols || row >= TH || col >= TW) return;
  const int c = cv * V;  // first input channel of the column
  const int Cout = g.C * g.dm;

  if constexpr (KW > 0) {
    constexpr int WN = (kS - 1) * SW + KW;
    float acc[kS][V];
#pragma unroll
    for (int s = 0; s < kS; ++s)
#pragma unroll
      for (int k = 0; k < V; ++k) acc[s][k] = 0.f;
    for (int i = 0; i < g.kh; ++i) {
      float wr[KW][V];
#pragma unroll
      for (int j = 0; j < KW; ++j) ldw<V>(w + (int64_t)(i * KW + j) * g.C + c, wr[j]);
      const int lrow = FLIP ? orow + (g.kh - 1 - i) * g.dh : orow * g.sh + i * g.dh;
      const Raw* rp = tile + (lrow * RW + ocol0 * SW) * kE + cl;
      float xw[WN][V];
#pragma unroll
      for (int q = 0; q < WN; ++q) IO::unpack(rp[q * kE], xw[q]);
#pragma unroll
      for (int s = 0; s < kS; ++s)
#pragma unroll
        for (int j = 0; j < KW; ++j)
#pragma unroll
          for (int k = 0; k < V; ++k)
            acc[s][k] = fmaf(xw[FLIP ? s + KW - 1 - j : s * SW + j][k], wr[j][k], acc[s][k]);
    }
    float bv[V];
#pragma unroll
    for (int k = 0; k < V; ++k) bv[k] = 0.f;
    if (!FLIP && bias != nullptr) ldw<V>(bias + c, bv);
#pragma unroll
    for (int s = 0; s < kS; ++s) {
      if (col + s >= TW) break;
      if (!FLIP) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          if (bias != nullptr) acc[s][k] += bv[k];
          if (act == 1) acc[s][k] = acc[s][k] > 0.f ? acc[s][k] : (acc[s][k] != acc[s][k] ? acc[s][k] : 0.f);
        }
      }
      const int64_t off = ((b.n * TH + row) * TW + col + s) * (int64_t)g.C + c;
      *reinterpret_cast<Raw*>(out + off) = IO::pack(acc[s]);
    }
  } else if constexpr (!FLIP) {
    for (int s = 0; s < kS && col + s < TW; ++s) {
      for (int m = 0; m < g.dm; ++m) {
        float acc[V];
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = 0.f;
        for (int i = 0; i < g.kh; ++i) {
          const Raw* rp = tile + ((orow * g.sh + i * g.dh) * RW + (ocol0 + s) * g.sw) * kE + cl;
          for (int j = 0; j < g.kw; ++j) {
            float xv[V], wv[V];
            IO::unpack(rp[j * g.dw * kE], xv);
            ldw<V>(w + ((int64_t)(i * g.kw + j) * g.C + c) * g.dm + m, wv);
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] = fmaf(xv[k], wv[k], acc[k]);
          }
        }
        const int co = c * g.dm + m;
        if (bias != nullptr) {
          float bv[V];
          ldw<V>(bias + co, bv);
#pragma unroll
          for (int k = 0; k < V; ++k) acc[k] += bv[k];
        }
        if (act == 1) {
#pragma unroll
          for (int k = 0; k < V; ++k) acc[k] = acc[k] > 0.f ? acc[k] : (acc[k] != acc[k] ? acc[k] : 0.f);
        }
        const int64_t off = ((b.n * TH + row) * TW + col + s) * (int64_t)Cout + co;
        *reinterpret_cast<Raw*>(out + off) = IO::pack(acc);
      }
    }
  } else {
    // the taps a row of dx meets: i0, i0 + per_h, ... (oh * sh == row + pt - i * dh); none when no i < per_h fits
    const int hp = row + g.pt;
    int i0 = -1;
    for (int i = per_h - 1; i >= 0; --i)
      if ((hp - i * g.dh) % g.sh == 0) i0 = i;
    for (int s = 0; s < kS && col + s < TW; ++s) {
      const int wp = col + s + g.pl;
      int j0 = -1;
      for (int j = per_w - 1; j >= 0; --j)
        if ((wp - j * g.dw) % g.sw == 0) j0 = j;
      float acc[V];
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] = 0.f;
      if (i0 >= 0 && j0 >= 0) {
        for (int i = i0; i < g.kh; i += per_h) {
          const int lrow = (hp - i * g.dh) / g.sh - r0;
          for (int j = j0; j < g.kw; j += per_w) {
            const int lcol = (wp - j * g.dw) / g.sw - c0;
            const Raw* rp = tile + (lrow * RW + lcol) * kE + cl * E;
            const float* wp_ = w + ((int64_t)(i * g.kw + j) * g.C + c) * g.dm;
            for (int m = 0; m < E; ++m) {
              float dv[V], wv[V];
              IO::unpack(rp[m], dv);
              ldw<V>(wp_ + m, wv);
#pragma unroll
              for (int k = 0; k < V; ++k) acc[k] = fmaf(dv[k], wv[k], acc[k]);
            }
          }
        }
      }
      const int64_t off = ((b.n * TH + row) * TW + col + s) * (int64_t)g.C + c;
      *reinterpret_cast<Raw*>(out + off) = IO::pack(acc);
    }
  }
}

// Weight / bias gradient, launch 1.  Lanes of a column: (tap slot ts, pixel lane ps), lane = ps * TS + ts.
// Virtual tap vt = t * dm + m, t < kh * kw the taps, t == kh * kw the bias (x := 1).
template <typename T, int V>
__global__ __launch_bounds__(kT) void k_dw_wgrad(const T* __restrict__ x, const T* __restrict__ dy,
                                                 const T* __restrict__ mask, double* __restrict__ part, DwGeom g,
                                                 DwPlan p, int tiles_h, int tiles_w) {
  using IO = Io<T, V>;
  using Raw = typename IO::Raw;
  extern __shared__ u4 smem[];
  double* red = reinterpret_cast<double*>(smem);  // [V][kT]
  Raw* xt = reinterpret_cast<Raw*>(red + V * kT);
  Raw* dyt = xt + p.hh * p.hw * p.tc;
  const Block b = decode(p, tiles_h, tiles_w);
  const int rt0 = b.th * p.toh, ct0 = b.tw * p.tow;
  const int kEd = p.tc * g.dm;
  dw_stage<T, V>(xt, x, nullptr, b.n, rt0 * g.sh - g.pt, ct0 * g.sw - g.pl, p.hh, p.hw, g.H, g.W, g.C, b.cb * p.tc * V,
                 p.tc);
  dw_stage<T, V>(dyt, dy, mask, b.n, rt0, ct0, p.toh, p.tow, g.OH, g.OW, g.C * g.dm, b.cb * p.tc * V * g.dm, kEd);
  __syncthreads();
  const int tid = threadIdx.x;
  const int cl = tid % p.tc, lane = tid / p.tc;
  const int TS = p.ts, PS = (kT / p.tc) / TS;
  const int ts = lane % TS, ps = lane / TS;
  const int cv = b.cb * p.tc + cl;
  const int T_ = g.kh * g.kw;
  const int VT = (T_ + 1) * g.dm;
  const int npix = p.toh * p.tow;
  const int64_t Cout = (int64_t)g.C * g.dm;
  const int64_t chunk = (b.n * tiles_h + b.th) * tiles_w + b.tw;
  for (int vt0 = 0; vt0 < VT; vt0 += TS) {
    const int vt = vt0 + ts;
    const bool live = vt < VT && cv < p.cols;
    const int t = vt / g.dm, m = vt - t * g.dm;
    double acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.0;
    if (live) {
      const int i = t / g.kw, j = t - i * g.kw;
      const int xoff = t < T_ ? (i * g.dh * p.hw + j * g.dw) * p.tc + cl : -1;
      for (int pix = ps; pix < npix; pix += PS) {
        const int orow = pix / p.tow, ocol = pix - orow * p.tow;
        float dv[V], xv[V];
        IO::unpack(dyt[pix * kEd + cl * g.dm + m], dv);
        if (xoff >= 0) {
          IO::unpack(xt[(orow * g.sh * p.hw + ocol * g.sw) * p.tc + xoff], xv);
#pragma unroll
          for (int k = 0; k < V; ++k) acc[k] = fma((double)dv[k], (double)xv[k], acc[k]);
        } else {
#pragma unroll
          for (int k = 0; k < V; ++k) acc[k] += (double)dv[k];
        }
      }
    }
    if (PS > 1) {  // pixel lane ps takes lane ps + h for h = PS / 2 ... 1
#pragma unroll
      for (int k = 0; k < V; ++k) red[k * kT + tid] = acc[k];
      __syncthreads();
      for (int h = PS >> 1; h > 0; h >>= 1) {
        if (ps < h) {
#pragma unroll
          for (int k = 0; k < V; ++k) red[k * kT + tid] += red[k * kT + tid + h * TS * p.tc];
        }
        __syncthreads();
      }
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] = red[k * kT + tid];
    }
    if (live && ps == 0) {
      double* o = part + (chunk * (T_ + 1) + t) * Cout + (int64_t)cv * V * g.dm + m;
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = acc[k];
    }
  }
}

// Launch 2: kFinOut outputs x kFinLanes chunk lanes per workgroup
constexpr int kFinOut = 16, kFinLanes = kT / kFinOut;
__global__ __launch_bounds__(kT) void k_dw_wgrad_finalize(const double* __restrict__ part, float* __restrict__ dW,
                                                          float* __restrict__ db, int acc, int64_t chunks,
                                                          int64_t n_w, int64_t n_out) {
  __shared__ double red[kT];
  const int tid = threadIdx.x;
  const int ol = tid % kFinOut, l = tid / kFinOut;
  const int64_t o = (int64_t)blockIdx.x * kFinOut + ol;
  double s = 0.0;
  if (o < n_out) {
    const double* q = part + o;
    int64_t k = l;
    for (; k + 3 * kFinLanes < chunks; k += 4 * kFinLanes) {
      double v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = q[(k + (int64_t)u * kFinLanes) * n_out];
#pragma unroll
      for (int u = 0; u < 4; ++u) s += v[u];
    }
    for (; k < chunks; k += kFinLanes) s += q[k * n_out];
  }
  red[tid] = s;
  __syncthreads();
  for (int h = kFinLanes >> 1; h > 0; h >>= 1) {
    if (l < h) red[tid] += red[tid + h * kFinOut];
    __syncthreads();
  }
  if (o < n_out && l == 0) {
    const float v = (float)red[tid];
    if (o < n_w) {
      dW[o] = (acc & 1) ? dW[o] + v : v;
    } else if (db != nullptr) {
      db[o - n_w] = (acc & 2) ? db[o - n_w] + v : v;
    }
  }
}

int gcd(int a, int b) { return b == 0 ? a : gcd(b, a % b); }
int ceil_div(int a, int b) { return (a + b - 1) / b; }
int esize(DwDType dt) { return dt == DwDType::kF32 ? 4 : 2; }

template <typename T, int V, int KW, int SW, bool FLIP>
void launch_conv(const void* src, const void* mask, const float* w, const float* bias, void* out, const DwGeom& g,
                 const DwPlan& p, int act, hipStream_t s) {
  const int TH = FLIP ? g.H : g.OH, TW = FLIP ? g.W : g.OW;
  const int tiles_h = ceil_div(TH, p.toh), tiles_w = ceil_div(TW, p.tow);
  const int64_t grid = (int64_t)g.N * p.colblocks * tiles_h * tiles_w;
  const size_t lds = (size_t)p.hh * p.hw * p.tc * (FLIP ? g.dm : 1) * V * sizeof(T);
  const int per_h = g.sh / gcd(g.sh, g.dh), per_w = g.sw / gcd(g.sw, g.dw);
  hipLaunchKernelGGL((k_dw_conv<T, V, KW, SW, FLIP>), dim3((unsigned)grid), dim3(p.tc * p.toh * p.nsw), lds, s,
                     (const T*)src, (const T*)mask, w, bias, (T*)out, g, p, act, tiles_h, tiles_w, per_h, per_w);
}

template <typename T, int V, bool FLIP>
void pick_conv(const void* src, const void* mask, const float* w, const float* bias, void* out, const DwGeom& g,
               const DwPlan& p, int act, hipStream_t s) {
  if constexpr (V > 1) {
    const bool s1 = g.sw == 1 && (!FLIP || g.sh == 1);
    if (g.dw == 1 && g.dm == 1 && s1) {
      if (g.kw == 3) return launch_conv<T, V, 3, 1, FLIP>(src, mask, w, bias, out, g, p, act, s);
      if (g.kw == 5) return launch_conv<T, V, 5, 1, FLIP>(src, mask, w, bias, out, g, p, act, s);
      if (g.kw == 7) return launch_conv<T, V, 7, 1, FLIP>(src, mask, w, bias, out, g, p, act, s);
    }
    if constexpr (!FLIP) {
      if (g.dw == 1 && g.dm == 1 && g.sw == 2 && g.kw == 3)
        return launch_conv<T, V, 3, 2, false>(src, mask, w, bias, out, g, p, act, s);
    }
  }
  launch_conv<T, V, 0, 1, FLIP>(src, mask, w, bias, out, g, p, act, s);
}

template <bool FLIP>
void conv(const void* src, const void* mask, const float* w, const float* bias, void* out, DwDType dt, const DwGeom& g,
          int act, hipStream_t s) {
  const DwPlan p = dw_plan(g, dt);
  if (dt == DwDType::kF32) {
    if (p.vec == 4) pick_conv<float, 4, FLIP>(src, mask, w, bias, out, g, p, act, s);
    else pick_conv<float, 1, FLIP>(src, mask, w, bias, out, g, p, act, s);
  } else {
    if (p.vec == 8) pick_conv<uint16_t, 8, FLIP>(src, mask, w, bias, out, g, p, act, s);
    else pick_conv<uint16_t, 1, FLIP>(src, mask, w, bias, out, g, p, act, s);
  }
}

template <typename T, int V>
void launch_wgrad(const void* x, const void* dy, const void* mask, double* part, const DwGeom& g, const DwPlan& p,
                  hipStream_t s) {
  const int tiles_h = ceil_div(g.OH, p.toh), tiles_w = ceil_div(g.OW, p.tow);
  const int64_t grid = (int64_t)g.N * p.colblocks * tiles_h * tiles_w;
  const size_t lds = (size_t)V * kT * sizeof(double) +
                     ((size_t)p.hh * p.hw + (size_t)p.toh * p.tow * g.dm) * p.tc * V * sizeof(T);
  hipLaunchKernelGGL((k_dw_wgrad<T, V>), dim3((unsigned)grid), dim3(kT), lds, s, (const T*)x, (const T*)dy,
                     (const T*)mask, part, g, p, tiles_h, tiles_w);
}

}  // namespace

DwPlan dw_plan(const DwGeom& g, DwDType dt) {
  const int es = esize(dt);
  DwPlan p;
  p.vec = (g.dm == 1 && ((int64_t)g.C * es) % 16 == 0) ? 16 / es : 1;
  p.cols = g.C / p.vec;
  const int maxc = p.vec > 1 ? kDwMaxColsVec : kDwMaxColsElem;
  p.tc = 1;
  while (p.tc * 2 <= p.cols && p.tc * 2 <= maxc) p.tc *= 2;
  p.colblocks = ceil_div(p.cols, p.tc);
  const int ns = kT / p.tc;  // strips of a workgroup
  const int mh = g.H > g.OH ? g.H : g.OH, mw = g.W > g.OW ? g.W : g.OW;  // the forward tiles [OH, OW], dgrad [H, W]
  p.nsw = 1;
  while (p.nsw * p.nsw * kS < ns && p.nsw * kS < mw) p.nsw *= 2;
  p.toh = ns / p.nsw;
  while (p.toh > 1 && p.toh / 2 >= mh) p.toh /= 2;
  p.fit = 1;
  for (;;) {
    p.tow = p.nsw * kS;
    p.hh = (p.toh - 1) * g.sh + (g.kh - 1) * g.dh + 1;
    p.hw = (p.tow - 1) * g.sw + (g.kw - 1) * g.dw + 1;
    const int64_t bytes = ((int64_t)p.hh * p.hw + (int64_t)p.toh * p.tow) * g.dm * p.tc * p.vec * es;
    if (bytes <= kDwTileBytes) break;
    if (p.toh > 1) p.toh /= 2;
    else if (p.nsw > 1) p.nsw /= 2;
    else {
      p.fit = 0;
      break;
    }
  }
  const int vt = (g.kh * g.kw + 1) * g.dm;
  p.ts = 1;
  while (p.ts < vt && p.ts < ns) p.ts *= 2;
  return p;
}

void dw_forward(const void* x, const float* w, const float* b, void* y, DwDType dt, const DwGeom& g, int act,
                hipStream_t s) {
  conv<false>(x, nullptr, w, b, y, dt, g, act, s);
}

void dw_dgrad(const void* dy, const void* ymask, const float* w, void* dx, DwDType dt, const DwGeom& g, hipStream_t s) {
  conv<true>(dy, ymask, w, nullptr, dx, dt, g, 0, s);
}

int64_t dw_wgrad_chunks(const DwGeom& g, DwDType dt) {
  const DwPlan p = dw_plan(g, dt);
  return (int64_t)g.N * ceil_div(g.OH, p.toh) * ceil_div(g.OW, p.tow);
}

void dw_wgrad(const void* x, const void* dy, const void* ymask, double* part, float* dW, float* db, int acc,
              DwDType dt, const DwGeom& g, hipStream_t s) {
  const DwPlan p = dw_plan(g, dt);
  if (dt == DwDType::kF32) {
    if (p.vec == 4) launch_wgrad<float, 4>(x, dy, ymask, part, g, p, s);
    else launch_wgrad<float, 1>(x, dy, ymask, part, g, p, s);
  } else {
    if (p.vec == 8) launch_wgrad<uint16_t, 8>(x, dy, ymask, part, g, p, s);
    else launch_wgrad<uint16_t, 1>(x, dy, ymask, part, g, p, s);
  }
  const int64_t n_w = (int64_t)g.kh * g.kw * g.C * g.dm, n_out = n_w + (int64_t)g.C * g.dm;
  hipLaunchKernelGGL(k_dw_wgrad_finalize, dim3((unsigned)((n_out + kFinOut - 1) / kFinOut)), dim3(kT), 0, s, part, dW,
                     db, acc, dw_wgrad_chunks(g, dt), n_w, n_out);
}

}  // namespace tdl
