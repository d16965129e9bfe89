// Seeded dropout: Philox4x32-10 keep masks recomputed in the backward, and a device-side call counter
// (the stream, the mask rule and the ticket protocol: dropout.h).
//
// Full-shape kernel: one 16-B vector per lane per load, kDropoutWgElems elements per workgroup and trip
// (8 vectors in flight per thread in f32, 4 in bf16, all loaded before the first use), a grid capped at
// kDropoutMaxGrid workgroups that strides over the rest; a trip that is not whole takes whole vectors
// while they fit and single elements after.  One Philox call covers four consecutive mask elements, i.e.
// one f32 vector or half a bf16 vector.  Tensors of up to kDropoutSmallN elements run the same kernel at
// kDropoutSmallWgElems elements per workgroup: at 8192 a 64 x 1600 activation would occupy 13 of the 256 CUs.
//
// Broadcast kernel (noise_shape): the mask index is the dot product of the element's coordinates with the
// noise strides (0 on a broadcast dimension).  A thread takes one 16-B vector along the innermost dimension
// (bf16: an 8-B one where that dimension is a multiple of 4 only) and one Philox call per four elements
// where their mask indices are m .. m + 3 of one group, or all m; other shapes take one element and one
// call per thread and trip.  The stream is the same either way.
#include "common.h"
#include "dropout.h"
#include "philox_ticket.h"

namespace tdl {
namespace {

constexpr int kT = kDropoutThreads;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

int g_max_grid = 0;

// the constants of one launch, and the words of a group
struct Rng {
  uint32_t k0, k1, t_lo, t_hi, thr_lo;
  bool all;  // thr == 2^32
  float scale;
  __device__ __forceinline__ void group(u64 g, uint32_t (&o)[4]) const {
    philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), t_lo, t_hi, k0, k1, o);
  }
  __device__ __forceinline__ float apply(float x, uint32_t w) const { return (all || w < thr_lo) ? 0.f : x * scale; }
};

__device__ __forceinline__ uint32_t pick(const uint32_t (&o)[4], uint32_t b) {  // o[b] without a runtime index
  return b == 0 ? o[0] : (b == 1 ? o[1] : (b == 2 ? o[2] : o[3]));
}

__device__ __forceinline__ float bf_lo(uint32_t p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float bf_hi(uint32_t p) { return __uint_as_float(p & 0xffff0000u); }
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const uint16_t* p) { return __uint_as_float((uint32_t)*p << 16); }
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(uint16_t* p, float v) { *p = (uint16_t)pack_bf16x2(v, 0.f); }

__device__ __forceinline__ Rng make_rng(u64 t, uint32_t k0, uint32_t k1, u64 thr, float scale) {
  Rng r;
  r.k0 = k0;
  r.k1 = k1;
  r.t_lo = (uint32_t)t;
  r.t_hi = (uint32_t)(t >> 32);
  r.thr_lo = (uint32_t)thr;
  r.all = (thr >> 32) != 0;
  r.scale = scale;
  return r;
}

// ---- one 16-B vector: 4 f32 (one group) or 8 bf16 (two groups); g = the vector's first group ----
__device__ __forceinline__ f4 vec_apply(const Rng& R, f4 v, u64 g) {
  uint32_t o[4];
  R.group(g, o);
  return f4{R.apply(v[0], o[0]), R.apply(v[1], o[1]), R.apply(v[2], o[2]), R.apply(v[3], o[3])};
}
__device__ __forceinline__ u32x2 half_apply(const Rng& R, uint32_t p0, uint32_t p1, u64 g) {
  uint32_t o[4];
  R.group(g, o);
  return u32x2{pack_bf16x2(R.apply(bf_lo(p0), o[0]), R.apply(bf_hi(p0), o[1])),
               pack_bf16x2(R.apply(bf_lo(p1), o[2]), R.apply(bf_hi(p1), o[3]))};
}
__device__ __forceinline__ u32x4 vec_apply(const Rng& R, u32x4 v, u64 g) {
  const u32x2 a = half_apply(R, v[0], v[1], g);
  const u32x2 b = half_apply(R, v[2], v[3], g + 1);
  return u32x4{a[0], a[1], b[0], b[1]};
}

template <typename T>
struct Vec;
template <>
struct Vec<float> {
  typedef f4 type;
  static constexpr int N = 4;
};
template <>
struct Vec<uint16_t> {
  typedef u32x4 type;
  static constexpr int N = 8;
};

// WG = elements per workgroup and trip: kDropoutWgElems, or kDropoutSmallWgElems (two vectors per thread in f32,
// one in bf16) for tensors of up to kDropoutSmallN elements, which would otherwise leave most CUs idle
template <typename T, int WG>
__global__ __launch_bounds__(kT) void k_dropout(const T* __restrict__ x, T* __restrict__ y, int64_t n, int64_t* state,
                                                const int64_t* ticket_in, int64_t* ticket_out, uint32_t k0,
                                                uint32_t k1, u64 thr, float scale, int64_t off) {
  typedef typename Vec<T>::type V;
  constexpr int N = Vec<T>::N;
  constexpr int U = WG / (kT * N);
  static_assert(WG % (kT * N) == 0 && U >= 1, "a workgroup sweeps its range in whole rows of 16-B vectors");
  const u64 t = ticket_read(state, ticket_in, ticket_out);
  const Rng R = make_rng(t, k0, k1, thr, scale);
  const int tid = threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * WG;
#pragma unroll 1
  for (int64_t base = (int64_t)blockIdx.x * WG; base < n; base += stride) {
    if (base + WG <= n) {
      V v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const V*>(x + base + ((int64_t)u * kT + tid) * N);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = base + ((int64_t)u * kT + tid) * N;
        *reinterpret_cast<V*>(y + i) = vec_apply(R, v[u], (u64)(i + off) >> 2);
      }
    } else {  // the last trip: whole vectors while they fit, then single elements
#pragma unroll 1
      for (int u = 0; u < U; ++u) {
        const int64_t i = base + ((int64_t)u * kT + tid) * N;
        if (i + N <= n) {
          const V v = *reinterpret_cast<const V*>(x + i);
          *reinterpret_cast<V*>(y + i) = vec_apply(R, v, (u64)(i + off) >> 2);
        } else {
          for (int64_t j = i; j < n; ++j) {
            uint32_t o[4];
            const u64 m = (u64)(j + off);
            R.group(m >> 2, o);
            st1(y + j, R.apply(ld1(x + j), pick(o, (uint32_t)m & 3u)));
          }
        }
      }
    }
  }
  ticket_arrive(state, t);
}

// ---- broadcast ----
struct Bcast {
  u64 d1, d2, d3;      // sizes of dimensions 1..3 (dimension 0 is what remains)
  u64 s0, s1, s2, s3;  // noise strides
};

template <typename I>
__device__ __forceinline__ u64 mask_index(const Bcast& b, I i) {  // i = element index
  const I d3 = (I)b.d3, d2 = (I)b.d2, d1 = (I)b.d1;
  const I c3 = i % d3;
  I r = i / d3;
  const I c2 = r % d2;
  r /= d2;
  const I c1 = r % d1;
  const I c0 = r / d1;
  return (u64)c0 * b.s0 + (u64)c1 * b.s1 + (u64)c2 * b.s2 + (u64)c3 * b.s3;
}

// W elements per thread and trip along the innermost dimension: 1, or 4 / 8 (one 16-B vector of f32 / bf16, or
// an 8-B one of bf16) where d3 % W == 0 and the elements' mask indices m + k * s3 fill whole groups (host-checked:
// s3 == 0, or s3 == 1 with every other stride a multiple of 4, so that m % 4 == 0)
template <typename T, typename I, int W>
__global__ __launch_bounds__(kT) void k_dropout_bcast(const T* __restrict__ x, T* __restrict__ y, int64_t n, Bcast b,
                                                      int64_t* state, const int64_t* ticket_in, int64_t* ticket_out,
                                                      uint32_t k0, uint32_t k1, u64 thr, float scale, int64_t off) {
  static_assert(W == 1 || W == 4 || (W == 8 && sizeof(T) == 2), "one element, or an 8-B / 16-B vector");
  const u64 t = ticket_read(state, ticket_in, ticket_out);
  const Rng R = make_rng(t, k0, k1, thr, scale);
  const I items = (I)(n / W);
  const I step = (I)gridDim.x * kT;
  const uint32_t s3 = (uint32_t)b.s3;  // W > 1: 0 or 1
#pragma unroll 1
  for (I it = (I)blockIdx.x * kT + threadIdx.x; it < items; it += step) {
    const I i = it * W;
    const u64 m = mask_index<I>(b, i) + (u64)off;
    uint32_t o[4];
    R.group(m >> 2, o);
    const uint32_t w0 = (uint32_t)m & 3u;  // s3 == 1: 0
    if constexpr (W == 1) {
      st1(y + i, R.apply(ld1(x + i), pick(o, w0)));
    } else {
      uint32_t w[W];
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = pick(o, w0 + k * s3);
      if constexpr (W == 8) {
        if (s3 != 0) R.group((m >> 2) + 1, o);  // elements 4-7 are the next group
#pragma unroll
        for (int k = 0; k < 4; ++k) w[4 + k] = pick(o, w0 + k * s3);
      }
      if constexpr (sizeof(T) == 4) {
        const f4 v = *reinterpret_cast<const f4*>(x + i);
        *reinterpret_cast<f4*>(y + i) =
            f4{R.apply(v[0], w[0]), R.apply(v[1], w[1]), R.apply(v[2], w[2]), R.apply(v[3], w[3])};
      } else {
        typedef uint32_t uv __attribute__((ext_vector_type(W / 2)));
        const uv v = *reinterpret_cast<const uv*>(x + i);
        uv r;
#pragma unroll
        for (int k = 0; k < W / 2; ++k)
          r[k] = pack_bf16x2(R.apply(bf_lo(v[k]), w[2 * k]), R.apply(bf_hi(v[k]), w[2 * k + 1]));
        *reinterpret_cast<uv*>(y + i) = r;
      }
    }
  }
  ticket_arrive(state, t);
}

unsigned grid_for(int64_t work_items, int64_t per_wg) {
  const int64_t cap = g_max_grid > 0 ? g_max_grid : kDropoutMaxGrid;
  int64_t g = (work_items + per_wg - 1) / per_wg;
  if (g < 1) g = 1;  // an empty tensor still takes its ticket
  return (unsigned)(g < cap ? g : cap);
}

template <typename T, typename I, int W>
void launch_bcast(const DropoutArgs& a, const Bcast& b, hipStream_t s) {
  hipLaunchKernelGGL((k_dropout_bcast<T, I, W>), dim3(grid_for(a.n / W, kT)), dim3(kT), 0, s,
                     static_cast<const T*>(a.x), static_cast<T*>(a.y), a.n, b, a.state, a.ticket_in, a.ticket_out, a.k0,
                     a.k1, (u64)a.thr, a.scale, a.elem_offset);
}

template <typename T, int W>
void dispatch_bcast(const DropoutArgs& a, const Bcast& b, hipStream_t s) {
  // 32-bit coordinates while every index (and the stride of the loop past the end) fits
  if (a.n < ((int64_t)1 << 31)) launch_bcast<T, uint32_t, W>(a, b, s);
  else launch_bcast<T, u64, W>(a, b, s);
}

template <typename T, int WG>
void launch_full(const DropoutArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((k_dropout<T, WG>), dim3(grid_for(a.n, WG)), dim3(kT), 0, s, static_cast<const T*>(a.x),
                     static_cast<T*>(a.y), a.n, a.state, a.ticket_in, a.ticket_out, a.k0, a.k1, (u64)a.thr, a.scale,
                     a.elem_offset);
}

}  // namespace

void dropout_force_max_grid(int64_t g) { g_max_grid = g > 0 ? (int)(g < kDropoutMaxGrid ? g : kDropoutMaxGrid) : 0; }

void dropout_apply(const DropoutArgs& a, hipStream_t s) {
  const bool small = a.n <= kDropoutSmallN;
  if (a.bf16) {
    if (small) launch_full<uint16_t, kDropoutSmallWgElems>(a, s);
    else launch_full<uint16_t, kDropoutWgElems>(a, s);
  } else {
    if (small) launch_full<float, kDropoutSmallWgElems>(a, s);
    else launch_full<float, kDropoutWgElems>(a, s);
  }
}

void dropout_apply_bcast(const DropoutArgs& a, const int64_t dims[4], const int64_t nstride[4], hipStream_t s) {
  Bcast b;
  b.d1 = (u64)dims[1];
  b.d2 = (u64)dims[2];
  b.d3 = (u64)dims[3];
  b.s0 = (u64)nstride[0];
  b.s1 = (u64)nstride[1];
  b.s2 = (u64)nstride[2];
  b.s3 = (u64)nstride[3];
  // several elements along the innermost dimension per thread: they must not cross a row (d3 % W == 0), and
  // their mask indices m + k * s3 must fill whole groups: s3 == 0, or s3 == 1 with m % 4 == 0, i.e. every
  // other stride a multiple of 4 (elem_offset is one)
  const bool groups = nstride[3] == 0 ||
                      (nstride[3] == 1 && nstride[0] % 4 == 0 && nstride[1] % 4 == 0 && nstride[2] % 4 == 0);
  const int w = !groups || a.n == 0 ? 1 : (a.bf16 && dims[3] % 8 == 0 ? 8 : (dims[3] % 4 == 0 ? 4 : 1));
  if (a.bf16) {
    if (w == 8) dispatch_bcast<uint16_t, 8>(a, b, s);
    else if (w == 4) dispatch_bcast<uint16_t, 4>(a, b, s);
    else dispatch_bcast<uint16_t, 1>(a, b, s);
  } else {
    if (w == 4) dispatch_bcast<float, 4>(a, b, s);
    else dispatch_bcast<float, 1>(a, b, s);
  }
}

}  // namespace tdl
