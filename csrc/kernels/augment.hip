// Seeded image augmentation: random flip, crop and whole-pixel translation of an NHWC batch in one launch per
// direction (the draws, the coordinate map, the fill modes and the backward's order: augment.h; the ticket
// protocol: dropout.h).
//
// Both kernels are memory bound: 256 threads, kAugmentWgElems work items per workgroup and grid-stride trip
// (four per thread, every load of a thread issued before its first store), a grid capped at kAugmentMaxGrid
// workgroups (the forward, whose workgroups all arrive at one counter word: kAugmentFwdMaxGrid).  A work item
// is one 16-B vector along C (a flip reverses pixels, never channels, so the vector stays whole) or, where
// C * element size is no multiple of 16 or a pointer is not 16-B aligned, one element.
// The forward moves bits and is instantiated per item size only; the backward adds in f32 and is instantiated
// per dtype.  A thread draws once per sample: consecutive items of a thread mostly share their sample, and the
// Philox call is repeated only where the sample changes.  Coordinates are 32-bit while every item index fits.
#include "common.h"
#include "augment.h"
#include "philox_ticket.h"

namespace tdl {
namespace {

constexpr int kT = kAugmentThreads;
constexpr int kU = kAugmentWgElems / kT;
static_assert(kAugmentWgElems % kT == 0 && kU >= 1, "a workgroup sweeps its range in whole rows of items");
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

int g_max_grid = 0;

struct Geo {
  int H, W, Ho, Wo, CV;  // CV: work items along C
};

struct Draw {
  int flip_h, flip_w, off_h, off_w;
};

__device__ __forceinline__ Draw draw_for(u64 n, u64 t, uint32_t k0, uint32_t k1, const AugmentSpec& sp) {
  uint32_t o[4];
  philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), (uint32_t)t, (uint32_t)(t >> 32), k0, k1, o);
  Draw d;
  d.flip_w = sp.flip_w ? (int)(o[0] >> 31) : 0;
  d.flip_h = sp.flip_h ? (int)(o[1] >> 31) : 0;
  d.off_h = sp.off_h_lo + (int)(((u64)o[2] * (uint32_t)sp.off_h_count) >> 32);
  d.off_w = sp.off_w_lo + (int)(((u64)o[3] * (uint32_t)sp.off_w_count) >> 32);
  return d;
}

// the forward map of one axis: the source coordinate of output coordinate o, or -1 = the fill value.
// Lo <= L and |off| <= L (host-checked) keep r in [-L, 2 L - 1]: one wrap or reflection suffices.
__device__ __forceinline__ int src_coord(int o, int flip, int off, int Lo, int L, int mode) {
  const int r = (flip ? Lo - 1 - o : o) + off;
  if ((unsigned)r < (unsigned)L) return r;
  if (mode == kConstant) return -1;
  if (mode == kNearest) return r < 0 ? 0 : L - 1;
  if (mode == kWrap) return r < 0 ? r + L : r - L;
  return r < 0 ? -1 - r : 2 * L - 1 - r;
}

// item index -> (n, row, column, item along C) of a [N, R, S, CV] tensor
template <typename I>
__device__ __forceinline__ void decode(I i, int R, int S, int CV, I& n, int& r, int& s, int& cv) {
  cv = (int)(i % (I)CV);
  I p = i / (I)CV;
  s = (int)(p % (I)S);
  p /= (I)S;
  r = (int)(p % (I)R);
  n = p / (I)R;
}

// ---- forward: y[n, oh, ow, :] = x[n, src(oh), src(ow), :] or the fill ----
template <typename V, typename I>
__global__ __launch_bounds__(kT) void k_augment_fwd(const V* __restrict__ x, V* __restrict__ y, I items, Geo g,
                                                    int64_t* state, const int64_t* ticket_in, int64_t* ticket_out,
                                                    uint32_t k0, uint32_t k1, AugmentSpec sp, V fill) {
  const u64 t = ticket_read(state, ticket_in, ticket_out);
  const I stride = (I)gridDim.x * kAugmentWgElems;
#pragma unroll 1
  for (I base = (I)blockIdx.x * kAugmentWgElems; base < items; base += stride) {
    V v[kU];
    I cur = ~(I)0;
    Draw d = {0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const I i = base + (I)(u * kT) + threadIdx.x;
      v[u] = fill;
      if (i < items) {
        I n;
        int oh, ow, cv;
        decode<I>(i, g.Ho, g.Wo, g.CV, n, oh, ow, cv);
        if (n != cur) {
          d = draw_for((u64)n, t, k0, k1, sp);
          cur = n;
        }
        const int rh = src_coord(oh, d.flip_h, d.off_h, g.Ho, g.H, sp.fill_mode);
        const int rw = src_coord(ow, d.flip_w, d.off_w, g.Wo, g.W, sp.fill_mode);
        if (rh >= 0 && rw >= 0) v[u] = x[((n * (I)g.H + (I)rh) * (I)g.W + (I)rw) * (I)g.CV + (I)cv];
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const I i = base + (I)(u * kT) + threadIdx.x;
      if (i < items) y[i] = v[u];
    }
  }
  ticket_arrive(state, t);
}

// ---- backward ----
// The output coordinates that may read input coordinate i along one axis, as up to three ascending,
// disjoint runs [a[k], b[k]] (empty: a > b); every member is still confirmed with src_coord.
__device__ __forceinline__ void candidates(int i, int flip, int off, int Lo, int L, int mode, int (&a)[3],
                                           int (&b)[3]) {
  // before the flip is undone (o' = r - off), ascending
  int lo[3] = {1, 1, 1}, hi[3] = {0, 0, 0};
  if (mode == kNearest) {  // an edge collects every r beyond it: a run of up to |off| + 1
    const int l = i == 0 ? 0 : i - off;
    const int h = i == L - 1 ? Lo - 1 : i - off;
    lo[0] = l > 0 ? l : 0;
    hi[0] = h < Lo - 1 ? h : Lo - 1;
  } else if (mode == kReflect) {  // r = -1 - i (below), i, 2 L - 1 - i (above)
    const int c[3] = {-1 - i - off, i - off, 2 * L - 1 - i - off};
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if ((unsigned)c[k] < (unsigned)Lo) lo[k] = hi[k] = c[k];
  } else {
    int c = i - off;  // in [-L, 2 L - 1]
    if (mode == kWrap) c = c < 0 ? c + L : (c >= L ? c - L : c);  // the one o' = i - off (mod L) below Lo <= L
    if ((unsigned)c < (unsigned)Lo) lo[0] = hi[0] = c;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a[k] = flip ? Lo - 1 - hi[2 - k] : lo[k];
    b[k] = flip ? Lo - 1 - lo[2 - k] : hi[k];
  }
}

__device__ __forceinline__ float bf_lo(uint32_t p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float bf_hi(uint32_t p) { return __uint_as_float(p & 0xffff0000u); }

// one work item of NV values of dtype T: the f32 accumulator, its load-and-add and its rounded store
template <typename T, bool VEC>
struct Item;
template <>
struct Item<float, false> {
  static constexpr int NV = 1;
  typedef float type;
  static __device__ __forceinline__ void add(float (&acc)[1], const float* p) { acc[0] += *p; }
  static __device__ __forceinline__ void store(float* p, const float (&acc)[1]) { *p = acc[0]; }
};
template <>
struct Item<float, true> {
  static constexpr int NV = 4;
  typedef f4 type;
  static __device__ __forceinline__ void add(float (&acc)[4], const f4* p) {
    const f4 v = *p;
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += v[k];
  }
  static __device__ __forceinline__ void store(f4* p, const float (&acc)[4]) { *p = f4{acc[0], acc[1], acc[2], acc[3]}; }
};
template <>
struct Item<uint16_t, false> {
  static constexpr int NV = 1;
  typedef uint16_t type;
  static __device__ __forceinline__ void add(float (&acc)[1], const uint16_t* p) {
    acc[0] += __uint_as_float((uint32_t)*p << 16);
  }
  static __device__ __forceinline__ void store(uint16_t* p, const float (&acc)[1]) {
    *p = (uint16_t)pack_bf16x2(acc[0], 0.f);
  }
};
template <>
struct Item<uint16_t, true> {
  static constexpr int NV = 8;
  typedef u32x4 type;
  static __device__ __forceinline__ void add(float (&acc)[8], const u32x4* p) {
    const u32x4 v = *p;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      acc[2 * k] += bf_lo(v[k]);
      acc[2 * k + 1] += bf_hi(v[k]);
    }
  }
  static __device__ __forceinline__ void store(u32x4* p, const float (&acc)[8]) {
    *p = u32x4{pack_bf16x2(acc[0], acc[1]), pack_bf16x2(acc[2], acc[3]), pack_bf16x2(acc[4], acc[5]),
               pack_bf16x2(acc[6], acc[7])};
  }
};

template <typename T, bool VEC, typename I>
__global__ __launch_bounds__(kT) void k_augment_bwd(const typename Item<T, VEC>::type* __restrict__ dy,
                                                    typename Item<T, VEC>::type* __restrict__ dx, I items, Geo g,
                                                    const int64_t* ticket_in, uint32_t k0, uint32_t k1,
                                                    AugmentSpec sp) {
  typedef Item<T, VEC> IT;
  constexpr int NV = IT::NV;
  const u64 t = ticket_read(nullptr, ticket_in, nullptr);
  const I stride = (I)gridDim.x * kAugmentWgElems;
  const int mode = sp.fill_mode;
#pragma unroll 1
  for (I base = (I)blockIdx.x * kAugmentWgElems; base < items; base += stride) {
    float acc[kU][NV];
    I cur = ~(I)0;
    Draw d = {0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < kU; ++u) {
#pragma unroll
      for (int k = 0; k < NV; ++k) acc[u][k] = 0.f;
      const I i = base + (I)(u * kT) + threadIdx.x;
      if (i < items) {
        I n;
        int ih, iw, cv;
        decode<I>(i, g.H, g.W, g.CV, n, ih, iw, cv);
        if (n != cur) {
          d = draw_for((u64)n, t, k0, k1, sp);
          cur = n;
        }
        int ah[3], bh[3], aw[3], bw[3];
        candidates(ih, d.flip_h, d.off_h, g.Ho, g.H, mode, ah, bh);
        candidates(iw, d.flip_w, d.off_w, g.Wo, g.W, mode, aw, bw);
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
#pragma unroll 1
          for (int oh = ah[kh]; oh <= bh[kh]; ++oh) {
            if (src_coord(oh, d.flip_h, d.off_h, g.Ho, g.H, mode) != ih) continue;
            const I row = (n * (I)g.Ho + (I)oh) * (I)g.Wo;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
#pragma unroll 1
              for (int ow = aw[kw]; ow <= bw[kw]; ++ow) {
                if (src_coord(ow, d.flip_w, d.off_w, g.Wo, g.W, mode) != iw) continue;
                IT::add(acc[u], dy + ((row + (I)ow) * (I)g.CV + (I)cv));
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const I i = base + (I)(u * kT) + threadIdx.x;
      if (i < items) IT::store(dx + i, acc[u]);
    }
  }
}

unsigned grid_for(int64_t items, int max_grid) {
  const int64_t cap = g_max_grid > 0 && g_max_grid < max_grid ? g_max_grid : max_grid;
  int64_t g = (items + kAugmentWgElems - 1) / kAugmentWgElems;
  if (g < 1) g = 1;  // an empty tensor still takes its ticket
  return (unsigned)(g < cap ? g : cap);
}

struct Plan {
  bool vec;
  int esize;
  Geo g;
  int64_t in_items, out_items;  // of [N, H, W, CV] and [N, Ho, Wo, CV]
  bool small;                   // every item index (and the loop's step past the end) fits 32 bits
};

Plan plan_for(const AugmentArgs& a) {
  Plan p;
  p.esize = a.bf16 ? 2 : 4;
  const int64_t row = (int64_t)a.C * p.esize;
  p.vec = row % 16 == 0 && reinterpret_cast<uintptr_t>(a.src) % 16 == 0 &&
          reinterpret_cast<uintptr_t>(a.dst) % 16 == 0;
  p.g = Geo{a.H, a.W, a.Ho, a.Wo, p.vec ? (int)(row / 16) : a.C};
  p.in_items = a.N * a.H * a.W * p.g.CV;
  p.out_items = a.N * a.Ho * a.Wo * p.g.CV;
  p.small = p.in_items < ((int64_t)1 << 31) && p.out_items < ((int64_t)1 << 31);
  return p;
}

template <typename V, typename I>
void launch_fwd(const AugmentArgs& a, const Plan& p, V fill, hipStream_t s) {
  hipLaunchKernelGGL((k_augment_fwd<V, I>), dim3(grid_for(p.out_items, kAugmentFwdMaxGrid)), dim3(kT), 0, s, static_cast<const V*>(a.src),
                     static_cast<V*>(a.dst), (I)p.out_items, p.g, a.state, a.ticket_in, a.ticket_out, a.k0, a.k1,
                     a.spec, fill);
}

template <typename V>
void dispatch_fwd(const AugmentArgs& a, const Plan& p, V fill, hipStream_t s) {
  if (p.small) launch_fwd<V, uint32_t>(a, p, fill, s);
  else launch_fwd<V, u64>(a, p, fill, s);
}

template <typename T, bool VEC>
void dispatch_bwd(const AugmentArgs& a, const Plan& p, hipStream_t s) {
  typedef typename Item<T, VEC>::type V;
  if (p.small)
    hipLaunchKernelGGL((k_augment_bwd<T, VEC, uint32_t>), dim3(grid_for(p.in_items, kAugmentMaxGrid)), dim3(kT), 0, s,
                       static_cast<const V*>(a.src), static_cast<V*>(a.dst), (uint32_t)p.in_items, p.g, a.ticket_in,
                       a.k0, a.k1, a.spec);
  else
    hipLaunchKernelGGL((k_augment_bwd<T, VEC, u64>), dim3(grid_for(p.in_items, kAugmentMaxGrid)), dim3(kT), 0, s,
                       static_cast<const V*>(a.src), static_cast<V*>(a.dst), (u64)p.in_items, p.g, a.ticket_in, a.k0,
                       a.k1, a.spec);
}

}  // namespace

void augment_force_max_grid(int64_t g) { g_max_grid = g > 0 ? (int)(g < kAugmentMaxGrid ? g : kAugmentMaxGrid) : 0; }

void augment_forward(const AugmentArgs& a, hipStream_t s) {
  const Plan p = plan_for(a);
  const uint32_t b = a.spec.fill_bits;
  if (p.vec) {
    const uint32_t w = a.bf16 ? ((b & 0xffffu) | (b << 16)) : b;
    dispatch_fwd<u32x4>(a, p, u32x4{w, w, w, w}, s);
  } else if (a.bf16) {
    dispatch_fwd<uint16_t>(a, p, (uint16_t)b, s);
  } else {
    dispatch_fwd<uint32_t>(a, p, b, s);
  }
}

void augment_backward(const AugmentArgs& a, hipStream_t s) {
  const Plan p = plan_for(a);
  if (a.bf16) {
    if (p.vec) dispatch_bwd<uint16_t, true>(a, p, s);
    else dispatch_bwd<uint16_t, false>(a, p, s);
  } else {
    if (p.vec) dispatch_bwd<float, true>(a, p, s);
    else dispatch_bwd<float, false>(a, p, s);
  }
}

}  // namespace tdl
