// Embedding gather and its ordered, atomic-free gradient for gfx950: see embedding.h for the scheme and the order
// of every sum.
#include "embedding.h"

#include <algorithm>
#include <type_traits>

#include "common.h"

namespace tdl {
namespace {

typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef uint16_t bf16_t;  // storage only

__device__ __forceinline__ float widen(unsigned hi16_in_place) { return __uint_as_float(hi16_in_place); }

// in range: compared as 64-bit signed values before anything is computed from the id
template <class IdT>
__device__ __forceinline__ bool id_in(IdT id, int64_t lo, int64_t hi) {
  return (int64_t)id >= lo && (int64_t)id < hi;
}

// ---------------------------------------------------------------------------------------------- forward
// one access of VEC elements: src is dereferenced only when `valid`
template <class In, class Out, int VEC>
__device__ __forceinline__ void move(const In* src, bool valid, Out* dst) {
  if constexpr (VEC == 1) {
    if constexpr (std::is_same<In, Out>::value) {
      In v = In(0);
      if (valid) v = *src;
      *dst = v;
    } else {
      float v = 0.f;
      if (valid) v = *src;
      *dst = (bf16_t)(pack_bf16x2(v, 0.f) & 0xffffu);
    }
  } else if constexpr (std::is_same<In, Out>::value) {  // 16 bytes in, 16 bytes out
    f4 v = zero4();
    if (valid) v = ld4(reinterpret_cast<const float*>(src));
    st4(reinterpret_cast<float*>(dst), v);
  } else {  // 8 f32 -> 8 bf16, one rounding each
    f4 lo = zero4(), hi = zero4();
    if (valid) {
      lo = ld4(src);
      hi = ld4(src + 4);
    }
    const u4 o = {pack_bf16x2(lo.x, lo.y), pack_bf16x2(lo.z, lo.w), pack_bf16x2(hi.x, hi.y), pack_bf16x2(hi.z, hi.w)};
    *reinterpret_cast<u4*>(dst) = o;
  }
}

// lshift = log2(L): L lanes per row, 64 >> lshift rows per wave
template <class In, class Out, int VEC, class IdT>
__global__ __launch_bounds__(kEmbFwdThreads) void k_embed_fwd(const IdT* __restrict__ ids, const In* __restrict__ table,
                                                              Out* __restrict__ y, int64_t N, int64_t V, int D,
                                                              int lshift) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int L = 1 << lshift, cols = D / VEC;
  const int64_t n = (((int64_t)blockIdx.x * (kEmbFwdThreads / 64) + w) << (6 - lshift)) + (l >> lshift);
  if (n >= N) return;
  const IdT id = ids[n];
  const bool valid = id_in(id, 0, V);
  const In* src = table;
  if (valid) src = table + (size_t)id * D;
  Out* dst = y + (size_t)n * D;
  for (int c = l & (L - 1); c < cols; c += L) move<In, Out, VEC>(src + c * VEC, valid, dst + c * VEC);
}

// ---------------------------------------------------------------------------------------------- count
template <class IdT>
__global__ __launch_bounds__(kEmbCountThreads) void k_embed_count(const IdT* __restrict__ ids, int64_t N, int64_t V,
                                                                 int rows_wg, int* __restrict__ counts) {
  const int64_t n = (int64_t)blockIdx.x * kEmbCountThreads + threadIdx.x;
  const int l = threadIdx.x & 63;
  int r = -1;
  if (n < N) {
    const IdT id = ids[n];
    if (id_in(id, 0, V)) r = (int)((int64_t)id / rows_wg);
  }
  bool act = r >= 0;
  // one atomic per distinct range among the wave's 64 ids
  for (uint64_t m = __ballot(act); m != 0; m = __ballot(act)) {
    const int first = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
    const int rr = __builtin_amdgcn_readlane(r, first);
    const bool same = act && r == rr;
    const uint64_t sm = __ballot(same);
    if (l == first) atomicAdd(&counts[rr], (int)__popcll(sm));
    act = act && !same;
  }
}

// ---------------------------------------------------------------------------------------------- backward
struct EmbBwdArgs {
  const void* ids;
  const void* dy;
  float* out;
  const int* counts;
  int64_t N, V;
  int D, rows_wg, target;
};

// VEC elements of dy in flight, and their addition into VEC f32 accumulators in LDS
template <bool BF, int VEC>
struct Chunk;
template <>
struct Chunk<false, 1> {
  float v;
  __device__ __forceinline__ void load(const float* p) { v = *p; }
  __device__ __forceinline__ void add(float* a) const { *a = *a + v; }
};
template <>
struct Chunk<true, 1> {
  bf16_t v;
  __device__ __forceinline__ void load(const bf16_t* p) { v = *p; }
  __device__ __forceinline__ void add(float* a) const { *a = *a + widen((unsigned)v << 16); }
};
template <>
struct Chunk<false, 4> {
  f4 v;
  __device__ __forceinline__ void load(const float* p) { v = ld4(p); }
  __device__ __forceinline__ void add(float* a) const { st4(a, ld4(a) + v); }
};
template <>
struct Chunk<true, 8> {
  u4 v;
  __device__ __forceinline__ void load(const bf16_t* p) { v = *reinterpret_cast<const u4*>(p); }
  __device__ __forceinline__ void add(float* a) const {
    const f4 lo = {widen(v.x << 16), widen(v.x & 0xffff0000u), widen(v.y << 16), widen(v.y & 0xffff0000u)};
    const f4 hi = {widen(v.z << 16), widen(v.z & 0xffff0000u), widen(v.w << 16), widen(v.w & 0xffff0000u)};
    st4(a, ld4(a) + lo);
    st4(a + 4, ld4(a + 4) + hi);
  }
};

// wave w adds the queue's entries of its rows (local row == w mod 8) into the tile, in queue order
template <bool BF, int VEC>
__device__ __forceinline__ void drain(const int2* queue, int qn, float* acc, int* flags,
                                      const typename std::conditional<BF, bf16_t, float>::type* dy, int D, int w, int l) {
  const int cols = D / VEC;
  for (int cb = 0; cb < cols; cb += 64) {
    const int c = cb + l;
    const bool act = c < cols;
    for (int base = 0; base < qn; base += 64) {
      int2 e = {0, -1};
      if (base + l < qn) e = queue[base + l];
      uint64_t m = __ballot(e.y >= 0 && (e.y & (kEmbBwdWaves - 1)) == w);
      while (m != 0) {
        int row[kEmbPrefetch];
        Chunk<BF, VEC> v[kEmbPrefetch];
#pragma unroll
        for (int k = 0; k < kEmbPrefetch; ++k) {  // the loads of up to 8 entries, ahead of their adds
          row[k] = -1;
          if (m != 0) {
            const int i = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
            m &= m - 1;
            const int n = __builtin_amdgcn_readlane(e.x, i);
            row[k] = __builtin_amdgcn_readlane(e.y, i);
            if (act) v[k].load(dy + (size_t)n * D + c * VEC);
          }
        }
#pragma unroll
        for (int k = 0; k < kEmbPrefetch; ++k) {
          if (row[k] >= 0) {
            if (act) v[k].add(acc + row[k] * D + c * VEC);
            if (cb == 0 && l == 0) flags[row[k]] = 1;
          }
        }
      }
    }
  }
}

template <bool BF, int VEC, class IdT>
__global__ __launch_bounds__(kEmbBwdThreads) void k_embed_bwd(const EmbBwdArgs a) {
  using T = typename std::conditional<BF, bf16_t, float>::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int2* queue = reinterpret_cast<int2*>(smem);                      // [kEmbQueue] (n, local row)
  int* flags = reinterpret_cast<int*>(smem + kEmbQueue * 8);        // [kEmbMaxRowsWg] touched
  int* wtot = flags + kEmbMaxRowsWg;                                // [2][kEmbBwdWaves]
  float* acc = reinterpret_cast<float*>(smem + kEmbLdsFixed);       // [rows_wg][D]
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int D = a.D, cols = D / VEC;
  const int64_t v0 = (int64_t)blockIdx.x * a.rows_wg;
  const int nrows = (int)((a.V - v0) < a.rows_wg ? (a.V - v0) : a.rows_wg);
  const int count = a.counts[blockIdx.x];
  float* out = a.out + (size_t)v0 * D;  // the nrows rows this workgroup owns
  if (count == 0) {
    if (!a.target)
      for (int r = w; r < nrows; r += kEmbBwdWaves)
        for (int c = l; c < cols; c += 64) {
          float* o = out + (size_t)r * D + c * VEC;
          if constexpr (VEC == 1) {
            *o = 0.f;
          } else {
#pragma unroll
            for (int k = 0; k < VEC; k += 4) st4(o + k, zero4());
          }
        }
    return;
  }
  for (int i = tid; i < nrows * D; i += kEmbBwdThreads) acc[i] = -0.f;
  if (tid < kEmbMaxRowsWg) flags[tid] = 0;
  __syncthreads();

  // ---- scan
  const IdT* ids = static_cast<const IdT*>(a.ids);
  const T* dy = static_cast<const T*>(a.dy);
  const int64_t N = a.N, nblk = (N + kEmbScanBlock - 1) / kEmbScanBlock;
  const uint64_t lt = (uint64_t(1) << l) - 1;
  IdT cur[kEmbScanItems], nxt[kEmbScanItems];
#pragma unroll
  for (int j = 0; j < kEmbScanItems; ++j) {
    const int64_t n = (int64_t)tid * kEmbScanItems + j;
    cur[j] = IdT(-1);
    if (n < N) cur[j] = ids[n];
  }
  int qn = 0, found = 0;
  for (int64_t blk = 0; blk < nblk; ++blk) {
    const int64_t n0 = blk * kEmbScanBlock + (int64_t)tid * kEmbScanItems;
#pragma unroll
    for (int j = 0; j < kEmbScanItems; ++j) {  // the next block's ids, ahead of this block's compaction
      const int64_t n = n0 + kEmbScanBlock + j;
      nxt[j] = IdT(-1);
      if (n < N) nxt[j] = ids[n];
    }
    int lr[kEmbScanItems], lower = 0, wt = 0;
#pragma unroll
    for (int j = 0; j < kEmbScanItems; ++j) {
      const bool in = id_in(cur[j], v0, v0 + nrows);
      lr[j] = in ? (int)((int64_t)cur[j] - v0) : -1;
      const uint64_t b = __ballot(in);
      lower += (int)__popcll(b & lt);
      wt += (int)__popcll(b);
    }
    int* tot_w = wtot + (int)(blk & 1) * kEmbBwdWaves;
    if (l == 0) tot_w[w] = wt;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < kEmbBwdWaves; ++i) {  // the waves' offsets, in wave order
      const int t = tot_w[i];
      off += i < w ? t : 0;
      tot += t;
    }
    if (tot != 0) {
      if (qn + tot > kEmbQueue) {  // (same decision in every thread)
        drain<BF, VEC>(queue, qn, acc, flags, dy, D, w, l);
        __syncthreads();
        qn = 0;
      }
      int pos = qn + off + lower;
#pragma unroll
      for (int j = 0; j < kEmbScanItems; ++j)
        if (lr[j] >= 0) queue[pos++] = int2{(int)(n0 + j), lr[j]};
      qn += tot;
      found += tot;
    }
#pragma unroll
    for (int j = 0; j < kEmbScanItems; ++j) cur[j] = nxt[j];
    if (found >= count) break;
  }
  __syncthreads();
  drain<BF, VEC>(queue, qn, acc, flags, dy, D, w, l);
  __syncthreads();

  // ---- epilogue
  for (int r = w; r < nrows; r += kEmbBwdWaves) {
    const bool touched = flags[r] != 0;
    if (a.target && !touched) continue;
    for (int c = l; c < cols; c += 64) {
      float* o = out + (size_t)r * D + c * VEC;
      const float* s = acc + r * D + c * VEC;
      if constexpr (VEC == 1) {
        if (a.target) *o = *o + *s;
        else *o = touched ? *s : 0.f;
      } else {
#pragma unroll
        for (int k = 0; k < VEC; k += 4) {
          if (a.target) st4(o + k, ld4(o + k) + ld4(s + k));
          else st4(o + k, touched ? ld4(s + k) : zero4());
        }
      }
    }
  }
}

int pow2_at_least(int x) {
  int p = 1;
  while (p < x) p <<= 1;
  return p;
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

template <class In, class Out, int VEC>
void launch_fwd(const void* ids, bool ids64, const void* table, void* y, int64_t N, int64_t V, int D, hipStream_t s) {
  const int L = std::min(64, pow2_at_least(D / VEC));
  int lshift = 0;
  while ((1 << lshift) < L) ++lshift;
  const int rows = kEmbFwdThreads / L;
  const dim3 grid((unsigned)((N + rows - 1) / rows));
  if (ids64)
    hipLaunchKernelGGL((k_embed_fwd<In, Out, VEC, int64_t>), grid, dim3(kEmbFwdThreads), 0, s,
                       static_cast<const int64_t*>(ids), static_cast<const In*>(table), static_cast<Out*>(y), N, V, D, lshift);
  else
    hipLaunchKernelGGL((k_embed_fwd<In, Out, VEC, int32_t>), grid, dim3(kEmbFwdThreads), 0, s,
                       static_cast<const int32_t*>(ids), static_cast<const In*>(table), static_cast<Out*>(y), N, V, D, lshift);
}

template <bool BF, int VEC, class IdT>
void launch_bwd(const EmbBwdArgs& a, const EmbPlan& p, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)k_embed_bwd<BF, VEC, IdT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              kEmbLdsBudget);
    attr = true;
  }
  hipLaunchKernelGGL((k_embed_bwd<BF, VEC, IdT>), dim3((unsigned)p.ranges), dim3(kEmbBwdThreads), p.lds_bwd, s, a);
}

template <bool BF, int VEC>
void launch_bwd_ids(const EmbBwdArgs& a, bool ids64, const EmbPlan& p, hipStream_t s) {
  if (ids64) launch_bwd<BF, VEC, int64_t>(a, p, s);
  else launch_bwd<BF, VEC, int32_t>(a, p, s);
}

}  // namespace

EmbPlan embed_plan(int64_t N, int64_t V, int D, bool bf16) {
  EmbPlan p;
  const int v = bf16 ? 8 : 4;
  p.vec = D % v == 0 ? v : 1;
  p.L = std::min(64, pow2_at_least(D / p.vec));
  p.rows_per_wave_fwd = 64 / p.L;
  const int rows = (kEmbFwdThreads / 64) * p.rows_per_wave_fwd;
  p.fwd_blocks = (N + rows - 1) / rows;
  p.rows_wg = std::min<int64_t>(kEmbMaxRowsWg, (kEmbLdsBudget - kEmbLdsFixed) / (int64_t(4) * D));
  p.ranges = (V + p.rows_wg - 1) / p.rows_wg;
  p.lds_bwd = kEmbLdsFixed + p.rows_wg * D * 4;
  return p;
}
static_assert((kEmbLdsBudget - kEmbLdsFixed) / (4 * kEmbMaxD) >= kEmbBwdWaves, "a row of the tile per wave at the widest D");
static_assert(kEmbLdsFixed % 16 == 0 && kEmbQueue >= kEmbScanBlock, "tile alignment; a scan block fits an empty queue");

void embed_forward(const void* ids, bool ids64, const void* table, bool table_bf16, void* y, bool out_bf16, int64_t N,
                   int64_t V, int D, hipStream_t s) {
  const EmbPlan p = embed_plan(N, V, D, out_bf16);
  const bool vec = p.vec > 1 && aligned16(table) && aligned16(y);
  if (!out_bf16) {
    if (vec) launch_fwd<float, float, 4>(ids, ids64, table, y, N, V, D, s);
    else launch_fwd<float, float, 1>(ids, ids64, table, y, N, V, D, s);
  } else if (table_bf16) {
    if (vec) launch_fwd<bf16_t, bf16_t, 8>(ids, ids64, table, y, N, V, D, s);
    else launch_fwd<bf16_t, bf16_t, 1>(ids, ids64, table, y, N, V, D, s);
  } else {
    if (vec) launch_fwd<float, bf16_t, 8>(ids, ids64, table, y, N, V, D, s);
    else launch_fwd<float, bf16_t, 1>(ids, ids64, table, y, N, V, D, s);
  }
}

void embed_backward(const void* ids, bool ids64, const void* dy, bool dy_bf16, float* out, bool target, int* counts,
                    int64_t N, int64_t V, int D, hipStream_t s) {
  const EmbPlan p = embed_plan(N, V, D, dy_bf16);
  const dim3 cgrid((unsigned)((N + kEmbCountThreads - 1) / kEmbCountThreads));
  if (ids64)
    hipLaunchKernelGGL(k_embed_count<int64_t>, cgrid, dim3(kEmbCountThreads), 0, s, static_cast<const int64_t*>(ids), N, V,
                       p.rows_wg, counts);
  else
    hipLaunchKernelGGL(k_embed_count<int32_t>, cgrid, dim3(kEmbCountThreads), 0, s, static_cast<const int32_t*>(ids), N, V,
                       p.rows_wg, counts);
  const EmbBwdArgs a{ids, dy, out, counts, N, V, D, p.rows_wg, target ? 1 : 0};
  const bool vec = p.vec > 1 && aligned16(dy) && aligned16(out);
  if (dy_bf16) {
    if (vec) launch_bwd_ids<true, 8>(a, ids64, p, s);
    else launch_bwd_ids<true, 1>(a, ids64, p, s);
  } else {
    if (vec) launch_bwd_ids<false, 4>(a, ids64, p, s);
    else launch_bwd_ids<false, 1>(a, ids64, p, s);
  }
}

}  // namespace tdl
