// Fused attention kernels for gfx950 (see attention.h).
#include "attention.h"

#include <algorithm>

#include "common.h"
#include "philox_ticket.h"

namespace tdl {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// Element type, 16-byte fragment and LDS layout of an instantiation.
template <bool BF, int HD>
struct Lay;
template <int HD>
struct Lay<false, HD> {
  using T = float;
  using Frag = f4;
  static constexpr int E = 4;  // elements per fragment
};
template <int HD>
struct Lay<true, HD> {
  using T = uint16_t;
  using Frag = bf16x8;
  static constexpr int E = 8;
};
template <bool BF, int HD>
struct Dim {
  static constexpr int E = Lay<BF, HD>::E;
  static constexpr int KC = 4 * E;             // k of one fragment step: 4 MFMAs of k = 4, or 1 of k = 32
  static constexpr int SN = HD + E;            // row stride of a [64][HD] tile
  static constexpr int ST = kAttnTile + E;     // row stride of a transposed [HD][64] tile and of a strip
  static constexpr int NCH = HD / KC;          // fragment steps along the head dimension
  static constexpr int NTH = HD / 16;          // column tiles along the head dimension
  static constexpr int KCH = kAttnTile / KC;   // fragment steps along a key / query tile
  static constexpr int NAT = kAttnTile * SN;   // elements of a tile
  static constexpr int TRN = HD * ST;          // elements of a transposed tile
  static constexpr int STRIP = 4 * 16 * ST;    // the four waves' strips
};

__device__ __forceinline__ f4 mma(f4 a, f4 b, f4 c) {
#pragma unroll
  for (int j = 0; j < 4; ++j) c = mfma16x16x4(a[j], b[j], c);
  return c;
}
__device__ __forceinline__ f4 mma(bf16x8 a, bf16x8 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

template <class Frag>
__device__ __forceinline__ Frag ldfrag(const void* p) {
  return __builtin_bit_cast(Frag, *reinterpret_cast<const u4v*>(p));
}
template <class Frag>
__device__ __forceinline__ Frag zfrag() {
  return __builtin_bit_cast(Frag, u4v{0u, 0u, 0u, 0u});
}
__device__ __forceinline__ void put(float* p, float v) { *p = v; }
__device__ __forceinline__ void put(uint16_t* p, float v) { *p = (uint16_t)(pack_bf16x2(v, 0.f) & 0xffffu); }

// all-reduce over the 16 lanes of a row (every lane ends with the same bits: each step adds a value to its
// partner's in both lanes)
__device__ __forceinline__ float row_max(float x) {
  x = fmaxf(x, dpp_xor8(x));
  x = fmaxf(x, dpp_mirror8(x));
  x = fmaxf(x, dpp_xor2(x));
  return fmaxf(x, dpp_xor1(x));
}
__device__ __forceinline__ float row_sum(float x) {
  x += dpp_xor8(x);
  x += dpp_mirror8(x);
  x += dpp_xor2(x);
  return x + dpp_xor1(x);
}

// rows [row0, row0 + 64) of a [rows][d] operand (row stride rs) into LDS: as they are (nat, [64][SN]) and / or
// transposed (tr, [HD][ST]); zeros past the last row and past d
template <bool BF, int HD, bool NAT, bool TR>
__device__ __forceinline__ void stage(typename Lay<BF, HD>::T* nat, typename Lay<BF, HD>::T* tr,
                                      const typename Lay<BF, HD>::T* g, int64_t rs, int row0, int rows, int d) {
  using T = typename Lay<BF, HD>::T;
  using Frag = typename Lay<BF, HD>::Frag;
  using M = Dim<BF, HD>;
  constexpr int FR = HD / M::E;
  for (int idx = threadIdx.x; idx < kAttnTile * FR; idx += kThreads) {
    const int r = idx / FR, f = idx % FR;
    union {
      Frag v;
      T e[M::E];
    } u;
    u.v = zfrag<Frag>();
    if (row0 + r < rows && f * M::E < d) u.v = ldfrag<Frag>(g + (int64_t)(row0 + r) * rs + f * M::E);
    if (NAT) *reinterpret_cast<Frag*>(nat + r * M::SN + f * M::E) = u.v;
    if (TR) {
#pragma unroll
      for (int e = 0; e < M::E; ++e) tr[(f * M::E + e) * M::ST + r] = u.e[e];
    }
  }
}

__device__ __forceinline__ bool admitted(const AttnArgs& a, int b, int h, int row, int key) {
  bool ok = row < a.T && key < a.S && (!a.causal || key <= row);
  if (ok && a.mask != nullptr) ok = a.mask[b * a.ms[0] + h * a.ms[1] + row * a.ms[2] + key * a.ms[3]] != 0;
  return ok;
}

// ---- attention dropout (attention.h): the constants of a launch, the words of a group, the keep rule ----
struct Drop {
  uint32_t k0, k1, t_lo, t_hi, thr_lo;
  bool all;  // thr == 2^32
  float c;
  __device__ __forceinline__ void block(uint64_t g, uint32_t (&o)[4]) const {
    philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), t_lo, t_hi, k0, k1, o);
  }
  __device__ __forceinline__ bool keep(uint32_t w) const { return !all && w >= thr_lo; }
};
__device__ __forceinline__ unsigned wg_linear() { return blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z); }
__device__ __forceinline__ unsigned wg_count() { return gridDim.x * gridDim.y * gridDim.z; }
__device__ __forceinline__ Drop make_drop(const AttnArgs& a, unsigned long long t) {
  Drop r;
  r.k0 = a.k0, r.k1 = a.k1;
  r.t_lo = (uint32_t)t, r.t_hi = (uint32_t)(t >> 32);
  r.thr_lo = (uint32_t)a.thr, r.all = (a.thr >> 32) != 0;
  r.c = a.keep;
  return r;
}
// group of mask elements (rows 4 rg .. 4 rg + 3, key 0) of (b, h); the key is added to it
__device__ __forceinline__ uint64_t drop_group(const AttnArgs& a, int b, int h, int rg) {
  return (((uint64_t)b * a.H + h) * (uint64_t)((a.T + 3) >> 2) + (uint64_t)rg) * (uint64_t)a.S;
}
__device__ __forceinline__ uint32_t quad_xor1(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t quad_xor2(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, false);
}
// the lane at position n of a quad enters with row n of a 4 x 4 matrix and leaves with column n (o[i] = word n of
// lane i's row): 2 x 2 blocks exchanged within the pairs (xor 1), then between them (xor 2)
__device__ __forceinline__ void quad_transpose(uint32_t (&o)[4], int n) {
  const bool b0 = (n & 1) != 0, b1 = (n & 2) != 0;
#pragma unroll
  for (int p = 0; p < 4; p += 2) {
    const uint32_t r = quad_xor1(b0 ? o[p] : o[p + 1]);
    o[p] = b0 ? r : o[p];
    o[p + 1] = b0 ? o[p + 1] : r;
  }
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const uint32_t r = quad_xor2(b1 ? o[p] : o[p + 2]);
    o[p] = b1 ? r : o[p];
    o[p + 2] = b1 ? o[p + 2] : r;
  }
}

// ---- forward ----
template <bool BF, int HD, bool DROP>
__global__ __launch_bounds__(kThreads) void k_attn_fwd(const AttnArgs a) {
  using T = typename Lay<BF, HD>::T;
  using Frag = typename Lay<BF, HD>::Frag;
  using M = Dim<BF, HD>;
  __shared__ __attribute__((aligned(16))) T sK[M::NAT];
  __shared__ __attribute__((aligned(16))) T sVt[M::TRN];
  __shared__ __attribute__((aligned(16))) T sP[M::STRIP];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 15, g = l >> 4;
  const int qt = blockIdx.x, h = blockIdx.y, b = blockIdx.z, q0 = qt * kAttnTile;
  const T* q = (const T*)a.q + b * a.qs[0] + h * a.qs[2];
  const T* k = (const T*)a.k + b * a.ks[0] + h * a.ks[2];
  const T* v = (const T*)a.v + b * a.vs[0] + h * a.vs[2];
  const float cs = a.scale * kLog2e;

  Frag aq[M::NCH];
  {
    const int row = q0 + 16 * w + c;
#pragma unroll
    for (int ch = 0; ch < M::NCH; ++ch) {
      const int d = ch * M::KC + g * M::E;
      aq[ch] = (row < a.T && d < a.D) ? ldfrag<Frag>(q + (int64_t)row * a.qs[1] + d) : zfrag<Frag>();
    }
  }
  f4 O[M::NTH];
#pragma unroll
  for (int t = 0; t < M::NTH; ++t) O[t] = zero4();
  float m[4], ls[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = -INFINITY, ls[i] = 0.f;
  const int r0 = q0 + 16 * w + 4 * g;  // this lane's accumulator rows r0 + i
  T* strip = sP + w * 16 * M::ST;
  Drop R;
  uint64_t gq = 0;  // the group of (rows r0 .. r0 + 3, key c)
  unsigned long long ticket = 0;
  if constexpr (DROP) {
    ticket = ticket_read(a.state, a.ticket_in, a.ticket_out, wg_linear());
    R = make_drop(a, ticket);
    gq = drop_group(a, b, h, r0 >> 2) + c;
  }

  const int kts = (a.S + kAttnTile - 1) / kAttnTile;
  const int nkt = a.causal ? min(kts, qt + 1) : kts;
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * kAttnTile;
    __syncthreads();
    stage<BF, HD, true, false>(sK, nullptr, k, a.ks[1], k0, a.S, a.D);
    stage<BF, HD, false, true>(nullptr, sVt, v, a.vs[1], k0, a.S, a.Dv);
    __syncthreads();
    // the tile's keep bits (bit 4 t + i: row r0 + i, key k0 + 16 t + c), from indices alone: ahead of the MFMA
    // chain, so that the scheduler runs the Philox rounds under it
    uint32_t zm = 0;
    if constexpr (DROP) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        uint32_t o[4];
        R.block(gq + (uint64_t)(k0 + 16 * t), o);
#pragma unroll
        for (int i = 0; i < 4; ++i) zm |= (uint32_t)R.keep(o[i]) << (4 * t + i);
      }
    }
    f4 s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s[t] = zero4();
#pragma unroll
      for (int ch = 0; ch < M::NCH; ++ch)
        s[t] = mma(aq[ch], ldfrag<Frag>(sK + (16 * t + c) * M::SN + ch * M::KC + g * M::E), s[t]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        s[t][i] = admitted(a, b, h, r0 + i, k0 + 16 * t + c) ? s[t][i] * cs : -INFINITY;
        mx = fmaxf(mx, s[t][i]);
      }
      const float mn = fmaxf(m[i], row_max(mx));
      const float mu = mn == -INFINITY ? 0.f : mn;
      const float al = __builtin_amdgcn_exp2f(m[i] - mu);
      float rs = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float p = __builtin_amdgcn_exp2f(s[t][i] - mu);
        rs += p;  // (the undropped row's sum)
        if constexpr (DROP) put(strip + (4 * g + i) * M::ST + 16 * t + c, (zm >> (4 * t + i)) & 1u ? p * R.c : 0.f);
        else put(strip + (4 * g + i) * M::ST + 16 * t + c, p);
      }
      ls[i] = ls[i] * al + row_sum(rs);
      m[i] = mn;
#pragma unroll
      for (int t = 0; t < M::NTH; ++t) O[t][i] *= al;
    }
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < M::KCH; ++ch) {
      const Frag ap = ldfrag<Frag>(strip + c * M::ST + ch * M::KC + g * M::E);
#pragma unroll
      for (int t = 0; t < M::NTH; ++t)
        if (16 * t < a.Dv) O[t] = mma(ap, ldfrag<Frag>(sVt + (16 * t + c) * M::ST + ch * M::KC + g * M::E), O[t]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = r0 + i;
    if (row >= a.T) continue;
    const float inv = ls[i] > 0.f ? 1.f / ls[i] : 0.f;
    const int64_t base = (((int64_t)b * a.T + row) * a.H + h) * a.Dv;
#pragma unroll
    for (int t = 0; t < M::NTH; ++t) {
      const int col = 16 * t + c;
      if (col < a.Dv) put((T*)a.o + base + col, O[t][i] * inv);
    }
    if (c == 0)
      a.lse[((int64_t)b * a.H + h) * a.T + row] = ls[i] > 0.f ? (m[i] + __builtin_amdgcn_logf(ls[i])) * kLn2 : -INFINITY;
  }
  if constexpr (DROP) ticket_arrive(a.state, ticket, wg_count());
}

// ---- delta = rowsum(do * o) ----
__device__ __forceinline__ float elem(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float elem(const uint16_t* p, int64_t i) { return __uint_as_float((uint32_t)p[i] << 16); }

template <class T>
__global__ __launch_bounds__(kThreads) void k_attn_delta(const AttnArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;  // (b, h, i)
  if (idx >= (int64_t)a.B * a.H * a.T) return;
  const int i = (int)(idx % a.T), h = (int)((idx / a.T) % a.H), b = (int)(idx / ((int64_t)a.T * a.H));
  const T* g = (const T*)a.dout + b * a.gs[0] + i * a.gs[1] + h * a.gs[2];
  const T* o = (const T*)a.o + (((int64_t)b * a.T + i) * a.H + h) * a.Dv;
  float s = 0.f;
  for (int d = 0; d < a.Dv; ++d) s = fmaf(elem(g, d), elem(o, d), s);
  a.delta[idx] = s;
}

// ---- dQ ----
template <bool BF, int HD, bool DROP>
__global__ __launch_bounds__(kThreads) void k_attn_dq(const AttnArgs a) {
  using T = typename Lay<BF, HD>::T;
  using Frag = typename Lay<BF, HD>::Frag;
  using M = Dim<BF, HD>;
  __shared__ __attribute__((aligned(16))) T sK[M::NAT];
  __shared__ __attribute__((aligned(16))) T sKt[M::TRN];
  __shared__ __attribute__((aligned(16))) T sV[M::NAT];
  __shared__ __attribute__((aligned(16))) T sP[M::STRIP];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 15, g = l >> 4;
  const int qt = blockIdx.x, h = blockIdx.y, b = blockIdx.z, q0 = qt * kAttnTile;
  const T* q = (const T*)a.q + b * a.qs[0] + h * a.qs[2];
  const T* k = (const T*)a.k + b * a.ks[0] + h * a.ks[2];
  const T* v = (const T*)a.v + b * a.vs[0] + h * a.vs[2];
  const T* go = (const T*)a.dout + b * a.gs[0] + h * a.gs[2];
  const float cs = a.scale * kLog2e;

  Frag aq[M::NCH], ag[M::NCH];
  {
    const int row = q0 + 16 * w + c;
#pragma unroll
    for (int ch = 0; ch < M::NCH; ++ch) {
      const int d = ch * M::KC + g * M::E;
      aq[ch] = (row < a.T && d < a.D) ? ldfrag<Frag>(q + (int64_t)row * a.qs[1] + d) : zfrag<Frag>();
      ag[ch] = (row < a.T && d < a.Dv) ? ldfrag<Frag>(go + (int64_t)row * a.gs[1] + d) : zfrag<Frag>();
    }
  }
  const int r0 = q0 + 16 * w + 4 * g;
  float l2[4], dl[4];  // lse in the log2 domain (+inf for an empty row: P = 0), delta
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t at = ((int64_t)b * a.H + h) * a.T + r0 + i;
    const float lv = r0 + i < a.T ? a.lse[at] : -INFINITY;
    l2[i] = lv == -INFINITY ? INFINITY : lv * kLog2e;
    dl[i] = r0 + i < a.T ? a.delta[at] : 0.f;
  }
  f4 dQ[M::NTH];
#pragma unroll
  for (int t = 0; t < M::NTH; ++t) dQ[t] = zero4();
  T* strip = sP + w * 16 * M::ST;
  Drop R;
  uint64_t gq = 0;  // the group of (rows r0 .. r0 + 3, key c)
  if constexpr (DROP) {
    R = make_drop(a, ticket_read(nullptr, a.ticket_in, nullptr, 0u));
    gq = drop_group(a, b, h, r0 >> 2) + c;
  }

  const int kts = (a.S + kAttnTile - 1) / kAttnTile;
  const int nkt = a.causal ? min(kts, qt + 1) : kts;
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * kAttnTile;
    __syncthreads();
    stage<BF, HD, true, true>(sK, sKt, k, a.ks[1], k0, a.S, a.D);
    stage<BF, HD, true, false>(sV, nullptr, v, a.vs[1], k0, a.S, a.Dv);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      uint32_t z[4];  // the words of rows r0 + i, key k0 + 16 t + c (indices alone: ahead of the MFMAs)
      if constexpr (DROP) R.block(gq + (uint64_t)(k0 + 16 * t), z);
      f4 s = zero4(), dp = zero4();
#pragma unroll
      for (int ch = 0; ch < M::NCH; ++ch) {
        s = mma(aq[ch], ldfrag<Frag>(sK + (16 * t + c) * M::SN + ch * M::KC + g * M::E), s);
        if (ch * M::KC < a.Dv) dp = mma(ag[ch], ldfrag<Frag>(sV + (16 * t + c) * M::SN + ch * M::KC + g * M::E), dp);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = admitted(a, b, h, r0 + i, k0 + 16 * t + c) ? __builtin_amdgcn_exp2f(s[i] * cs - l2[i]) : 0.f;
        if constexpr (DROP) put(strip + (4 * g + i) * M::ST + 16 * t + c, p * ((R.keep(z[i]) ? R.c * dp[i] : 0.f) - dl[i]));
        else put(strip + (4 * g + i) * M::ST + 16 * t + c, p * (dp[i] - dl[i]));
      }
    }
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < M::KCH; ++ch) {
      const Frag ad = ldfrag<Frag>(strip + c * M::ST + ch * M::KC + g * M::E);
#pragma unroll
      for (int t = 0; t < M::NTH; ++t)
        if (16 * t < a.D) dQ[t] = mma(ad, ldfrag<Frag>(sKt + (16 * t + c) * M::ST + ch * M::KC + g * M::E), dQ[t]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = r0 + i;
    if (row >= a.T) continue;
    const int64_t base = (((int64_t)b * a.T + row) * a.H + h) * a.D;
#pragma unroll
    for (int t = 0; t < M::NTH; ++t)
      if (16 * t + c < a.D) put((T*)a.dq + base + 16 * t + c, dQ[t][i] * a.scale);
  }
}

// ---- dK, dV ----
template <bool BF, int HD, bool DROP>
__global__ __launch_bounds__(kThreads) void k_attn_dkv(const AttnArgs a) {
  using T = typename Lay<BF, HD>::T;
  using Frag = typename Lay<BF, HD>::Frag;
  using M = Dim<BF, HD>;
  __shared__ __attribute__((aligned(16))) T sQ[M::NAT];
  __shared__ __attribute__((aligned(16))) T sQt[M::TRN];
  __shared__ __attribute__((aligned(16))) T sG[M::NAT];
  __shared__ __attribute__((aligned(16))) T sGt[M::TRN];
  __shared__ __attribute__((aligned(16))) T sP[M::STRIP];
  __shared__ float sL[kAttnTile], sD[kAttnTile];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 15, g = l >> 4;
  const int kt = blockIdx.x, h = blockIdx.y, b = blockIdx.z, k0 = kt * kAttnTile;
  const T* q = (const T*)a.q + b * a.qs[0] + h * a.qs[2];
  const T* k = (const T*)a.k + b * a.ks[0] + h * a.ks[2];
  const T* v = (const T*)a.v + b * a.vs[0] + h * a.vs[2];
  const T* go = (const T*)a.dout + b * a.gs[0] + h * a.gs[2];
  const float cs = a.scale * kLog2e;

  Frag ak[M::NCH], av[M::NCH];
  {
    const int key = k0 + 16 * w + c;
#pragma unroll
    for (int ch = 0; ch < M::NCH; ++ch) {
      const int d = ch * M::KC + g * M::E;
      ak[ch] = (key < a.S && d < a.D) ? ldfrag<Frag>(k + (int64_t)key * a.ks[1] + d) : zfrag<Frag>();
      av[ch] = (key < a.S && d < a.Dv) ? ldfrag<Frag>(v + (int64_t)key * a.vs[1] + d) : zfrag<Frag>();
    }
  }
  const int j0 = k0 + 16 * w + 4 * g;  // this lane's accumulator rows: keys j0 + i
  f4 dK[M::NTH], dV[M::NTH];
#pragma unroll
  for (int t = 0; t < M::NTH; ++t) dK[t] = zero4(), dV[t] = zero4();
  T* strip = sP + w * 16 * M::ST;
  Drop R;
  uint64_t gk = 0;  // the group of (row group 0, key j0 + n), n = c & 3: this lane's share of its quad's four blocks
  if constexpr (DROP) {
    R = make_drop(a, ticket_read(nullptr, a.ticket_in, nullptr, 0u));
    gk = drop_group(a, b, h, 0) + (uint64_t)(j0 + (c & 3));
  }

  const int qts = (a.T + kAttnTile - 1) / kAttnTile;
  for (int qt = a.causal ? kt : 0; qt < qts; ++qt) {
    const int q0 = qt * kAttnTile;
    __syncthreads();
    stage<BF, HD, true, true>(sQ, sQt, q, a.qs[1], q0, a.T, a.D);
    stage<BF, HD, true, true>(sG, sGt, go, a.gs[1], q0, a.T, a.Dv);
    if (threadIdx.x < kAttnTile) {
      const int row = q0 + threadIdx.x;
      const int64_t at = ((int64_t)b * a.H + h) * a.T + row;
      const float lv = row < a.T ? a.lse[at] : -INFINITY;
      sL[threadIdx.x] = lv == -INFINITY ? INFINITY : lv * kLog2e;
      sD[threadIdx.x] = row < a.T ? a.delta[at] : 0.f;
    }
    __syncthreads();
    f4 ds[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      // z[i]: the word of (query q0 + 16 t + c, key j0 + i).  The query is row c & 3 of its group of four, which
      // the lanes of a quad share: each computes the block of one of the four keys, the quad transposes the words
      uint32_t z[4];
      if constexpr (DROP) {
        R.block(gk + (uint64_t)((q0 + 16 * t + c) >> 2) * (uint64_t)a.S, z);
        quad_transpose(z, c & 3);
      }
      f4 s = zero4(), dp = zero4();
#pragma unroll
      for (int ch = 0; ch < M::NCH; ++ch) {
        s = mma(ak[ch], ldfrag<Frag>(sQ + (16 * t + c) * M::SN + ch * M::KC + g * M::E), s);
        if (ch * M::KC < a.Dv) dp = mma(av[ch], ldfrag<Frag>(sG + (16 * t + c) * M::SN + ch * M::KC + g * M::E), dp);
      }
      const float l2 = sL[16 * t + c], dl = sD[16 * t + c];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = admitted(a, b, h, q0 + 16 * t + c, j0 + i) ? __builtin_amdgcn_exp2f(s[i] * cs - l2) : 0.f;
        if constexpr (DROP) {
          const bool kept = R.keep(z[i]);
          put(strip + (4 * g + i) * M::ST + 16 * t + c, kept ? p * R.c : 0.f);
          ds[t][i] = p * ((kept ? R.c * dp[i] : 0.f) - dl);
        } else {
          put(strip + (4 * g + i) * M::ST + 16 * t + c, p);
          ds[t][i] = p * (dp[i] - dl);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < M::KCH; ++ch) {
      const Frag ap = ldfrag<Frag>(strip + c * M::ST + ch * M::KC + g * M::E);
#pragma unroll
      for (int t = 0; t < M::NTH; ++t)
        if (16 * t < a.Dv) dV[t] = mma(ap, ldfrag<Frag>(sGt + (16 * t + c) * M::ST + ch * M::KC + g * M::E), dV[t]);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) put(strip + (4 * g + i) * M::ST + 16 * t + c, ds[t][i]);
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < M::KCH; ++ch) {
      const Frag ad = ldfrag<Frag>(strip + c * M::ST + ch * M::KC + g * M::E);
#pragma unroll
      for (int t = 0; t < M::NTH; ++t)
        if (16 * t < a.D) dK[t] = mma(ad, ldfrag<Frag>(sQt + (16 * t + c) * M::ST + ch * M::KC + g * M::E), dK[t]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int key = j0 + i;
    if (key >= a.S) continue;
    const int64_t row = ((int64_t)b * a.S + key) * a.H + h;
#pragma unroll
    for (int t = 0; t < M::NTH; ++t) {
      const int col = 16 * t + c;
      if (col < a.D) put((T*)a.dk + row * a.D + col, dK[t][i] * a.scale);
      if (col < a.Dv) put((T*)a.dv + row * a.Dv + col, dV[t][i]);
    }
  }
}

template <bool BF, int HD>
constexpr int lds_bytes(int which) {  // 0 forward, 1 dq, 2 dkv
  using M = Dim<BF, HD>;
  const int el = BF ? 2 : 4;
  return which == 0   ? (M::NAT + M::TRN + M::STRIP) * el
         : which == 1 ? (2 * M::NAT + M::TRN + M::STRIP) * el
                      : (2 * M::NAT + 2 * M::TRN + M::STRIP) * el + 2 * kAttnTile * 4;
}
static_assert(lds_bytes<false, 128>(2) <= 160 * 1024, "LDS of a workgroup on gfx950");

template <bool BF, int HD>
void launch_fwd(const AttnArgs& a, hipStream_t s) {
  const dim3 grid((a.T + kAttnTile - 1) / kAttnTile, a.H, a.B);
  if (a.state != nullptr) hipLaunchKernelGGL((k_attn_fwd<BF, HD, true>), grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL((k_attn_fwd<BF, HD, false>), grid, dim3(kThreads), 0, s, a);
}
template <bool BF, int HD>
void launch_bwd(const AttnArgs& a, hipStream_t s) {
  using T = typename Lay<BF, HD>::T;
  const int64_t rows = (int64_t)a.B * a.H * a.T;
  hipLaunchKernelGGL((k_attn_delta<T>), dim3((unsigned)((rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
  const dim3 gq((a.T + kAttnTile - 1) / kAttnTile, a.H, a.B), gk((a.S + kAttnTile - 1) / kAttnTile, a.H, a.B);
  if (a.ticket_in != nullptr) {
    hipLaunchKernelGGL((k_attn_dq<BF, HD, true>), gq, dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL((k_attn_dkv<BF, HD, true>), gk, dim3(kThreads), 0, s, a);
  } else {
    hipLaunchKernelGGL((k_attn_dq<BF, HD, false>), gq, dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL((k_attn_dkv<BF, HD, false>), gk, dim3(kThreads), 0, s, a);
  }
}

}  // namespace

int attn_head_pad(int D, int Dv) {
  const int d = std::max(D, Dv);
  if (D < 8 || Dv < 8 || D % 8 || Dv % 8 || d > kAttnMaxHead) return 0;
  return d <= 32 ? 32 : d <= 64 ? 64 : 128;
}

AttnPlan attn_plan(int B, int H, int T, int S, int D, int Dv, bool bf16, bool causal) {
  AttnPlan p{};
  p.hd = attn_head_pad(D, Dv);
  p.q_tiles = (T + kAttnTile - 1) / kAttnTile;
  p.k_tiles = (S + kAttnTile - 1) / kAttnTile;
  int64_t visited = 0;
  for (int qt = 0; qt < p.q_tiles; ++qt) visited += causal ? std::min(p.k_tiles, qt + 1) : p.k_tiles;
  p.causal_skipped = (int64_t)p.q_tiles * p.k_tiles - visited;
  auto lds = [&](int which) {
    if (bf16) return p.hd == 32 ? lds_bytes<true, 32>(which) : p.hd == 64 ? lds_bytes<true, 64>(which) : lds_bytes<true, 128>(which);
    return p.hd == 32 ? lds_bytes<false, 32>(which) : p.hd == 64 ? lds_bytes<false, 64>(which) : lds_bytes<false, 128>(which);
  };
  p.lds_fwd = lds(0), p.lds_dq = lds(1), p.lds_dkv = lds(2);
  // per wave and visited tile pair: a 16 x 64 x hd product costs 4 * hd / kc steps, a 16 x dtiles x 64 one
  // dtiles * 64 / kc; a step is 4 MFMAs (f32) or 1 (bf16)
  const int kc = bf16 ? 32 : 16, per = bf16 ? 1 : 4;
  const int64_t qk = 4 * (p.hd / kc), dvs = 4 * ((Dv + kc - 1) / kc), pv = (int64_t)((Dv + 15) / 16) * (64 / kc),
                dk = (int64_t)((D + 15) / 16) * (64 / kc);
  const int64_t pairs = visited * B * H * 4;
  p.mfma_fwd = pairs * per * (qk + pv);
  p.mfma_bwd = pairs * per * ((qk + dvs + dk) + (qk + dvs + pv + dk));
  return p;
}

#define TDL_ATTN_DISPATCH(fn)                                                     \
  do {                                                                            \
    const int hd = attn_head_pad(a.D, a.Dv);                                      \
    if (bf16) {                                                                   \
      if (hd == 32) fn<true, 32>(a, s);                                           \
      else if (hd == 64) fn<true, 64>(a, s);                                      \
      else fn<true, 128>(a, s);                                                   \
    } else {                                                                      \
      if (hd == 32) fn<false, 32>(a, s);                                          \
      else if (hd == 64) fn<false, 64>(a, s);                                     \
      else fn<false, 128>(a, s);                                                  \
    }                                                                             \
  } while (0)

void attn_forward(const AttnArgs& a, bool bf16, hipStream_t s) { TDL_ATTN_DISPATCH(launch_fwd); }
void attn_backward(const AttnArgs& a, bool bf16, hipStream_t s) { TDL_ATTN_DISPATCH(launch_bwd); }

}  // namespace tdl
