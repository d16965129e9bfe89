// LSTM scan kernels for gfx950 (see lstm.h).
#include "lstm.h"

#include <algorithm>

#include "common.h"

namespace tdl {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));

// Element type and 16-byte MFMA fragment of an instantiation.
template <bool BF>
struct El;
template <>
struct El<false> {
  using T = float;
  using Frag = f4;
  static constexpr int E = 4;    // elements per fragment
  static constexpr int KC = 16;  // k of one fragment step: four MFMAs of k = 4
};
template <>
struct El<true> {
  using T = uint16_t;
  using Frag = bf16x8;
  static constexpr int E = 8;
  static constexpr int KC = 32;  // one MFMA of k = 32
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
__device__ __forceinline__ float ldf(const float* p) { return *p; }
__device__ __forceinline__ float ldf(const uint16_t* p) { return __uint_as_float((uint32_t)*p << 16); }
__device__ __forceinline__ void put(float* p, float v) { *p = v; }
__device__ __forceinline__ void put(uint16_t* p, float v) { *p = (uint16_t)(pack_bf16x2(v, 0.f) & 0xffffu); }

// the two activations of lstm.h (the file is built without fma contraction)
__device__ __forceinline__ float sigm(float z) { return 1.0f / (1.0f + expf(-z)); }
__device__ __forceinline__ float tanh2(float z) { return 2.0f * sigm(2.0f * z) - 1.0f; }

constexpr int round_up(int v, int m) { return (v + m - 1) / m * m; }

// rows [0, rows) of a global [rows][cols] operand into LDS rows of stride `stride` (cols rounded up to a whole
// fragment and one pad fragment: zeros)
template <bool BF>
__device__ __forceinline__ void stage_rows(typename El<BF>::T* dst, const typename El<BF>::T* src, int rows, int cols,
                                           int stride) {
  using Frag = typename El<BF>::Frag;
  constexpr int E = El<BF>::E;
  const int fr = stride / E;
  for (int idx = threadIdx.x; idx < rows * fr; idx += kLstmThreads) {
    const int r = idx / fr, k = (idx % fr) * E;
    const Frag v = k < cols ? ldfrag<Frag>(src + (int64_t)r * cols + k) : zfrag<Frag>();
    *reinterpret_cast<Frag*>(dst + r * stride + k) = v;
  }
}

// acc[q] += A [16, K] (LDS, this lane's row `arow`) x the K-vectors b[q] (this lane's column of B, K contiguous
// elements each; LDS of row stride >= K rounded up to KC with zeros behind K, or global, read one slab ahead)
template <bool BF, bool RES, int NQ>
__device__ __forceinline__ void dot_rows(f4 (&acc)[NQ], const typename El<BF>::T* arow,
                                         const typename El<BF>::T* (&b)[NQ], int K, int g) {
  using Frag = typename El<BF>::Frag;
  constexpr int E = El<BF>::E, KC = El<BF>::KC;
  const int nk = (K + KC - 1) / KC;
  if constexpr (RES) {
    for (int kc = 0; kc < nk; ++kc) {
      const int k = kc * KC + g * E;
      const Frag a = ldfrag<Frag>(arow + k);
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[q] = mma(a, ldfrag<Frag>(b[q] + k), acc[q]);
    }
  } else {
    Frag nxt[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) nxt[q] = g * E < K ? ldfrag<Frag>(b[q] + g * E) : zfrag<Frag>();
    for (int kc = 0; kc < nk; ++kc) {
      Frag cur[NQ];
      const int k = kc * KC + g * E, kn = k + KC;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        cur[q] = nxt[q];
        nxt[q] = kn < K ? ldfrag<Frag>(b[q] + kn) : zfrag<Frag>();
      }
      const Frag a = ldfrag<Frag>(arow + k);
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[q] = mma(a, cur[q], acc[q]);
    }
  }
}

// ---- forward ----
template <bool BF, int TPW, bool RES>
__global__ __launch_bounds__(kLstmThreads) void k_lstm_fwd(const LstmArgs a) {
  using T = typename El<BF>::T;
  constexpr int E = El<BF>::E, KC = El<BF>::KC;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int U = a.U, Tn = a.T, NT = U >> 4, U4 = 4 * U;
  const int SH = round_up(U, KC) + E;  // row stride of h and of R^T in LDS
  T* sH = reinterpret_cast<T*>(smem);  // [2][16][SH]
  T* sR = sH + 2 * kLstmRows * SH;     // [4U][SH] (RES)
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 15, g = l >> 4;
  const int b0 = blockIdx.x * kLstmRows;
  const T* zx = (const T*)a.zx;
  const T* rt = (const T*)a.r;

  for (int idx = threadIdx.x; idx < 2 * kLstmRows * SH; idx += kLstmThreads) sH[idx] = (T)0;
  if constexpr (RES) stage_rows<BF>(sR, rt, U4, U, SH);
  __syncthreads();
  if (a.h0 != nullptr) {
    for (int idx = threadIdx.x; idx < kLstmRows * U; idx += kLstmThreads) {
      const int r = idx / U, u = idx % U;
      if (b0 + r < a.B) sH[r * SH + u] = ((const T*)a.h0)[(int64_t)(b0 + r) * U + u];
    }
  }
  __syncthreads();

  // this lane's elements: rows 4 g + i of the workgroup, unit 16 j + c of the tiles j = w + 4 tp
  f4 cst[TPW], zn[TPW][4];
#pragma unroll
  for (int tp = 0; tp < TPW; ++tp) {
    const int j = w + 4 * tp;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = b0 + 4 * g + i;
      cst[tp][i] = (a.c0 != nullptr && j < NT && row < a.B) ? a.c0[(int64_t)row * U + 16 * j + c] : 0.f;
    }
  }
  auto load_zx = [&](int t) {
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp) {
      const int j = w + 4 * tp;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = b0 + 4 * g + i;
        const bool ok = j < NT && row < a.B;
        const T* p = zx + ((int64_t)row * Tn + t) * U4 + 16 * j + c;
#pragma unroll
        for (int q = 0; q < 4; ++q) zn[tp][q][i] = ok ? ldf(p + q * U) : 0.f;
      }
    }
  };
  const int tstep = a.rev ? -1 : 1;
  int t = a.rev ? Tn - 1 : 0;
  load_zx(t);

  for (int s = 0; s < Tn; ++s, t += tstep) {
    f4 acc[TPW][4];
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[tp][q] = zn[tp][q];
    if (s + 1 < Tn) load_zx(t + tstep);

    const T* hb = sH + (s & 1) * kLstmRows * SH;
    T* hn = sH + ((s + 1) & 1) * kLstmRows * SH;
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp) {
      const int j = w + 4 * tp;
      if (j < NT) {
        const T* bq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = q * U + 16 * j + c;  // column of R: row of R^T
          bq[q] = RES ? sR + n * SH : rt + (int64_t)n * U;
        }
        dot_rows<BF, RES, 4>(acc[tp], hb + c * SH, bq, U, g);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int lr = 4 * g + i, row = b0 + lr, unit = 16 * j + c;
          const float gi = sigm(acc[tp][0][i]), gf = sigm(acc[tp][1][i]), gg = tanh2(acc[tp][2][i]),
                      go = sigm(acc[tp][3][i]);
          const float cn = gf * cst[tp][i] + gi * gg;
          const float h = go * tanh2(cn);
          cst[tp][i] = cn;
          put(hn + lr * SH + unit, h);
          if (row < a.B) {
            const int64_t bs = (int64_t)row * Tn + s;
            put((T*)a.hs + bs * U + unit, h);
            if (a.gates != nullptr) {
              T* gp = (T*)a.gates + bs * U4 + unit;
              put(gp, gi), put(gp + U, gf), put(gp + 2 * U, gg), put(gp + 3 * U, go);
              a.cs[bs * U + unit] = cn;
            }
            if (s == Tn - 1) {
              put((T*)a.h_last + (int64_t)row * U + unit, h);
              a.c_last[(int64_t)row * U + unit] = cn;
            }
          }
        }
      }
    }
    __syncthreads();
  }
}

// ---- backward ----
template <bool BF, int TPW, bool RES>
__global__ __launch_bounds__(kLstmThreads) void k_lstm_bwd(const LstmArgs a) {
  using T = typename El<BF>::T;
  constexpr int E = El<BF>::E;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int U = a.U, Tn = a.T, NT = U >> 4, U4 = 4 * U;
  const int SZ = U4 + E;               // row stride of dZ and of R in LDS (4U is a multiple of KC)
  T* sZ = reinterpret_cast<T*>(smem);  // [16][SZ]
  T* sR = sZ + kLstmRows * SZ;         // [U][SZ] (RES)
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 15, g = l >> 4;
  const int b0 = blockIdx.x * kLstmRows;
  const T* rn = (const T*)a.r;

  for (int idx = threadIdx.x; idx < kLstmRows * SZ; idx += kLstmThreads) sZ[idx] = (T)0;
  if constexpr (RES) stage_rows<BF>(sR, rn, U, U4, SZ);
  __syncthreads();

  f4 dc[TPW], dh[TPW];
#pragma unroll
  for (int tp = 0; tp < TPW; ++tp) {
    const int j = w + 4 * tp;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = b0 + 4 * g + i;
      const bool ok = j < NT && row < a.B;
      const int64_t o = (int64_t)row * U + 16 * j + c;
      dc[tp][i] = (ok && a.dc_last != nullptr) ? a.dc_last[o] : 0.f;
      dh[tp][i] = (ok && a.dh_last != nullptr) ? ldf((const T*)a.dh_last + o) : 0.f;
    }
  }

  for (int s = Tn - 1; s >= 0; --s) {
    const int t = a.rev ? Tn - 1 - s : s;
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp) {
      const int j = w + 4 * tp;
      if (j < NT) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int lr = 4 * g + i, row = b0 + lr, unit = 16 * j + c;
          float zi = 0.f, zf = 0.f, zg = 0.f, zo = 0.f;
          if (row < a.B) {
            const int64_t bs = (int64_t)row * Tn + s;
            const T* gp = (const T*)a.gates + bs * U4 + unit;
            const float gi = ldf(gp), gf = ldf(gp + U), gg = ldf(gp + 2 * U), go = ldf(gp + 3 * U);
            const float ct = a.cs[bs * U + unit];
            const float cp = s > 0 ? a.cs[(bs - 1) * U + unit]
                                   : (a.c0 != nullptr ? a.c0[(int64_t)row * U + unit] : 0.f);
            float d = dh[tp][i];
            if (a.dhs != nullptr) d = d + ldf((const T*)a.dhs + bs * U + unit);
            const float tc = tanh2(ct);
            zo = d * tc * (go * (1.0f - go));
            const float dcv = dc[tp][i] + d * go * (1.0f - tc * tc);
            zi = dcv * gg * (gi * (1.0f - gi));
            zf = dcv * cp * (gf * (1.0f - gf));
            zg = dcv * gi * (1.0f - gg * gg);
            dc[tp][i] = dcv * gf;
            T* zp = (T*)a.dz + ((int64_t)row * Tn + t) * U4 + unit;
            put(zp, zi), put(zp + U, zf), put(zp + 2 * U, zg), put(zp + 3 * U, zo);
          }
          T* sp = sZ + lr * SZ + unit;
          put(sp, zi), put(sp + U, zf), put(sp + 2 * U, zg), put(sp + 3 * U, zo);
        }
      }
    }
    __syncthreads();
    if (s > 0 || a.dh0 != nullptr) {  // dh_rec = dZ_t R^T
#pragma unroll
      for (int tp = 0; tp < TPW; ++tp) {
        const int j = w + 4 * tp;
        if (j < NT) {
          f4 acc[1] = {zero4()};
          const T* bq[1] = {RES ? sR + (16 * j + c) * SZ : rn + (int64_t)(16 * j + c) * U4};
          dot_rows<BF, RES, 1>(acc, sZ + c * SZ, bq, U4, g);
          dh[tp] = acc[0];
        }
      }
    }
    __syncthreads();
  }

  if (a.dh0 != nullptr) {
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp) {
      const int j = w + 4 * tp;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = b0 + 4 * g + i;
        if (j < NT && row < a.B) {
          const int64_t o = (int64_t)row * U + 16 * j + c;
          put((T*)a.dh0 + o, dh[tp][i]);
          a.dc0[o] = dc[tp][i];
        }
      }
    }
  }
}

constexpr int el_bytes(bool bf16) { return bf16 ? 2 : 4; }
int lds_fwd(int U, bool bf16, bool res) {
  const int E = bf16 ? 8 : 4, KC = bf16 ? 32 : 16, SH = round_up(U, KC) + E;
  return (2 * kLstmRows * SH + (res ? 4 * U * SH : 0)) * el_bytes(bf16);
}
int lds_bwd(int U, bool bf16, bool res) {
  const int E = bf16 ? 8 : 4, SZ = 4 * U + E;
  return (kLstmRows * SZ + (res ? U * SZ : 0)) * el_bytes(bf16);
}
bool fits(int U, bool bf16) {
  return lds_fwd(U, bf16, true) <= kLstmLdsBudget && lds_bwd(U, bf16, true) <= kLstmLdsBudget;
}
static_assert(kLstmMaxU % 16 == 0 && kLstmMaxU / 16 <= 4 * 4, "four tiles per wave at most");

template <bool BF, int TPW, bool RES>
void launch(const LstmArgs& a, bool bwd, int lds, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)k_lstm_fwd<BF, TPW, RES>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              kLstmLdsBudget);
    (void)hipFuncSetAttribute((const void*)k_lstm_bwd<BF, TPW, RES>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              kLstmLdsBudget);
    attr = true;
  }
  const dim3 grid((unsigned)((a.B + kLstmRows - 1) / kLstmRows));
  if (bwd) hipLaunchKernelGGL((k_lstm_bwd<BF, TPW, RES>), grid, dim3(kLstmThreads), lds, s, a);
  else hipLaunchKernelGGL((k_lstm_fwd<BF, TPW, RES>), grid, dim3(kLstmThreads), lds, s, a);
}

// resident plans hold at most two tiles per wave (U <= 128); a streamed plan of one tile runs as two
template <bool BF>
void dispatch(const LstmArgs& a, bool bwd, hipStream_t s) {
  const LstmPlan p = lstm_plan(a.B, a.T, a.U, BF);
  const int lds = bwd ? p.lds_bwd : p.lds_fwd;
  if (p.resident) {
    if (p.tiles_wave == 1) launch<BF, 1, true>(a, bwd, lds, s);
    else launch<BF, 2, true>(a, bwd, lds, s);
  } else if (p.tiles_wave <= 2) {
    launch<BF, 2, false>(a, bwd, lds, s);
  } else {
    launch<BF, 4, false>(a, bwd, lds, s);
  }
}

}  // namespace

LstmPlan lstm_plan(int64_t B, int64_t T, int U, bool bf16) {
  (void)T;
  LstmPlan p{};
  p.resident_max_u = 0;
  for (int u = 16; u <= 128 && fits(u, bf16); u += 16) p.resident_max_u = u;
  p.resident = U <= p.resident_max_u;
  p.lds_fwd = lds_fwd(U, bf16, p.resident);
  p.lds_bwd = lds_bwd(U, bf16, p.resident);
  p.workgroups = (int)((B + kLstmRows - 1) / kLstmRows);
  const int per_wave = (U / 16 + 3) / 4;
  p.tiles_wave = per_wave <= 1 ? 1 : per_wave <= 2 ? 2 : 4;
  return p;
}

void lstm_forward(const LstmArgs& a, bool bf16, hipStream_t s) {
  if (bf16) dispatch<true>(a, false, s);
  else dispatch<false>(a, false, s);
}

void lstm_backward(const LstmArgs& a, bool bf16, hipStream_t s) {
  if (bf16) dispatch<true>(a, true, s);
  else dispatch<false>(a, true, s);
}

}  // namespace tdl
