// GRU scan kernels for gfx950 (see gru.h).  The fragment helpers are lstm.hip's, kept file-local in both.
#include "gru.h"

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
// what a store in the data's dtype keeps
__device__ __forceinline__ float kept(float v, const float*) { return v; }
__device__ __forceinline__ float kept(float v, const uint16_t*) { return __uint_as_float(pack_bf16x2(v, 0.f) << 16); }

// the two activations of gru.h (the file is built without fma contraction)
__device__ __forceinline__ float sigm(float z) { return 1.0f / (1.0f + expf(-z)); }
__device__ __forceinline__ float tanh2(float z) { return 2.0f * sigm(2.0f * z) - 1.0f; }

constexpr int round_up(int v, int m) { return (v + m - 1) / m * m; }

// rows [0, rows) of a global [rows][cols] operand into LDS rows of stride `stride` (cols rounded up to a whole
// k step and one pad fragment: zeros)
template <bool BF>
__device__ __forceinline__ void stage_rows(typename El<BF>::T* dst, const typename El<BF>::T* src, int rows, int cols,
                                           int stride) {
  using Frag = typename El<BF>::Frag;
  constexpr int E = El<BF>::E;
  const int fr = stride / E;
  for (int idx = threadIdx.x; idx < rows * fr; idx += kGruThreads) {
    const int r = idx / fr, k = (idx % fr) * E;
    const Frag v = k < cols ? ldfrag<Frag>(src + (int64_t)r * cols + k) : zfrag<Frag>();
    *reinterpret_cast<Frag*>(dst + r * stride + k) = v;
  }
}

// acc[q] += A [16, K] (LDS, this lane's row `arow`, zeros behind K up to a whole k step) x the K-vectors b[q]
// (this lane's column of B, K contiguous elements each; LDS with the same zeros, or global, read one slab ahead)
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
__global__ __launch_bounds__(kGruThreads) void k_gru_fwd(const GruArgs a) {
  using T = typename El<BF>::T;
  constexpr int E = El<BF>::E, KC = El<BF>::KC;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int U = a.U, Tn = a.T, NT = U >> 4, U3 = 3 * U, U4 = 4 * U;
  const int SH = round_up(U, KC) + E;  // row stride of h and of R^T in LDS
  T* sH = reinterpret_cast<T*>(smem);  // [2][16][SH]
  T* sR = sH + 2 * kGruRows * SH;      // [3U][SH] (RES)
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 15, g = l >> 4;
  const int b0 = blockIdx.x * kGruRows;
  const T* zx = (const T*)a.zx;
  const T* rt = (const T*)a.r;

  for (int idx = threadIdx.x; idx < 2 * kGruRows * SH; idx += kGruThreads) sH[idx] = (T)0;
  if constexpr (RES) stage_rows<BF>(sR, rt, U3, U, SH);
  __syncthreads();
  if (a.h0 != nullptr) {
    for (int idx = threadIdx.x; idx < kGruRows * U; idx += kGruThreads) {
      const int r = idx / U, u = idx % U;
      if (b0 + r < a.B) sH[r * SH + u] = ((const T*)a.h0)[(int64_t)(b0 + r) * U + u];
    }
  }
  __syncthreads();

  // this lane's elements: rows 4 g + i of the workgroup, unit 16 j + c of the tiles j = w + 4 tp
  f4 hst[TPW], zn[TPW][3];
  float br[TPW][3];
#pragma unroll
  for (int tp = 0; tp < TPW; ++tp) {
    const int j = w + 4 * tp;
#pragma unroll
    for (int q = 0; q < 3; ++q) br[tp][q] = (a.b_rec != nullptr && j < NT) ? a.b_rec[q * U + 16 * j + c] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = b0 + 4 * g + i;
      hst[tp][i] = (a.h0 != nullptr && j < NT && row < a.B) ? ldf((const T*)a.h0 + (int64_t)row * U + 16 * j + c) : 0.f;
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
        const T* p = zx + ((int64_t)row * Tn + t) * U3 + 16 * j + c;
#pragma unroll
        for (int q = 0; q < 3; ++q) zn[tp][q][i] = ok ? ldf(p + q * U) : 0.f;
      }
    }
  };
  const int tstep = a.rev ? -1 : 1;
  int t = a.rev ? Tn - 1 : 0;
  load_zx(t);

  for (int s = 0; s < Tn; ++s, t += tstep) {
    // z, r: mx + b_rec + h R; the h column: b_rec + h R alone, mx_h waits for the multiply by r
    f4 acc[TPW][3], mxh[TPW];
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[tp][0][i] = zn[tp][0][i] + br[tp][0];
        acc[tp][1][i] = zn[tp][1][i] + br[tp][1];
        acc[tp][2][i] = br[tp][2];
      }
      mxh[tp] = zn[tp][2];
    }
    if (s + 1 < Tn) load_zx(t + tstep);

    const T* hb = sH + (s & 1) * kGruRows * SH;
    T* hn = sH + ((s + 1) & 1) * kGruRows * SH;
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp) {
      const int j = w + 4 * tp;
      if (j < NT) {
        const T* bq[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const int n = q * U + 16 * j + c;  // column of R: row of R^T
          bq[q] = RES ? sR + n * SH : rt + (int64_t)n * U;
        }
        dot_rows<BF, RES, 3>(acc[tp], hb + c * SH, bq, U, g);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int lr = 4 * g + i, row = b0 + lr, unit = 16 * j + c;
          const float gz = sigm(acc[tp][0][i]), gr = sigm(acc[tp][1][i]), q = acc[tp][2][i];
          const float hh = tanh2(mxh[tp][i] + gr * q);
          const float h = kept(gz * hst[tp][i] + (1.0f - gz) * hh, (const T*)nullptr);
          hst[tp][i] = h;
          put(hn + lr * SH + unit, h);
          if (row < a.B) {
            const int64_t bs = (int64_t)row * Tn + s;
            put((T*)a.hs + bs * U + unit, h);
            if (a.saved != nullptr) {
              T* gp = (T*)a.saved + bs * U4 + unit;
              put(gp, gz), put(gp + U, gr), put(gp + 2 * U, hh), put(gp + 3 * U, q);
            }
            if (s == Tn - 1) put((T*)a.h_last + (int64_t)row * U + unit, h);
          }
        }
      }
    }
    __syncthreads();
  }
}

// ---- backward ----
template <bool BF, int TPW, bool RES>
__global__ __launch_bounds__(kGruThreads) void k_gru_bwd(const GruArgs a) {
  using T = typename El<BF>::T;
  constexpr int E = El<BF>::E, KC = El<BF>::KC;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int U = a.U, Tn = a.T, NT = U >> 4, U3 = 3 * U, U4 = 4 * U;
  const int SZ = round_up(U3, KC) + E;  // row stride of dzh and of R in LDS
  T* sZ = reinterpret_cast<T*>(smem);   // [16][SZ]
  T* sR = sZ + kGruRows * SZ;           // [U][SZ] (RES)
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 15, g = l >> 4;
  const int b0 = blockIdx.x * kGruRows;
  const T* rn = (const T*)a.r;

  for (int idx = threadIdx.x; idx < kGruRows * SZ; idx += kGruThreads) sZ[idx] = (T)0;
  if constexpr (RES) stage_rows<BF>(sR, rn, U, U3, SZ);
  __syncthreads();

  f4 dh[TPW];
#pragma unroll
  for (int tp = 0; tp < TPW; ++tp) {
    const int j = w + 4 * tp;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = b0 + 4 * g + i;
      const bool ok = j < NT && row < a.B && a.dh_last != nullptr;
      dh[tp][i] = ok ? ldf((const T*)a.dh_last + (int64_t)row * U + 16 * j + c) : 0.f;
    }
  }

  for (int s = Tn - 1; s >= 0; --s) {
    const int t = a.rev ? Tn - 1 - s : s;
    f4 seed[TPW];  // d z: the element-wise part of the carried gradient
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp) {
      const int j = w + 4 * tp;
      seed[tp] = zero4();
      if (j < NT) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int lr = 4 * g + i, row = b0 + lr, unit = 16 * j + c;
          float az = 0.f, ar = 0.f, ah = 0.f, ahr = 0.f;
          if (row < a.B) {
            const int64_t bs = (int64_t)row * Tn + s;
            const T* gp = (const T*)a.saved + bs * U4 + unit;
            const float gz = ldf(gp), gr = ldf(gp + U), hh = ldf(gp + 2 * U), q = ldf(gp + 3 * U);
            const float hp = s > 0 ? ldf((const T*)a.hs + (bs - 1) * U + unit)
                                   : (a.h0 != nullptr ? ldf((const T*)a.h0 + (int64_t)row * U + unit) : 0.f);
            float d = dh[tp][i];
            if (a.dhs != nullptr) d = d + ldf((const T*)a.dhs + bs * U + unit);
            const float omz = 1.0f - gz;
            ah = (d * omz) * (1.0f - hh * hh);
            az = (d * (hp - hh)) * (gz * omz);
            ar = (ah * q) * (gr * (1.0f - gr));
            ahr = ah * gr;
            seed[tp][i] = d * gz;
            const int64_t o = ((int64_t)row * Tn + t) * U3 + unit;
            T* xp = (T*)a.dzx + o;
            T* hp_ = (T*)a.dzh + o;
            put(xp, az), put(xp + U, ar), put(xp + 2 * U, ah);
            put(hp_, az), put(hp_ + U, ar), put(hp_ + 2 * U, ahr);
          }
          T* sp = sZ + lr * SZ + unit;
          put(sp, az), put(sp + U, ar), put(sp + 2 * U, ahr);
        }
      }
    }
    __syncthreads();
    if (s > 0 || a.dh0 != nullptr) {  // dh = d z + dzh_t R^T
#pragma unroll
      for (int tp = 0; tp < TPW; ++tp) {
        const int j = w + 4 * tp;
        if (j < NT) {
          // (summed from zero and added once: every MFMA step of an accumulator seeded with d z would round at
          // the larger value's ulp)
          f4 acc[1] = {zero4()};
          const T* bq[1] = {RES ? sR + (16 * j + c) * SZ : rn + (int64_t)(16 * j + c) * U3};
          dot_rows<BF, RES, 1>(acc, sZ + c * SZ, bq, U3, g);
          dh[tp] = seed[tp] + acc[0];
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
        if (j < NT && row < a.B) put((T*)a.dh0 + (int64_t)row * U + 16 * j + c, dh[tp][i]);
      }
    }
  }
}

// ---- column sums (db_rec): 32 columns x 32 row lanes per workgroup, f64, a fixed order ----
constexpr int kSumCols = 32, kSumLanes = 32;
template <class T>
__global__ __launch_bounds__(kSumCols* kSumLanes) void k_gru_colsum(const T* x, int64_t rows, int cols, float* out,
                                                                      int accumulate) {
  __shared__ double part[kSumLanes][kSumCols + 1];
  const int cl = threadIdx.x % kSumCols, rl = threadIdx.x / kSumCols;
  const int col = blockIdx.x * kSumCols + cl;
  double s = 0.0;
  if (col < cols)
    for (int64_t r = rl; r < rows; r += kSumLanes) s += (double)ldf(x + r * cols + col);
  part[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && col < cols) {
    double tot = 0.0;
    for (int i = 0; i < kSumLanes; ++i) tot += part[i][cl];
    out[col] = accumulate ? out[col] + (float)tot : (float)tot;
  }
}

constexpr int el_bytes(bool bf16) { return bf16 ? 2 : 4; }
int lds_fwd(int U, bool bf16, bool res) {
  const int E = bf16 ? 8 : 4, KC = bf16 ? 32 : 16, SH = round_up(U, KC) + E;
  return (2 * kGruRows * SH + (res ? 3 * U * SH : 0)) * el_bytes(bf16);
}
int lds_bwd(int U, bool bf16, bool res) {
  const int E = bf16 ? 8 : 4, KC = bf16 ? 32 : 16, SZ = round_up(3 * U, KC) + E;
  return (kGruRows * SZ + (res ? U * SZ : 0)) * el_bytes(bf16);
}
bool fits(int U, bool bf16) {
  return lds_fwd(U, bf16, true) <= kGruLdsBudget && lds_bwd(U, bf16, true) <= kGruLdsBudget;
}
static_assert(kGruMaxU % 16 == 0 && kGruMaxU / 16 <= 4 * 4, "four tiles per wave at most");

template <bool BF, int TPW, bool RES>
void launch(const GruArgs& a, bool bwd, int lds, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)k_gru_fwd<BF, TPW, RES>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              kGruLdsBudget);
    (void)hipFuncSetAttribute((const void*)k_gru_bwd<BF, TPW, RES>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              kGruLdsBudget);
    attr = true;
  }
  const dim3 grid((unsigned)((a.B + kGruRows - 1) / kGruRows));
  if (bwd) hipLaunchKernelGGL((k_gru_bwd<BF, TPW, RES>), grid, dim3(kGruThreads), lds, s, a);
  else hipLaunchKernelGGL((k_gru_fwd<BF, TPW, RES>), grid, dim3(kGruThreads), lds, s, a);
}

// resident f32 plans hold at most two tiles per wave (U <= 96), bf16 ones up to three (U <= 144: the
// four-tile instantiation); a streamed plan of one tile runs as two
template <bool BF>
void dispatch(const GruArgs& a, bool bwd, hipStream_t s) {
  const GruPlan p = gru_plan(a.B, a.T, a.U, BF);
  const int lds = bwd ? p.lds_bwd : p.lds_fwd;
  if (p.resident) {
    if (p.tiles_wave == 1) launch<BF, 1, true>(a, bwd, lds, s);
    else if (p.tiles_wave == 2) launch<BF, 2, true>(a, bwd, lds, s);
    else launch<BF, 4, true>(a, bwd, lds, s);
  } else if (p.tiles_wave <= 2) {
    launch<BF, 2, false>(a, bwd, lds, s);
  } else {
    launch<BF, 4, false>(a, bwd, lds, s);
  }
}

}  // namespace

GruPlan gru_plan(int64_t B, int64_t T, int U, bool bf16) {
  (void)T;
  GruPlan p{};
  p.resident_max_u = 0;
  for (int u = 16; u <= kGruMaxU && fits(u, bf16); u += 16) p.resident_max_u = u;
  p.resident = U <= p.resident_max_u;
  p.lds_fwd = lds_fwd(U, bf16, p.resident);
  p.lds_bwd = lds_bwd(U, bf16, p.resident);
  p.workgroups = (int)((B + kGruRows - 1) / kGruRows);
  const int per_wave = (U / 16 + 3) / 4;
  p.tiles_wave = per_wave <= 1 ? 1 : per_wave <= 2 ? 2 : 4;
  return p;
}

void gru_forward(const GruArgs& a, bool bf16, hipStream_t s) {
  if (bf16) dispatch<true>(a, false, s);
  else dispatch<false>(a, false, s);
}

void gru_backward(const GruArgs& a, bool bf16, hipStream_t s) {
  if (bf16) dispatch<true>(a, true, s);
  else dispatch<false>(a, true, s);
}

void gru_colsum(const void* x, bool bf16, int64_t rows, int cols, float* out, bool accumulate, hipStream_t s) {
  const dim3 grid((unsigned)((cols + kSumCols - 1) / kSumCols)), block(kSumCols * kSumLanes);
  if (bf16) hipLaunchKernelGGL(k_gru_colsum<uint16_t>, grid, block, 0, s, (const uint16_t*)x, rows, cols, out, accumulate ? 1 : 0);
  else hipLaunchKernelGGL(k_gru_colsum<float>, grid, block, 0, s, (const float*)x, rows, cols, out, accumulate ? 1 : 0);
}

}  // namespace tdl
