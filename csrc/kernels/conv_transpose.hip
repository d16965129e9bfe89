// Transposed convolution on v_mfma_f32_16x16x4_f32: see conv_transpose.h for the work split.
#include "conv_transpose.h"

#include "common.h"

namespace tdl {
namespace {

// One axis of a stride phase `res` = (o + pad) mod s: its taps i0, i0 + step, ... (nt of them) and its output
// positions o0, o0 + s, ... (Q of them).
struct CtAxis {
  int i0, step, nt, o0, Q;
};
__host__ __device__ inline CtAxis ct_axis(int res, int k, int s, int d, int pad, int O) {
  int a = d % s, b = s;  // gcd(d, s)
  while (a != 0) {
    const int t = b % a;
    b = a;
    a = t;
  }
  CtAxis x;
  x.step = s / b;
  x.i0 = k;
  for (int i = 0; i < k && i < s; ++i) {
    if ((i * d) % s == res) {
      x.i0 = i;
      break;
    }
  }
  x.nt = x.i0 < k ? (k - 1 - x.i0) / x.step + 1 : 0;
  x.o0 = ((res - pad) % s + s) % s;
  x.Q = x.o0 < O ? (O - 1 - x.o0) / s + 1 : 0;
  return x;
}

template <bool BF16>
__device__ __forceinline__ f4 ct_ld4(const void* p, int i) {
  if constexpr (BF16) {
    const uint2 v = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(p) + i);
    return f4{__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16),
              __uint_as_float(v.y & 0xffff0000u)};
  } else {
    return ld4(static_cast<const float*>(p) + i);
  }
}
template <bool BF16>
__device__ __forceinline__ float ct_ld1(const void* p, int i) {
  if constexpr (BF16) return __uint_as_float((uint32_t) static_cast<const uint16_t*>(p)[i] << 16);
  else return static_cast<const float*>(p)[i];
}
template <bool BF16>
__device__ __forceinline__ void ct_st1(void* p, int i, float v) {
  if constexpr (BF16) static_cast<uint16_t*>(p)[i] = (uint16_t)pack_bf16x2(v, 0.f);
  else static_cast<float*>(p)[i] = v;
}
__device__ __forceinline__ float ct_round_bf16(float v) { return __uint_as_float(pack_bf16x2(v, 0.f) << 16); }

constexpr int kCtFar = -(1 << 28);  // a coordinate no tap offset brings back into the image
constexpr int kFwd = 0, kDgrad = 1;

struct CtArgs {
  const void* in;     // gathered operand: x (forward) / dy (input gradient), [N][IH][IW][IC]
  const void* mask;   // input gradient: the saved ReLU output, shaped as dy (or null)
  const float* w;     // [kh][kw][F][C]
  const float* bias;  // forward (or null)
  void* out;          // [N][PH][PW][OC]
  int N, IH, IW, IC, PH, PW, OC;
  int F, C, kh, kw, sh, sw, dh, dw, pt, pl;
  int NT, mr, act;  // column tiles; row tiles per wave; forward: 1 = ReLU
};

template <int MODE, bool BF16, bool VEC>
__global__ __launch_bounds__(kCtThreads) void k_convt(const CtArgs a) {
  __shared__ __attribute__((aligned(16))) float wl[kCtColTiles * kCtChunkUnits * 64];
  __shared__ int4 tab[kCtChunkUnits * 4];
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // forward: this workgroup's phase; input gradient: one dense "phase" with every tap
  CtAxis ay{0, 1, a.kh, 0, a.PH}, ax{0, 1, a.kw, 0, a.PW};
  int osh = 1, osw = 1;
  if constexpr (MODE == kFwd) {
    const int py = blockIdx.z / a.sw, px = blockIdx.z - py * a.sw;
    ay = ct_axis(py, a.kh, a.sh, a.dh, a.pt, a.PH);
    ax = ct_axis(px, a.kw, a.sw, a.dw, a.pl, a.PW);
    osh = a.sh;
    osw = a.sw;
  }
  const int R = a.IC;                 // reduction channels per tap
  const int T = ay.nt * ax.nt * R;    // reduction indices
  const int QHW = ay.Q * ax.Q, P = a.N * QHW;
  const int wg_p0 = blockIdx.x * (64 * a.mr);
  if (wg_p0 >= P) return;  // a phase with fewer pixel tiles than the grid has
  const int tile0 = blockIdx.y * kCtColTiles;
  const int nct = a.NT - tile0 < kCtColTiles ? a.NT - tile0 : kCtColTiles;

  // tap t of the phase: kernel position (i, j)
  auto tap_ij = [&](int t, int& i, int& j) {
    const int ta = t / ax.nt;
    i = ay.i0 + ta * ay.step;
    j = ax.i0 + (t - ta * ax.nt) * ax.step;
  };

  int by[kCtMaxMr], bx[kCtMaxMr], pn[kCtMaxMr];
  bool mact[kCtMaxMr];
#pragma unroll
  for (int m = 0; m < kCtMaxMr; ++m) {
    const int t0 = wg_p0 + (wave * a.mr + m) * 16;
    mact[m] = m < a.mr && t0 < P;
    const int p = t0 + lr;
    by[m] = kCtFar;
    bx[m] = 0;
    pn[m] = 0;
    if (mact[m] && p < P) {
      const int n = p / QHW, rem = p - n * QHW, qy = rem / ax.Q, qx = rem - qy * ax.Q;
      by[m] = MODE == kFwd ? qy : qy * a.sh - a.pt;
      bx[m] = MODE == kFwd ? qx : qx * a.sw - a.pl;
      pn[m] = n * a.IH * a.IW;
    }
  }

  f4 acc[kCtColTiles][kCtMaxMr];
#pragma unroll
  for (int ct = 0; ct < kCtColTiles; ++ct)
#pragma unroll
    for (int m = 0; m < kCtMaxMr; ++m) acc[ct][m] = zero4();

  // 4 channels of pixel row m at table entry t (zeros off the image)
  auto load4 = [&](int m, const int4 t) -> f4 {
    const int iy = by[m] + t.x, ix = bx[m] + t.y;
    f4 v = zero4();
    if ((unsigned)iy < (unsigned)a.IH && (unsigned)ix < (unsigned)a.IW) {
      const int i = (pn[m] + iy * a.IW + ix) * a.IC + t.z;
      v = ct_ld4<BF16>(a.in, i);
      if (MODE == kDgrad && a.mask != nullptr) {
        const f4 k = ct_ld4<BF16>(a.mask, i);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = k[e] > 0.f ? v[e] : 0.f;
      }
    }
    return v;
  };
  auto load1 = [&](int m, const int4 t) -> float {
    const int iy = by[m] + t.x, ix = bx[m] + t.y;
    float v = 0.f;
    if ((unsigned)iy < (unsigned)a.IH && (unsigned)ix < (unsigned)a.IW) {
      const int i = (pn[m] + iy * a.IW + ix) * a.IC + t.z;
      v = ct_ld1<BF16>(a.in, i);
      if (MODE == kDgrad && a.mask != nullptr) v = ct_ld1<BF16>(a.mask, i) > 0.f ? v : 0.f;
    }
    return v;
  };

  const int slices = (T + 3) / 4;  // 4-index slices of the reduction (VEC: T is a multiple of 4)
  const int kchunks = (slices + kCtChunkUnits - 1) / kCtChunkUnits;
  for (int kc = 0; kc < kchunks; ++kc) {
    const int r0 = kc * kCtChunkUnits * 4;
    if (kc > 0) __syncthreads();
    // the chunk's table: VEC one entry per 4-index unit, else one per index
    if (tid < (VEC ? kCtChunkUnits : kCtChunkUnits * 4)) {
      const int r = VEC ? r0 + tid * 4 : r0 + tid;
      int4 e{kCtFar, 0, 0, 0};
      if (r < T) {
        const int t = r / R;
        int i, j;
        tap_ij(t, i, j);
        // forward: input row of phase row qy is qy + (oy0 + pt - i dh) / sh, an exact division
        e.x = MODE == kFwd ? (ay.o0 + a.pt - i * a.dh) / a.sh : i * a.dh;
        e.y = MODE == kFwd ? (ax.o0 + a.pl - j * a.dw) / a.sw : j * a.dw;
        e.z = r - t * R;
      }
      tab[tid] = e;
    }
    // the block's weights of this chunk: wl[tile][index / 4][column][index % 4]
    if constexpr (MODE == kFwd && VEC) {  // w[i,j,f,c .. c+3]: 16 bytes along the reduction
      for (int idx = tid; idx < nct * (kCtChunkUnits * 16); idx += kCtThreads) {
        const int u = idx & 15, c = (idx >> 4) & 15, ct = idx >> 8, r = r0 + u * 4, col = (tile0 + ct) * 16 + c;
        f4 v = zero4();
        if (r < T && col < a.OC) {
          const int t = r / R;
          int i, j;
          tap_ij(t, i, j);
          v = ld4(a.w + ((i * a.kw + j) * a.F + col) * a.C + (r - t * R));
          if (BF16) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = ct_round_bf16(v[e]);
          }
        }
        *reinterpret_cast<f4*>(wl + (ct * kCtChunkUnits + u) * 64 + c * 4) = v;
      }
    } else if constexpr (MODE == kFwd) {
      for (int idx = tid; idx < nct * (kCtChunkUnits * 64); idx += kCtThreads) {
        const int rr = idx & 63, c = (idx >> 6) & 15, ct = idx >> 10, r = r0 + rr, col = (tile0 + ct) * 16 + c;
        float v = 0.f;
        if (r < T && col < a.OC) {
          const int t = r / R;
          int i, j;
          tap_ij(t, i, j);
          v = a.w[((i * a.kw + j) * a.F + col) * a.C + (r - t * R)];
          if (BF16) v = ct_round_bf16(v);
        }
        wl[(ct * kCtChunkUnits + (rr >> 2)) * 64 + c * 4 + (rr & 3)] = v;
      }
    } else {  // input gradient: index (tap, f) and column c of w as the [kh kw F][C] matrix
      for (int idx = tid; idx < nct * (kCtChunkUnits * 64); idx += kCtThreads) {
        const int c = idx & 15, rr = (idx >> 4) & 63, ct = idx >> 10, r = r0 + rr, col = (tile0 + ct) * 16 + c;
        float v = 0.f;
        if (r < T && col < a.OC) {
          v = a.w[r * a.C + col];
          if (BF16) v = ct_round_bf16(v);
        }
        wl[(ct * kCtChunkUnits + (rr >> 2)) * 64 + c * 4 + (rr & 3)] = v;
      }
    }
    __syncthreads();
    const int nu = slices - kc * kCtChunkUnits < kCtChunkUnits ? slices - kc * kCtChunkUnits : kCtChunkUnits;
    // the gathered operand is loaded once per unit and shared by the block's column tiles
    if constexpr (VEC) {
      int u = 0;
      for (; u + 4 <= nu; u += 4) {  // 16 indices: lane k gathers 4k .. 4k + 3, MFMA j takes 4k + j
        const int4 t = tab[u + lk];
        f4 av[kCtMaxMr];
#pragma unroll
        for (int m = 0; m < kCtMaxMr; ++m) av[m] = mact[m] ? load4(m, t) : zero4();
#pragma unroll
        for (int ct = 0; ct < kCtColTiles; ++ct) {
          if (ct < nct) {
            const f4 b = *reinterpret_cast<const f4*>(wl + (ct * kCtChunkUnits + u + lk) * 64 + lr * 4);
#pragma unroll
            for (int m = 0; m < kCtMaxMr; ++m) {
              if (mact[m]) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[ct][m] = mfma16x16x4(av[m][e], b[e], acc[ct][m]);
              }
            }
          }
        }
      }
      for (; u < nu; ++u) {  // the last units one MFMA each: lane k takes element k of the unit
        const int4 t = tab[u];
        float a1[kCtMaxMr];
#pragma unroll
        for (int m = 0; m < kCtMaxMr; ++m) {
          const f4 av = mact[m] ? load4(m, t) : zero4();
          a1[m] = lk == 0 ? av[0] : lk == 1 ? av[1] : lk == 2 ? av[2] : av[3];
        }
#pragma unroll
        for (int ct = 0; ct < kCtColTiles; ++ct) {
          if (ct < nct) {
            const float b = wl[(ct * kCtChunkUnits + u) * 64 + lr * 4 + lk];
#pragma unroll
            for (int m = 0; m < kCtMaxMr; ++m)
              if (mact[m]) acc[ct][m] = mfma16x16x4(a1[m], b, acc[ct][m]);
          }
        }
      }
    } else {
      for (int u = 0; u < nu; ++u) {
        const int4 t = tab[u * 4 + lk];
        float a1[kCtMaxMr];
#pragma unroll
        for (int m = 0; m < kCtMaxMr; ++m) a1[m] = mact[m] ? load1(m, t) : 0.f;
#pragma unroll
        for (int ct = 0; ct < kCtColTiles; ++ct) {
          if (ct < nct) {
            const float b = wl[(ct * kCtChunkUnits + u) * 64 + lr * 4 + lk];
#pragma unroll
            for (int m = 0; m < kCtMaxMr; ++m)
              if (mact[m]) acc[ct][m] = mfma16x16x4(a1[m], b, acc[ct][m]);
          }
        }
      }
    }
  }

  // epilogue: lane holds rows lk * 4 + r of its row tile, column lr of the tile
#pragma unroll
  for (int m = 0; m < kCtMaxMr; ++m) {
    if (mact[m]) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = wg_p0 + (wave * a.mr + m) * 16 + lk * 4 + r;
        if (p < P) {
          const int n = p / QHW, rem = p - n * QHW, qy = rem / ax.Q, qx = rem - qy * ax.Q;
          const int o = ((n * a.PH + qy * osh + ay.o0) * a.PW + qx * osw + ax.o0) * a.OC;
#pragma unroll
          for (int ct = 0; ct < kCtColTiles; ++ct) {
            const int col = (tile0 + ct) * 16 + lr;
            if (ct < nct && col < a.OC) {
              float v = acc[ct][m][r];
              if (MODE == kFwd) {
                if (a.bias != nullptr) v += a.bias[col];
                if (a.act == 1) v = fmaxf(v, 0.f);
              }
              ct_st1<BF16>(a.out, o + col, v);
            }
          }
        }
      }
    }
  }
}

struct CtWArgs {
  const void* x;
  const void* dy;
  const void* mask;
  float* ws;  // [splits][T][C]
  int H, W, C, OH, OW, F;
  int kw, sh, sw, dh, dw, pt, pl;
  int T;   // kh * kw * F
  int RT;  // row tiles
  int P, chunk;
};

template <bool BF16>
__global__ __launch_bounds__(kCtThreads) void k_convt_wgrad(const CtWArgs a) {
  __shared__ f4 red[3][kCtItems][64];
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int item0 = blockIdx.x * kCtItems;
  const int nq = a.RT - item0 < kCtItems ? a.RT - item0 : kCtItems;
  const int c0 = blockIdx.y * 16, ncol = a.C - c0 < 16 ? a.C - c0 : 16;

  // this lane's (tap, f) row of each item: dy offsets from (iy sh, ix sw) and the filter; -1: no row
  int idy[kCtItems], idx[kCtItems], ich[kCtItems];
  f4 acc[kCtItems];
#pragma unroll
  for (int q = 0; q < kCtItems; ++q) {
    acc[q] = zero4();
    idy[q] = idx[q] = 0;
    ich[q] = -1;
    if (q < nq) {
      const int r = (item0 + q) * 16 + lr;
      if (r < a.T) {
        const int tap = r / a.F, i = tap / a.kw;
        idy[q] = i * a.dh - a.pt;
        idx[q] = (tap - i * a.kw) * a.dw - a.pl;
        ich[q] = r - tap * a.F;
      }
    }
  }

  const int ps = blockIdx.z * a.chunk, pe = ps + a.chunk < a.P ? ps + a.chunk : a.P;
  for (int p0 = ps + wave * 4; p0 < pe; p0 += 16) {
    const int p = p0 + lk;
    const bool valid = p < pe;
    int n = 0, iy = 0, ix = 0;
    float bv = 0.f;
    if (valid) {
      n = p / (a.H * a.W);
      const int rem = p - n * (a.H * a.W);
      iy = rem / a.W;
      ix = rem - iy * a.W;
      if (lr < ncol) bv = ct_ld1<BF16>(a.x, p * a.C + c0 + lr);
    }
    const int oy0 = iy * a.sh, ox0 = ix * a.sw, base = n * a.OH * a.OW;
#pragma unroll
    for (int q = 0; q < kCtItems; ++q) {
      if (q < nq) {
        float av = 0.f;
        if (valid && ich[q] >= 0) {
          const int oy = oy0 + idy[q], ox = ox0 + idx[q];
          if ((unsigned)oy < (unsigned)a.OH && (unsigned)ox < (unsigned)a.OW) {
            const int i = (base + oy * a.OW + ox) * a.F + ich[q];
            av = ct_ld1<BF16>(a.dy, i);
            if (a.mask != nullptr) av = ct_ld1<BF16>(a.mask, i) > 0.f ? av : 0.f;
          }
        }
        acc[q] = mfma16x16x4(av, bv, acc[q]);
      }
    }
  }

  // waves 1 .. 3 hand their sums to wave 0, which adds them in that order
  if (wave > 0) {
#pragma unroll
    for (int q = 0; q < kCtItems; ++q)
      if (q < nq) red[wave - 1][q][lane] = acc[q];
  }
  __syncthreads();
  if (wave == 0) {
    float* ws = a.ws + (size_t)blockIdx.z * a.T * a.C;
#pragma unroll
    for (int q = 0; q < kCtItems; ++q) {
      if (q < nq) {
        f4 s = acc[q];
#pragma unroll
        for (int w = 0; w < 3; ++w) {
          const f4 o = red[w][q][lane];
#pragma unroll
          for (int e = 0; e < 4; ++e) s[e] += o[e];
        }
        if (lr < ncol) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = (item0 + q) * 16 + lk * 4 + e;
            if (r < a.T) ws[r * a.C + c0 + lr] = s[e];
          }
        }
      }
    }
  }
}

// wsb[split][F]: column sums of the masked dy over the split's output pixels.  A workgroup is FL filters (a
// power of two) by 256 / FL pixel lanes; a lane adds its pixels in ascending order, lane 0 then the lanes.
template <bool BF16>
__global__ __launch_bounds__(kCtThreads) void k_convt_dbias(const void* __restrict__ dy, const void* __restrict__ mask,
                                                            float* __restrict__ wsb, int P, int F, int chunk, int FL) {
  __shared__ float red[kCtThreads];
  const int tid = threadIdx.x, fl = tid & (FL - 1), pl = tid / FL, PL = kCtThreads / FL;
  const int f = blockIdx.x * FL + fl;
  const int ps = blockIdx.y * chunk, pe = ps + chunk < P ? ps + chunk : P;
  float s = 0.f;
  if (f < F) {
    for (int p = ps + pl; p < pe; p += PL) {
      float v = ct_ld1<BF16>(dy, p * F + f);
      if (mask != nullptr) v = ct_ld1<BF16>(mask, p * F + f) > 0.f ? v : 0.f;
      s += v;
    }
  }
  red[tid] = s;
  __syncthreads();
  if (pl == 0 && f < F) {
    for (int k = 1; k < PL; ++k) s += red[k * FL + fl];
    wsb[blockIdx.y * F + f] = s;
  }
}

// dW [T][C] and db [F] from the workspace slices, added in ascending order
__global__ __launch_bounds__(kCtThreads) void k_convt_wreduce(const float* __restrict__ ws, float* __restrict__ dW,
                                                              float* __restrict__ db, int splits, int TC, int F,
                                                              int accumulate) {
  const int e = blockIdx.x * kCtThreads + threadIdx.x;
  if (e < TC) {
    float s = ws[e];
    for (int z = 1; z < splits; ++z) s += ws[(size_t)z * TC + e];
    dW[e] = accumulate ? dW[e] + s : s;
  } else if (e < TC + F && db != nullptr) {
    const float* wsb = ws + (size_t)splits * TC;
    float s = wsb[e - TC];
    for (int z = 1; z < splits; ++z) s += wsb[z * F + e - TC];
    db[e - TC] = accumulate ? db[e - TC] + s : s;
  }
}

// pmax: pixels of the largest phase (sets the pixel tile and the grid)
void ct_pass(CtPass& q, int64_t pmax, int R, int cols) {
  q.vec = R % 4 == 0;
  q.tiles = (cols + 15) / 16;
  q.colblocks = (q.tiles + kCtColTiles - 1) / kCtColTiles;
  q.mr = 1;
  for (int mr = kCtMaxMr; mr > 1; mr /= 2) {  // the largest pixel tile that still gives 512 workgroups
    if ((pmax + 64 * mr - 1) / (64 * mr) * q.colblocks >= 512) {
      q.mr = mr;
      break;
    }
  }
  q.ptile = 64 * q.mr;
  q.ptiles = (int)((pmax + q.ptile - 1) / q.ptile);
}

template <int MODE>
void ct_launch(const CtArgs& a, const CtPass& q, int phases, CtDType dt, hipStream_t s) {
  const dim3 grid(q.ptiles, q.colblocks, phases);
  const bool bf = dt == CtDType::kBF16;
  if (bf && q.vec) hipLaunchKernelGGL((k_convt<MODE, true, true>), grid, dim3(kCtThreads), 0, s, a);
  else if (bf) hipLaunchKernelGGL((k_convt<MODE, true, false>), grid, dim3(kCtThreads), 0, s, a);
  else if (q.vec) hipLaunchKernelGGL((k_convt<MODE, false, true>), grid, dim3(kCtThreads), 0, s, a);
  else hipLaunchKernelGGL((k_convt<MODE, false, false>), grid, dim3(kCtThreads), 0, s, a);
}

}  // namespace

CtPlan convt_plan(const CtGeom& g) {
  CtPlan p{};
  p.phases = g.sh * g.sw;
  int64_t pmax = 0, mfma = 0;
  int tmax = 0;
  const int ftiles = (g.F + 15) / 16, ctiles = (g.C + 15) / 16;
  for (int py = 0; py < g.sh; ++py) {
    const CtAxis ay = ct_axis(py, g.kh, g.sh, g.dh, g.pt, g.OH);
    for (int px = 0; px < g.sw; ++px) {
      const CtAxis ax = ct_axis(px, g.kw, g.sw, g.dw, g.pl, g.OW);
      const int nt = ay.nt * ax.nt;
      const int64_t P = (int64_t)g.N * ay.Q * ax.Q;
      p.phase_taps[py * g.sw + px] = nt;
      p.empty_phases += nt == 0;
      pmax = P > pmax ? P : pmax;
      tmax = nt > tmax ? nt : tmax;
      mfma += (P + 15) / 16 * ((nt * g.C + 3) / 4) * ftiles;
    }
  }
  ct_pass(p.fwd, pmax, g.C, g.F);
  p.fwd.kchunks = (tmax * g.C + kCtChunkUnits * 4 - 1) / (kCtChunkUnits * 4);
  p.fwd.mfma = mfma;
  const int64_t PI = (int64_t)g.N * g.H * g.W, PO = (int64_t)g.N * g.OH * g.OW;
  const int T = g.kh * g.kw * g.F;
  ct_pass(p.dgrad, PI, g.F, g.C);
  p.dgrad.kchunks = (T + kCtChunkUnits * 4 - 1) / (kCtChunkUnits * 4);
  p.dgrad.mfma = (PI + 15) / 16 * ((T + 3) / 4) * ctiles;
  p.wrowtiles = (T + 15) / 16;
  p.witemblocks = (p.wrowtiles + kCtItems - 1) / kCtItems;
  p.wcoltiles = ctiles;
  const int64_t wgs = (int64_t)p.wcoltiles * p.witemblocks;
  const int64_t want = (1024 + wgs - 1) / wgs;  // splits that fill the device, of at least 256 pixels each
  int64_t chunk = (PI + want - 1) / want;
  if (chunk < 256) chunk = 256;
  if ((PI + chunk - 1) / chunk > kCtMaxSplits) chunk = (PI + kCtMaxSplits - 1) / kCtMaxSplits;
  chunk = (chunk + 15) / 16 * 16;
  p.wchunk = (int)chunk;
  p.wsplits = (int)((PI + chunk - 1) / chunk);
  p.bchunk = (int)((PO + p.wsplits - 1) / p.wsplits);
  p.wmfma = (PI + 3) / 4 * p.wrowtiles * p.wcoltiles;
  p.ws_elems = (int64_t)p.wsplits * ((int64_t)T * g.C + g.F);
  return p;
}

void convt_forward(const void* x, const float* w, const float* b, void* y, CtDType dt, const CtGeom& g, int act,
                   hipStream_t s) {
  const CtPlan p = convt_plan(g);
  CtArgs a{x, nullptr, w, b, y, g.N, g.H, g.W, g.C, g.OH, g.OW, g.F, g.F, g.C, g.kh, g.kw, g.sh, g.sw, g.dh, g.dw,
           g.pt, g.pl, p.fwd.tiles, p.fwd.mr, act};
  ct_launch<kFwd>(a, p.fwd, p.phases, dt, s);
}

void convt_dgrad(const void* dy, const void* ymask, const float* w, void* dx, CtDType dt, const CtGeom& g,
                 hipStream_t s) {
  const CtPlan p = convt_plan(g);
  CtArgs a{dy, ymask, w, nullptr, dx, g.N, g.OH, g.OW, g.F, g.H, g.W, g.C, g.F, g.C, g.kh, g.kw, g.sh, g.sw, g.dh,
           g.dw, g.pt, g.pl, p.dgrad.tiles, p.dgrad.mr, 0};
  ct_launch<kDgrad>(a, p.dgrad, 1, dt, s);
}

void convt_wgrad(const void* x, const void* dy, const void* ymask, float* ws, float* dW, float* db, int accumulate,
                 CtDType dt, const CtGeom& g, hipStream_t s) {
  const CtPlan p = convt_plan(g);
  const int T = g.kh * g.kw * g.F, PO = g.N * g.OH * g.OW;
  const bool bf = dt == CtDType::kBF16;
  CtWArgs a{x, dy, ymask, ws, g.H, g.W, g.C, g.OH, g.OW, g.F, g.kw, g.sh, g.sw, g.dh, g.dw, g.pt, g.pl,
            T, p.wrowtiles, g.N * g.H * g.W, p.wchunk};
  const dim3 grid(p.witemblocks, p.wcoltiles, p.wsplits);
  if (bf) hipLaunchKernelGGL(k_convt_wgrad<true>, grid, dim3(kCtThreads), 0, s, a);
  else hipLaunchKernelGGL(k_convt_wgrad<false>, grid, dim3(kCtThreads), 0, s, a);
  if (db != nullptr) {
    int FL = 1;
    while (FL < g.F && FL < kCtThreads) FL <<= 1;
    float* wsb = ws + (size_t)p.wsplits * T * g.C;
    const dim3 bgrid((g.F + FL - 1) / FL, p.wsplits);
    if (bf) hipLaunchKernelGGL(k_convt_dbias<true>, bgrid, dim3(kCtThreads), 0, s, dy, ymask, wsb, PO, g.F, p.bchunk, FL);
    else hipLaunchKernelGGL(k_convt_dbias<false>, bgrid, dim3(kCtThreads), 0, s, dy, ymask, wsb, PO, g.F, p.bchunk, FL);
  }
  const int n = T * g.C + g.F;
  hipLaunchKernelGGL(k_convt_wreduce, dim3((n + kCtThreads - 1) / kCtThreads), dim3(kCtThreads), 0, s, ws, dW, db,
                     p.wsplits, T * g.C, g.F, accumulate);
}

}  // namespace tdl
