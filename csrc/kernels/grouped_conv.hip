// Grouped convolution on v_mfma_f32_16x16x4_f32: see grouped_conv.h for the work split.
#include "grouped_conv.h"

#include "common.h"

namespace tdl {
namespace {

// column tile j of a pass whose groups own Og consecutive columns each: first group, groups, first column, columns
struct GcTile {
  int g0, ng, f0, ncol;
};
__host__ __device__ inline GcTile gc_tile(int j, int Og, int G) {
  GcTile t;
  if (Og >= 16) {
    const int tpg = (Og + 15) / 16, grp = j / tpg, off = (j - grp * tpg) * 16;
    t.g0 = grp;
    t.ng = 1;
    t.f0 = grp * Og + off;
    t.ncol = Og - off < 16 ? Og - off : 16;  // a short last tile ends with its group
  } else {
    const int gpt = 16 / Og;
    t.g0 = j * gpt;
    t.ng = G - t.g0 < gpt ? G - t.g0 : gpt;
    t.f0 = t.g0 * Og;
    t.ncol = t.ng * Og;
  }
  return t;
}

template <bool BF16>
__device__ __forceinline__ f4 gc_ld4(const void* p, int i) {
  if constexpr (BF16) {
    const uint2 v = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(p) + i);
    return f4{__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16),
              __uint_as_float(v.y & 0xffff0000u)};
  } else {
    return ld4(static_cast<const float*>(p) + i);
  }
}
template <bool BF16>
__device__ __forceinline__ float gc_ld1(const void* p, int i) {
  if constexpr (BF16) return __uint_as_float((uint32_t) static_cast<const uint16_t*>(p)[i] << 16);
  else return static_cast<const float*>(p)[i];
}
template <bool BF16>
__device__ __forceinline__ void gc_st1(void* p, int i, float v) {
  if constexpr (BF16) static_cast<uint16_t*>(p)[i] = (uint16_t)pack_bf16x2(v, 0.f);
  else static_cast<float*>(p)[i] = v;
}
__device__ __forceinline__ float gc_round_bf16(float v) { return __uint_as_float(pack_bf16x2(v, 0.f) << 16); }

constexpr int kGcFar = -(1 << 28);  // a coordinate no tap offset brings back into the image

struct GcArgs {
  const void* in;     // gathered operand: x (forward) / dy (input gradient), [N][IH][IW][IC]
  const void* mask;   // input gradient: the saved ReLU output, shaped as dy (or null)
  const float* w;     // [kh][kw][Cg][F]
  const float* bias;  // forward (or null)
  void* out;          // [N][PH][PW][OC]
  int IH, IW, IC, PH, PW, OC;
  int G, Rg, Og;  // groups; reduction channels / output columns per group
  int Cg, F, kw, sh, sw, dh, dw, pt, pl;
  int T;          // reduction indices per group: kh * kw * Rg
  int NT, mr, act, P, kchunks;
};

// MODE 0: input row of output row oy and tap i: oy sh - pt + i dh.  MODE 1: dy row of input row h and tap i:
// (h + pt - i dh) / sh where that divides.  (py, px) hold the tap-independent part, (tdy, tdx) the tap's.
template <int MODE>
__device__ __forceinline__ bool gc_coord(const GcArgs& a, int py, int px, int tdy, int tdx, int& iy, int& ix) {
  iy = py + tdy;
  ix = px + tdx;
  if constexpr (MODE == 1) {
    if (iy < 0 || ix < 0) return false;
    if (a.sh > 1) {
      const int q = iy / a.sh;
      if (q * a.sh != iy) return false;
      iy = q;
    }
    if (a.sw > 1) {
      const int q = ix / a.sw;
      if (q * a.sw != ix) return false;
      ix = q;
    }
  }
  return (unsigned)iy < (unsigned)a.IH && (unsigned)ix < (unsigned)a.IW;
}

template <int MODE, bool BF16, bool VEC>
__global__ __launch_bounds__(kGcThreads) void k_gconv(const GcArgs a) {
  __shared__ __attribute__((aligned(16))) float wl[kGcColTiles * kGcChunkUnits * 64];
  __shared__ int4 tab[kGcChunkUnits * 4];
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Og = a.Og, Rg = a.Rg, T = a.T;
  const int tile0 = blockIdx.y * kGcColTiles;
  const int nct = a.NT - tile0 < kGcColTiles ? a.NT - tile0 : kGcColTiles;
  const int cg = Og >= 16 ? 0 : lr / Og;  // this lane's column belongs to the tile's cg-th group
  const int wg_p0 = blockIdx.x * (64 * a.mr);

  int py[kGcMaxMr], px[kGcMaxMr], pn[kGcMaxMr];
  bool mact[kGcMaxMr];
#pragma unroll
  for (int m = 0; m < kGcMaxMr; ++m) {
    const int t0 = wg_p0 + (wave * a.mr + m) * 16;
    mact[m] = m < a.mr && t0 < a.P;
    const int p = t0 + lr;
    py[m] = kGcFar;
    px[m] = 0;
    pn[m] = 0;
    if (mact[m] && p < a.P) {
      const int n = p / (a.PH * a.PW), rem = p - n * (a.PH * a.PW), oy = rem / a.PW, ox = rem - oy * a.PW;
      py[m] = MODE == 0 ? oy * a.sh - a.pt : oy + a.pt;
      px[m] = MODE == 0 ? ox * a.sw - a.pl : ox + a.pl;
      pn[m] = n * a.IH * a.IW;
    }
  }

  f4 acc[kGcColTiles][kGcMaxMr];
#pragma unroll
  for (int ct = 0; ct < kGcColTiles; ++ct)
#pragma unroll
    for (int m = 0; m < kGcMaxMr; ++m) acc[ct][m] = zero4();

  // 4 channels of pixel row m at table entry t of the group whose channels start at gch (zeros off the image)
  auto load4 = [&](int m, const int4 t, int gch) -> f4 {
    int iy, ix;
    f4 v = zero4();
    if (gc_coord<MODE>(a, py[m], px[m], t.x, t.y, iy, ix)) {
      const int i = (pn[m] + iy * a.IW + ix) * a.IC + gch + t.z;
      v = gc_ld4<BF16>(a.in, i);
      if (MODE == 1 && a.mask != nullptr) {
        const f4 k = gc_ld4<BF16>(a.mask, i);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = k[e] > 0.f ? v[e] : 0.f;
      }
    }
    return v;
  };
  auto load1 = [&](int m, const int4 t, int gch) -> float {
    int iy, ix;
    float v = 0.f;
    if (gc_coord<MODE>(a, py[m], px[m], t.x, t.y, iy, ix)) {
      const int i = (pn[m] + iy * a.IW + ix) * a.IC + gch + t.z;
      v = gc_ld1<BF16>(a.in, i);
      if (MODE == 1 && a.mask != nullptr) v = gc_ld1<BF16>(a.mask, i) > 0.f ? v : 0.f;
    }
    return v;
  };

  const int slices = (T + 3) / 4;  // 4-index slices of the reduction (VEC: T is a multiple of 4)
  for (int kc = 0; kc < a.kchunks; ++kc) {
    const int r0 = kc * kGcChunkUnits * 4;
    if (kc > 0) __syncthreads();
    // the chunk's table: VEC one entry per 4-index unit, else one per index
    if (tid < (VEC ? kGcChunkUnits : kGcChunkUnits * 4)) {
      const int r = VEC ? r0 + tid * 4 : r0 + tid;
      int4 e{kGcFar, 0, 0, 0};
      if (r < T) {
        const int tap = r / Rg, i = tap / a.kw, j = tap - i * a.kw;
        e.x = MODE == 0 ? i * a.dh : -i * a.dh;
        e.y = MODE == 0 ? j * a.dw : -j * a.dw;
        e.z = r - tap * Rg;
      }
      tab[tid] = e;
    }
    // the block's weights of this chunk: wl[tile][index / 4][column][index % 4]
    for (int idx = tid; idx < nct * (kGcChunkUnits * 64); idx += kGcThreads) {
      const int c = idx & 15, rr = (idx >> 4) & 63, ct = idx >> 10, r = r0 + rr;
      const GcTile tl = gc_tile(tile0 + ct, Og, a.G);
      float v = 0.f;
      if (r < T && c < tl.ncol) {
        const int tap = r / Rg, rch = r - tap * Rg, col = tl.f0 + c;
        int wi;
        if (MODE == 0) {
          wi = (tap * a.Cg + rch) * a.F + col;
        } else {  // column = input channel grp Cg + oc, reduction channel = filter grp Kg + rch
          const int grp = col / Og, oc = col - grp * Og;
          wi = (tap * a.Cg + oc) * a.F + grp * Rg + rch;
        }
        v = a.w[wi];
        if (BF16) v = gc_round_bf16(v);
      }
      wl[(ct * kGcChunkUnits + (rr >> 2)) * 64 + c * 4 + (rr & 3)] = v;
    }
    __syncthreads();
    const int nu = slices - kc * kGcChunkUnits < kGcChunkUnits ? slices - kc * kGcChunkUnits : kGcChunkUnits;
#pragma unroll
    for (int ct = 0; ct < kGcColTiles; ++ct) {
      if (ct < nct) {
        const GcTile tl = gc_tile(tile0 + ct, Og, a.G);
        const float* wt = wl + ct * kGcChunkUnits * 64;
        for (int gi = 0; gi < tl.ng; ++gi) {
          const int gch = (tl.g0 + gi) * Rg;
          const bool mine = cg == gi;
          if constexpr (VEC) {
            int u = 0;
            for (; u + 4 <= nu; u += 4) {  // 16 indices: lane k gathers 4k .. 4k + 3, MFMA j takes 4k + j
              const int4 t = tab[u + lk];
              f4 b = *reinterpret_cast<const f4*>(wt + (u + lk) * 64 + lr * 4);
              if (!mine) b = zero4();
#pragma unroll
              for (int m = 0; m < kGcMaxMr; ++m) {
                if (mact[m]) {
                  const f4 av = load4(m, t, gch);
#pragma unroll
                  for (int e = 0; e < 4; ++e) acc[ct][m] = mfma16x16x4(av[e], b[e], acc[ct][m]);
                }
              }
            }
            for (; u < nu; ++u) {  // the last units one MFMA each: lane k takes element k of the unit
              const int4 t = tab[u];
              float b = wt[u * 64 + lr * 4 + lk];
              if (!mine) b = 0.f;
#pragma unroll
              for (int m = 0; m < kGcMaxMr; ++m) {
                if (mact[m]) {
                  const f4 av = load4(m, t, gch);
                  const float a1 = lk == 0 ? av[0] : lk == 1 ? av[1] : lk == 2 ? av[2] : av[3];
                  acc[ct][m] = mfma16x16x4(a1, b, acc[ct][m]);
                }
              }
            }
          } else {
            for (int u = 0; u < nu; ++u) {
              const int4 t = tab[u * 4 + lk];
              float b = wt[u * 64 + lr * 4 + lk];
              if (!mine) b = 0.f;
#pragma unroll
              for (int m = 0; m < kGcMaxMr; ++m)
                if (mact[m]) acc[ct][m] = mfma16x16x4(load1(m, t, gch), b, acc[ct][m]);
            }
          }
        }
      }
    }
  }

  // epilogue: lane holds rows lk * 4 + r of its row tile, column lr of the tile
#pragma unroll
  for (int ct = 0; ct < kGcColTiles; ++ct) {
    if (ct < nct) {
      const GcTile tl = gc_tile(tile0 + ct, Og, a.G);
      if (lr < tl.ncol) {
        const int col = tl.f0 + lr;
        const float bv = (MODE == 0 && a.bias != nullptr) ? a.bias[col] : 0.f;
#pragma unroll
        for (int m = 0; m < kGcMaxMr; ++m) {
          if (mact[m]) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int p = wg_p0 + (wave * a.mr + m) * 16 + lk * 4 + r;
              if (p < a.P) {
                float v = acc[ct][m][r] + bv;
                if (MODE == 0 && a.act == 1) v = fmaxf(v, 0.f);
                gc_st1<BF16>(a.out, p * a.OC + col, v);
              }
            }
          }
        }
      }
    }
  }
}

struct GcWArgs {
  const void* x;
  const void* dy;
  const void* mask;
  float* ws;  // [splits][T + 1][F]
  int H, W, C, OH, OW, F, G, Cg, Kg;
  int kw, sh, sw, dh, dw, pt, pl;
  int T;   // kh * kw * Cg: row T is the row of ones (bias gradient)
  int RT;  // row tiles per group
  int P, chunk;
};

template <bool BF16>
__global__ __launch_bounds__(kGcThreads) void k_gconv_wgrad(const GcWArgs a) {
  __shared__ f4 red[3][kGcItems][64];
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const GcTile tl = gc_tile(blockIdx.y, a.Kg, a.G);
  const int item0 = blockIdx.x * kGcItems, nitems = tl.ng * a.RT;
  const int nq = nitems - item0 < kGcItems ? nitems - item0 : kGcItems;
  const int cg = a.Kg >= 16 ? 0 : lr / a.Kg;

  // this lane's row of each item: tap offsets and channel; ich -1: the row of ones, -2: no row
  int idy[kGcItems], idx[kGcItems], ich[kGcItems];
  f4 acc[kGcItems];
#pragma unroll
  for (int q = 0; q < kGcItems; ++q) {
    acc[q] = zero4();
    idy[q] = idx[q] = 0;
    ich[q] = -2;
    if (q < nq) {
      const int it = item0 + q, gi = it / a.RT, r = (it - gi * a.RT) * 16 + lr;
      if (r < a.T) {
        const int tap = r / a.Cg, i = tap / a.kw;
        idy[q] = i * a.dh;
        idx[q] = (tap - i * a.kw) * a.dw;
        ich[q] = (tl.g0 + gi) * a.Cg + (r - tap * a.Cg);
      } else if (r == a.T) {
        ich[q] = -1;
      }
    }
  }

  const int ps = blockIdx.z * a.chunk, pe = ps + a.chunk < a.P ? ps + a.chunk : a.P;
  for (int p0 = ps + wave * 4; p0 < pe; p0 += 16) {
    const int p = p0 + lk;
    const bool valid = p < pe;
    int n = 0, oy = 0, ox = 0;
    float bv = 0.f;
    if (valid) {
      n = p / (a.OH * a.OW);
      const int rem = p - n * (a.OH * a.OW);
      oy = rem / a.OW;
      ox = rem - oy * a.OW;
      if (lr < tl.ncol) {
        const int i = p * a.F + tl.f0 + lr;
        bv = gc_ld1<BF16>(a.dy, i);
        if (a.mask != nullptr) bv = gc_ld1<BF16>(a.mask, i) > 0.f ? bv : 0.f;
      }
    }
    const int iy0 = oy * a.sh - a.pt, ix0 = ox * a.sw - a.pl, base = n * a.H * a.W;
#pragma unroll
    for (int q = 0; q < kGcItems; ++q) {
      if (q < nq) {
        float av = 0.f;
        if (valid) {
          if (ich[q] >= 0) {
            const int iy = iy0 + idy[q], ix = ix0 + idx[q];
            if ((unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W)
              av = gc_ld1<BF16>(a.x, (base + iy * a.W + ix) * a.C + ich[q]);
          } else if (ich[q] == -1) {
            av = 1.f;
          }
        }
        acc[q] = mfma16x16x4(av, bv, acc[q]);
      }
    }
  }

  // waves 1 .. 3 hand their sums to wave 0, which adds them in that order
  if (wave > 0) {
#pragma unroll
    for (int q = 0; q < kGcItems; ++q)
      if (q < nq) red[wave - 1][q][lane] = acc[q];
  }
  __syncthreads();
  if (wave == 0) {
    float* ws = a.ws + (size_t)blockIdx.z * (a.T + 1) * a.F;
#pragma unroll
    for (int q = 0; q < kGcItems; ++q) {
      if (q < nq) {
        f4 s = acc[q];
#pragma unroll
        for (int w = 0; w < 3; ++w) {
          const f4 o = red[w][q][lane];
#pragma unroll
          for (int e = 0; e < 4; ++e) s[e] += o[e];
        }
        const int it = item0 + q, gi = it / a.RT, rt = it - gi * a.RT;
        if (lr < tl.ncol && cg == gi) {  // the other groups' columns of this row tile are not this group's dW
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = rt * 16 + lk * 4 + e;
            if (r <= a.T) ws[r * a.F + tl.f0 + lr] = s[e];
          }
        }
      }
    }
  }
}

// dW [T][F] and db [F] from the workspace slices, added in ascending order
__global__ __launch_bounds__(kGcThreads) void k_gconv_wreduce(const float* __restrict__ ws, float* __restrict__ dW,
                                                              float* __restrict__ db, int splits, int TF, int F,
                                                              int accumulate) {
  const int e = blockIdx.x * kGcThreads + threadIdx.x;
  if (e >= TF + F) return;
  float s = ws[e];
  for (int z = 1; z < splits; ++z) s += ws[(size_t)z * (TF + F) + e];
  if (e < TF) {
    dW[e] = accumulate ? dW[e] + s : s;
  } else if (db != nullptr) {
    db[e - TF] = accumulate ? db[e - TF] + s : s;
  }
}

GcPass gc_pass(int64_t P, int G, int Rg, int Og, int taps) {
  GcPass q;
  q.vec = Rg % 4 == 0;
  q.gpt = Og >= 16 ? 1 : 16 / Og;
  q.tpg = Og >= 16 ? (Og + 15) / 16 : 1;
  q.tiles = Og >= 16 ? G * q.tpg : (G + q.gpt - 1) / q.gpt;
  q.colblocks = (q.tiles + kGcColTiles - 1) / kGcColTiles;
  q.mr = 1;
  for (int mr = kGcMaxMr; mr > 1; mr /= 2) {  // the largest pixel tile that still gives 512 workgroups
    if ((P + 64 * mr - 1) / (64 * mr) * q.colblocks >= 512) {
      q.mr = mr;
      break;
    }
  }
  q.ptile = 64 * q.mr;
  q.ptiles = (int)((P + q.ptile - 1) / q.ptile);
  q.red = (taps * Rg + 3) / 4 * 4;
  q.kchunks = (q.red + kGcChunkUnits * 4 - 1) / (kGcChunkUnits * 4);
  q.mfma = (P + 15) / 16 * (q.red / 4) * (int64_t)(Og >= 16 ? G * q.tpg : G);
  return q;
}

template <int MODE>
void gc_launch(const GcArgs& a, const GcPass& q, GcDType dt, hipStream_t s) {
  const dim3 grid(q.ptiles, q.colblocks);
  const bool bf = dt == GcDType::kBF16;
  if (bf && q.vec) hipLaunchKernelGGL((k_gconv<MODE, true, true>), grid, dim3(kGcThreads), 0, s, a);
  else if (bf) hipLaunchKernelGGL((k_gconv<MODE, true, false>), grid, dim3(kGcThreads), 0, s, a);
  else if (q.vec) hipLaunchKernelGGL((k_gconv<MODE, false, true>), grid, dim3(kGcThreads), 0, s, a);
  else hipLaunchKernelGGL((k_gconv<MODE, false, false>), grid, dim3(kGcThreads), 0, s, a);
}

}  // namespace

GcPlan gconv_plan(const GcGeom& g) {
  GcPlan p;
  const int Cg = g.C / g.G, Kg = g.F / g.G, taps = g.kh * g.kw;
  const int64_t P = (int64_t)g.N * g.OH * g.OW;
  p.fwd = gc_pass(P, g.G, Cg, Kg, taps);
  p.dgrad = gc_pass((int64_t)g.N * g.H * g.W, g.G, Kg, Cg, taps);
  p.wrows = taps * Cg + 1;
  p.wrowtiles = (p.wrows + 15) / 16;
  p.witemblocks = (p.fwd.gpt * p.wrowtiles + kGcItems - 1) / kGcItems;
  const int64_t wgs = (int64_t)p.fwd.tiles * p.witemblocks;
  const int64_t want = (1024 + wgs - 1) / wgs;  // splits that fill the device, of at least 256 pixels each
  int64_t chunk = (P + want - 1) / want;
  if (chunk < 256) chunk = 256;
  if ((P + chunk - 1) / chunk > kGcMaxSplits) chunk = (P + kGcMaxSplits - 1) / kGcMaxSplits;
  chunk = (chunk + 15) / 16 * 16;
  p.wchunk = (int)chunk;
  p.wsplits = (int)((P + chunk - 1) / chunk);
  p.wmfma = (P + 3) / 4 * p.wrowtiles * (int64_t)(Kg >= 16 ? g.G * p.fwd.tpg : g.G);
  p.ws_elems = (int64_t)p.wsplits * p.wrows * g.F;
  return p;
}

void gconv_forward(const void* x, const float* w, const float* b, void* y, GcDType dt, const GcGeom& g, int act,
                   hipStream_t s) {
  const GcPlan p = gconv_plan(g);
  const int Cg = g.C / g.G, Kg = g.F / g.G;
  GcArgs a{x, nullptr, w, b, y, g.H, g.W, g.C, g.OH, g.OW, g.F, g.G, Cg, Kg, Cg, g.F, g.kw, g.sh, g.sw, g.dh, g.dw,
           g.pt, g.pl, g.kh * g.kw * Cg, p.fwd.tiles, p.fwd.mr, act, g.N * g.OH * g.OW, p.fwd.kchunks};
  gc_launch<0>(a, p.fwd, dt, s);
}

void gconv_dgrad(const void* dy, const void* ymask, const float* w, void* dx, GcDType dt, const GcGeom& g,
                 hipStream_t s) {
  const GcPlan p = gconv_plan(g);
  const int Cg = g.C / g.G, Kg = g.F / g.G;
  GcArgs a{dy, ymask, w, nullptr, dx, g.OH, g.OW, g.F, g.H, g.W, g.C, g.G, Kg, Cg, Cg, g.F, g.kw, g.sh, g.sw, g.dh,
           g.dw, g.pt, g.pl, g.kh * g.kw * Kg, p.dgrad.tiles, p.dgrad.mr, 0, g.N * g.H * g.W, p.dgrad.kchunks};
  gc_launch<1>(a, p.dgrad, dt, s);
}

void gconv_wgrad(const void* x, const void* dy, const void* ymask, float* ws, float* dW, float* db, int accumulate,
                 GcDType dt, const GcGeom& g, hipStream_t s) {
  const GcPlan p = gconv_plan(g);
  const int Cg = g.C / g.G, Kg = g.F / g.G, T = g.kh * g.kw * Cg;
  GcWArgs a{x, dy, ymask, ws, g.H, g.W, g.C, g.OH, g.OW, g.F, g.G, Cg, Kg, g.kw, g.sh, g.sw, g.dh, g.dw, g.pt, g.pl,
            T, p.wrowtiles, g.N * g.OH * g.OW, p.wchunk};
  const dim3 grid(p.witemblocks, p.fwd.tiles, p.wsplits);
  if (dt == GcDType::kBF16) hipLaunchKernelGGL(k_gconv_wgrad<true>, grid, dim3(kGcThreads), 0, s, a);
  else hipLaunchKernelGGL(k_gconv_wgrad<false>, grid, dim3(kGcThreads), 0, s, a);
  const int n = T * g.F + g.F;
  hipLaunchKernelGGL(k_gconv_wreduce, dim3((n + kGcThreads - 1) / kGcThreads), dim3(kGcThreads), 0, s, ws, dW, db,
                     p.wsplits, T * g.F, g.F, accumulate);
}

}  // namespace tdl
