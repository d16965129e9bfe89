// Transposed 2-D convolution over channels-last activations: x [N,H,W,C], y [N,OH,OW,F], f32 or bf16 data, the
// Keras kernel w [kh,kw,F,C] (filters before input channels) and the bias [F] always f32.  Used by
// keras.layers.Conv2DTranspose on the GPU (ops/conv_transpose.py).
//
//   y[n,oy,ox,f] = b[f] + sum x[n,iy,ix,c] w[i,j,f,c]   over oy = iy sh - pt + i dh, ox = ix sw - pl + j dw
//
// Every operation is an implicit GEMM on v_mfma_f32_16x16x4_f32 with f32 accumulation.  bf16 activations are
// widened in the loader and the weight is rounded to bf16 (RNE) as it is staged into LDS, so every product is
// the exact product of two bf16 values: the arithmetic of the bf16 MFMA, on the f32 form (a
// v_mfma_f32_16x16x32_bf16 instantiation is a follow-up).
//
// Forward (k_convt<FWD>), one dense GEMM per stride phase.  Output pixels are partitioned by
// (py, px) = ((oy + pt) mod sh, (ox + pl) mod sw); phase py owns the taps { i : i dh = py (mod sh) }, which are
// i0, i0 + sh / gcd(dh, sh), ... -- the phases' tap sets partition the kh kw taps.  Within a phase the output
// rows oy0 + qy sh (qy = 0 .. QH - 1) read input row qy + (oy0 + pt - i dh) / sh for tap i: the division is
// exact, so no element is tested for divisibility and no MFMA multiplies a structural zero.  blockIdx.z is the
// phase; a workgroup of 4 waves owns 64 * mr pixels (n, qy, qx) of the phase grid (a wave: mr row tiles of 16)
// and a block of up to 4 column tiles (64 filters).  The reduction index is the flattened (tap of the phase,
// channel), cut into k-chunks of 64; per chunk the block's weights are staged once into LDS as
// [column tile][index / 4][column][index % 4] (zeros past the reduction's end and past the last filter), with
// 16-byte loads along c where C % 4 == 0, beside a table of each index's input offsets and channel.  A lane
// gathers 4 consecutive channels of its input pixel with one vector load and feeds them to 4 MFMAs (MFMA j
// takes elements 4k + j of the 16; the B side is one ds_read_b128), once for all of the block's column tiles;
// channel counts that are not a multiple of 4
// take one element per lane and MFMA with the index zero-padded to a multiple of 4.  Positions outside the
// image are not read.  A phase without taps runs no MFMA and stores act(b).
//
// Input gradient (k_convt<DGRAD>, the same template): dx[n,iy,ix,c] = sum dy[n, iy sh - pt + i dh,
// ix sw - pl + j dw, f] w[i,j,f,c], a dense strided gather over dy in which every tap is live; the reduction is
// (tap, f), w is read as the [kh kw F][C] matrix it is, and dy is selected to 0 where the saved ReLU output is
// <= 0 as it is loaded.
//
// Weight / bias gradient (k_convt_wgrad, k_convt_dbias, k_convt_wreduce): D rows are 16 (tap, f) rows gathered
// from the masked dy, columns a 16-channel tile of x, the MFMA's k four input pixels.  A wave holds up to 8 row
// tiles that share one x fragment; the 4 waves of a workgroup take alternate pixel quads of their split and
// are added in a fixed order through LDS.  The N*H*W pixels are cut into `wsplits` slices written to a workspace
// [split][kh kw F][C].  db is not a sum over taps (an output pixel is reached by several taps or by none): the
// masked dy is column-summed over the N*OH*OW output pixels in the same number of slices, [split][F] behind the
// dW slices.  The last kernel adds the slices in ascending order and stores, or adds into what the targets hold.
//
// No atomics and no inter-workgroup dependence: bit-identical from run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdl {

enum class CtDType { kF32 = 0, kBF16 = 1 };

struct CtGeom {
  int N, H, W, C;  // input
  int F;           // filters
  int OH, OW;
  int kh, kw, sh, sw, dh, dw;
  int pt, pl;  // leading crop of the full transposed convolution
};

constexpr int kCtThreads = 256;
constexpr int kCtColTiles = 4;     // column tiles (of 16) per workgroup
constexpr int kCtChunkUnits = 16;  // 4-index units of the reduction per k-chunk (64 indices)
constexpr int kCtMaxMr = 4;        // row tiles of 16 pixels per wave
constexpr int kCtItems = 8;        // wgrad: row-tile accumulators per wave
constexpr int kCtLdsBytes = kCtColTiles * kCtChunkUnits * 64 * 4 + kCtChunkUnits * 4 * 16;  // forward / dgrad
constexpr int kCtWgradLdsBytes = 3 * kCtItems * 64 * 16;
static_assert(kCtLdsBytes <= 65536 && kCtWgradLdsBytes <= 65536, "LDS budget of a workgroup");
constexpr int kCtMaxSplits = 1024;
constexpr int kCtMaxRed = 1 << 20;  // kh * kw * max(C, F)
constexpr int kCtMaxStride = 8;

struct CtPass {   // forward (columns: filters) or input gradient (columns: channels)
  int vec;        // 1: 4-channel vector gathers, 0: per element
  int tiles;      // column tiles
  int colblocks;  // ceil(tiles / kCtColTiles)
  int mr;         // row tiles per wave
  int ptile;      // pixels per workgroup = 64 * mr
  int ptiles;     // pixel tiles (forward: of the largest phase)
  int kchunks;    // k-chunks (forward: of the phase with the most taps)
  int64_t mfma;   // MFMA instructions issued (1024 MACs each)
};
struct CtPlan {
  int phases;                                       // sh * sw
  int phase_taps[kCtMaxStride * kCtMaxStride];      // taps of phase py * sw + px
  int empty_phases;                                 // phases without a tap: bias-only pixels
  CtPass fwd, dgrad;
  int wrowtiles;    // ceil(kh kw F / 16)
  int witemblocks;  // ceil(wrowtiles / kCtItems)
  int wcoltiles;    // ceil(C / 16)
  int wchunk;       // input pixels per split
  int bchunk;       // output pixels per split (bias gradient)
  int wsplits;
  int64_t wmfma;
  int64_t ws_elems;  // f32 elements of the wgrad workspace
};
CtPlan convt_plan(const CtGeom& g);

// y = act(convT(x, w) + b); b nullable; act: 0 none, 1 ReLU
void convt_forward(const void* x, const float* w, const float* b, void* y, CtDType dt, const CtGeom& g, int act,
                   hipStream_t s);
// dx; ymask (nullable): the forward's ReLU output, dy counts where ymask > 0
void convt_dgrad(const void* dy, const void* ymask, const float* w, void* dx, CtDType dt, const CtGeom& g,
                 hipStream_t s);
// ws: f32 [plan.ws_elems]; dW f32 [kh,kw,F,C]; db f32 [F] (nullable); accumulate: added into dW / db
void convt_wgrad(const void* x, const void* dy, const void* ymask, float* ws, float* dW, float* db, int accumulate,
                 CtDType dt, const CtGeom& g, hipStream_t s);

}  // namespace tdl
