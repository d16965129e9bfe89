// Grouped 2-D convolution over channels-last activations: x [N,H,W,C], y [N,OH,OW,F], f32 or bf16 data, the
// Keras kernel w [kh,kw,Cg,F] (Cg = C / G; filter f belongs to group f / Kg, Kg = F / G) and the bias [F]
// always f32.  Used by keras.layers.Conv2D(groups > 1) on the GPU (ops/grouped_conv.py).
//
// Every operation is an implicit GEMM per group on v_mfma_f32_16x16x4_f32 with f32 accumulation.  bf16
// activations are widened in the loader and the weight is rounded to bf16 (RNE) as it is staged into LDS, so
// every product is the exact product of two bf16 values: the arithmetic of the bf16 MFMA, on the f32 form
// (a v_mfma_f32_16x16x32_bf16 instantiation is a follow-up).
//
// Column tiles.  The F output columns are cut into tiles of at most 16 consecutive filters that never cross
// into a group they do not own: Kg >= 16 gives ceil(Kg / 16) tiles per group (the last one short), Kg < 16
// puts floor(16 / Kg) whole groups side by side in one tile.  In such a shared tile a k-slice carries ONE
// group's reduction elements and the B fragment holds zeros in the other groups' columns: the within-tile
// block diagonal, at most 16 / Kg times the useful MACs.  (The 4x4x1 x 16-block form would need Kg = 4 AND
// a 4-pixel row tile per block; it was not used.)
//
// Forward / input gradient (one kernel template, k_gconv<MODE>): a workgroup of 4 waves owns 64 * mr output
// pixels (a wave: mr row tiles of 16) and a block of up to 4 consecutive column tiles (64 output channels).
// The reduction index of a group is the flattened (tap, channel in group), cut into k-chunks of 64; per chunk
// the block's weights are staged once into LDS as [tile][index / 4][column][index % 4] (zeros past the
// reduction's end and past a short tile's columns), beside a table of each index's tap offsets and channel.
// Where the group's channel count is a multiple of 4 a lane gathers 4 consecutive channels of its pixel with
// one vector load (16 bytes f32, 8 bytes bf16) and feeds them to 4 MFMAs (MFMA j takes elements 4k + j of the
// 16: A and B agree on the order, read as one ds_read_b128); otherwise one element per lane and MFMA, the
// index zero-padded to a multiple of 4.  Padding taps are not read.  The input gradient is the same GEMM
// with dy as the gathered operand (selected to 0 where the saved ReLU output is <= 0), Kg as the reduction
// channels and w read transposed; a tap that does not hit a strided output position is not read.
//
// Weight / bias gradient (k_gconv_wgrad + k_gconv_wreduce): D rows are 16 reduction rows (tap, ci) of one
// group -- plus a row of ones whose sums are the bias gradient --, columns a column tile of dy, the MFMA's k
// four pixels.  A wave holds up to 8 (group, row tile) accumulators that share one dy fragment; the 4 waves
// of a workgroup take alternate pixel quads of their split and are added in a fixed order through LDS.  The
// N*OH*OW pixels are cut into `wsplits` slices written to a workspace [split][kh*kw*Cg + 1][F], which the
// second kernel adds in ascending order and stores, or adds into what the targets hold.
//
// No atomics and no inter-workgroup dependence: bit-identical from run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdl {

enum class GcDType { kF32 = 0, kBF16 = 1 };

struct GcGeom {
  int N, H, W, C;  // input
  int F, G;        // filters, groups
  int OH, OW;
  int kh, kw, sh, sw, dh, dw;
  int pt, pl;  // leading padding (trailing padding is implied by OH / OW)
};

constexpr int kGcThreads = 256;
constexpr int kGcColTiles = 4;    // column tiles (of 16 filters) per workgroup
constexpr int kGcChunkUnits = 16; // 4-index units of the reduction per k-chunk (64 indices)
constexpr int kGcMaxMr = 4;       // row tiles of 16 pixels per wave
constexpr int kGcItems = 8;       // wgrad: (group, row tile) accumulators per wave
constexpr int kGcLdsBytes = kGcColTiles * kGcChunkUnits * 64 * 4 + kGcChunkUnits * 4 * 16;  // forward / dgrad
constexpr int kGcWgradLdsBytes = 3 * kGcItems * 64 * 16;
constexpr int kGcMaxSplits = 1024;
constexpr int kGcMaxRed = 1 << 20;  // kh * kw * max(Cg, Kg)

struct GcPass {   // forward (over Kg columns per group) or input gradient (over Cg columns per group)
  int vec;        // 1: 4-channel vector gathers, 0: per element
  int tiles;      // column tiles in all
  int gpt, tpg;   // groups per tile (columns per group < 16) / tiles per group
  int colblocks;  // ceil(tiles / kGcColTiles)
  int mr;         // row tiles per wave
  int ptile;      // pixels per workgroup = 64 * mr
  int ptiles;     // ceil(pixels / ptile)
  int red;        // reduction indices per group, padded to a multiple of 4
  int kchunks;    // ceil(red / 64)
  int64_t mfma;   // MFMA instructions issued (1024 MACs each)
};
struct GcPlan {
  GcPass fwd, dgrad;
  int wrows;       // wgrad rows per group: kh * kw * Cg + 1
  int wrowtiles;   // ceil(wrows / 16)
  int witemblocks; // ceil(groups per tile * wrowtiles / kGcItems)
  int wchunk;      // pixels per split
  int wsplits;
  int64_t wmfma;
  int64_t ws_elems;  // f32 elements of the wgrad workspace
};
GcPlan gconv_plan(const GcGeom& g);

// y = act(conv_g(x, w) + b); b nullable; act: 0 none, 1 ReLU
void gconv_forward(const void* x, const float* w, const float* b, void* y, GcDType dt, const GcGeom& g, int act,
                   hipStream_t s);
// dx; ymask (nullable): the forward's ReLU output, dy counts where ymask > 0
void gconv_dgrad(const void* dy, const void* ymask, const float* w, void* dx, GcDType dt, const GcGeom& g,
                 hipStream_t s);
// ws: f32 [plan.ws_elems]; dW f32 [kh,kw,Cg,F]; db f32 [F] (nullable); accumulate: added into dW / db
void gconv_wgrad(const void* x, const void* dy, const void* ymask, float* ws, float* dW, float* db, int accumulate,
                 GcDType dt, const GcGeom& g, hipStream_t s);

}  // namespace tdl
