// Depthwise 2-D convolution over channels-last activations: x [N,H,W,C], y [N,OH,OW,C*dm], bf16 or f32 data,
// the Keras depthwise kernel w [kh,kw,C,dm] and the bias b [C*dm] always f32.  Output channel c*dm + m reads
// input channel c.  Used by keras.layers.DepthwiseConv2D / SeparableConv2D on the GPU (ops/depthwise.py).
//
// There is no reduction over channels, so no MFMA: every kernel is a stencil over an LDS tile.  A work item
// is a column: one 16-byte vector of channels (4 f32 / 8 bf16) when dm == 1 and C * sizeof(elem) % 16 == 0,
// one input channel otherwise (odd C, dm > 1) -- the same kernels, one element at a time.
//
// Work split (dw_plan): a workgroup owns one sample, a tile of toh x tow pixels and up to tc columns.  It
// stages the tile's source with its halo into LDS once with 16-byte loads, positions outside the image as
// zeros, so no compute loop tests a bound; consecutive lanes hold consecutive columns.  A thread then owns
// one column and a strip of kDwStrip pixels along W.
//
//   forward   acc = +0; taps in ascending (i, j): acc = fmaf(f32(x), w, acc); acc += b; max(acc, 0) when ReLU is
//             fused; one rounding to the dtype.  3x3 / 5x5 / 7x7 rows at stride 1 (3x3 also stride 2) without
//             dilation along W keep a kernel row's weights and the strip's row window in registers: an LDS
//             vector is read once per kernel row.  Every other shape reads each tap from LDS.
//   dgrad     gather over the staged dy tile (masked by the saved y > 0 as it is loaded when the forward fused
//             ReLU), f32 from +0 in ascending (i, j, m).  Stride 1 is the forward structure with flipped taps.
//             With strides a row (column) of dx meets the taps i0, i0 + per, ...: per = s / gcd(s, d) is fixed
//             at launch, i0 found once per thread row (strip element), nothing is tested per tap.
//   wgrad     launch 1: the workgroup stages the x halo tile and the (masked) dy tile; its lanes are (column,
//             tap slot, pixel lane): a lane holds ONE tap's V sums in f64 -- the register-sized group -- and
//             walks the tile's pixels in ascending order over LDS, acc = fma(f64(dy), f64(x), acc) (the
//             product is exact), db = the tap of ones.  Pixel lanes combine in a fixed LDS tree; the workgroup
//             writes f64 partials [chunk][kh*kw + 1][C*dm], chunk = (n, tile).  Launch 2: 16 lanes per output
//             add the chunks l, l + 16, ... in ascending order, combine in a fixed tree, round once to f32 and
//             store, or add into what the target holds (acc bit 0: dW, bit 1: db).
//
// No float atomics, no workgroup waits for another; every order depends on the shape alone, so results are
// bit-identical across runs.  Partials beside the data: a workgroup at the full tc = 8 columns and the 3x3
// stride-1 tile of 8 x 16 pixels reads 128 pixels of x and dy (32 KiB bf16, 64 KiB f32 without the halo) and
// writes 10 x 64 (32) f64 = 5 (2.5) KiB: 16 % (4 %) of the traffic; 25 taps: 41 % (10 %) -- see the follow-up
// in the README note.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdl {

enum class DwDType { kF32 = 0, kBF16 = 1 };

struct DwGeom {
  int N, H, W, C;  // input
  int OH, OW;      // output (C * dm channels)
  int kh, kw, sh, sw, dh, dw;
  int pt, pl;  // leading padding (trailing padding is implied by OH / OW)
  int dm;      // depth multiplier
};

constexpr int kDwThreads = 256;
constexpr int kDwStrip = 4;              // outputs a thread produces along W
constexpr int kDwMaxColsVec = 8;         // 16-byte columns per workgroup (128 contiguous bytes per pixel)
constexpr int kDwMaxColsElem = 32;       // single-element columns per workgroup
constexpr int kDwTileBytes = 32 * 1024;  // staged halo tile + output tile, x dm: with wgrad's 16 KiB tree, 3 / CU
constexpr int kDwMaxTaps = 49, kDwMaxDm = 8, kDwMaxCout = 16384;

struct DwPlan {
  int vec;        // elements per column: 16 bytes' worth, or 1
  int cols;       // C / vec
  int tc;         // columns per workgroup: a power of two
  int colblocks;  // ceil(cols / tc)
  int toh, tow;   // tile (tow = kDwStrip * nsw)
  int nsw;        // strips per tile row
  int hh, hw;     // forward halo tile: (toh - 1) sh + (kh - 1) dh + 1, likewise along W
  int ts;         // wgrad: tap slots among the 256 / tc lanes of a column (a power of two)
  int fit;        // 0: even the smallest tile exceeds kDwTileBytes (unsupported)
};
DwPlan dw_plan(const DwGeom& g, DwDType dt);

// y = act(conv(x, w) + b); b nullable; act: 0 none, 1 ReLU
void dw_forward(const void* x, const float* w, const float* b, void* y, DwDType dt, const DwGeom& g, int act,
                hipStream_t s);
// dx; ymask (nullable): the forward's ReLU output, dy counts where ymask > 0
void dw_dgrad(const void* dy, const void* ymask, const float* w, void* dx, DwDType dt, const DwGeom& g, hipStream_t s);
// part: f64 [dw_wgrad_chunks][kh*kw + 1][C*dm] scratch; dW f32 [kh,kw,C,dm]; db f32 [C*dm] (nullable)
int64_t dw_wgrad_chunks(const DwGeom& g, DwDType dt);
void dw_wgrad(const void* x, const void* dy, const void* ymask, double* part, float* dW, float* db, int acc,
              DwDType dt, const DwGeom& g, hipStream_t s);

}  // namespace tdl
