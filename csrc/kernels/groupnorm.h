// Group normalisation (Wu & He) over channels-last activations [N, P, C] (P = product of the spatial
// dims, 1 for a [N, C] input), G groups of C / G consecutive channels, bf16 or f32 data, f32 gamma /
// beta, f64 statistics.  Used by keras.layers.GroupNormalization on the GPU (ops/groupnorm.py).
//
// Either direction is three launches: a streaming pass that reduces per (sample, channel) over the
// pixels, a tiny finalize that folds the channel sums into groups and writes per-(sample, channel)
// coefficient tables, and an elementwise pass that reads those tables.  Because the streaming passes
// never look at a group, a 16-byte vector may straddle a group boundary: the vector path needs only
// C * sizeof(elem) % 16 == 0, everything else takes the same kernels one element at a time.
//
// Every sum is taken in f64 from the first add (a product of two f32 / bf16 values is exact in f64) and
// in an order fixed by (P, C, dtype) alone -- gn_plan below; never by N, an address or the run: thread
// (row lane rl, column) of workgroup (n, column block, chunk) adds its pixels p = chunk * rows_wg + rl,
// + RL, ... in ascending order, the row lanes combine in a fixed LDS tree, the finalize adds the chunks
// in ascending order, then the channels of a group (the lanes of its slot, a power of two up to 64, each
// ascending over its channels, then an xor butterfly; small groups share a wave).
// Nothing crosses a sample except dgamma / dbeta (n ascending), so a sample's y and dx bits depend on
// that sample alone.  No float atomics, no workgroup waits for another, no host synchronisation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdl {

enum class GnDType { kF32 = 0, kBF16 = 1 };

// What one workgroup of a streaming / elementwise pass covers: at most kGnMaxCols 16-byte columns (one wave
// across: 1 KiB contiguous per pixel row) and kGnChunkBytes of x, but no more than kGnMaxRows pixels, rounded
// up to whole iterations.  Each (workgroup, channel) leaves two f64 partials, so a workgroup must read many
// pixels per channel for the partials to stay small beside x: at the full 64 columns it reads 128 pixels
// (6 % of a bf16 tensor, 3 % of an f32 one), with fewer columns more.  Compile-time constants: changing them
// changes the order of the sums
constexpr int kGnChunkBytes = 131072;
constexpr int kGnMaxCols = 64;
constexpr int kGnMaxRows = 512;
constexpr int kGnThreads = 256;
constexpr int kGnUnroll = 4;  // rows a thread has in flight

struct GnPlan {
  int vec;          // elements per access: 16 bytes' worth when C * sizeof(elem) % 16 == 0, else 1
  int cols;         // C / vec columns of such accesses in a pixel row
  int tc;           // columns per workgroup = min(cols, kGnMaxCols)
  int rl;           // row lanes = 256 / tc: rows a workgroup reads per iteration
  int colblocks;    // ceil(cols / tc)
  int64_t rows_wg;  // pixels per workgroup: a multiple of rl * kGnUnroll
  int64_t chunks;   // ceil(P / rows_wg): partial sums per (sample, channel)
};
GnPlan gn_plan(int64_t P, int C, GnDType dt);

// phases of either direction (a bench hook: the default runs all three)
constexpr int kGnSums = 1, kGnFinalize = 2, kGnApply = 4, kGnAll = 7;

// forward.  part: f64 [N][chunks][2][C] scratch (sums of x and x^2); stats: f64 [N][G][2] out (mean,
// r = 1 / sqrt(var + eps), var = max(E[x^2] - mean^2, 0) over the m = P * C / G values of a group);
// coef: f32 [2][N][C] scratch (scale = gamma r, shift = beta - mean gamma r, each formed in f64 and
// rounded once); y = fmaf(x, scale, shift) rounded once to the dtype.  gamma / beta nullable (1 / 0).
void gn_forward(const void* x, void* y, GnDType dt, int64_t N, int64_t P, int C, int G, const float* gamma,
                const float* beta, double eps, double* part, double* stats, float* coef, hipStream_t s,
                int phases = kGnAll);

// backward.  part: f64 [N][chunks][2][C] scratch (a = sum dy, b = sum dy x); coef: f32 [3][N][C] scratch;
// dx = fmaf(A, dy, fmaf(B, x, D)) with, per (n, g), S1 = sum_c gamma a, S2 = r sum_c gamma (b - mean a):
//   A = gamma r,  B = -r^2 S2 / m,  D = r^2 mean S2 / m - r S1 / m     (f64, rounded to f32 once)
// dbeta_c = sum_n a, dgamma_c = sum_n r (b - mean a), n ascending, rounded to f32 once and stored, or
// (acc bit 0 dgamma, bit 1 dbeta) added into what the target holds.
void gn_backward(const void* dy, const void* x, void* dx, GnDType dt, int64_t N, int64_t P, int C, int G,
                 const float* gamma, const double* stats, double* part, float* coef, float* dgamma, float* dbeta,
                 int acc, hipStream_t s, int phases = kGnAll);

}  // namespace tdl
