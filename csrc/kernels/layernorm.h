// Layer normalisation (Ba et al.) and RMS normalisation (Zhang & Sennrich) over the last C contiguous
// elements of an [R, C] view, bf16 or f32 data, f32 gamma / beta, f64 statistics.  Used by
// keras.layers.LayerNormalization on the GPU (ops/layernorm.py).
//
// A row fits in registers, so x is read once and everything is done from registers: the forward is one
// launch, the backward two (k_ln_bwd, then the small k_ln_dgb that folds the per-block dgamma / dbeta
// partials).  The lanes of a row each hold up to `ept` elements, as vectors of `vec` elements at the vector
// columns lr, lr + L, lr + 2 L, ... of the row (lr: the lane's index in its row, L: lanes per row), so every
// access of a row is a contiguous run of 16-byte loads.
//
// Plans (ln_plan): what decides them is C, the dtype and -- for rows_wg / blocks only -- R.
//   kLnSub    8 elements per lane, L = 4 ... 64 lanes per row (the smallest power of two that holds the row);
//             256 / L rows per workgroup iteration, 64 / L of them in each wave.             C <=  512
//   kLnWave   32 elements per lane, L = 64: a wave per row, 4 rows per workgroup iteration.   C <= 2048
//   kLnGroup  32 elements per thread, all 256 threads on one row; the four waves' sums meet in
//             LDS and are added in wave order ((w0 + w1) + w2) + w3.                         C <= 8192
// These are the forward's plans.  The backward holds x, dy and two f64 column accumulators per element: at 32
// elements per lane the compiler needs 300 to 512 VGPRs and spills in the per-element instantiation, so every
// backward lane takes 8 elements, with the accumulators in registers (not in LDS), and a row wider than 512
// spreads over Lb = 128 ... 1024 lanes: the workgroup is the row's lanes, its Lb / 64 waves meet in LDS and
// are added in ascending wave order.  A 1024-thread workgroup may hold 128 VGPRs per lane, which is what
// 8 elements need (profiles/layernorm_cost.txt has every instantiation).
// kLnMaxC = 8192 = 1024 backward lanes x 8 elements = 256 forward threads x 32 elements: the widest row the
// largest workgroup holds at the widths per lane that compile without scratch.  No instantiation uses scratch.
//
// Order of every sum (a function of (R, C, dtype) alone; never of an address or the run):
//   row sums      a lane adds its elements in ascending (vector, element) order in f64, then the L lanes of
//                 the row combine in an xor butterfly (offsets 1, 2, ... L / 2; both partners form the same
//                 a + b), then, where a row has several waves, those in LDS in ascending wave order.
//   dgamma/dbeta  a lane owns the same columns for every row of its block (rows_wg consecutive rows) and
//                 adds them in ascending row order into f64 registers; in kLnSub the row groups of a wave
//                 then combine in an xor butterfly (offsets L ... 32) and the waves of the workgroup are added
//                 into wave 0 in wave order through LDS; the block writes part[block][2][C].  k_ln_dgb adds the
//                 blocks of 8 fixed sub-ranges (ceil(blocks / 8) consecutive blocks each, ascending), then
//                 the 8 sub-range sums ascending, and rounds once to f32.
// No float atomics, no workgroup waits for another, no host synchronisation.  Nothing but dgamma / dbeta
// crosses a row, so a row's y and dx bits depend on that row alone.
//
// Forward, per row (RMS: mean = 0 and no beta):
//   mean = (sum x) / C;  var = (sum (x - mean)^2) / C  (centred, from the same registers);
//   r = 1 / sqrt(var + eps)                                                      -- all f64
//   a = f32(r), b = f32(-mean r);  xhat = fmaf(x, a, b)        (RMS: xhat = x * a)
//   y = fmaf(xhat, gamma, beta) | xhat * gamma | xhat + beta | xhat;  one rounding to the dtype
// Backward, per row, with a, b, xhat recomputed exactly as above from the saved (mean, r):
//   g = dy * gamma (f32, one rounding; g = dy without gamma)
//   S1 = sum g, S2 = sum g xhat in f64 (the product of two f32 values is exact in f64)
//   m1 = f32(S1 / C), m2 = f32(S2 / C)
//   u = g - m1 (RMS: u = g);  t = fmaf(-xhat, m2, u);  dx = a * t;  one rounding to the dtype
//   dgamma_c += f64(dy) f64(xhat) (one fma), dbeta_c += f64(dy)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdl {

enum class LnDType { kF32 = 0, kBF16 = 1 };

constexpr int kLnSub = 0, kLnWave = 1, kLnGroup = 2;
constexpr int kLnThreads = 256;
constexpr int kLnMaxThreads = 1024;  // the widest backward workgroup
constexpr int kLnEptSub = 8;    // elements per lane, kLnSub and every backward
constexpr int kLnEpt = 32;      // elements per lane / thread, kLnWave and kLnGroup
constexpr int kLnSubWaveMaxC = 32 * kLnEptSub;       // widest row that shares its wave (L = 32)
constexpr int kLnSubMaxC = 64 * kLnEptSub;           // widest kLnSub row
constexpr int kLnWaveMaxC = 64 * kLnEpt;             // widest row one wave holds
constexpr int kLnMaxC = kLnThreads * kLnEpt;         // 8192
// widest per-element row (vec = 1): its backward needs 130 VGPRs at 8 elements per lane, more than a 1024-thread
// workgroup may hold, so it spreads over 512 lanes at most
constexpr int kLnMaxCPerElement = kLnMaxThreads / 2 * kLnEptSub;  // 4096
constexpr int kLnTargetBlocks = 1024;                // backward blocks aimed at (4 per CU)
constexpr int kLnDgbRanges = 8;                      // first-level sub-ranges of k_ln_dgb

struct LnPlan {
  int vec;          // elements per access: 16 bytes' worth when C * sizeof(elem) % 16 == 0, else 1
  int cols;         // C / vec
  int plan;         // kLnSub / kLnWave / kLnGroup
  int L;            // lanes per row: 4 ... 64, or 256 in kLnGroup
  int rpi;          // rows per forward workgroup: 256 / L
  int Lb;           // lanes per row in the backward: L in kLnSub, else 128 ... 1024 (the workgroup)
  int64_t rows_wg;  // consecutive rows per workgroup in the backward (kLnSub: a multiple of rpi)
  int64_t blocks;   // ceil(R / rows_wg): backward workgroups and dgamma / dbeta partials
  int64_t fwd_blocks;  // ceil(R / rpi)
};
// C in [1, kLnMaxC], R >= 1
LnPlan ln_plan(int64_t R, int C, LnDType dt);

// stats: f64 [R][2] out (mean, r); gamma / beta nullable (1 / 0); rms: no centring, beta ignored
void ln_forward(const void* x, void* y, LnDType dt, int64_t R, int C, const float* gamma, const float* beta,
                double eps, bool rms, double* stats, hipStream_t s);

// part: f64 [blocks][2][C] scratch (untouched when both dgamma and dbeta are null).  dgamma / dbeta nullable;
// stored, or (acc bit 0 dgamma, bit 1 dbeta) added into what the target holds
void ln_backward(const void* dy, const void* x, void* dx, LnDType dt, int64_t R, int C, const float* gamma,
                 const double* stats, bool rms, double* part, float* dgamma, float* dbeta, int acc, hipStream_t s);

}  // namespace tdl
