// LSTM scan (Hochreiter & Schmidhuber; Keras / cuDNN gate order i, f, c, o) for keras.layers.LSTM on the GPU
// (ops/lstm.py).  Only the sequential part lives here: the input projection Zx = x W + b and every weight /
// input gradient are batched GEMMs the callers already have.
//
//   z_t = Zx_t + h_{t-1} R;  i, f, o = sigma(z_i), sigma(z_f), sigma(z_o);  g = tanh(z_c)
//   c_t = f c_{t-1} + i g;   h_t = o tanh(c_t)
//
// Ownership (both kernels): one workgroup of 256 threads owns 16 batch rows (the MFMA M tile) and all U units
// for all T steps; workgroups never wait for each other (no atomics, no flags).  Rows past B are computed on
// zeros and never stored.  Wave w owns the 16-unit tiles j = w, w + 4, ...; for each it keeps four 16 x 16
// accumulators, the i / f / c / o columns of the same 16 units, so in the MFMA C layout (lane l: rows
// 4 (l >> 4) + r, column l & 15) the four gates of one (row, unit) sit in the same lane and register index and
// the gate math, the c update and h are lane-local.  c (forward) and dc (backward) stay in registers for the
// whole sequence.
//
// Forward: h_{t-1} is the A operand, read from LDS as 16-byte fragments (f32: four k = 4 MFMAs per fragment;
// bf16: one k = 32 MFMA); h is double-buffered in LDS, one barrier per step; Zx of step t + 1 is loaded before
// step t's MFMAs.  The B operand is R^T [4U][U] (a transposed copy made once per call): resident in LDS for
// the whole sequence when lstm_plan says so, else streamed from global memory (L2-resident: the same 4 U^2
// elements every step) as 16-byte loads one k-slab ahead.
// Backward: the reverse scan.  dZ_t goes to global memory (Zx's layout) and to LDS, then
// dh_rec = dZ_t [16, 4U] R^T on the same MFMAs with K = 4U, N = U; its B operand is R [U][4U] as stored.
//
// bf16 contract: R is rounded to bf16 once per call; h_t is rounded to bf16 when stored (the output and the next
// step's operand); the saved gates and dZ are rounded to bf16 when stored (the backward reads the rounded gates,
// its recurrence the rounded dZ); c, dc, the accumulators and the gate math are f32.  K is padded with zeros
// in LDS when U % 32 != 0.
//
// sigma(z) = 1 / (1 + expf(-z)), tanh(z) = 2 sigma(2 z) - 1, in f32 with one rounding per operation (no
// contraction into fma), the same two functions in both kernels.  expf overflows to +inf for very negative z,
// which gives sigma = 0, never NaN.
//
// Sequences (hs, gates, cs) are indexed by processing step s; Zx and dZ by time t = s, or T - 1 - s with rev.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdl {

constexpr int kLstmThreads = 256;
constexpr int kLstmRows = 16;               // batch rows per workgroup
// 4 tiles per wave: 64 accumulator registers per lane and 64 more of the next step's Zx.  At 8 tiles (U = 512) the
// forward needs more than the 512 registers of a lane and spills, with or without the Zx look-ahead.
constexpr int kLstmMaxU = 256;
constexpr int kLstmLdsBudget = 160 * 1024;  // LDS of a workgroup on gfx950

struct LstmPlan {
  bool resident;    // R in LDS for the whole sequence (forward and backward)
  int lds_fwd;      // bytes of dynamic LDS of the forward / backward launch
  int lds_bwd;
  int workgroups;   // ceil(B / 16)
  int tiles_wave;   // 16-unit tiles per wave the instantiation holds: 1, 2, 4
  int resident_max_u;
};
// U % 16 == 0, 16 <= U <= kLstmMaxU
LstmPlan lstm_plan(int64_t B, int64_t T, int U, bool bf16);

struct LstmArgs {
  int B, T, U, rev;
  const void* zx;      // [B,T,4U]
  const void* r;       // forward: R^T [4U][U]; backward: R [U][4U]; 16-byte aligned
  const void* h0;      // [B,U] or null
  const float* c0;     // [B,U] or null
  // forward outputs (gates / cs may be null: inference)
  void* hs;            // [B,T,U]
  void* gates;         // [B,T,4U] activated
  float* cs;           // [B,T,U]
  void* h_last;        // [B,U]
  float* c_last;       // [B,U]
  // backward inputs (each nullable) and outputs (dh0 / dc0 nullable)
  const void* dhs;     // [B,T,U]
  const void* dh_last; // [B,U]
  const float* dc_last;
  void* dz;            // [B,T,4U]
  void* dh0;           // [B,U]
  float* dc0;
};

void lstm_forward(const LstmArgs& a, bool bf16, hipStream_t s);
void lstm_backward(const LstmArgs& a, bool bf16, hipStream_t s);

}  // namespace tdl
