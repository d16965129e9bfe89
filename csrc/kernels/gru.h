// GRU scan (Cho et al.; Keras reset_after = True, gate columns z, r, h: also cuDNN's and torch.nn.GRU's formula) for
// keras.layers.GRU on the GPU (ops/gru.py).  Only the sequential part lives here: the input projection
// mx = x W + b_in and every weight / input gradient are batched GEMMs the callers already have.
//
//   mh_t = h_{t-1} R + b_rec;  z = sigma(mx_z + mh_z);  r = sigma(mx_r + mh_r);  q = mh_h
//   hh = tanh(mx_h + r q);     h_t = z h_{t-1} + (1 - z) hh
//
// Ownership (both kernels): one workgroup of 256 threads owns 16 batch rows (the MFMA M tile) and all U units
// for all T steps; workgroups never wait for each other (no atomics, no flags).  Rows past B are computed on
// zeros and never stored.  Wave w owns the 16-unit tiles j = w, w + 4, ...; for each it keeps three 16 x 16
// accumulators, the z / r / h columns of the same 16 units, so in the MFMA C layout (lane l: rows
// 4 (l >> 4) + i, column l & 15) the three gates, h_{t-1} and the new h of one (row, unit) sit in the same lane
// and register index and the gate math and the state update are lane-local.
//
// Forward: the state lives twice: as an f32 register value per lane (bf16: the value already rounded to bf16, so
// hs holds exactly the state) for the element-wise update, and in double-buffered LDS as the next step's A
// operand, read as 16-byte fragments (f32: four k = 4 MFMAs per fragment; bf16: one k = 32 MFMA); one barrier
// per step.  The z and r accumulators start from mx_z + b_rec_z and mx_r + b_rec_r, the h accumulator from
// b_rec_h alone: the candidate multiplies the whole recurrent part by r before mx_h, kept in a register of its
// own, is added.  mx of step t + 1 is loaded before step t's MFMAs.  The B operand is R^T [3U][U] (a transposed
// copy made once per call): resident in LDS for the whole sequence when gru_plan says so, else streamed from
// global memory (L2-resident: the same 3 U^2 elements every step) as 16-byte loads one k-slab ahead.
// The forward writes hs, h_last and, when saving, one [B,T,4U] tensor with the planes z, r, hh, q.
//
// Backward: the reverse scan, with d = dh + dhs_s and h_{t-1} read from hs (h0 at s = 0):
//   da_h = d (1 - z) (1 - hh^2);  da_z = d (h_{t-1} - hh) z (1 - z);  da_r = da_h q r (1 - r)
//   dzx_t = [da_z, da_r, da_h] (gradient of mx);  dzh_t = [da_z, da_r, da_h r] (gradient of mh)
//   dh = d z + dzh_t R^T
// dzx and dzh go to global memory (mx's layout, by time); dzh_t is also staged in LDS, then dzh_t [16, 3U] R^T
// runs on the same MFMAs with K = 3U, N = U (summed from zero; d z is added once, afterwards); its B operand is
// R [U][3U] as stored.  dh is carried in registers.
//
// bf16 contract: R is rounded to bf16 once per call; h_t is rounded to bf16 when stored (the output, the state and
// the next step's operand); the saved planes, dzx and dzh are rounded to bf16 when stored (the backward reads the
// rounded planes, its recurrence the rounded dzh); the accumulators, b_rec, dh and the gate math are f32.  K is
// padded with zeros in LDS when U % 32 != 0 (forward) or 3U % 32 != 0 (backward).
//
// sigma(z) = 1 / (1 + expf(-z)), tanh(z) = 2 sigma(2 z) - 1, in f32 with one rounding per operation (no
// contraction into fma), the same two functions in both kernels and in lstm.hip.
//
// Sequences (hs, saved) are indexed by processing step s; mx, dzx and dzh by time t = s, or T - 1 - s with rev.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdl {

constexpr int kGruThreads = 256;
constexpr int kGruRows = 16;               // batch rows per workgroup
// 4 tiles per wave: per lane 48 accumulator registers, 48 of the next step's mx, 16 of mx_h and 16 of state
constexpr int kGruMaxU = 256;
constexpr int kGruLdsBudget = 160 * 1024;  // LDS of a workgroup on gfx950

struct GruPlan {
  bool resident;    // R in LDS for the whole sequence (forward and backward)
  int lds_fwd;      // bytes of dynamic LDS of the forward / backward launch
  int lds_bwd;
  int workgroups;   // ceil(B / 16)
  int tiles_wave;   // 16-unit tiles per wave the instantiation holds: 1, 2, 4
  int resident_max_u;
};
// U % 16 == 0, 16 <= U <= kGruMaxU
GruPlan gru_plan(int64_t B, int64_t T, int U, bool bf16);

struct GruArgs {
  int B, T, U, rev;
  const void* zx;      // forward: mx [B,T,3U]
  const void* r;       // forward: R^T [3U][U]; backward: R [U][3U]; 16-byte aligned
  const float* b_rec;  // [3U] or null
  const void* h0;      // [B,U] or null
  void* hs;            // [B,T,U]: forward output, backward input
  void* saved;         // [B,T,4U] planes z, r, hh, q: forward output (null: inference), backward input
  void* h_last;        // [B,U]
  // backward inputs (each nullable) and outputs (dh0 nullable)
  const void* dhs;     // [B,T,U]
  const void* dh_last; // [B,U]
  void* dzx;           // [B,T,3U]
  void* dzh;           // [B,T,3U]
  void* dh0;           // [B,U]
};

void gru_forward(const GruArgs& a, bool bf16, hipStream_t s);
void gru_backward(const GruArgs& a, bool bf16, hipStream_t s);

// out[c] (+)= sum over the rows of x [rows][cols] (f32 or bf16), summed in f64 in a fixed order (no atomics)
void gru_colsum(const void* x, bool bf16, int64_t rows, int cols, float* out, bool accumulate, hipStream_t s);

}  // namespace tdl
