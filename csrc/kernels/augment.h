// Seeded image augmentation (augment.hip): random flip, crop and whole-pixel translation of an NHWC batch as
// ONE coordinate transform per sample, drawn from the Philox stream of dropout.h.
//
// Draws.  Sample n of the call with ticket t takes the four words of
//   Philox4x32-10(key, counter = (n_lo, n_hi, t_lo, t_hi))
// (ops/dropout.py philox_words(key, t, 4 n + j), j = 0..3):
//   flip_w = flip_w_enabled ? w0 >> 31 : 0        flip_h = flip_h_enabled ? w1 >> 31 : 0
//   off_h = off_h_lo + ((w2 * off_h_count) >> 32) off_w = off_w_lo + ((w3 * off_w_count) >> 32)   (64-bit products)
//
// Map, per axis (height shown): output row o reads  r = (flip ? Ho - 1 - o : o) + off.  r in [0, H) is the
// source row; otherwise the fill mode decides: kConstant = the element is `fill` (already rounded to the
// tensor's dtype by the host), kNearest = clamp, kWrap = r mod H, kReflect = the edge-inclusive mirror
// (-1 - r below, 2 H - 1 - r above).  The host guarantees Ho <= H and -H <= off <= H, so r is in
// [-H, 2 H - 1] and one reflection suffices.  The forward copies bits: no arithmetic on x or on the fill.
//
// Backward (gather form, no atomics): dx[n, ih, iw, :] = +0 + the dy of every output pixel that read it, added
// in ascending (oh, ow) order as f32 (bf16: f32 sum, rounded once).  Per axis the candidates of an input
// coordinate are enumerated (one for constant and wrap, up to three for reflect, a run at an edge for
// nearest) and each is confirmed with the forward map.
//
// Ticket: the [calls, arrivals] protocol of dropout.h, unchanged.  Nothing but the ticket is saved for the
// backward, which recomputes the draws.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdl {

constexpr int kAugmentThreads = 256;
// work items (16-B vectors on the vector path, elements on the element path) a workgroup covers per
// grid-stride trip: four per thread, all loaded before the first store
constexpr int kAugmentWgElems = 4 * kAugmentThreads;
constexpr int kAugmentMaxGrid = 2048;  // 256 CUs x 8 workgroups
// The forward launches at most half of that: each of its workgroups ends with an atomic add on the ONE
// arrivals word of the ticket protocol, and 2048 of them in a row cost more than the shorter stride saves
// (256 x 56 x 56 x 64 bf16: 70 us at 2048 workgroups, 39 us at 1024, 36 us at 512; 256 x 224 x 224 x 3 f32: 153 /
// 123 / 169 us; the backward, which does not arrive, is fastest at 2048: profiles/augment_cost.txt)
constexpr int kAugmentFwdMaxGrid = 1024;

enum AugmentFill : int { kConstant = 0, kNearest = 1, kWrap = 2, kReflect = 3 };

struct AugmentSpec {
  int flip_h, flip_w;         // enable flags
  int off_h_lo, off_h_count;  // off_h in [off_h_lo, off_h_lo + off_h_count)
  int off_w_lo, off_w_count;
  int fill_mode;       // AugmentFill
  uint32_t fill_bits;  // the fill value in the tensor's dtype: f32 bits, or bf16 bits in the low half
};

struct AugmentArgs {
  const void* src;  // forward: x [N, H, W, C]; backward: dy [N, Ho, Wo, C]
  void* dst;        // forward: y [N, Ho, Wo, C]; backward: dx [N, H, W, C]
  int64_t N;
  int H, W, Ho, Wo, C;
  int64_t* state;            // forward: [calls, arrivals]; backward: null
  const int64_t* ticket_in;  // backward: the forward's ticket; forward: null
  int64_t* ticket_out;       // forward: receives the ticket used; backward: null
  uint32_t k0, k1;
  AugmentSpec spec;
  bool bf16;
};

// The 16-B vector path is taken when C * element size is a multiple of 16 and both pointers are 16-B aligned,
// the per-element path otherwise.
void augment_forward(const AugmentArgs& a, hipStream_t s);
void augment_backward(const AugmentArgs& a, hipStream_t s);
// test hook: grid cap of both kernels (0 = kAugmentFwdMaxGrid / kAugmentMaxGrid)
void augment_force_max_grid(int64_t g);

}  // namespace tdl
