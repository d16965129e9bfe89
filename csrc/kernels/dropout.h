// Seeded dropout (dropout.hip): the keep mask is a pure function of (key, ticket, element index), so the
// backward recomputes it and no mask tensor exists.
//
// Stream.  Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl 0x9E3779B9 / 0xBB67AE85), key
// (k0, k1), counter (g_lo, g_hi, t_lo, t_hi): g = (mask index + elem_offset) >> 2 names a group of four
// consecutive mask elements, t is the ticket (the call number of the layer on this device).  Mask element
// m takes word (m + elem_offset) & 3 of its group and is DROPPED iff word < thr (thr = int(rate * 2^32),
// up to 2^32 = drop everything).  Kept: x * scale in one f32 multiply; dropped: +0 by a select.  bf16
// computes in f32 and rounds to nearest even.  ops/dropout.py philox_reference is the same stream in numpy.
//
// Ticket.  state = [calls, arrivals] (int64, device).  Every workgroup reads calls at entry, workgroup 0
// writes it to ticket_out, each workgroup's thread 0 adds 1 to arrivals after the workgroup's last store, and
// the workgroup that observes gridDim.x - 1 stores arrivals = 0 and calls = t + 1.  Every read of calls
// precedes its own workgroup's arrival, so the increment cannot race a read; no workgroup waits for another.
// The backward passes state = null and reads the forward's ticket from ticket_in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdl {

constexpr int kDropoutThreads = 256;
constexpr int kDropoutWgElems = 8192;  // elements a workgroup covers per grid-stride trip (both dtypes)
constexpr int kDropoutMaxGrid = 2048;  // 256 CUs x 8 workgroups
// tensors of up to kDropoutSmallN elements (64 workgroups of kDropoutWgElems: a quarter of the CUs) take
// kDropoutSmallWgElems elements per workgroup and trip instead: two 16-B vectors per thread in f32, one in bf16
constexpr int kDropoutSmallWgElems = 2048;
constexpr int64_t kDropoutSmallN = 64 * (int64_t)kDropoutWgElems;

struct DropoutArgs {
  const void* x;
  void* y;
  int64_t n;
  int64_t* state;            // forward: [calls, arrivals]; backward: null
  const int64_t* ticket_in;  // backward: the forward's ticket; forward: null
  int64_t* ticket_out;       // forward: receives the ticket used; backward: null
  uint32_t k0, k1;
  uint64_t thr;  // <= 2^32
  float scale;
  int64_t elem_offset;  // multiple of 4
  bool bf16;
};

// full-shape mask: mask index = element index
void dropout_apply(const DropoutArgs& a, hipStream_t s);
// broadcast mask over a (collapsed) shape of up to 4 dimensions: mask index = sum coord_d * nstride[d]
void dropout_apply_bcast(const DropoutArgs& a, const int64_t dims[4], const int64_t nstride[4], hipStream_t s);
// test hook: grid cap of both kernels (0 = kDropoutMaxGrid)
void dropout_force_max_grid(int64_t g);

}  // namespace tdl
