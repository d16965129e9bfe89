// Embedding lookup and its gradient: y[n, :] = E[ids[n], :] over ids [N] (int32 or int64, read as they come),
// a table E [V, D] in f32 (or its bf16 compute copy), y / dy [N, D] in f32 or bf16, dE [V, D] in f32.  Used by
// keras.layers.Embedding on the GPU (ops/embedding.py).
//
// An id outside [0, V) -- negative ids and 64-bit ids beyond 2^32 included -- is defined: its forward row is
// zeros and it contributes nothing to dE.  The id is compared before anything is computed from it, so no
// address is ever formed from such an id.
//
// Forward, k_embed_fwd, one launch.  A row is `cols = D / vec` accesses of `vec` elements: 16 bytes of the output
// where a row is a multiple of 16 bytes and every pointer is 16-byte aligned (vec = 4 in f32, 8 in bf16), else
// one element.  L = the smallest power of two >= cols (at most 64) lanes hold a row, so 64 / L rows share a
// wave (16 rows at D = 16 in f32) and a workgroup of four waves moves 256 / L rows; a wider row is walked by
// its 64 lanes.  bf16 output is either one round-to-nearest-even per element of the f32 table or a plain copy
// of a bf16 table: the same bits, half the bytes read.
//
// Backward: ordered owner-computes, two launches, no sort and no float atomics.
//   dE[v, :] = the f32 left fold of dy[n, :] over the tokens n with ids[n] == v, in ascending n, started from
//   the first term (bf16 dy widened exactly first); then target[v] = target[v] + s (the gradient is added into
//   a slab view) or dE[v] = s, and zeros for a row no token names (a fresh tensor).
//   One rounding per addition, in an order that depends on ids alone.
//   k_embed_count  counts[r] = number of tokens whose id lies in range r, a range being rows_wg consecutive rows
//                  of the vocabulary.  Integer atomics, one per distinct range of a wave's 64 ids (the order of
//                  integer additions does not matter).  THE HOST PROVIDES THE ZEROED counts WORKSPACE, one int
//                  per range, for every backward; no kernel here clears a word, and nothing persists between calls.
//   k_embed_bwd    one workgroup of 8 waves owns each range and keeps its f32 accumulator tile [rows_wg, D] in LDS
//                  (started at -0, the one value with -0 + x == x for every x, so the fold starts from its first
//                  term bit for bit).  An owner whose count is zero returns at once (fresh: after storing its zero
//                  rows).  Otherwise it scans ids in ascending blocks of scan_block = 8 waves x 64 lanes x 4 ids,
//                  the next block's ids loaded ahead of the current block's compaction, and compacts the tokens of
//                  its range into an LDS queue of (n, local row) that keeps their order: a ballot and a prefix
//                  count per wave, the waves' totals added in wave order.  It drains the queue when the next block
//                  would not fit and at the end, and stops scanning once it has found its count.
//       drain      wave w takes the entries whose local row is == w modulo 8 and walks them in queue order, its
//                  lanes across D (64 accesses at a time): the dy loads of the next 8 of its entries are issued
//                  ahead of their LDS adds, which then run in entry order.  A row's additions are thus in
//                  ascending n on one wave; different rows run on different waves.
//       epilogue   fresh: every row of the range is stored (zeros for a row without a touched flag), so there is
//                  no memset; target: only touched rows are read, added and written.  No other workgroup
//                  writes those rows.
//   No workgroup waits for another, nothing can hang and no co-residency is assumed.  Every owner scans all of
//   ids: the cost grows with ranges x N (profiles/embedding_cost.txt, and the bound in ops/embedding.py).
//
// LDS of k_embed_bwd: queue 16 KiB + flags and wave totals < 1 KiB + the tile, within the 160 KiB of a
// workgroup (kLstmLdsBudget); rows_wg = min(64, what fits), a function of D alone; D <= kEmbMaxD leaves 8 rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdl {

constexpr int kEmbFwdThreads = 256;
constexpr int kEmbBwdThreads = 512;
constexpr int kEmbBwdWaves = kEmbBwdThreads / 64;
constexpr int kEmbScanItems = 4;                                // ids per thread and scan block
constexpr int kEmbScanBlock = kEmbBwdThreads * kEmbScanItems;   // 2048
constexpr int kEmbQueue = kEmbScanBlock;                        // queue capacity (entries of 8 bytes)
constexpr int kEmbPrefetch = 8;                                 // dy rows in flight per wave in the drain
constexpr int kEmbMaxRowsWg = 64;
constexpr int kEmbCountThreads = 256;
constexpr int kEmbLdsBudget = 160 * 1024;                       // = kLstmLdsBudget
constexpr int kEmbLdsFixed = kEmbQueue * 8 + kEmbMaxRowsWg * 4 + 2 * kEmbBwdWaves * 4;
constexpr int kEmbMaxD = 4096;                                  // 8 rows of the tile: one per wave
constexpr int64_t kEmbMaxBlocks = int64_t(1) << 24;             // (a launch of 2^32 threads and more is refused)

struct EmbPlan {
  int vec;                // elements per access: 4 (f32) / 8 (bf16) when D % vec == 0, else 1
  int L;                  // forward lanes per row: 1 ... 64
  int rows_per_wave_fwd;  // 64 / L
  int64_t fwd_blocks;     // ceil(N / (4 * rows_per_wave_fwd))
  int rows_wg;            // vocabulary rows per backward workgroup
  int64_t ranges;         // ceil(V / rows_wg): backward workgroups and count words
  int lds_bwd;            // bytes
};
// D in [1, kEmbMaxD], N >= 1, V >= 1; bf16: the dtype of y / dy
EmbPlan embed_plan(int64_t N, int64_t V, int D, bool bf16);

// table_bf16 needs out_bf16.  The 16-byte form runs when plan.vec > 1 and ids aside every pointer is aligned
void embed_forward(const void* ids, bool ids64, const void* table, bool table_bf16, void* y, bool out_bf16, int64_t N,
                   int64_t V, int D, hipStream_t s);

// counts: `ranges` zeroed ints (see above).  target: out [V, D] is added into; else every row of it is stored
void embed_backward(const void* ids, bool ids64, const void* dy, bool dy_bf16, float* out, bool target, int* counts,
                    int64_t N, int64_t V, int D, hipStream_t s);

}  // namespace tdl
