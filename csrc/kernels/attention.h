// Fused scaled-dot-product attention, forward and backward, f32 or bf16 operands, f32 accumulation.  Used by
// keras.layers.MultiHeadAttention on the GPU (ops/attention.py).
//
//   o[b,i,h,:] = sum_j softmax_j(scale q[b,i,h,:] . k[b,j,h,:]) v[b,j,h,:]      over the admitted keys j of row i
//
// q [B,T,H,D], k [B,S,H,D], v [B,S,H,Dv] with arbitrary element strides on the first three axes (the innermost is
// contiguous and 16-byte aligned): projection outputs and slices of a packed qkv buffer are consumed as views.
// Key j is admitted for row i iff j < S, (not causal or j <= i) and (no mask or mask[b,(h),i,j] != 0); the mask is
// bytes, read with its strides (a stride of 0 broadcasts the heads).  A row without an admitted key gives o = 0,
// lse = -inf and takes no part in any gradient -- never a NaN.  (Keras gives the mean of v there, torch NaN.)
//
// Every product runs on the MFMA: f32 operands on v_mfma_f32_16x16x4_f32 (a lane loads 4 consecutive k as one
// 16-byte vector and feeds element j to MFMA j: the k order of a sum is permuted the same way on both sides),
// bf16 operands on v_mfma_f32_16x16x32_bf16.  All operands of all GEMMs are "row-major along k": a lane's fragment
// is one ds_read_b128 (or one global 16-byte load) at [row or column l % 16][k0 + (l / 16) * E], E = 4 or 8
// elements.  Operands whose k axis is the key / query index (V for P V, K for dS K, dO and Q in the dK/dV kernel)
// are transposed as they are staged into LDS.  LDS rows are padded by one fragment (16 bytes), which spreads the 16
// rows a b128 read touches over all banks.  Head dimensions are zero-padded in LDS to HD = 32, 64 or 128.
//
// k_attn_fwd: a workgroup of 4 waves per (batch, head, 64 queries); a wave owns 16 query rows and keeps its Q
//   fragments in registers.  Per 64-key tile: K and V^T are staged, S = Q K^T, the online softmax runs in registers
//   in the log2 domain (scale log2(e) folded into one factor, v_exp_f32), row max / sum over the 16 lanes that
//   share a row by DPP, P goes through a per-wave LDS strip into A-operand layout (rounded once to bf16 for bf16
//   operands), O += P V.  Causal: key tiles above the diagonal are not visited, everything else is masked by index.
// k_attn_delta: delta[b,h,i] = sum_d do o, one thread per row, f32.
// k_attn_dq: the forward's split; recomputes P = exp2(s c - lse log2 e), dS = P (dO V^T - delta), dQ = scale dS K.
// k_attn_dkv: a workgroup per (batch, head, 64 keys), a wave owns 16 keys and keeps K and V fragments in registers;
//   loops over the query tiles (causal: from the diagonal), S^T = K Q^T, dP^T = V dO^T, dV += P^T dO,
//   dK += scale dS^T Q.
// No atomics; every sum's order is fixed by the shape: bit-identical from run to run.  All staging is single
// (one tile resident): at HD = 128 in f32 the dK/dV kernel's four operand tiles and strip take 155,136 B of the
// 160 KiB LDS.
//
// Attention dropout (the DROP instantiations of the three tile kernels; state or ticket_in set).  With the keep mask
// z and c = 1 / (1 - rate):  P~ = c z P (rounded once to bf16 for bf16 operands), o = P~ V; the row maximum, the row
// sum and lse stay those of the undropped row.  Backward: delta = sum_d do o as before (= sum_j P~ dP~), dP~ = dO V^T,
// dS = P (c z dP~ - delta), dV = P~^T dO.  Nothing is saved but o, lse and the ticket: every kernel recomputes z.
// Stream: element (b, h, i, j) has mask index m = 4 (((b H + h) ceil(T / 4) + (i >> 2)) S + j) + (i & 3) -- the linear
// index into a contiguous [B H, ceil(T / 4), S, 4] array -- and from there on it is the stream of dropout.h (group
// m >> 2, word m & 3, dropped iff word < thr), so the mask is independent of the tiling.  Four rows of one key share a
// Philox block: in k_attn_fwd and k_attn_dq a lane's accumulator holds rows r0 .. r0 + 3 (r0 a multiple of 4) of key
// k0 + 16 t + c, i.e. the four words of one block per t, four calls per lane and 64-key tile, issued ahead of the
// S = Q K^T MFMAs they do not depend on.  In k_attn_dkv the accumulator is transposed (keys j0 .. j0 + 3 of query
// q0 + 16 t + c): the four lanes of a quad share a row group, the lane at quad position n computes the block of key
// j0 + n, and the quad transposes the 4 x 4 words by two DPP quad_perm exchanges (xor 1, xor 2) with selects -- four
// calls per lane and tile again.  The forward takes and advances the ticket by the protocol of dropout.h over the
// linear workgroup id of its three-dimensional grid; the backward kernels read it from ticket_in.  No LDS is added.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdl {

constexpr int kAttnTile = 64;     // queries / keys per tile
constexpr int kAttnMaxHead = 128;

struct AttnArgs {
  const void *q, *k, *v, *dout;  // dout: the gradient of o (backward)
  const uint8_t* mask;           // nullable
  void* o;                       // [B,T,H,Dv] contiguous: written by the forward, read by the backward
  float* lse;                    // [B,H,T]: written by the forward, read by the backward
  float* delta;                  // [B,H,T] workspace of the backward
  void *dq, *dk, *dv;            // contiguous [B,T,H,D], [B,S,H,D], [B,S,H,Dv]
  int64_t qs[3], ks[3], vs[3], gs[3];  // element strides of (batch, sequence, head)
  int64_t ms[4];                       // mask strides of (batch, head, row, key)
  int B, H, T, S, D, Dv;
  int causal;
  float scale;
  // attention dropout: on iff state or ticket_in is set (dropout.h: the stream and the ticket protocol)
  int64_t* state;            // forward: [calls, arrivals]; backward: null
  const int64_t* ticket_in;  // backward: the forward's ticket; forward: null
  int64_t* ticket_out;       // forward: receives the ticket used; backward: null
  uint32_t k0, k1;
  uint64_t thr;  // <= 2^32
  float keep;    // 1 / (1 - rate)
};

struct AttnPlan {
  int hd;                  // padded head dimension of the instantiation
  int q_tiles, k_tiles;    // per (batch, head)
  int64_t causal_skipped;  // (query tile, key tile) pairs per (batch, head) the causal mask leaves unvisited
  int lds_fwd, lds_dq, lds_dkv;  // bytes per workgroup
  int64_t mfma_fwd, mfma_bwd;    // MFMA instructions issued
};
int attn_head_pad(int D, int Dv);  // 32, 64 or 128; 0 outside the limits
AttnPlan attn_plan(int B, int H, int T, int S, int D, int Dv, bool bf16, bool causal);

void attn_forward(const AttnArgs& a, bool bf16, hipStream_t s);
void attn_backward(const AttnArgs& a, bool bf16, hipStream_t s);  // delta, dq, dkv

}  // namespace tdl
