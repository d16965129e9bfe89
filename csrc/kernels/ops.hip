// Generic data-movement kernels: device-resident dataset batch gather (SURVEY.md §3.2 target:
// zero H2D traffic in the hot loop).  One workgroup per gathered row, 16-byte vector accesses.
#include "common.h"
#include "ops.h"

#include <algorithm>

namespace tdl {

// a batch of (f32 feature row, label) pairs of a device-resident dataset in ONE launch (the generic
// engine's device input path): workgroup r copies row idx[r] and its thread 0 the label (4 or 8 bytes)
__global__ __launch_bounds__(256) void k_gather_xy(const float* __restrict__ src, const void* __restrict__ lab,
                                                   const int* __restrict__ idx, float* __restrict__ out,
                                                   void* __restrict__ out_lab, int64_t row_elems, int lab_bytes) {
  const int64_t r = blockIdx.x;
  const int64_t i = idx[r];
  const float* s = src + i * row_elems;
  float* o = out + r * row_elems;
  if ((row_elems & 3) == 0) {
    for (int64_t e = threadIdx.x * 4; e < row_elems; e += 1024) st4(o + e, ld4(s + e));
  } else {
    for (int64_t e = threadIdx.x; e < row_elems; e += 256) o[e] = s[e];
  }
  if (threadIdx.x == 0) {
    if (lab_bytes == 8)
      static_cast<long long*>(out_lab)[r] = static_cast<const long long*>(lab)[i];
    else
      static_cast<int*>(out_lab)[r] = static_cast<const int*>(lab)[i];
  }
}

void gather_xy(const float* src, const void* lab, const int* idx, float* out, void* out_lab, int64_t rows,
               int64_t row_elems, int lab_bytes, hipStream_t s) {
  if (rows == 0) return;
  hipLaunchKernelGGL(k_gather_xy, dim3((unsigned)rows), dim3(256), 0, s, src, lab, idx, out, out_lab, row_elems,
                     lab_bytes);
}

namespace {

__global__ __launch_bounds__(256) void k_slab_transpose_bf16(const float* __restrict__ src, uint16_t* __restrict__ dst,
                                                            const int4* __restrict__ entries,
                                                            const int4* __restrict__ tiles) {
  __shared__ float t[64][65];
  const int4 tl = tiles[blockIdx.x];
  const int4 e = entries[tl.x];
  const int R = e.z, K = e.w, r0 = tl.y * 64, k0 = tl.z * 64;
  const int tid = threadIdx.x;
  // read 64 rows (r) x 64 columns (k): thread -> column k0 + (tid & 63), rows (tid >> 6) + 4 i
  const int kc = tid & 63;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = (tid >> 6) + 4 * i;
    t[r][kc] = (r0 + r < R && k0 + kc < K) ? src[(long long)e.x + (long long)(r0 + r) * K + k0 + kc] : 0.f;
  }
  __syncthreads();
  // write 64 rows (k) x 64 columns (r): thread -> r column r0 + (tid & 63), k rows (tid >> 6) + 4 i
  const int rc = tid & 63;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int k = (tid >> 6) + 4 * i;
    if (k0 + k < K && r0 + rc < R) {
      dst[(long long)e.y + (long long)(k0 + k) * R + r0 + rc] = (uint16_t)pack_bf16x2(t[rc][k], 0.f);
    }
  }
}

}  // namespace

void slab_transpose_bf16(const float* src, uint16_t* dst, const int* entries, const int* tiles, int ntiles,
                         hipStream_t s) {
  if (ntiles <= 0) return;
  hipLaunchKernelGGL(k_slab_transpose_bf16, dim3(ntiles), dim3(256), 0, s, src, dst,
                     reinterpret_cast<const int4*>(entries), reinterpret_cast<const int4*>(tiles));
}

namespace {

// dst[i] = bf16(src[i]), 8 elements (two 16-B loads, one 16-B store) per thread per iteration
__global__ __launch_bounds__(256) void k_cast_bf16(const float* __restrict__ src, uint16_t* __restrict__ dst,
                                                  long long n8) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < n8; v += stride) {
    const f4 a = reinterpret_cast<const f4*>(src)[2 * v], b = reinterpret_cast<const f4*>(src)[2 * v + 1];
    const float f[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(f[2 * j], f[2 * j + 1]);  // (keeps NaN: a diverged slab stays NaN)
    reinterpret_cast<uint4*>(dst)[v] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

}  // namespace

void cast_bf16(const float* src, uint16_t* dst, long long n, hipStream_t s) {
  const long long n8 = n / 8;
  if (n8 > 0) {
    const long long blocks = std::min<long long>((n8 + 255) / 256, 256 * 8);
    hipLaunchKernelGGL(k_cast_bf16, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, n8);
  }
}

}  // namespace tdl
