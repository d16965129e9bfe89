// Device helpers shared by the seeded kernels (dropout.hip, augment.hip): the Philox4x32-10 block function
// and the call-counter ("ticket") protocol.  The stream and the protocol are specified in dropout.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdl {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&o)[4]) {
  typedef unsigned long long u64;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const u64 p0 = (u64)0xD2511F53u * c0;
    const u64 p1 = (u64)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o[0] = c0;
  o[1] = c1;
  o[2] = c2;
  o[3] = c3;
}

// ---- ticket (dropout.h): state = [calls, arrivals], or null with the ticket in *ticket_in ----
__device__ __forceinline__ unsigned long long ticket_read(int64_t* state, const int64_t* ticket_in,
                                                          int64_t* ticket_out) {
  typedef unsigned long long u64;
  u64 t;
  if (state != nullptr)
    t = __hip_atomic_load(reinterpret_cast<u64*>(state), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    t = (u64)*ticket_in;
  if (ticket_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *ticket_out = (int64_t)t;
  return t;
}

__device__ __forceinline__ void ticket_arrive(int64_t* state, unsigned long long t) {
  typedef unsigned long long u64;
  if (state == nullptr) return;
  __syncthreads();  // the workgroup's last store is issued
  if (threadIdx.x == 0) {
    u64* s = reinterpret_cast<u64*>(state);
    const u64 prev = __hip_atomic_fetch_add(s + 1, (u64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == (u64)gridDim.x - 1) {  // every workgroup has read calls: advance it for the next launch
      __hip_atomic_store(s + 1, (u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(s, t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace tdl
