// Gradient accumulation over the flat gradient slab (accum.hip): one streaming kernel keeps the f32
// accumulator slab A of an optimizer built with gradient_accumulation_steps = k (keras/optimizers.py).
//
// The phase p = iterations mod k of a micro-step is known to the host at launch and at capture time, so it
// is a launch argument (the mode), never a device counter:
//   mode 0 (p == 0):       A = G
//   mode 1 (0 < p < k-1):  A = A + G
//   mode 2 (p == k-1):     G = (A + G) * c,  c = float32(1 / k);  A is left as it is
// every operation a single f32 rounding (no FMA, no division): numpy reproduces the bits.
// zero_g (modes 0 and 1 only): G = +0 once it is read, what the update kernels' zero_grad leaves behind.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdl {

constexpr int kAccumThreads = 256;  // threads of a k_grad_accum workgroup
constexpr int kAccumVecs = 4;       // 16-B accesses per thread per tensor, all loads issued before the first store
constexpr int kAccumBlockElems = kAccumThreads * kAccumVecs * 4;  // elements a workgroup handles per grid pass
constexpr int kAccumMaxBlocks = 2048;  // grid cap: 256 CUs x 8 workgroups; larger slabs grid-stride

// g, a: whole n-element slabs, 16-byte aligned, not overlapping.  n == 0 launches nothing.
// max_blocks: the grid cap, 1 .. kAccumMaxBlocks (tests and scripts/bench_accum.py lower it).
void grad_accum_apply(float* g, float* a, int64_t n, int mode, float c, bool zero_g, hipStream_t s,
                      int max_blocks = kAccumMaxBlocks);

}  // namespace tdl
