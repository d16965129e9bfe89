// The moving average of the weights as a launch of its own (ema.hip): one streaming kernel over the weight
// slab W and the average slab E of an optimizer built with use_ema (keras/optimizers.py), for every update
// that did not run in one of the update kernels -- those keep E themselves (WeightEma, optim.h): the SGD
// inside the fused step's finalize, the xGMI all-reduce with SGD fused into it, a torch-formula update.
//
//   mode 1: E = m * E + c * W                 W is only read
//   mode 2: E = m * E + c * W,  W = E         an overwrite step (ema_overwrite_frequency)
// two products and a sum, three f32 roundings, never contracted: numpy reproduces the bits.  The mode of a
// step is known to the host at launch and at capture time, so it is a launch argument, never a device counter.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdl {

constexpr int kEmaThreads = 256;  // threads of a k_weight_ema workgroup
constexpr int kEmaVecs = 4;       // 16-B accesses per thread per tensor, all loads issued before the first store
constexpr int kEmaBlockElems = kEmaThreads * kEmaVecs * 4;  // elements a workgroup handles per grid pass
constexpr int kEmaMaxBlocks = 2048;  // grid cap: 256 CUs x 8 workgroups; larger slabs grid-stride

// w, e: whole n-element slabs, 16-byte aligned, not overlapping.  n == 0 launches nothing.
// max_blocks: the grid cap, 1 .. kEmaMaxBlocks (tests and scripts/bench_ema.py lower it).
void weight_ema_apply(float* w, float* e, int64_t n, float m, float c, int mode, hipStream_t s,
                      int max_blocks = kEmaMaxBlocks);

}  // namespace tdl
