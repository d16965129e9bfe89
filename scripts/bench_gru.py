#!/usr/bin/env python3
"""What the GRU scan kernels cost beside the torch formula and the library, on one GPU.

    python scripts/bench_gru.py [--repeats 7] [--inner 3] [--out FILE]

For B in {64, 256}, T in {32, 128}, U in {64, 128, 256}, f32 and bf16, over a projected input ``zx [B, T, 3U]`` (f32: U = 64 is LDS-resident, 128 and 256 streamed; bf16: 64 and 128 resident, 256 streamed):

* ``k_gru_fwd`` and ``k_gru_bwd`` of csrc/kernels/gru.hip through the bindings (the scan alone),
* ``gru_torch`` (ops/gru.py) forward on the GPU: the per-step torch ops, and
* ``torch.nn.GRU`` forward and forward + backward (the library; it also computes the input projection, D = U).

All arms of a shape alternate in one process after a warm-up; a sample is ``inner`` consecutive calls between two
device events, the figure is the median of ``repeats`` samples with (min .. max); us / step = kernel time / T.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner  # us per call


def alternate(cases, repeats, inner, warmup=2):
    for _ in range(warmup):
        for fn in cases.values():
            timed(fn, inner)
    samples = {k: [] for k in cases}
    for _ in range(repeats):
        for k, fn in cases.items():
            samples[k].append(timed(fn, inner))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def bench_shape(K, B, T, U, dtype, repeats, inner):
    from tensorflow_distributed_learning_amd.ops.gru import gru_torch

    g = torch.Generator().manual_seed(0)
    zx = torch.randn(B, T, 3 * U, generator=g).to(dtype).cuda()
    R = (torch.randn(U, 3 * U, generator=g) * U ** -0.5).to(dtype).cuda()
    b = torch.randn(3 * U, generator=g).cuda()
    dhs = torch.randn(B, T, U, generator=g).to(dtype).cuda()
    hs, _, saved = K.gru_forward(zx, R, b, None, False, True)
    lib = torch.nn.GRU(U, U, batch_first=True).to(device="cuda", dtype=dtype)
    x = torch.randn(B, T, U, generator=g).to(dtype).cuda().requires_grad_()

    def lib_step():
        lib.zero_grad(set_to_none=True)
        lib(x)[0].backward(dhs)

    def formula():
        with torch.no_grad():
            gru_torch(zx, R, b)

    def lib_fwd():
        with torch.no_grad():
            lib(x)

    cases = {"k_gru_fwd": lambda: K.gru_forward(zx, R, b, None, False, True),
             "k_gru_bwd": lambda: K.gru_backward(saved, hs, R, None, dhs, None, False, False),
             "gru_torch forward": formula, "torch.nn.GRU forward": lib_fwd, "torch.nn.GRU fwd + bwd": lib_step}
    res = alternate(cases, repeats, inner)
    return [f"  {k:24s} {med:10.1f} us  ({lo:.1f} .. {hi:.1f})  {med / T:8.2f} us / step" for k, (med, lo, hi) in res.items()]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 7:
        ap.error("--repeats must be >= 7")
    from tensorflow_distributed_learning_amd.ops import hip

    K = hip()
    lines = [f"scripts/bench_gru.py --repeats {args.repeats} --inner {args.inner}: us per call, median (min .. max) of "
             f"{args.repeats} samples of {args.inner} consecutive calls, the arms alternating in one process",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    for dtype in (torch.float32, torch.bfloat16):
        for B in (64, 256):
            for T in (32, 128):
                for U in (64, 128, 256):
                    p = K.gru_plan(B, T, U, dtype == torch.bfloat16)
                    lines.append(f"B {B} T {T} U {U} {str(dtype).replace('torch.', '')} (R "
                                 f"{'LDS-resident' if p['resident'] else 'streamed from L2'}, {p['workgroups']} workgroups, "
                                 f"LDS {p['lds_fwd']} / {p['lds_bwd']} B)")
                    lines += bench_shape(K, B, T, U, dtype, args.repeats, args.inner) + [""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
