#!/usr/bin/env python3
"""What the layer-normalisation kernels cost beside the library and a copy, on one GPU.

    python scripts/bench_layernorm.py [--repeats 9] [--inner 10] [--rows 16384 65536] [--out FILE]

For every shape ``[rows, C]``, C in {256, 768, 1024, 4096, 8192}, f32 and bf16: the forward launch (k_ln_fwd)
and the two backward launches (k_ln_bwd + k_ln_dgb) of csrc/kernels/layernorm.hip through the bindings, beside

* ``F.layer_norm`` forward and its backward (``torch.ops.aten.native_layer_norm_backward`` on the saved mean /
  rstd, all three gradients), and
* a plain device copy of the same tensor (``y.copy_(x)``: one read and one write).

All arms of a shape alternate in one process after a warm-up; a sample is ``inner`` consecutive calls between
two device events, the figure is the median of ``repeats`` samples with (min .. max).  TB/s counts what the
call must move: forward and copy 2 passes over the tensor, backward 3.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTHS = [256, 768, 1024, 4096, 8192]
EPS = 1e-3


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


def bench_shape(K, rows, C, dtype, repeats, inner):
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(rows, C, generator=g) * 2 + 0.5).to(dtype).cuda()
    dy = torch.randn(rows, C, generator=g).to(dtype).cuda()
    # (the library wants the parameters in the data's dtype; the kernels take them in f32)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), torch.randn(C, generator=g).cuda()
    gl, bl = gamma.to(dtype), beta.to(dtype)
    _, st = K.ln_forward(x, gamma, beta, EPS)
    _, mean, rstd = torch.ops.aten.native_layer_norm(x, [C], gl, bl, EPS)
    out = torch.empty_like(x)
    cases = {
        "k_ln_fwd": lambda: K.ln_forward(x, gamma, beta, EPS),
        "F.layer_norm": lambda: F.layer_norm(x, (C,), gl, bl, EPS),
        "k_ln_bwd + k_ln_dgb": lambda: K.ln_backward(dy, x, gamma, st),
        "library backward": lambda: torch.ops.aten.native_layer_norm_backward(dy, x, [C], mean, rstd, gl, bl,
                                                                              [True, True, True]),
        "device copy": lambda: out.copy_(x),
    }
    passes = {"k_ln_fwd": 2, "F.layer_norm": 2, "k_ln_bwd + k_ln_dgb": 3, "library backward": 3, "device copy": 2}
    res = alternate(cases, repeats, inner)
    nbytes = x.numel() * x.element_size()
    return nbytes, [f"  {k:22s} {med:9.2f} us  ({lo:.2f} .. {hi:.2f})  {passes[k] * nbytes / med / 1e6:8.2f} TB/s"
                    for k, (med, lo, hi) in res.items()]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--rows", type=int, nargs="+", default=[16384, 65536])
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 7:
        ap.error("--repeats must be >= 7")
    from tensorflow_distributed_learning_amd.ops import hip

    K = hip()
    lines = [f"scripts/bench_layernorm.py --repeats {args.repeats} --inner {args.inner}: us per call, median (min .. max) "
             f"of {args.repeats} samples of {args.inner} consecutive calls, the arms alternating in one process",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    for dtype in (torch.float32, torch.bfloat16):
        for rows in args.rows:
            for C in WIDTHS:
                p = K.ln_plan(rows, C, dtype == torch.bfloat16)
                nbytes, ls = bench_shape(K, rows, C, dtype, args.repeats, args.inner)
                lines.append(f"{rows} x {C} {str(dtype).replace('torch.', '')} ({nbytes / 1e6:.2f} MB; forward plan "
                             f"{p['plan']}, {p['L']} lanes per row; backward {p['L_bwd']} lanes per row, "
                             f"{p['rows_wg']} rows per workgroup, {p['blocks']} workgroups)")
                lines += ls + [""]
                torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
