#!/usr/bin/env python3
"""Times the fused attention kernels (ops/attention.py) against F.scaled_dot_product_attention and the unfused torch
formula: forward and forward + backward, f32 and bf16, and with attention dropout (rate 0.1): inside the kernels
against the formula with F.dropout.  Device time from HIP events around a window of back-to-back
calls sized to `--window` seconds from a first estimate (a short window measures the scheduler); the three paths are
timed in turn within each of `--reps` rounds, so drift hits them alike.  Prints one JSON line per (shape, dtype,
path): the median and the [min, max] of the rounds, ms per call.

    python scripts/bench_attention.py [--window 0.3] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensorflow_distributed_learning_amd.ops import attention as A  # noqa: E402

SHAPES = [(64, 8, 128, 128, 64, False), (8, 12, 512, 512, 64, False), (4, 16, 2048, 2048, 128, True)]
RATE, KEY = 0.1, (0x243F6A88, 0x85A308D3)


def _window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _time_all(fns, window, reps):
    """{name: (median, min, max)} ms per call; every round times each function once, in turn."""
    iters = {}
    for name, fn in fns.items():
        _window(fn, 3)  # warm-up: code objects, the library's algorithm choice
        iters[name] = max(5, int(window * 1e3 / _window(fn, 5)))
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            times[name].append(_window(fn, iters[name]))
    return {n: (statistics.median(t), min(t), max(t)) for n, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated paths to time (default: all)")
    args = ap.parse_args()
    state = torch.zeros(2, dtype=torch.int64, device="cuda")  # the dropout call counter [calls, arrivals]
    for B, H, T, S, D, causal in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            g = torch.Generator(device="cuda").manual_seed(0)
            q, k, v = (torch.randn(B, n, H, D, device="cuda", dtype=dtype, generator=g).requires_grad_() for n in (T, S, S))
            do = torch.randn(B, T, H, D, device="cuda", dtype=dtype, generator=g)
            paths = {
                "kernels": lambda: A.sdpa(q, k, v, None, causal),
                "library": lambda: F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                                                                  is_causal=causal).transpose(1, 2),
                "formula": lambda: A.sdpa_torch(q, k, v, None, causal),
                # attention dropout at RATE: inside the kernels (seeded Philox), and the formula with F.dropout
                "kernels_dropout": lambda: A.sdpa(q, k, v, None, causal, rate=RATE, key=KEY, state=state),
                "formula_dropout": lambda: A.sdpa_torch(q, k, v, None, causal, dropout=lambda p: F.dropout(p, RATE, True)),
            }
            if args.only:
                paths = {n: f for n, f in paths.items() if n in args.only.split(",")}

            def both(fn):
                def run():
                    fn().backward(do)
                    q.grad = k.grad = v.grad = None
                return run

            with torch.no_grad():
                fwd = _time_all(paths, args.window, args.reps)
            bwd = _time_all({n: both(f) for n, f in paths.items()}, args.window, args.reps)
            for name in paths:
                r4 = lambda t: [round(x, 4) for x in t]  # noqa: E731
                print(json.dumps({"shape": [B, H, T, S, D], "causal": causal, "dtype": str(dtype).replace("torch.", ""),
                                  "path": name, "fwd_ms": r4(fwd[name]), "fwd_bwd_ms": r4(bwd[name])}), flush=True)


if __name__ == "__main__":
    main()
