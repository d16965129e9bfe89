#!/usr/bin/env python3
"""What the seeded dropout kernels cost against ``torch.nn.functional.dropout``, on one GPU.

    python scripts/bench_dropout.py [--repeats 9] [--inner 20] [--out FILE]

Forward + backward (``y = op(x); y.backward(dy)``) of

* ``tdl``    ops.dropout.dropout: one launch per direction, the Philox mask recomputed in the backward, the
             call counter advanced by the forward kernel;
* ``torch``  F.dropout (F.dropout2d over the NHWC tensor's channels for the broadcast case): the global
             generator, and a byte mask (or a noise tensor) saved for the backward

on the tensor of ``bench.py --variant dropout`` (64 x 1600), on one ResNet-scale NHWC tensor (256 x 56 x 56 x
256) and on that tensor with SpatialDropout2D's ``(N, 1, 1, C)`` mask, in f32 and bf16.  The two arms alternate
in one process after a warm-up; a sample is ``inner`` consecutive forward + backward pairs between two device
events, and the figure is the median of ``repeats`` samples.  GB/s counts what the algorithm needs: one read
and one write of the tensor per direction (4 passes); F.dropout moves a byte mask on top of that.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tensorflow_distributed_learning_amd.ops import dropout as D  # noqa: E402

KEY = D.stream_key(3, 0, 0)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner  # us per forward + backward


def alternate(cases, repeats, inner, warmup=3):
    for _ in range(warmup):
        for fn in cases.values():
            timed(fn, inner)
    samples = {k: [] for k in cases}
    for _ in range(repeats):
        for k, fn in cases.items():
            samples[k].append(timed(fn, inner))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def bench_case(shape, dtype, rate, spatial, repeats, inner):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(shape, generator=g).to(dtype).cuda().requires_grad_(True)
    dy = torch.randn(shape, generator=g).to(dtype).cuda()
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    ns = (shape[0], 1, 1, shape[3]) if spatial else None

    def tdl_path():
        D.dropout(x, rate, KEY, state=state, noise_shape=ns).backward(dy)
        x.grad = None

    def torch_path():
        if spatial:
            y = F.dropout2d(x.permute(0, 3, 1, 2), rate, training=True).permute(0, 2, 3, 1)
        else:
            y = F.dropout(x, rate, training=True)
        y.backward(dy)
        x.grad = None

    res = alternate({"tdl": tdl_path, "torch": torch_path}, repeats, inner)
    calls = int(state.cpu()[0])
    assert calls == (3 + repeats) * inner, f"the call counter reads {calls}"
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 7:
        ap.error("--repeats must be >= 7")
    from tensorflow_distributed_learning_amd.ops import hip

    C = hip()
    lines = [f"scripts/bench_dropout.py --repeats {args.repeats} --inner {args.inner}: us per forward + backward, median "
             f"(min .. max) of {args.repeats} samples of {args.inner} consecutive pairs, the arms alternating in one process",
             f"device: {torch.cuda.get_device_name(0)}; DROPOUT_WG_ELEMS = {C.DROPOUT_WG_ELEMS}, "
             f"DROPOUT_MAX_GRID = {C.DROPOUT_MAX_GRID}", ""]
    cases = [("bench variant, Dropout(0.25) on 64 x 1600", (64, 1600), 0.25, False),
             ("ResNet scale, Dropout(0.25) on 256 x 56 x 56 x 256", (256, 56, 56, 256), 0.25, False),
             ("ResNet scale, SpatialDropout2D(0.25) on 256 x 56 x 56 x 256", (256, 56, 56, 256), 0.25, True)]
    for name, shape, rate, spatial in cases:
        for dtype in (torch.float32, torch.bfloat16):
            res = bench_case(shape, dtype, rate, spatial, args.repeats, args.inner)
            n = 1
            for d in shape:
                n *= d
            nbytes = 4 * n * torch.empty((), dtype=dtype).element_size()
            lines.append(f"{name}, {str(dtype).replace('torch.', '')} ({nbytes / 4e6:.2f} MB per pass, 4 passes)")
            for k, (med, lo, hi) in res.items():
                lines.append(f"  {k:6s} {med:10.2f}  ({lo:.2f} .. {hi:.2f})   {nbytes / med / 1e3:8.1f} GB/s")
            lines.append(f"  tdl / torch = {res['tdl'][0] / res['torch'][0]:.2f}")
            lines.append("")
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
