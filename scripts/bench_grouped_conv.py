#!/usr/bin/env python3
"""What the grouped-convolution kernels cost beside the library path, on one GPU.

    python scripts/bench_grouped_conv.py [--batch 32] [--repeats 7] [--inner 5] [--out FILE]

Shapes: the four 3x3 convolutions of ResNeXt-50 32x4d (56x56x128, 28x28x256, 14x14x512, 7x7x1024, 32 groups,
stride 1, 'same'), f32 and bf16.  Per shape ``gconv_forward`` / ``gconv_dgrad`` / ``gconv_wgrad`` (both launches)
of csrc/kernels/grouped_conv.hip beside what Conv2D(groups=32) ran before them: ``F.conv2d(groups=)`` over the
permuted view with the kernel cast to the data dtype -- its forward, and its input and weight gradients through
autograd (one figure, to be set beside dgrad + wgrad).  All arms of a shape alternate in one process after a
warm-up; a sample is ``inner`` consecutive calls between two device events, the figure is the median (min .. max)
of ``repeats`` samples.  The MFMA / useful MAC ratio of each pass is computed from the plan.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MAPS = [(56, 128), (28, 256), (14, 512), (7, 1024)]
GROUPS = 32


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


def bench_shape(C, batch, hw, ch, dtype, repeats, inner):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(batch, hw, hw, ch, generator=g).to(dtype).cuda()
    w = (torch.randn(3, 3, ch // GROUPS, ch, generator=g) / (9 * ch // GROUPS) ** 0.5).cuda()
    b = torch.randn(ch, generator=g).cuda()
    dy = torch.randn(batch, hw, hw, ch, generator=g).to(dtype).cuda()
    geo = [1, 1, 1, 1, 1, 1]
    cases = {"gconv forward": lambda: C.gconv_forward(x, w, b, GROUPS, geo, hw, hw),
             "gconv dgrad": lambda: C.gconv_dgrad(dy, w, GROUPS, hw, hw, geo),
             "gconv wgrad (2 launches)": lambda: C.gconv_wgrad(x, dy, 3, 3, GROUPS, geo)}

    def lib(xx, ww, bb):
        return F.conv2d(xx.permute(0, 3, 1, 2), ww.to(xx.dtype).permute(3, 2, 0, 1), bb.to(xx.dtype), padding=1,
                        groups=GROUPS).permute(0, 2, 3, 1)

    def lib_fwd():
        with torch.no_grad():
            lib(x, w, b)

    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    yl = lib(xr, wr, b)
    cases["library forward"] = lib_fwd
    cases["library backward (dx, dW)"] = lambda: torch.autograd.grad(yl, (xr, wr), dy, retain_graph=True)
    y = C.gconv_forward(x, w, b, GROUPS, geo, hw, hw).float()
    agree = float((y - yl.detach().float()).abs().max() / yl.detach().float().abs().max())
    res = alternate(cases, repeats, inner)
    lines = [f"  {name:28s} {med:9.2f} us  ({lo:.2f} .. {hi:.2f})" for name, (med, lo, hi) in res.items()]
    r = {k: v[0] for k, v in res.items()}
    lines.append(f"  library / kernels: forward {r['library forward'] / r['gconv forward']:.2f}x, backward "
                 f"{r['library backward (dx, dW)'] / (r['gconv dgrad'] + r['gconv wgrad (2 launches)']):.2f}x; "
                 f"largest forward difference / largest output {agree:.1e}")
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from tensorflow_distributed_learning_amd.ops import hip

    C = hip()
    out = open(args.out, "w") if args.out else None

    def emit(*ls):
        for s in ls:
            print(s, flush=True)
            if out:
                out.write(s + "\n")
                out.flush()

    emit(f"scripts/bench_grouped_conv.py --batch {args.batch} --repeats {args.repeats} --inner {args.inner}: us per "
         f"call, median (min .. max) of {args.repeats} samples of {args.inner} consecutive calls, the arms alternating "
         f"in one process", f"device: {torch.cuda.get_device_name(0)}", "")
    for dt in (torch.float32, torch.bfloat16):
        for hw, ch in MAPS:
            p = C.gconv_plan([args.batch, hw, hw, ch], ch, GROUPS, 3, 3, hw, hw, [1, 1, 1, 1, 1, 1])
            useful = args.batch * hw * hw * 9 * (ch // GROUPS) * ch  # MACs of each of the three passes
            emit(f"{args.batch} x {hw} x {hw} x {ch} {str(dt).replace('torch.', '')}, 3x3 stride 1 same, {GROUPS} groups "
                 f"(plan: {p['fwd_pixels_per_tile']} pixels x {min(4, p['fwd_tiles'])} column tiles of "
                 f"{p['fwd_groups_per_tile']} groups, {p['fwd_kchunks']} k-chunk(s), {p['wgrad_splits']} wgrad splits; "
                 f"MFMA / useful MACs: forward {p['fwd_mfma'] * 1024 / useful:.2f}, dgrad "
                 f"{p['dgrad_mfma'] * 1024 / useful:.2f}, wgrad {p['wgrad_mfma'] * 1024 / useful:.2f})",
                 *bench_shape(C, args.batch, hw, ch, dt, args.repeats, args.inner), "")
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
