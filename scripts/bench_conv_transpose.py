#!/usr/bin/env python3
"""What the transposed-convolution kernels cost beside the library path and the generic input gradient, on one GPU.

    python scripts/bench_conv_transpose.py [--batch 64] [--repeats 7] [--inner 10] [--out FILE]

Shapes: decoder layers, 4x4 / stride 2 'same' at 8x8x512->256, 16x16x256->128, 32x32x128->64 and 64x64x64->32, and
3x3 / stride 2 'same' at 28x28x128->64, f32 and bf16.  Per shape ``convt_forward`` / ``convt_dgrad`` / ``convt_wgrad``
(all its launches) of csrc/kernels/conv_transpose.hip beside (b) ``F.conv_transpose2d`` over the permuted view with
the kernel cast to the data dtype -- its forward, and its input and weight gradients through autograd (one figure,
to be set beside dgrad + wgrad) -- and, f32 forward only, (c) ``ops.conv_f32.dgrad`` on the same problem: the
generic input-gradient kernel, which walks every tap per output pixel and predicates the strided misses away (for a
kernel of more than 65536 elements -- every shape here but 64x64x64->32 -- that call also copies the weight into
its [R][S][K][C] order, inside the timed region: what a caller of it pays).  All
arms of a shape alternate in one process after a warm-up; a sample is ``inner`` consecutive calls between two
device events, the figure is the median (min .. max) of ``repeats`` samples.  MFMA counts come from the plan.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (H = W, C, F, k)
SHAPES = [(8, 512, 256, 4), (16, 256, 128, 4), (32, 128, 64, 4), (64, 64, 32, 4), (28, 128, 64, 3)]
STRIDE = 2


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


def bench_shape(C, batch, hw, ch, f, k, dtype, repeats, inner):
    from tensorflow_distributed_learning_amd.ops import conv_f32
    from tensorflow_distributed_learning_amd.ops import conv_transpose as CT

    g = torch.Generator().manual_seed(0)
    x = torch.randn(batch, hw, hw, ch, generator=g).to(dtype).cuda()
    w = (torch.randn(k, k, f, ch, generator=g) / (k * k * ch / 4) ** 0.5).cuda()
    b = torch.randn(f, generator=g).cuda()
    o, lead = CT.out_size(hw, k, STRIDE, 1, "same")
    dy = torch.randn(batch, o, o, f, generator=g).to(dtype).cuda()
    geo = [STRIDE, STRIDE, 1, 1, lead, lead]
    cases = {"convt forward": lambda: C.convt_forward(x, w, b, geo, o, o),
             "convt dgrad": lambda: C.convt_dgrad(dy, w, hw, hw, geo),
             "convt wgrad (3 launches)": lambda: C.convt_wgrad(x, dy, k, k, geo, dbias=torch.empty_like(b))}

    def lib(xx, ww, bb):
        return CT.conv2d_transpose_torch(xx, ww, bb, (STRIDE, STRIDE), "same")

    def lib_fwd():
        with torch.no_grad():
            lib(x, w, b)

    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    yl = lib(xr, wr, b)
    cases["library forward"] = lib_fwd
    cases["library backward (dx, dW)"] = lambda: torch.autograd.grad(yl, (xr, wr), dy, retain_graph=True)
    if dtype == torch.float32:
        cases["generic dgrad as forward"] = lambda: conv_f32.dgrad(x, w, (o, o), (STRIDE, STRIDE), (lead, 0, lead, 0))
    y = C.convt_forward(x, w, b, geo, o, o).float()
    agree = float((y - yl.detach().float()).abs().max() / yl.detach().float().abs().max())
    res = alternate(cases, repeats, inner)
    lines = [f"  {name:28s} {med:9.2f} us  ({lo:.2f} .. {hi:.2f})" for name, (med, lo, hi) in res.items()]
    r = {n: v[0] for n, v in res.items()}
    tail = (f", generic dgrad / kernels forward {r['generic dgrad as forward'] / r['convt forward']:.2f}x"
            if dtype == torch.float32 else "")
    lines.append(f"  library / kernels: forward {r['library forward'] / r['convt forward']:.2f}x, backward "
                 f"{r['library backward (dx, dW)'] / (r['convt dgrad'] + r['convt wgrad (3 launches)']):.2f}x{tail}; "
                 f"largest forward difference / largest output {agree:.1e}")
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from tensorflow_distributed_learning_amd.ops import conv as CONV
    from tensorflow_distributed_learning_amd.ops import conv_transpose as CT
    from tensorflow_distributed_learning_amd.ops import hip

    C = hip()
    out = open(args.out, "w") if args.out else None

    def emit(*ls):
        for s in ls:
            print(s, flush=True)
            if out:
                out.write(s + "\n")
                out.flush()

    emit(f"scripts/bench_conv_transpose.py --batch {args.batch} --repeats {args.repeats} --inner {args.inner}: us per "
         f"call, median (min .. max) of {args.repeats} samples of {args.inner} consecutive calls, the arms alternating "
         f"in one process", f"device: {torch.cuda.get_device_name(0)}", "")
    for dt in (torch.float32, torch.bfloat16):
        for hw, ch, f, k in SHAPES:
            o, lead = CT.out_size(hw, k, STRIDE, 1, "same")
            p = C.convt_plan([args.batch, hw, hw, ch], f, k, k, o, o, [STRIDE, STRIDE, 1, 1, lead, lead])
            generic = (args.batch * o * o + 15) // 16 * (k * k * ch // 4) * ((f + 15) // 16)  # every tap per output pixel
            emit(f"{args.batch} x {hw} x {hw} x {ch} -> {o} x {o} x {f} {str(dt).replace('torch.', '')}, {k}x{k} stride 2 "
                 f"same (plan: phase taps {p['phase_taps']}, {p['fwd_pixels_per_tile']} pixels x "
                 f"{min(4, p['fwd_tiles'])} column tiles, {p['fwd_kchunks']} k-chunk(s), {p['wgrad_splits']} wgrad splits; "
                 f"MFMAs: forward {p['fwd_mfma']} = {p['fwd_mfma'] / generic:.3f} of the generic dgrad's {generic}, "
                 f"dgrad {p['dgrad_mfma']}, wgrad {p['wgrad_mfma']})",
                 *bench_shape(C, args.batch, hw, ch, f, k, dt, args.repeats, args.inner), "")
            torch.cuda.empty_cache()
    CONV.reset_library_calls()
    if out:
        out.close()


if __name__ == "__main__":
    main()
