#!/usr/bin/env python3
"""What the depthwise-convolution kernels cost, launch by launch, on one GPU.

    python scripts/bench_depthwise.py [--repeats 7] [--inner 5] [--out FILE] [--quick]

For every shape: ``dw_forward``, ``dw_dgrad`` and ``dw_wgrad`` (both launches) of csrc/kernels/depthwise.hip,
each timed alone, beside

* a plain device copy that reads and writes as many bytes as the forward / the input gradient must move (x and
  y once each): their floor,
* the library path on the same shape (``ops.depthwise.depthwise_conv2d_torch``: F.conv2d(groups=C) over the
  permuted view): its forward, and its backward through autograd (input and weight gradient together, to be
  set beside dgrad + wgrad), and
* ``Conv2D(groups=C)``, the only way to write the layer before these kernels, as that layer runs it: the kernel
  cast to the data dtype and F.conv2d(groups=C) in that dtype (the library path above computes bf16 data in
  f32): forward, and backward through autograd.

Shapes: MobileNet-like maps at batch 256 -- 112x112x32, 56x56x128, 28x28x256, 14x14x512, 7x7x1024 -- with a
3x3 kernel at stride 1 and stride 2, 'same' padding, bf16 and f32; then 5x5 and 7x7 at 14x14x512 (ConvNeXt).
All arms of a shape alternate in one process after a warm-up; a sample is ``inner`` consecutive calls between
two device events, the figure is the median of ``repeats`` samples.  TB/s counts x and y once each (forward,
dgrad) and x and dy once each (wgrad).
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MAPS = [(112, 32), (56, 128), (28, 256), (14, 512), (7, 1024)]
BATCH = 256


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


def bench_shape(C, hw, ch, k, stride, dtype, repeats, inner):
    import torch.nn.functional as F

    from tensorflow_distributed_learning_amd.keras.layers import _same_pads
    from tensorflow_distributed_learning_amd.ops import depthwise as DW

    g = torch.Generator().manual_seed(0)
    x = torch.randn(BATCH, hw, hw, ch, generator=g).to(dtype).cuda()
    w = torch.randn(k, k, ch, 1, generator=g).cuda()
    b = torch.randn(ch, generator=g).cuda()
    p = _same_pads(hw, k, stride)
    pads, o = (p[0], p[1], p[0], p[1]), -(-hw // stride)
    geo = [stride, stride, 1, 1, p[0], p[0]]
    dy = torch.randn(BATCH, o, o, ch, generator=g).to(dtype).cuda()
    part = C.dw_wgrad(x, dy, k, k, geo)[2]
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    cases = {"dw forward": lambda: C.dw_forward(x, w, b, geo, o, o, out=y),
             "dw dgrad": lambda: C.dw_dgrad(dy, w, hw, hw, geo, out=dx),
             "dw wgrad (2 launches)": lambda: C.dw_wgrad(x, dy, k, k, geo, ws=[part])}
    n = (x.numel() + dy.numel()) // 2
    src, dst = torch.empty(n, dtype=dtype, device="cuda").normal_(), torch.empty(n, dtype=dtype, device="cuda")
    cases["device copy of the same bytes"] = lambda: dst.copy_(src)
    xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()

    def lib_fwd():
        with torch.no_grad():
            DW.depthwise_conv2d_torch(x, w, b, (stride, stride), pads)

    cases["library forward"] = lib_fwd
    yl = DW.depthwise_conv2d_torch(xr, wr, br, (stride, stride), pads)
    cases["library backward (dx, dW, db)"] = lambda: torch.autograd.grad(yl, (xr, wr, br), dy, retain_graph=True)
    # Conv2D(groups=C)'s own path (keras/layers.py, its last branch): the kernel [kh,kw,1,C] cast to the data dtype,
    # F.pad for asymmetric 'same' padding, F.conv2d(groups=C) over the permuted view
    def conv_groups(xx, ww, bb):
        h = xx.permute(0, 3, 1, 2)
        if p[0] != p[1]:
            h, pad = F.pad(h, (p[0], p[1], p[0], p[1])), 0
        else:
            pad = p[0]
        wk = ww.to(xx.dtype).reshape(k, k, 1, ch).permute(3, 2, 0, 1)
        return F.conv2d(h, wk, bb.to(xx.dtype), stride=stride, padding=pad, groups=ch).permute(0, 2, 3, 1)

    xc, wc, bc = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    yc = conv_groups(xc, wc, bc)

    def conv_fwd():
        with torch.no_grad():
            conv_groups(x, w, b)

    cases["Conv2D(groups=C) forward"] = conv_fwd
    cases["Conv2D(groups=C) backward"] = lambda: torch.autograd.grad(yc, (xc, wc, bc), dy, retain_graph=True)
    res = alternate(cases, repeats, inner)
    nbytes = (x.numel() + dy.numel()) * x.element_size()
    lines = []
    for name, (med, lo, hi) in res.items():
        lines.append(f"  {name:32s} {med:9.2f} us  ({lo:.2f} .. {hi:.2f})  {nbytes / med / 1e6:7.2f} TB/s")
    return nbytes, lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="bf16 only, three of the maps")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 7:
        ap.error("--repeats must be >= 7")
    from tensorflow_distributed_learning_amd.ops import conv as CONV
    from tensorflow_distributed_learning_amd.ops import hip

    C = hip()
    out = open(args.out, "w") if args.out else None

    def emit(*ls):
        for s in ls:
            print(s, flush=True)
            if out:
                out.write(s + "\n")
                out.flush()

    emit(f"scripts/bench_depthwise.py --repeats {args.repeats} --inner {args.inner}: us per call, median (min .. max) of "
         f"{args.repeats} samples of {args.inner} consecutive calls, the arms alternating in one process",
         f"device: {torch.cuda.get_device_name(0)}", "")
    dtypes = [torch.bfloat16] if args.quick else [torch.bfloat16, torch.float32]
    maps = MAPS[1:4] if args.quick else MAPS
    shapes = [(hw, ch, 3, s, dt) for dt in dtypes for hw, ch in maps for s in (1, 2)]
    shapes += [(14, 512, k, 1, dt) for dt in dtypes for k in (5, 7)]
    for hw, ch, k, s, dt in shapes:
        o = -(-hw // s)
        p = (k - 1) // 2 if s == 1 else max((o - 1) * s + k - hw, 0) // 2
        plan = C.dw_plan([BATCH, hw, hw, ch], k, k, 1, o, o, [s, s, 1, 1, p, p], dt == torch.bfloat16)
        nbytes, ls = bench_shape(C, hw, ch, k, s, dt, args.repeats, args.inner)
        emit(f"{BATCH} x {hw} x {hw} x {ch} {str(dt).replace('torch.', '')}, {k}x{k} stride {s} same "
             f"({nbytes / 1e6:.2f} MB of x and y; plan: {plan[2]} columns of {plan[0]}, tile {plan[4]} x {plan[5]}, "
             f"halo {plan[6]} x {plan[7]}, {plan[8]} tap slots)", *ls, "")
        torch.cuda.empty_cache()
    emit(f"library convolutions counted: {sum(CONV.library_calls().values())}")
    if out:
        out.close()


if __name__ == "__main__":
    main()
