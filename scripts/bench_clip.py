#!/usr/bin/env python3
"""What gradient clipping costs in the optimizer update, on one GPU.

    python scripts/bench_clip.py [--repeats 9] [--inner 20] [--out profiles/clip_cost.txt]

Three ways to apply one Adam update to a flat slab, at the reference CNN's slab size and at ResNet-50's:

* ``clipped``   clip_norm (k_clip_partials + k_clip_scale) + k_adam with the clip operands: this framework's
                clipped update;
* ``unclipped`` k_adam alone;
* ``torch``     the parent commit's clipped update: ``Optimizer._clip`` (clamp_, vector_norm, clamp, mul_) and
                Adam's torch formulas (``_update``).

The three alternate in one process after a warm-up; a sample is ``inner`` consecutive updates between two
device events, and the figure is the median of ``repeats`` samples.  The floor of the added work is one more
read of G: 4 n bytes at the streaming rate of the BN passes (README: 5.2-6.2 TB/s).  The same is done for
clip_norm alone at every candidate chunk size (elements per partial sum) behind kClipChunk.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import tensorflow_distributed_learning_amd as tdl  # noqa: E402
from tensorflow_distributed_learning_amd.ops import hip  # noqa: E402

CANDIDATES = (2048, 4096, 8192, 16384)
STREAM_TBS = (5.2, 6.2)


def slab_sizes():
    """{name: floats} of the two models' parameter slabs (SlabLayout.total, alignment padding included)."""
    from tensorflow_distributed_learning_amd.models.mnist_cnn import build_mnist_cnn

    out = {}
    with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
        m = build_mnist_cnn()
        m._ensure_slabs()
        out["reference CNN"] = int(m._layout.total)
        del m
        r = tdl.keras.applications.ResNet50(weights=None, classes=1000, classifier_activation=None)
        r._ensure_slabs()
        out["ResNet-50"] = int(r._layout.total)
        del r
    tdl.keras.backend.clear_session()
    torch.cuda.empty_cache()
    return out


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner  # us per call


def alternate(cases, repeats, inner, warmup=3):
    for _ in range(warmup):
        for fn in cases.values():
            timed(fn, inner)
    samples = {k: [] for k in cases}
    for _ in range(repeats):
        for k, fn in cases.items():
            samples[k].append(timed(fn, inner))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def bench_size(n, repeats, inner):
    O = tdl.keras.optimizers
    g = torch.Generator().manual_seed(0)
    G0 = (torch.randn(n, generator=g) * 0.1).cuda()
    clip = dict(global_clipnorm=1.0, clipvalue=0.25)

    def make(**kw):
        opt = O.Adam(1e-3, **kw)
        W, G = torch.randn(n, generator=g).cuda(), G0.clone()
        opt.build(n, W.device)
        return opt, W, G

    oc, Wc, Gc = make(**clip)
    ou, Wu, Gu = make()
    ot, Wt, Gt = make(**clip)

    def clipped():
        assert oc.device_update(Wc, Gc)

    def unclipped():
        assert ou.device_update(Wu, Gu)

    def torch_path():  # Optimizer.apply_flat of the parent commit for a clipped Adam
        Gt.copy_(G0)  # (_clip rewrites G; the copy is timed separately and subtracted below)
        ot._clip(Gt)
        ot._update(Wt, Gt)

    def copy_only():
        Gt.copy_(G0)

    res = alternate({"clipped": clipped, "unclipped": unclipped, "torch": torch_path, "copy": copy_only}, repeats, inner)
    C = hip()
    out = torch.zeros(4, device="cuda")
    cand = {}
    for ch in CANDIDATES:
        part = torch.zeros(max(1, (n + ch - 1) // ch), dtype=torch.float64, device="cuda")
        cand[f"clip_norm CH={ch}"] = (lambda ch=ch, part=part: C.clip_norm_chunk(Gc, part, out, 1.0, 0.25, ch))
    res.update(alternate(cand, repeats, inner))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 7:
        ap.error("--repeats must be >= 7")
    lines = [f"scripts/bench_clip.py --repeats {args.repeats} --inner {args.inner}: us per update, median (min .. max) "
             f"of {args.repeats} samples of {args.inner} consecutive updates, the cases alternating in one process",
             f"device: {torch.cuda.get_device_name(0)}; CLIP_CHUNK = {hip().CLIP_CHUNK}", ""]
    for name, n in slab_sizes().items():
        res = bench_size(n, args.repeats, args.inner)
        floor = [4.0 * n / (t * 1e12) * 1e6 for t in STREAM_TBS]
        lines.append(f"{name}: slab of {n} floats ({4 * n / 1e6:.2f} MB); one more read of G at "
                     f"{STREAM_TBS[1]}-{STREAM_TBS[0]} TB/s = {floor[1]:.2f}-{floor[0]:.2f} us")
        for k, (med, lo, hi) in res.items():
            lines.append(f"  {k:22s} {med:9.2f}  ({lo:.2f} .. {hi:.2f})")
        t = res["torch"][0] - res["copy"][0]
        c, u = res["clipped"][0], res["unclipped"][0]
        lines.append(f"  clipped - unclipped = {c - u:.2f} us; parent's torch path (copy subtracted) = {t:.2f} us: "
                     f"the kernels take {c / t:.2f}x its time")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
