#!/usr/bin/env python3
"""What the layer-wise optimizers (LARS, LAMB) cost per step, on one GPU.

    python scripts/bench_layerwise.py [--repeats 9] [--inner 20] [--out profiles/layerwise_cost.txt]

On the reference CNN's layout (8 variables) and on ResNet-50's (214 trainable variables, batch-norm scales and
offsets included), one optimizer step each of

* ``lars``          the three launches of csrc/kernels/layerwise.hip (k_layer_sums_lars, k_layer_ratio,
                    k_lars_apply) through ``LARS.device_update``;
* ``lamb``          the same for LAMB (k_layer_sums_lamb, k_layer_ratio, k_lamb_apply);
* ``sgd_momentum``  ``_C.sgd_momentum`` over the same slab (one launch): what LARS adds its norms to;
* ``adam``          ``_C.adam`` over the same slab (one launch): what LAMB adds its norms to;

each of the layer-wise launches alone, and the three launches at every candidate chunk size (elements per
workgroup) behind kLayerChunk.  The cases alternate in one process after a warm-up; a sample is
``inner`` consecutive steps between two device events, and the figure is the median of ``repeats`` samples.
Beside them the byte floors: LAMB moves 24 B + 16 B = 40 B per element (Adam 28 B), LARS 8 B + 20 B = 28 B
(momentum SGD 20 B), at the streaming rate of the BN passes (README: 5.2-6.2 TB/s).
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

CANDIDATES = (2048, 4096, 8192)  # chunk sizes (elements per workgroup) behind kLayerChunk
STREAM_TBS = (5.2, 6.2)
BYTES = {"lars": 28, "lamb": 40, "sgd_momentum": 20, "adam": 28}


def layouts():
    """{name: SlabLayout} of the two models' trainable variables."""
    from tensorflow_distributed_learning_amd.models.mnist_cnn import build_mnist_cnn

    out = {}
    with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
        m = build_mnist_cnn()
        m._ensure_slabs()
        out["reference CNN"] = m._layout
        del m
        r = tdl.keras.applications.ResNet50(weights=None, classes=1000, classifier_activation=None)
        r._ensure_slabs()
        out["ResNet-50"] = r._layout
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


def bench_layout(layout, repeats, inner):
    O = tdl.keras.optimizers
    C = hip()
    n = layout.total
    gen = torch.Generator().manual_seed(0)

    def slab(scale=1.0):
        return (torch.randn(n, generator=gen) * scale).cuda()

    kw = dict(weight_decay_rate=1e-4, exclude_from_weight_decay=["bias", "gamma", "beta"])
    lars, lamb = O.LARS(1e-3, **kw), O.LAMB(1e-4, **kw)
    ops = {}
    for name, opt in (("lars", lars), ("lamb", lamb)):
        opt.set_layout(layout)
        opt.build(n, torch.device("cuda", 0))
        ops[name] = (opt, slab(), slab(0.1))
    Ws, Gs, Vs = slab(), slab(0.1), torch.zeros(n, device="cuda")
    Wa, Ga, Ma, Va = slab(), slab(0.1), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    lr = torch.full((1,), 1e-4, device="cuda")
    t0 = torch.zeros(1, device="cuda")

    def step(name):
        opt, W, G = ops[name]
        return lambda: opt.device_update(W, G)

    cases = {"lars": step("lars"), "lamb": step("lamb"),
             "sgd_momentum": lambda: C.sgd_momentum(Ws, Gs, Vs, lr, 0.9, False),
             "adam": lambda: C.adam(Wa, Ga, Ma, Va, None, lr, t0, 0, 0.9, 0.999, 1e-7)}
    res = alternate(cases, repeats, inner)
    o, W, G = ops["lars"]
    T, P, Rt, Nm = o._tables, o._layer_partials, o._layer_ratio, o._layer_norms
    parts = {"  k_layer_sums_lars": lambda: C.lars_sums(T, W, G, P),
             "  k_layer_ratio": lambda: C.lars_ratio(T, P, Rt, Nm, 0.001, 0.0),
             "  k_lars_apply": lambda: C.lars_update(T, W, G, o._slots["momentum"], Rt, o.lr_dev, 0.9, False)}
    o2, W2, G2 = ops["lamb"]
    T2, P2, R2, N2 = o2._tables, o2._layer_partials, o2._layer_ratio, o2._layer_norms
    hp = (o2.t_dev, 0, 0.9, 0.999, 1e-6)
    parts["  k_layer_sums_lamb"] = lambda: C.lamb_sums(T2, W2, G2, o2._slots["m"], o2._slots["v"], P2, *hp)
    parts["  k_lamb_apply"] = lambda: C.lamb_update(T2, W2, o2._slots["m"], o2._slots["v"], R2, o2.lr_dev, *hp)
    res.update(alternate(parts, repeats, inner))
    # the candidates behind kLayerChunk: the three launches at each chunk size, on the same operands
    offs, sizes, _ = layout.layer_spans()
    cand = {}
    for ch in CANDIDATES:
        Tc = C.layer_tables_chunk(offs, sizes, n, o._wd, o._adapt, ch)
        Pc = torch.zeros(max(2, 2 * Tc.C), dtype=torch.float64, device="cuda")

        def lars_ch(Tc=Tc, Pc=Pc):
            C.lars_sums(Tc, W, G, Pc)
            C.lars_ratio(Tc, Pc, Rt, Nm, 0.001, 0.0)
            C.lars_update(Tc, W, G, o._slots["momentum"], Rt, o.lr_dev, 0.9, False)

        def lamb_ch(Tc=Tc, Pc=Pc):
            C.lamb_sums(Tc, W2, G2, o2._slots["m"], o2._slots["v"], Pc, *hp)
            C.lamb_ratio(Tc, Pc, R2, N2)
            C.lamb_update(Tc, W2, o2._slots["m"], o2._slots["v"], R2, o2.lr_dev, *hp)

        cand[f"lars CH={ch} ({Tc.C} chunks)"] = lars_ch
        cand[f"lamb CH={ch} ({Tc.C} chunks)"] = lamb_ch
    res.update(alternate(cand, repeats, inner))
    return res, int(T.V), int(T.C)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 7:
        ap.error("--repeats must be >= 7")
    lines = [f"scripts/bench_layerwise.py --repeats {args.repeats} --inner {args.inner}: us per optimizer step, median "
             f"(min .. max) of {args.repeats} samples of {args.inner} consecutive steps, the cases alternating in one "
             f"process", f"device: {torch.cuda.get_device_name(0)}; LAYER_CHUNK = {hip().LAYER_CHUNK}", ""]
    for name, layout in layouts().items():
        res, V, C = bench_layout(layout, args.repeats, args.inner)
        n, p = layout.total, layout.num_params
        lines.append(f"{name}: {V} variables, {p} parameters in a slab of {n} floats ({4 * n / 1e6:.2f} MB), {C} chunks")
        for k, (med, lo, hi) in res.items():
            floor = ""
            if k in BYTES:
                f = [BYTES[k] * p / (t * 1e12) * 1e6 for t in STREAM_TBS]
                floor = f"   floor {BYTES[k]} B/element at {STREAM_TBS[1]}-{STREAM_TBS[0]} TB/s = {f[1]:.2f}-{f[0]:.2f}"
            lines.append(f"  {k:30s} {med:9.2f}  ({lo:.2f} .. {hi:.2f}){floor}")
        lines.append(f"  lars / sgd_momentum = {res['lars'][0] / res['sgd_momentum'][0]:.2f}x, lamb / adam = "
                     f"{res['lamb'][0] / res['adam'][0]:.2f}x")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
