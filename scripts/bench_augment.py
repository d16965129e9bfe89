#!/usr/bin/env python3
"""What the seeded augmentation kernels cost, on one GPU.

    python scripts/bench_augment.py [--repeats 9] [--inner 20] [--steps 1000] [--rounds 5] [--out FILE]

1. Kernels.  ``augment_fwd`` and ``augment_bwd`` (csrc/kernels/augment.hip, called through the bindings: one
   launch each) for a RandomTranslation(0.1, 0.1, "reflect") + horizontal RandomFlip transform, next to a plain
   device copy of the same bytes (``Tensor.copy_``), at an MNIST batch, a CIFAR batch, an ImageNet batch (f32 and
   bf16, C = 3: the per-element path) and a ResNet activation (bf16, C = 64: the 16-byte vector path).  The arms
   alternate in one process after a warm-up; a sample is ``inner`` consecutive calls between two device events,
   the figure is the median of ``repeats`` samples.  GB/s counts one read and one write of the tensor.  The two
   largest shapes are also run with the grid cap lowered through the test hook.
2. The step.  The generic engine's reference-CNN step (``bench.py --engine generic``: device-resident input,
   execution graphs of 25 steps) with ``RandomTranslation(0.1, 0.1)`` and ``RandomFlip("horizontal")`` in front
   of the model against the same model without them: ``rounds`` alternating runs of ``steps`` steps each, a host
   clock around ``run_train`` and a device synchronise.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import tensorflow_distributed_learning_amd as tdl  # noqa: E402
from tensorflow_distributed_learning_amd.ops import augment as A  # noqa: E402
from tensorflow_distributed_learning_amd.ops import dropout as D  # noqa: E402

KEY = D.stream_key(3, 0, 0)


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


def bench_kernels(shape, dtype, repeats, inner):
    from tensorflow_distributed_learning_amd.ops import hip

    C = hip()
    N, H, W, Ch = shape
    g = torch.Generator().manual_seed(0)
    x = torch.randn(shape, generator=g).to(dtype).cuda()
    dy = torch.randn(shape, generator=g).to(dtype).cuda()
    dst = torch.empty_like(x)
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    th, tw = int(0.1 * H), int(0.1 * W)
    spec = A.Spec(flip_w=True, off_h_lo=-th, off_h_count=2 * th + 1, off_w_lo=-tw, off_w_count=2 * tw + 1, out_h=H,
                  out_w=W, fill_mode="reflect")
    args = spec.args()
    _, ticket = C.augment_fwd(x, state, KEY[0], KEY[1], *args)
    res = alternate({"copy": lambda: dst.copy_(x),
                     "fwd": lambda: C.augment_fwd(x, state, KEY[0], KEY[1], *args),
                     "bwd": lambda: C.augment_bwd(dy, ticket, KEY[0], KEY[1], *args, H, W)}, repeats, inner)
    calls = int(state.cpu()[0])
    assert calls == 1 + (3 + repeats) * inner, f"the call counter reads {calls}"
    return res


def bench_grid_caps(shape, dtype, caps, repeats, inner):
    """Forward and backward at lowered grid caps (the test hook): fewer workgroups stride further, and fewer
    arrive at the forward's call counter."""
    from tensorflow_distributed_learning_amd.ops import hip

    C = hip()
    N, H, W, Ch = shape
    g = torch.Generator().manual_seed(0)
    x = torch.randn(shape, generator=g).to(dtype).cuda()
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    th, tw = int(0.1 * H), int(0.1 * W)
    args = A.Spec(flip_w=True, off_h_lo=-th, off_h_count=2 * th + 1, off_w_lo=-tw, off_w_count=2 * tw + 1, out_h=H,
                  out_w=W, fill_mode="reflect").args()
    _, ticket = C.augment_fwd(x, state, KEY[0], KEY[1], *args)
    out = {}
    try:
        for cap in caps:
            C.augment_force_max_grid(cap)
            out[cap] = alternate({"fwd": lambda: C.augment_fwd(x, state, KEY[0], KEY[1], *args),
                                  "bwd": lambda: C.augment_bwd(x, ticket, KEY[0], KEY[1], *args, H, W)}, repeats, inner)
    finally:
        C.augment_force_max_grid(0)
    return out


def build_model(augment, spe):
    L = tdl.keras.layers
    tdl.keras.backend.clear_session()
    tdl.keras.utils.set_random_seed(0)
    first = [L.RandomTranslation(0.1, 0.1, input_shape=(28, 28, 1)), L.RandomFlip("horizontal")] if augment else []
    shape = {} if augment else {"input_shape": (28, 28, 1)}
    with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
        m = tdl.keras.Sequential(first + [
            L.Conv2D(32, 3, activation="relu", **shape), L.MaxPooling2D(), L.Conv2D(64, 3, activation="relu"),
            L.MaxPooling2D(), L.Flatten(), L.Dense(128, activation="relu"), L.Dense(10)])
        m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                  optimizer=tdl.keras.optimizers.SGD(learning_rate=0.001),
                  metrics=[tdl.keras.metrics.SparseCategoricalAccuracy()], steps_per_execution=spe)
    return m


def bench_step(steps, rounds, warmup=50, spe=25, batch=64):
    from tensorflow_distributed_learning_amd.data import tfds

    os.environ["TDL_DISABLE_FUSED"] = "1"
    ds_all, _ = tfds.load("mnist", as_supervised=True, with_info=True)

    def scale(image, label):
        return image.to(torch.float32) / 255, label

    arms = {}
    for name, augment in (("plain", False), ("augmented", True)):
        tdl.data.set_global_seed(0)
        train = ds_all["train"].map(scale).cache().shuffle(10000).batch(batch).repeat()
        m = build_model(augment, spe)
        tr = m._get_trainer()
        handler = tr.prepare(train)
        if tr.kind != "generic" or handler is None:
            raise SystemExit(f"bench_augment: {name}: the generic engine's device path was not taken")
        tr.run_train(handler, warmup)
        tr.warm_graphs(steps)
        arms[name] = (m, tr, handler)
    out = {k: [] for k in arms}
    for _ in range(rounds):
        for name, (m, tr, handler) in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            done = tr.run_train(handler, steps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert done == steps and bool(tr._graphs)
            out[name].append(dt / steps * 1e6)
    calls = [l.rng_calls("cuda:0") for l in arms["augmented"][0].layers[:2]]
    assert calls == [warmup + rounds * steps] * 2, calls
    return out, batch


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 7:
        ap.error("--repeats must be >= 7")
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: needs a GPU")
    from tensorflow_distributed_learning_amd.ops import hip

    C = hip()
    lines = [f"scripts/bench_augment.py --repeats {args.repeats} --inner {args.inner} --steps {args.steps} --rounds "
             f"{args.rounds}", f"device: {torch.cuda.get_device_name(0)}; AUGMENT_WG_ELEMS = {C.AUGMENT_WG_ELEMS}, "
             f"AUGMENT_MAX_GRID = {C.AUGMENT_MAX_GRID}, AUGMENT_FWD_MAX_GRID = {C.AUGMENT_FWD_MAX_GRID}", "",
             f"Kernels: us per call, median (min .. max) of {args.repeats} samples of {args.inner} consecutive calls, "
             "the arms alternating; translation +-10 % (reflect) and a horizontal flip", ""]
    cases = [((64, 28, 28, 1), torch.float32), ((256, 32, 32, 3), torch.float32), ((256, 224, 224, 3), torch.float32),
             ((256, 224, 224, 3), torch.bfloat16), ((256, 56, 56, 64), torch.bfloat16)]
    for shape, dtype in cases:
        res = bench_kernels(shape, dtype, args.repeats, args.inner)
        n = 1
        for d in shape:
            n *= d
        nbytes = 2 * n * torch.empty((), dtype=dtype).element_size()
        path = "vector" if shape[3] * torch.empty((), dtype=dtype).element_size() % 16 == 0 else "element"
        lines.append(f"{' x '.join(map(str, shape))} {str(dtype).replace('torch.', '')} ({nbytes / 2e6:.2f} MB read + "
                     f"as much written, {path} path)")
        for k, (med, lo, hi) in res.items():
            lines.append(f"  {k:5s} {med:10.2f}  ({lo:.2f} .. {hi:.2f})   {nbytes / med / 1e3:8.1f} GB/s")
        lines.append(f"  fwd / copy = {res['fwd'][0] / res['copy'][0]:.2f}   "
                     f"bwd / copy = {res['bwd'][0] / res['copy'][0]:.2f}")
        lines.append("")
        torch.cuda.empty_cache()
    lines.append(f"Grid cap (augment_force_max_grid; the forward never exceeds AUGMENT_FWD_MAX_GRID = {C.AUGMENT_FWD_MAX_GRID}, "
                 "so its first two figures are one setting): us per call, median")
    for shape, dtype in (cases[2], cases[4]):
        res = bench_grid_caps(shape, dtype, (2048, 1024, 512, 256), args.repeats, args.inner)
        lines.append(f"  {' x '.join(map(str, shape))} {str(dtype).replace('torch.', '')}: " + "; ".join(
            f"cap {cap}: fwd {r['fwd'][0]:.2f} bwd {r['bwd'][0]:.2f}" for cap, r in res.items()))
        torch.cuda.empty_cache()
    lines.append("")
    out, batch = bench_step(args.steps, args.rounds)
    lines.append(f"Generic reference-CNN step, batch {batch}, execution graphs of 25 steps, {args.steps} steps per run, "
                 "the arms alternating: us per step")
    for r in range(args.rounds):
        for k in out:
            lines.append(f"  round {r + 1}  {k:10s} {out[k][r]:9.2f} us/step   {batch / out[k][r] * 1e6:11.1f} img/s")
    mp, ma = statistics.mean(out["plain"]), statistics.mean(out["augmented"])
    lines.append(f"  mean: plain {mp:.2f} us/step, augmented {ma:.2f} us/step: the two layers add {ma - mp:+.2f} us "
                 f"per step ({(ma / mp - 1) * 100:+.1f} %)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
