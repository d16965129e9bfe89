#!/usr/bin/env python3
"""What the group-normalisation kernels cost, launch by launch, on one GPU.

    python scripts/bench_groupnorm.py [--repeats 9] [--inner 10] [--out FILE] [--skip-step]

For every shape: the three forward launches (sums, finalize, apply) and the three backward launches of
csrc/kernels/groupnorm.hip, each timed alone on the buffers of a complete call (the ``phases`` hook of the
bindings), beside

* a plain device copy of the same tensor (``y.copy_(x)``: one read and one write), and
* the batch-norm kernels of csrc/kernels/bn.hip on the same shape: ``bn_forward_train`` (statistics pass +
  finalize + apply: the tensor is read twice and written once) and ``bn_backward`` mode 0 (sums pass + dx pass:
  read four times, written once).

Shapes: the normalisation inputs of ResNet-50 at batch 256 in bf16 (groups 32) and 64 x 26 x 26 x 32 in f32
(groups 8), the first conv's output of the small CNN below; then two of the ResNet maps again with one group per
channel (``groups=-1``, instance normalisation), where the finalize kernels pack 64 one-channel groups into a
wave.  All arms of a shape alternate in one process after a warm-up; a sample is ``inner`` consecutive launches
between two device events, the figure is the median of ``repeats`` samples.  TB/s counts what the launch must
move: sums forward 1 pass over the tensor, apply forward 2, sums backward 2, apply backward 3, copy 2, BN forward 3,
BN backward 5.

Last: the generic-engine training step (graph-captured) of Conv2D(32, 3) -> [GroupNormalization(8)] -> ReLU ->
MaxPooling2D -> Flatten -> Dense(10) on 28 x 28 x 1 inputs at batch 64, with and without the layer: wall-clock
time of ``fit`` over ``steps`` steps ending in a device synchronise, the two models alternating.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RESNET_B256 = [(256, 112, 112, 64), (256, 56, 56, 64), (256, 56, 56, 256), (256, 28, 28, 128), (256, 28, 28, 512),
               (256, 14, 14, 256), (256, 14, 14, 1024), (256, 7, 7, 512), (256, 7, 7, 2048)]
EPS = 1e-3


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner  # us per launch


def alternate(cases, repeats, inner, warmup=2):
    for _ in range(warmup):
        for fn in cases.values():
            timed(fn, inner)
    samples = {k: [] for k in cases}
    for _ in range(repeats):
        for k, fn in cases.items():
            samples[k].append(timed(fn, inner))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def bench_shape(C, shape, dtype, groups, repeats, inner):
    g = torch.Generator().manual_seed(0)
    ch = shape[-1]
    x = (torch.randn(shape, generator=g) * 2 + 0.5).to(dtype).cuda()
    dy = torch.randn(shape, generator=g).to(dtype).cuda()
    gamma = (torch.rand(ch, generator=g) + 0.5).cuda()
    beta = torch.randn(ch, generator=g).cuda()
    y, st, part, coef = C.gn_forward(x, groups, gamma, beta, EPS)
    fws = [y, st, part, coef]
    dx, dg, db, bpart, bcoef = C.gn_backward(dy, x, groups, gamma, st)
    bws = [dx, bpart, bcoef]
    cases = {}
    for name, ph in (("gn fwd sums", 1), ("gn fwd finalize", 2), ("gn fwd apply", 4)):
        cases[name] = (lambda ph=ph: C.gn_forward(x, groups, gamma, beta, EPS, ph, fws))
    for name, ph in (("gn bwd sums", 1), ("gn bwd finalize", 2), ("gn bwd apply", 4)):
        cases[name] = (lambda ph=ph: C.gn_backward(dy, x, groups, gamma, st, None, None, ph, bws))
    out = torch.empty_like(x)
    cases["device copy"] = lambda: out.copy_(x)
    passes = {"gn fwd sums": 1, "gn fwd finalize": 0, "gn fwd apply": 2, "gn bwd sums": 2, "gn bwd finalize": 0,
              "gn bwd apply": 3, "device copy": 2}
    if ch % 8 == 0 and ch <= 2048:
        mm, mv = torch.zeros(ch, device="cuda"), torch.ones(ch, device="cuda")
        _, bst = C.bn_forward_train(x, gamma, beta, mm, mv, 0.99, EPS)
        cases["bn forward (3 launches)"] = lambda: C.bn_forward_train(x, gamma, beta, mm, mv, 0.99, EPS)
        cases["bn backward (3 launches)"] = lambda: C.bn_backward(dy, x, None, gamma, bst, 0)
        passes.update({"bn forward (3 launches)": 3, "bn backward (3 launches)": 5})
    res = alternate(cases, repeats, inner)
    nbytes = x.numel() * x.element_size()
    lines = []
    for k, (med, lo, hi) in res.items():
        rate = f"{passes[k] * nbytes / med / 1e6:8.2f} TB/s" if passes[k] else " " * 13
        lines.append(f"  {k:26s} {med:9.2f} us  ({lo:.2f} .. {hi:.2f})  {rate}")
    f3 = sum(res[k][0] for k in ("gn fwd sums", "gn fwd finalize", "gn fwd apply"))
    b3 = sum(res[k][0] for k in ("gn bwd sums", "gn bwd finalize", "gn bwd apply"))
    lines.append(f"  gn forward, three launches  {f3:9.2f} us   {3 * nbytes / f3 / 1e6:8.2f} TB/s")
    lines.append(f"  gn backward, three launches {b3:9.2f} us   {5 * nbytes / b3 / 1e6:8.2f} TB/s")
    return nbytes, lines


def bench_step(repeats, steps):
    import tensorflow_distributed_learning_amd as tdl

    L = tdl.keras.layers
    os.environ["TDL_DISABLE_FUSED"] = "1"
    g = torch.Generator().manual_seed(0)
    x, y = torch.rand(64 * 8, 28, 28, 1, generator=g), torch.randint(0, 10, (64 * 8,), generator=g)

    def make(with_gn):
        tdl.keras.backend.clear_session()
        tdl.keras.utils.set_random_seed(3)
        with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
            m = tdl.keras.Sequential([L.Conv2D(32, 3, input_shape=(28, 28, 1))] +
                                     ([L.GroupNormalization(groups=8)] if with_gn else []) +
                                     [L.ReLU(), L.MaxPooling2D(), L.Flatten(), L.Dense(10)])
            m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                      optimizer=tdl.keras.optimizers.SGD(learning_rate=0.05))
        ds = tdl.data.Dataset.from_tensor_slices((x, y)).batch(64).repeat()
        m.fit(ds, epochs=1, steps_per_epoch=16, verbose=0)  # warm-up and graph capture
        assert m._trainer.kind == "generic" and m._trainer._graphs
        return m, ds

    arms = {"without the layer": make(False), "with GroupNormalization(8)": make(True)}
    samples = {k: [] for k in arms}
    for _ in range(repeats):
        for k, (m, ds) in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.fit(ds, epochs=1, steps_per_epoch=steps, verbose=0)
            torch.cuda.synchronize()
            samples[k].append((time.perf_counter() - t0) * 1e6 / steps)
    lines = [f"generic-engine step, small CNN at batch 64 (us per step over fit of {steps} steps, median (min .. max) "
             f"of {repeats})"]
    for k, v in samples.items():
        lines.append(f"  {k:28s} {statistics.median(v):9.2f}  ({min(v):.2f} .. {max(v):.2f})")
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 7:
        ap.error("--repeats must be >= 7")
    from tensorflow_distributed_learning_amd.ops import hip

    C = hip()
    lines = [f"scripts/bench_groupnorm.py --repeats {args.repeats} --inner {args.inner}: us per launch, median (min .. max) "
             f"of {args.repeats} samples of {args.inner} consecutive launches, the arms alternating in one process",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    shapes = [(s, torch.bfloat16, 32) for s in RESNET_B256] + [((64, 26, 26, 32), torch.float32, 8)]
    # instance normalisation (groups=-1: one group per channel): the most (sample, group) pairs a finalize sees
    shapes += [((256, 56, 56, 64), torch.bfloat16, -1), ((256, 14, 14, 1024), torch.bfloat16, -1)]
    for shape, dtype, groups in shapes:
        groups = shape[-1] if groups == -1 else groups
        P = 1
        for d in shape[1:-1]:
            P *= d
        plan = C.gn_plan(P, shape[-1], dtype == torch.bfloat16)
        nbytes, ls = bench_shape(C, shape, dtype, groups, args.repeats, args.inner)
        lines.append(f"{' x '.join(map(str, shape))} {str(dtype).replace('torch.', '')}, {groups} groups "
                     f"({nbytes / 1e6:.2f} MB; plan: {plan[2]} columns x {plan[3]} row lanes, {plan[5]} pixels per "
                     f"workgroup, {plan[6]} chunks, {shape[0] * plan[4] * plan[6]} workgroups)")
        lines += ls + [""]
        torch.cuda.empty_cache()
    if not args.skip_step:
        lines += bench_step(args.repeats, args.steps)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
