#!/usr/bin/env python3
"""What sample weights, class weights and label smoothing cost in the loss head, on one GPU.

    python scripts/bench_loss_head.py [--repeats 9] [--inner 20] [--steps 200] [--out profiles/loss_head_cost.txt]

Part 1, the kernels, at the reference CNN's head (64 x 10 logits: one workgroup, the K <= 64 path) and at
ResNet-50's (256 x 1000: rows + finish): ``xent_head`` (csrc/kernels/gemm.hip), and ``xent_head_w``
(csrc/kernels/loss_head.hip) without weights, with a sample-weight column, with a class-weight table, with both,
with label smoothing 0.1, with everything, and on dense one-hot targets; plus the torch formulas the weighted step
ran before (cross_entropy, the weight products, the sums and the metric updates), forward only.

The cases alternate in one process after a warm-up; a sample is ``inner`` consecutive calls between two device
events, and the figure is the median (min .. max) of ``repeats`` samples.

Part 2, the step: the reference CNN on the generic engine (TDL_DISABLE_FUSED=1, plain SGD, batch 64,
steps_per_execution 20, device-resident input, execution graphs) without weights, with ``class_weight``, and with a
sample-weight column: us per step, wall clock around ``steps`` steps of ``run_train`` with a device sync, the
configurations alternating.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["TDL_DISABLE_FUSED"] = "1"

import tensorflow_distributed_learning_amd as tdl  # noqa: E402
from tensorflow_distributed_learning_amd.ops import hip  # noqa: E402

HEADS = {"reference CNN": (64, 10), "ResNet-50": (256, 1000)}
EPS = 0.1


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner  # us per call


def alternate(cases, repeats, sample, warmup=3):
    for _ in range(warmup):
        for fn in cases.values():
            sample(fn)
    samples = {k: [] for k in cases}
    for _ in range(repeats):
        for k, fn in cases.items():
            samples[k].append(sample(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def bench_kernels(N, K, repeats, inner):
    C = hip()
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(N, K, generator=g) * 3).cuda()
    y = torch.randint(0, K, (N,), generator=g).cuda()
    t = torch.nn.functional.one_hot(y, K).float()
    sw = (torch.rand(N, generator=g) * 3.75 + 0.25).cuda()
    cw = (torch.rand(K, generator=g) * 3.75 + 0.25).cuda()
    accs = [torch.zeros(1, dtype=torch.float64, device="cuda") for _ in range(4)]
    gn = float(N)

    def torch_head():
        per = torch.nn.functional.cross_entropy(z, y, reduction="none", label_smoothing=EPS)
        w = sw * cw[y]
        per = per * w
        loss = per.sum() / gn
        accs[0].add_(per.double().sum())
        accs[1].add_(float(N))
        cor = (z.argmax(-1) == y).double()
        accs[2].add_((cor * w.double()).sum())
        accs[3].add_(w.double().sum())
        return loss

    cases = {
        "xent_head": lambda: C.xent_head(z, y, gn, *accs),
        "xent_head_w  no weights": lambda: C.xent_head_w(z, y, gn, None, None, 0.0, *accs),
        "xent_head_w  sw": lambda: C.xent_head_w(z, y, gn, sw, None, 0.0, *accs),
        "xent_head_w  cw": lambda: C.xent_head_w(z, y, gn, None, cw, 0.0, *accs),
        "xent_head_w  sw cw": lambda: C.xent_head_w(z, y, gn, sw, cw, 0.0, *accs),
        "xent_head_w  eps": lambda: C.xent_head_w(z, y, gn, None, None, EPS, *accs),
        "xent_head_w  sw cw eps": lambda: C.xent_head_w(z, y, gn, sw, cw, EPS, *accs),
        "xent_head_w  dense": lambda: C.xent_head_w(z, t, gn, None, None, 0.0, *accs),
        "xent_head_w  dense sw cw eps": lambda: C.xent_head_w(z, t, gn, sw, cw, EPS, *accs),
        "torch        sw cw eps, forward": torch_head,
    }
    return alternate(cases, repeats, lambda fn: timed(fn, inner))


def make_step(kind, spe, n=8192):
    """(trainer, handler) of the reference CNN on the generic engine: ``kind`` in none / class_weight / sample_weight."""
    from tensorflow_distributed_learning_amd.data.tfds import synthetic_mnist
    from tensorflow_distributed_learning_amd.models.mnist_cnn import build_mnist_cnn

    x, y = synthetic_mnist(n, 0)
    x, y = torch.as_tensor(x).reshape(-1, 28, 28, 1), torch.as_tensor(y).long()
    table = torch.linspace(0.25, 4.0, 10)
    cols = (x, y, table[y]) if kind == "sample_weight" else (x, y)

    def scale(image, *rest):
        return (image.to(torch.float32) / 255,) + rest

    train = tdl.data.Dataset.from_tensor_slices(cols).map(scale).cache().shuffle(n).batch(64).repeat()
    with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
        model = build_mnist_cnn()
        model.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                      optimizer=tdl.keras.optimizers.SGD(learning_rate=0.001),
                      metrics=[tdl.keras.metrics.SparseCategoricalAccuracy()], steps_per_execution=spe)
    trainer = model._get_trainer()
    trainer.set_class_weight(table if kind == "class_weight" else None)
    handler = trainer.prepare(train)
    if trainer.kind != "generic" or handler is None:
        raise SystemExit(f"bench_loss_head: wanted the generic engine on device-resident data, got {trainer.kind}")
    return model, trainer, handler


def bench_steps(repeats, steps, spe=20):
    runs = {}
    for name, kind in (("no weights       (xent_head)", "none"), ("class_weight    (xent_head_w cw)", "class_weight"),
                       ("sample weights  (xent_head_w sw, gather_xyw)", "sample_weight")):
        model, trainer, handler = make_step(kind, spe)
        trainer.run_train(handler, 2 * spe)
        trainer.warm_graphs(steps)
        trainer.run_train(handler, 2 * spe)
        if not any(k[0] == "dev" for k in trainer._graphs):
            raise SystemExit(f"bench_loss_head: no execution graph was captured for {name!r}")
        runs[f"{name:46s}"] = (model, trainer, handler)

    def sample(run):
        _, trainer, handler = run
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = trainer.run_train(handler, steps)
        torch.cuda.synchronize()
        assert done == steps
        return (time.perf_counter() - t0) * 1e6 / steps

    return alternate(runs, repeats, sample, warmup=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 7:
        ap.error("--repeats must be >= 7")
    if args.steps % 20:
        ap.error("--steps must be a multiple of 20 (whole executions)")
    lines = [f"scripts/bench_loss_head.py --repeats {args.repeats} --inner {args.inner} --steps {args.steps}: median "
             f"(min .. max) of {args.repeats} interleaved samples",
             f"device: {torch.cuda.get_device_name(0)}", "",
             f"us per call ({args.inner} consecutive calls per sample); label smoothing {EPS}, weights in [0.25, 4]"]
    for name, (N, K) in HEADS.items():
        lines.append(f"{name}: {N} x {K} logits")
        res = bench_kernels(N, K, args.repeats, args.inner)
        base = res["xent_head"][0]
        for k, (med, lo, hi) in res.items():
            lines.append(f"  {k:34s} {med:9.2f}  ({lo:.2f} .. {hi:.2f})   {med - base:+.2f} us against xent_head")
        lines.append("")
    torch.cuda.empty_cache()
    lines.append("generic reference-CNN step, plain SGD, batch 64, steps_per_execution 20, device-resident input: us per "
                 f"step over {args.steps} steps of run_train (wall clock, device sync)")
    res = bench_steps(args.repeats, args.steps)
    base = next(iter(res.values()))[0]
    for k, (med, lo, hi) in res.items():
        lines.append(f"  {k} {med:9.2f}  ({lo:.2f} .. {hi:.2f})   {med - base:+.2f} us against no weights")
    lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
