#!/usr/bin/env python3
"""What the weight EMA (``use_ema``) costs, on one GPU.

    python scripts/bench_ema.py [--repeats 9] [--inner 20] [--steps 200] [--out profiles/ema_cost.txt]

Part 1, the kernels, at the reference CNN's slab (225,152 floats) and at ResNet-50's (25,583,616): an update
kernel without the average, the same kernel with the average inside (its EMA instantiation: one more slab read
and written in the same pass), and the kernel without it followed by the stand-alone ``_C.weight_ema``
(csrc/kernels/ema.hip: W read again, E read and written, one more launch); plus the stand-alone kernel alone in
both modes against its byte floor (mode 1: read W, read E, write E = 3 streams; mode 2 also writes W = 4) at the
5.2-6.2 TB/s copy rate that profiles/clip_cost.txt records, and against the naive torch form.

The cases alternate in one process after a warm-up; a sample is ``inner`` consecutive calls between two device
events, and the figure is the median (min .. max) of ``repeats`` samples.

Part 2, the step: the fused reference-CNN step (plain SGD, per-replica batch 64, steps_per_execution 20) with EMA
off, with EMA on the way the engine runs it (plain SGD stays plain: the SGD inside the finalize launch, then the
stand-alone kernel), and with EMA on after leaving the plain path (the trainer's ``leave_plain_for_ema``, a
measurement switch: finalize without SGD, then ``k_sgd`` with the average inside): us per step, wall clock around ``steps``
steps of ``run_train`` with a device sync, the configurations alternating.
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
from tensorflow_distributed_learning_amd.ops import hip  # noqa: E402

SLABS = {"reference CNN": 225_152, "ResNet-50": 25_583_616}
STREAM_TBS = (5.2, 6.2)
M = 0.99


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


def bench_kernels(n, repeats, inner):
    C = hip()
    g = torch.Generator().manual_seed(0)
    W = torch.randn(n, generator=g).cuda()
    G = (torch.randn(n, generator=g) * 1e-3).cuda()
    E, V, Mo = W.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    V2 = torch.full((n,), 1e-3, device="cuda")
    lr = torch.tensor([1e-3], device="cuda")
    t0 = torch.tensor([10.0], device="cuda")
    ema = dict(ema=E, ema_momentum=M, ema_mode=1)
    m32, c32 = M, 1.0 - M

    def mom(**kw):
        C.sgd_momentum(W, G, V, lr, 0.9, False, **kw)

    def adam(**kw):
        C.adam(W, G, Mo, V2, None, lr, t0, 0, 0.9, 0.999, 1e-7, **kw)

    cases = {
        "k_sgd           no EMA": lambda: C.sgd(W, G, lr),
        "k_sgd           EMA inside": lambda: C.sgd(W, G, lr, **ema),
        "k_sgd           + stand-alone": lambda: (C.sgd(W, G, lr), C.weight_ema(W, E, M, 1)),
        "k_sgd_momentum  no EMA": mom,
        "k_sgd_momentum  EMA inside": lambda: mom(**ema),
        "k_sgd_momentum  + stand-alone": lambda: (mom(), C.weight_ema(W, E, M, 1)),
        "k_adam          no EMA": adam,
        "k_adam          EMA inside": lambda: adam(**ema),
        "k_adam          + stand-alone": lambda: (adam(), C.weight_ema(W, E, M, 1)),
        "k_weight_ema    mode 1": lambda: C.weight_ema(W, E, M, 1),
        "k_weight_ema    mode 2": lambda: C.weight_ema(W, E, M, 2),
        "torch           mode 1": lambda: E.mul_(m32).add_(W * c32),
    }
    return alternate(cases, repeats, lambda fn: timed(fn, inner))


def make_step(use_ema, leave_plain, spe, take):
    """(model, trainer, handler) of the reference CNN with plain SGD on the fused engine."""
    from tensorflow_distributed_learning_amd.data import tfds
    from tensorflow_distributed_learning_amd.models.mnist_cnn import build_mnist_cnn

    ds_all, _ = tfds.load("mnist", as_supervised=True, with_info=True)

    def scale(image, label):
        return image.to(torch.float32) / 255, label

    train = ds_all["train"].take(take).map(scale).cache().shuffle(10000).batch(64).repeat()
    with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
        model = build_mnist_cnn()
        model.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                      optimizer=tdl.keras.optimizers.SGD(learning_rate=0.001, use_ema=use_ema, ema_momentum=M),
                      metrics=[tdl.keras.metrics.SparseCategoricalAccuracy()], steps_per_execution=spe)
    trainer = model._get_trainer()
    trainer.leave_plain_for_ema = bool(leave_plain)
    handler = trainer.prepare(train)
    if trainer.kind != "fused" or handler is None:
        raise SystemExit(f"bench_ema: wanted the fused engine on device-resident data, got {trainer.kind} "
                         f"({getattr(model, '_fused_reason', '?')})")
    return model, trainer, handler


def bench_steps(repeats, steps, spe=20, take=8192):
    runs = {}
    for name, use_ema, leave in (("EMA off (SGD in finalize)", False, False),
                                 ("EMA, stays plain + stand-alone kernel", True, False),
                                 ("EMA, leaves plain: k_sgd, average inside", True, True)):
        model, trainer, handler = make_step(use_ema, leave, spe, take)
        trainer.run_train(handler, 2 * spe)
        trainer.warm_graphs(steps)
        trainer.run_train(handler, 2 * spe)
        runs[f"{name:42s} [{trainer.update_path}]"] = (model, trainer, handler)

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
    C = hip()
    lines = [f"scripts/bench_ema.py --repeats {args.repeats} --inner {args.inner} --steps {args.steps}: median "
             f"(min .. max) of {args.repeats} interleaved samples",
             f"device: {torch.cuda.get_device_name(0)}; EMA_BLOCK_ELEMS = {C.EMA_BLOCK_ELEMS}, "
             f"EMA_MAX_BLOCKS = {C.EMA_MAX_BLOCKS}", "",
             f"us per call ({args.inner} consecutive calls per sample); k_weight_ema's floor = streams x 4 n bytes at "
             f"{STREAM_TBS[1]}-{STREAM_TBS[0]} TB/s"]
    for name, n in SLABS.items():
        lines.append(f"{name}: slab of {n} floats ({4 * n / 1e6:.2f} MB)")
        res = bench_kernels(n, args.repeats, args.inner)
        for k, (med, lo, hi) in res.items():
            extra = ""
            if k.startswith("k_weight_ema"):
                streams = 3 if k.endswith("1") else 4
                floor = [streams * 4.0 * n / (t * 1e12) * 1e6 for t in STREAM_TBS]
                extra = f"   floor {floor[1]:.2f}-{floor[0]:.2f} ({streams} streams)"
            elif not k.endswith("no EMA") and not k.startswith("torch"):
                extra = f"   {med - res[k.split('  ')[0].ljust(14) + '  no EMA'][0]:+.2f} us against no EMA"
            lines.append(f"  {k:32s} {med:9.2f}  ({lo:.2f} .. {hi:.2f}){extra}")
        lines.append("")
    torch.cuda.empty_cache()
    lines.append(f"fused reference-CNN step, plain SGD, batch 64, steps_per_execution 20: us per step over {args.steps} "
                 "steps of run_train (wall clock, device sync); [the engine's update path]")
    res = bench_steps(args.repeats, args.steps)
    base = next(iter(res.values()))[0]
    for k, (med, lo, hi) in res.items():
        lines.append(f"  {k} {med:9.2f}  ({lo:.2f} .. {hi:.2f})   {med - base:+.2f} us against EMA off")
    lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
