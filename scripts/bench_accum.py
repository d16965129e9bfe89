#!/usr/bin/env python3
"""What gradient accumulation costs, on one GPU.

    python scripts/bench_accum.py [--repeats 9] [--inner 20] [--steps 200] [--out profiles/accum_cost.txt]

Part 1, the kernel: every mode of ``_C.grad_accum`` (csrc/kernels/accum.hip) at the reference CNN's slab
(225,152 floats) and at ResNet-50's (25,583,616), against

* the byte floor: streams x 4 n bytes (mode 0 + zero_grad: read G, write A, write G = 3; mode 1 + zero_grad:
  read A, read G, write A, write G = 4; mode 2: read A, read G, write G = 3) at the 5.2-6.2 TB/s copy rate that
  profiles/clip_cost.txt records;
* the naive torch form in the same process: ``A.copy_(G); G.zero_()`` / ``A.add_(G); G.zero_()`` /
  ``torch.add(A, G).mul_(c)``.

The cases alternate in one process after a warm-up; a sample is ``inner`` consecutive calls between two device
events, and the figure is the median (min .. max) of ``repeats`` samples.

Part 2, the step: the reference CNN (plain SGD, per-replica batch 64, steps_per_execution 20) on the fused and on
the generic engine with gradient_accumulation_steps off, 2 and 4: us per micro-step, wall clock around ``steps``
steps of ``run_train`` with a device sync, the six configurations alternating.  With accumulation off the fused
engine takes its headline path (the SGD update inside the finalize kernel); an accumulating optimizer leaves it
(finalize, accumulate, and on every k-th micro-step the SGD kernel), so on ONE GPU it is expected to be slower:
what it saves is the gradient exchange of k - 1 of k micro-steps at R > 1.
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


def bench_kernel(n, repeats, inner):
    C = hip()
    g = torch.Generator().manual_seed(0)
    G = (torch.randn(n, generator=g) * 0.1).cuda()
    A = torch.zeros(n, device="cuda")
    c = 0.25
    cases = {
        "mode 0 + zero_grad  kernel": (3, lambda: C.grad_accum(G, A, 0, c, zero_grad=True)),
        "mode 0 + zero_grad  torch": (3, lambda: (A.copy_(G), G.zero_())),
        "mode 1 + zero_grad  kernel": (4, lambda: C.grad_accum(G, A, 1, c, zero_grad=True)),
        "mode 1 + zero_grad  torch": (4, lambda: (A.add_(G), G.zero_())),
        "mode 1              kernel": (3, lambda: C.grad_accum(G, A, 1, c)),
        "mode 2              kernel": (3, lambda: C.grad_accum(G, A, 2, c)),
        "mode 2              torch": (3, lambda: torch.add(A, G).mul_(c)),
    }
    res = alternate({k: fn for k, (_, fn) in cases.items()}, repeats, lambda fn: timed(fn, inner))
    return {k: (cases[k][0],) + v for k, v in res.items()}


def make_step(fused, k, spe, take):
    """(trainer, handler) of the reference CNN with plain SGD on one engine."""
    from tensorflow_distributed_learning_amd.data import tfds
    from tensorflow_distributed_learning_amd.models.mnist_cnn import build_mnist_cnn

    os.environ["TDL_DISABLE_FUSED"] = "0" if fused else "1"
    try:
        ds_all, _ = tfds.load("mnist", as_supervised=True, with_info=True)

        def scale(image, label):
            return image.to(torch.float32) / 255, label

        train = ds_all["train"].take(take).map(scale).cache().shuffle(10000).batch(64).repeat()
        with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
            model = build_mnist_cnn()
            model.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                          optimizer=tdl.keras.optimizers.SGD(learning_rate=0.001, gradient_accumulation_steps=k),
                          metrics=[tdl.keras.metrics.SparseCategoricalAccuracy()], steps_per_execution=spe)
        trainer = model._get_trainer()
        handler = trainer.prepare(train)
        if trainer.kind != ("fused" if fused else "generic") or handler is None:
            raise SystemExit(f"bench_accum: wanted the {'fused' if fused else 'generic'} engine on device-resident "
                             f"data, got {trainer.kind} ({getattr(model, '_fused_reason', '?')})")
        return model, trainer, handler
    finally:
        os.environ.pop("TDL_DISABLE_FUSED", None)


def bench_steps(repeats, steps, spe=20, take=8192):
    runs = {}
    for fused in (True, False):
        for k in (None, 2, 4):
            name = f"{'fused' if fused else 'generic':8s} k = {k or 'off'}"
            model, trainer, handler = make_step(fused, k, spe, take)
            trainer.run_train(handler, 2 * spe)  # (eager first execution of the generic engine, allocator warm-up)
            trainer.warm_graphs(steps)
            trainer.run_train(handler, 2 * spe)
            runs[name] = (model, trainer, handler)

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
        ap.error("--steps must be a multiple of 20 (whole executions, every one starting at phase 0)")
    C = hip()
    lines = [f"scripts/bench_accum.py --repeats {args.repeats} --inner {args.inner} --steps {args.steps}: median "
             f"(min .. max) of {args.repeats} interleaved samples",
             f"device: {torch.cuda.get_device_name(0)}; ACCUM_BLOCK_ELEMS = {C.ACCUM_BLOCK_ELEMS}, "
             f"ACCUM_MAX_BLOCKS = {C.ACCUM_MAX_BLOCKS}", "",
             f"k_grad_accum, us per call ({args.inner} consecutive calls per sample); floor = streams x 4 n bytes at "
             f"{STREAM_TBS[1]}-{STREAM_TBS[0]} TB/s"]
    for name, n in SLABS.items():
        lines.append(f"{name}: slab of {n} floats ({4 * n / 1e6:.2f} MB)")
        for k, (streams, med, lo, hi) in bench_kernel(n, args.repeats, args.inner).items():
            floor = [streams * 4.0 * n / (t * 1e12) * 1e6 for t in STREAM_TBS]
            lines.append(f"  {k:28s} {med:9.2f}  ({lo:.2f} .. {hi:.2f})   floor {floor[1]:.2f}-{floor[0]:.2f} "
                         f"({streams} streams): {med / floor[0]:.2f}x-{med / floor[1]:.2f}x the floor")
        lines.append("")
    torch.cuda.empty_cache()
    lines.append(f"reference CNN, plain SGD, batch 64, steps_per_execution 20: us per micro-step over {args.steps} "
                 "steps of run_train (wall clock, device sync)")
    res = bench_steps(args.repeats, args.steps)
    for k, (med, lo, hi) in res.items():
        base = res[k.split(" k = ")[0] + " k = off"][0]
        lines.append(f"  {k:18s} {med:9.2f}  ({lo:.2f} .. {hi:.2f})   {med - base:+.2f} us against k off")
    lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
