#!/usr/bin/env python3
"""What the embedding kernels cost beside the ``F.embedding`` path they replace, on one GPU.

    python scripts/bench_embedding.py [--repeats 7] [--inner 3] [--out FILE]

For (N, V, D) in {(96, 50, 16), (8192, 8192, 128), (16384, 32768, 256), (32768, 50304, 512)} and three shapes between
the first two, f32 and bf16, ids drawn uniformly and from a Zipf law with exponent 1 (id = rank - 1: the hottest rows
share one owner, whose queue is long):

* ``k_embed_fwd``, and ``k_embed_count`` + ``k_embed_bwd`` into a slab view and into a fresh tensor, through the bindings
  (int32 ids; bf16: the forward reads the bf16 copy of the table), and
* the path before: ``F.embedding(ids.long(), table)`` (bf16: and the next layer's cast of the f32 rows), its
  backward (bf16: after the cast's backward to f32) and the add of the dense ``[V, D]`` gradient into the slab view.

All arms of a shape alternate in one process after a warm-up; a sample is ``inner`` consecutive calls between two
device events, the figure is the median of ``repeats`` samples with (min .. max).  ``scan`` = ranges x N is what
ops/embedding.py bounds with ``MAX_SCAN``.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_gru import alternate  # noqa: E402  (the alternating timer of the other cost scripts)

# (the three shapes of N = 1024 ... 4096 bracket the token bound of ops/embedding.py under the skewed law)
SHAPES = [(96, 50, 16), (1024, 8192, 128), (2048, 8192, 128), (4096, 8192, 128), (8192, 8192, 128), (16384, 32768, 256),
          (32768, 50304, 512)]


def draw(N, V, law, rng):
    if law == "uniform":
        return rng.integers(0, V, N)
    p = 1.0 / np.arange(1, V + 1)
    return rng.choice(V, N, p=p / p.sum())


def bench_shape(K, N, V, D, dtype, law, repeats, inner):
    rng, bf16 = np.random.default_rng(0), dtype == torch.bfloat16
    ids = torch.from_numpy(draw(N, V, law, rng)).to(torch.int32).cuda()
    g = torch.Generator().manual_seed(0)
    table = torch.randn(V, D, generator=g).cuda()
    src = table.to(dtype)
    dy = torch.randn(N, D, generator=g).to(dtype).cuda()
    slab = torch.zeros(V, D, device="cuda")
    ids64 = ids.long()

    def old_fwd():
        y = F.embedding(ids.long(), table)
        return y.to(dtype) if bf16 else y

    def old_bwd():
        slab.add_(torch.ops.aten.embedding_dense_backward(dy.float() if bf16 else dy, ids64, V, -1, False))

    cases = {"k_embed_fwd": lambda: K.embed_forward(ids, src, bf16),
             "k_embed bwd -> slab": lambda: K.embed_backward(ids, dy, V, slab),
             "k_embed bwd -> fresh": lambda: K.embed_backward(ids, dy, V),
             "F.embedding forward": old_fwd, "F.embedding backward + add": old_bwd}
    res = alternate(cases, repeats, inner)
    new = res["k_embed_fwd"][0] + res["k_embed bwd -> slab"][0]
    old = res["F.embedding forward"][0] + res["F.embedding backward + add"][0]
    lines = [f"  {k:28s} {med:10.1f} us  ({lo:.1f} .. {hi:.1f})" for k, (med, lo, hi) in res.items()]
    return lines + [f"  forward + backward into the slab: kernels {new:.1f} us, before {old:.1f} us, ratio {new / old:.2f}"]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 7:
        ap.error("--repeats must be >= 7")
    from tensorflow_distributed_learning_amd.ops import hip

    K = hip()
    lines = [f"scripts/bench_embedding.py --repeats {args.repeats} --inner {args.inner}: us per call, median (min .. max) "
             f"of {args.repeats} samples of {args.inner} consecutive calls, the arms alternating in one process",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    for dtype in (torch.float32, torch.bfloat16):
        for N, V, D in SHAPES:
            p = K.embed_plan(N, V, D, dtype == torch.bfloat16)
            for law in ("uniform", "zipf"):
                lines.append(f"N {N} V {V} D {D} {str(dtype).replace('torch.', '')} {law} (rows_wg {p['rows_wg']}, "
                             f"{p['ranges']} ranges, scan {p['ranges'] * N}, LDS {p['lds_bwd']} B)")
                lines += bench_shape(K, N, V, D, dtype, law, args.repeats, args.inner) + [""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
