"""Wiring of the fused MNIST step's kernel arguments, pinned bit for bit.

k_fwd_conv and k_finalize_x take the fields they need first as leading scalar kernel parameters, filled
by their launchers from the same MnistArgs as the struct that follows.  A field wired to the wrong
parameter (two offsets or two pointers swapped) is a wrong result, not a fault, so it is pinned here
against tests/golden/mnist_launch_args.npz, written by scripts/make_mnist_launch_args_golden.py at the
commit before the parameters moved.

Per batch size -- 1 and 17 (four consecutive workgroups per image: b % 8 != 0), 8 and 64 (the XCD
workgroup map) -- three SGD steps on evolving weights over a shuffled index vector that repeats a sample,
with a non-default learning rate in the device scalar (training: head 1, fused backward, finalize with
SGD), then an evaluation of the trained weights (head 2, logits).  Compared as bits: the weights and
the last step's gradient ranges (CRC-32 per variable; dW1 / db1 raw), the logits, the accuracy and
sample counts.  Not the loss sums: float atomics add them in arrival order.  One more case runs b = 8
with the finalize's grid capped (TDL_FX_GRID: the range loop, LOOP = true) against the same record."""
import os
import zlib

import numpy as np
import pytest
import torch

from tensorflow_distributed_learning_amd.models import mnist_cnn as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mnist_launch_args.npz")
BATCHES = (1, 8, 17, 64)
LR = 0.0375  # (the default is 0.01)
VARS = ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")


def _crc(t):
    return np.uint32(zlib.crc32(t.detach().cpu().contiguous().numpy().tobytes()))


def launch_args_record(cuda, b, N=256, seed=3):
    """What the golden file stores for per-replica batch b (both sides of the comparison run this)."""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(N, 28, 28, 1, generator=g)
    Y = torch.randint(0, 10, (N,), generator=g, dtype=torch.int32)
    params = M.init_mnist_params(seed)
    for i in (1, 3, 5, 7):
        params[i] = (torch.rand(params[i].shape, generator=g) - 0.5) * 0.1
    idx = torch.randperm(N, generator=g)[: 3 * b].to(torch.int32)
    idx[2 * b] = idx[0]  # a sample seen again in a later step
    if b > 1:
        idx[b + b // 2] = idx[b]  # and twice within one batch
    layout = M.mnist_layout()
    W = layout.pack(params, device=cuda)
    G = torch.zeros_like(W)
    lr = torch.tensor([LR], device=cuda)
    metrics = torch.zeros(4, device=cuda)
    step = M.FusedMnistTrainStep(X.to(cuda), Y.to(cuda), idx.to(cuda), W, G, layout, b, 1, lr, metrics)
    assert step.fused_bwd
    for k in range(3):
        step.forward_backward(k * b)
        step.finalize(True)
    torch.cuda.synchronize()
    step.check()
    rec = {}
    m = metrics.cpu().numpy()
    rec["train_correct"], rec["train_count"] = m[1].copy(), m[2].copy()
    for name, w, gr in zip(VARS, layout.views(W.cpu()), layout.views(G.cpu())):
        rec["crc_" + name] = _crc(w)
        rec["crc_d" + name] = _crc(gr)
    dw1, db1 = layout.views(G.cpu())[:2]
    rec["dw1"] = dw1.reshape(-1).numpy().copy()
    rec["db1"] = db1.reshape(-1).numpy().copy()
    metrics.zero_()
    logits = torch.zeros(b * 10, device=cuda)
    step.forward_eval(b, logits)
    torch.cuda.synchronize()
    m = metrics.cpu().numpy()
    rec["eval_correct"], rec["eval_count"] = m[1].copy(), m[2].copy()
    rec["logits"] = logits.cpu().numpy().copy()
    rec["crc_w_after_eval"] = _crc(W)  # evaluation writes no weight
    return rec


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _compare(rec, gold, b, what):
    assert rec["train_count"] == 3 * b and rec["eval_count"] == b  # (the case ran what it says)
    for name, got in rec.items():
        want = gold[f"b{b}_{name}"]
        got = np.asarray(got)
        assert got.shape == want.shape and got.dtype == want.dtype, f"{what} {name}"
        bad = np.flatnonzero(_bits(got).reshape(-1) != _bits(want).reshape(-1))
        assert bad.size == 0, f"{what} {name}: {bad.size} of {got.size} words differ, first at {bad[:4]}: " \
                              f"{got.reshape(-1)[bad[:4]]} vs golden {want.reshape(-1)[bad[:4]]}"


@pytest.mark.gpu
@pytest.mark.parametrize("b", BATCHES)
def test_launch_args_match_golden(cuda, b, monkeypatch):
    monkeypatch.delenv("TDL_FX_GRID", raising=False)
    _compare(launch_args_record(cuda, b), np.load(GOLDEN), b, f"b={b}")


@pytest.mark.gpu
def test_launch_args_capped_finalize_grid_matches_golden(cuda, monkeypatch):
    # 48 workgroups loop over the 375 ranges: same ranges, same sums, so the same bits as one each
    monkeypatch.setenv("TDL_FX_GRID", "48")
    _compare(launch_args_record(cuda, 8), np.load(GOLDEN), 8, "b=8 capped grid")
