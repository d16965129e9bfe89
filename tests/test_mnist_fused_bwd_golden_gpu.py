"""The fused MNIST step's conv backward (the end of k_fwd_conv), pinned two ways.

Golden: the gradients and the weights after SGD that the kernel computed before its backward was
re-scheduled (tests/golden/mnist_fused_bwd.npz, written by scripts/make_mnist_golden.py), bit for
bit.  The gradients have no atomics and a fixed reduction order, so the fixture holds on every MI355X.

Edges: inputs that put exact zeros where the backward's epilogue masks and routes (closed ReLU masks,
an all-zero dC2 grid, zeros in dH, pool windows of exact ties), against the fp64 reference with the
tolerance of tests/test_mnist_fused_gpu.py (2e-5 of the tensor's max)."""
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tensorflow_distributed_learning_amd.models import mnist_cnn as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mnist_fused_bwd.npz")
GOLDEN_BATCHES = (8, 17)  # XCD workgroup map on (b % 8 == 0) / off and ragged


def _setup(cuda, b, R=1, N=512, seed=0, mutate=None):
    """The inputs of tests/test_mnist_fused_gpu.py::_setup (seeded CPU generator, non-zero biases);
    mutate(X, params, idx) edits them in place before they go to the device."""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(N, 28, 28, 1, generator=g)
    Y = torch.randint(0, 10, (N,), generator=g, dtype=torch.int32)
    params = M.init_mnist_params(seed)
    for i in (1, 3, 5, 7):
        params[i] = (torch.rand(params[i].shape, generator=g) - 0.5) * 0.1
    idx = torch.randperm(N, generator=g)[: 3 * b].to(torch.int32)
    if mutate is not None:
        mutate(X, params, idx)
    layout = M.mnist_layout()
    W = layout.pack(params, device=cuda)
    G = torch.zeros_like(W)
    lr = torch.tensor([0.01], device=cuda)
    step = M.FusedMnistTrainStep(X.to(cuda), Y.to(cuda), idx.to(cuda), W, G, layout, b, R, lr)
    return X, Y, params, layout, W, G, idx, step


def _crc(t):
    return np.uint32(zlib.crc32(t.detach().cpu().contiguous().numpy().tobytes()))


def golden_record(cuda, b):
    """What the golden file stores for per-replica batch b (also what make_mnist_golden.py writes)."""
    X, Y, params, layout, W, G, idx, step = _setup(cuda, b)
    assert step.fused_bwd
    step.forward_backward(b)
    step.finalize(False)
    torch.cuda.synchronize()
    step.check()
    dw1, db1, dw2, db2 = layout.views(G.cpu())[:4]
    rec = {
        "dw1": dw1.reshape(-1).numpy().copy(),
        "db1": db1.reshape(-1).numpy().copy(),
        "crc_dw2": _crc(dw2),
        "crc_db2": _crc(db2),
        "crc_g": _crc(G),
    }
    X, Y, params, layout, W, G, idx, step = _setup(cuda, b)
    for k in range(3):
        step.forward_backward(k * b)
        step.finalize(True)
    torch.cuda.synchronize()
    step.check()
    rec["crc_w3steps"] = _crc(W)
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize("b", GOLDEN_BATCHES)
def test_fused_bwd_matches_golden(cuda, b):
    gold = np.load(GOLDEN)
    rec = golden_record(cuda, b)
    assert rec["dw1"].size + rec["db1"].size == 320
    for name, got in rec.items():
        want = gold[f"b{b}_{name}"]
        if name in ("dw1", "db1"):
            # compared as bit patterns: -0.0 / 0.0 and NaN payloads count
            bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, f"b={b} {name}: {bad.size} of {got.size} floats differ, first at {bad[:4]}: " \
                                  f"{got[bad[:4]]} vs golden {want[bad[:4]]}"
        else:
            assert int(got) == int(want), f"b={b} {name}: crc {int(got):#010x} vs golden {int(want):#010x}"


def test_reference_pool_routes_ties_to_first():
    """The fp64 reference's max-pool backward sends the gradient of a window of exact ties to its
    first element -- what the kernel's strict `>` argmax scan does; the all-zero-image case relies on it."""
    x = torch.zeros(1, 2, 4, 4, dtype=torch.float64, requires_grad=True)
    F.max_pool2d(x, 2).sum().backward()
    want = torch.zeros(4, 4, dtype=torch.float64)
    want[0::2, 0::2] = 1.0
    assert torch.equal(x.grad[0, 0], want) and torch.equal(x.grad[0, 1], want)


def _conv1_bias_closed(X, params, idx):
    params[1][::2] = -10.0  # half of conv1's channels: closed ReLU masks, exact-zero dP1 lanes


def _conv2_quarter_closed(X, params, idx):
    params[3][16:32] = -10.0  # channel quarter 1: an all-zero dC2 grid for that workgroup


def _dense1_half_closed(X, params, idx):
    params[5][::2] = -10.0  # zeros in H and dH


def _zero_image(X, params, idx):
    # the first image of every batch chunk: each pool-1 window an exact tie (argmax 0)
    b = idx.numel() // 3
    X[idx[b].long()] = 0.0


EDGES = {"conv1_bias_closed": _conv1_bias_closed, "conv2_quarter_closed": _conv2_quarter_closed,
         "dense1_half_closed": _dense1_half_closed, "zero_image": _zero_image}


@pytest.mark.gpu
@pytest.mark.parametrize("b", [1, 8])
@pytest.mark.parametrize("case", sorted(EDGES))
def test_fused_bwd_edges_match_fp64(cuda, case, b):
    X, Y, params, layout, W, G, idx, step = _setup(cuda, b, mutate=EDGES[case])
    assert step.fused_bwd
    step.forward_backward(b)
    step.finalize(False)
    torch.cuda.synchronize()
    ids = idx[b:2 * b].long()
    x, y = X[ids], Y[ids]
    if case == "zero_image":
        assert not x[0].any() and (b == 1 or x[1:].any())
    p = [t.double().clone().requires_grad_(True) for t in params]
    loss, logits, ce = M.reference_loss(p, x.double(), y, 1)
    loss.backward()
    if case == "conv1_bias_closed":
        assert not p[0].grad[..., ::2].any() and not p[1].grad[::2].any()  # (the case does what it says)
    if case == "conv2_quarter_closed":
        assert not p[2].grad[..., 16:32].any() and not p[3].grad[16:32].any()
    got = layout.views(G.cpu())
    for (name, _), t, gg in zip(M.MNIST_CNN_VARIABLES, p, got):
        gr = t.grad
        err = (gg.double() - gr).abs().max().item()
        scale = gr.abs().max().item() + 1e-12
        assert err <= 2e-5 * scale + 1e-9, f"{case} b={b} {name}: max err {err} vs scale {scale}"
    step.check()  # no in-kernel hand-off timed out
