"""Nothing reads P1 row / column 12 (conv1 outputs 24..25, input rows / columns 26..27), and the fused
MNIST step computes conv1 over the live 12 x 12 pool windows only: gradients at the edges of that
region vs fp64, invariance to the dead input border, run-to-run determinism."""
import pytest
import torch

from tensorflow_distributed_learning_amd.models import mnist_cnn as M

pytestmark = pytest.mark.gpu

N = 64  # images in the device-resident dataset of every test here


def _images(kind, g):
    X = torch.rand(N, 28, 28, 1, generator=g)
    if kind == "dense":
        return X
    lo, hi = (22, 26) if kind == "last" else (0, 4)
    band = torch.zeros(28, dtype=torch.bool)
    band[lo:hi] = True
    mask = band[:, None] | band[None, :]  # rows lo..hi-1 and columns lo..hi-1
    return X * mask[None, :, :, None]


def _setup(cuda, b, kind="dense", seed=0, X=None):
    g = torch.Generator().manual_seed(seed)
    Xg = _images(kind, g)
    if X is None:
        X = Xg
    Y = torch.randint(0, 10, (N,), generator=g, dtype=torch.int32)
    params = M.init_mnist_params(seed)
    for i in (1, 3, 5, 7):  # non-zero biases so bias paths are exercised
        params[i] = (torch.rand(params[i].shape, generator=g) - 0.5) * 0.1
    layout = M.mnist_layout()
    W = layout.pack(params, device=cuda)
    G = torch.zeros_like(W)
    idx = torch.randperm(N, generator=g)[: 3 * b].to(torch.int32)
    lr = torch.tensor([0.01], device=cuda)
    step = M.FusedMnistTrainStep(X.to(cuda), Y.to(cuda), idx.to(cuda), W, G, layout, b, 1, lr)
    return X, Y, params, layout, W, G, idx, step


def _check_step(step, X, Y, params, layout, G, idx, off, b):
    ids = idx[off:off + b].long()
    x, y = X[ids], Y[ids]
    p = [t.double().clone().requires_grad_(True) for t in params]
    loss, logits, ce = M.reference_loss(p, x.double(), y, 1)
    loss.backward()
    got = layout.views(G.cpu())
    for (name, _), t, gg in zip(M.MNIST_CNN_VARIABLES, p, got):
        gr = t.grad
        err = (gg.double() - gr).abs().max().item()
        scale = gr.abs().max().item() + 1e-12
        print(f"{name}: max err {err:.3e} scale {scale:.3e}")
        assert err <= 2e-5 * scale + 1e-9, f"{name}: max err {err} vs scale {scale}"
    m = step.metrics.cpu()
    assert abs(m[0].item() - ce.sum().item()) < 1e-3 * max(1.0, ce.sum().item())
    assert m[1].item() == (logits.argmax(1) == y.long()).sum().item()
    assert m[2].item() == b


@pytest.mark.parametrize("kind", ["last", "first", "dense"])
@pytest.mark.parametrize("b", [1, 8, 17])
@pytest.mark.parametrize("mode,fused", [("1", "1"), ("1", "0"), ("0", "1")])
def test_edge_gradients_match_fp64(cuda, monkeypatch, mode, fused, b, kind):
    """Images that are non-zero only in rows / columns 22..25 (the last live conv1 rows, P1 rows /
    columns 10..11), only in rows / columns 0..3, or everywhere: an off-by-one in a 12-wide tile
    map of the fused step moves a gradient here.  b = 8 runs the XCD
    block map, b = 1 and b = 17 the consecutive one."""
    monkeypatch.setenv("TDL_MNIST_DP2_FWD", mode)
    monkeypatch.setenv("TDL_MNIST_FUSED_BWD", fused)
    X, Y, params, layout, W, G, idx, step = _setup(cuda, b, kind)
    assert step.dp2_in_forward == (mode == "1")
    assert step.fused_bwd == (mode == "1" and fused == "1")
    off = b
    step.forward_backward(off)
    step.finalize(False)
    torch.cuda.synchronize()
    step.check()
    _check_step(step, X, Y, params, layout, G, idx, off, b)


def test_dead_input_border_is_never_read(cuda, monkeypatch):
    """Input rows / columns 26..27 feed only conv1 outputs 24..25 -> P1 row / column 12, which conv2
    and the second pool never use: large finite values there change no bit of G, the metrics or W."""
    monkeypatch.delenv("TDL_MNIST_DP2_FWD", raising=False)
    monkeypatch.delenv("TDL_MNIST_FUSED_BWD", raising=False)
    b = 8
    X = _images("dense", torch.Generator().manual_seed(0))
    X2 = X.clone()
    sign = torch.where(torch.rand(N, 28, 28, 1, generator=torch.Generator().manual_seed(1)) < 0.5, -1.0, 1.0)
    dead = torch.zeros(28, dtype=torch.bool)
    dead[26:] = True
    dead = (dead[:, None] | dead[None, :])[None, :, :, None].expand_as(X2)
    X2[dead] = (sign * 1e30)[dead]
    outs = []
    for x in (X, X2):
        _, _, _, _, W, G, _, step = _setup(cuda, b, X=x)
        assert step.fused_bwd
        step.forward_backward(0)
        step.finalize(True)
        torch.cuda.synchronize()
        step.check()
        bufs = step.buffers()
        outs.append((G.clone(), W.clone(), step.metrics[1:3].clone(), bufs["H"].clone(), bufs["dL"].clone(),
                     step.metrics[0].item()))
    assert bool(torch.isfinite(outs[1][0]).all())
    for u, v, name in zip(outs[0], outs[1], ("G", "W", "correct / sample counts", "H", "dlogits")):
        assert torch.equal(u, v), f"{name} depends on the dead input border"
    # The loss sum is the one value here that is not reproducible bit for bit between ANY two runs:
    # the heads of the b images add their loss terms with one f32 atomic each, in arrival order.
    # Every term is pinned bit for bit by the image's dlogits and dense1 output above; the sum may
    # differ by the reordering of b non-negative f32 terms: each order is within (b - 1) roundings
    # of 2^-24 of the sum from the exact sum, so two orders are within twice that of each other.
    l0, l1 = outs[0][5], outs[1][5]
    print(f"loss sums {l0!r} {l1!r}")
    assert abs(l0 - l1) <= 2 * (b - 1) * 2.0 ** -24 * max(l0, l1)


def test_three_steps_deterministic(cuda, monkeypatch):
    monkeypatch.delenv("TDL_MNIST_DP2_FWD", raising=False)
    monkeypatch.delenv("TDL_MNIST_FUSED_BWD", raising=False)
    b = 8
    ws = []
    for _ in range(2):
        _, _, _, _, W, G, _, step = _setup(cuda, b)
        assert step.fused_bwd
        for k in range(3):
            step.forward_backward(k * b)
            step.finalize(True)
        torch.cuda.synchronize()
        step.check()
        ws.append(W.clone())
    assert torch.equal(ws[0], ws[1])
