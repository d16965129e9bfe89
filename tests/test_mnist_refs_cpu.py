"""mnist_refs.py checked on the CPU: the explicit f64 stages against autograd of the model's own reference
(models/mnist_cnn.py reference_loss), the conventions the GPU tests rely on (first maximum, quarter map,
the two part2 layouts), and the integer-coded generator's conditions (a) - (d) for every case that
test_mnist_exact_gpu.py runs."""
import numpy as np
import pytest
import torch

import mnist_refs as MR
from tensorflow_distributed_learning_amd.models import mnist_cnn as M


def _autograd(params, x, y, scale):
    p = [torch.from_numpy(np.asarray(t, np.float64)).clone().requires_grad_(True) for t in params]
    logits = M.reference_logits(p, torch.from_numpy(np.asarray(x, np.float64)))
    ce = torch.nn.functional.cross_entropy(logits, torch.from_numpy(np.asarray(y)).long(), reduction="none")
    (ce.sum() * scale).backward()
    return [t.grad.numpy() for t in p], logits.detach().numpy(), ce.detach().numpy()


def _close(got, want, what, rel=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max()
    assert err <= rel * max(np.abs(want).max(), 1e-300), f"{what}: {err} vs {np.abs(want).max()}"


def _random_case(b, seed):
    g = torch.Generator().manual_seed(seed)
    params = [t.double().numpy() for t in M.init_mnist_params(seed)]
    for i in (1, 3, 5, 7):
        params[i] = ((torch.rand(params[i].shape, generator=g, dtype=torch.float64) - 0.5) * 0.1).numpy()
    x = torch.rand(b, 28, 28, 1, generator=g, dtype=torch.float64).numpy()
    y = torch.randint(0, 10, (b,), generator=g).numpy()
    return params, x, y


@pytest.mark.parametrize("b,R", [(3, 1), (5, 2)])
def test_stages_match_autograd_random(b, R):
    params, x, y = _random_case(b, 3)
    scale = 1.0 / (b * R)
    S, AB = MR.step_ref(params, x, y, scale)
    grads, logits, ce = _autograd(params, x, y, scale)
    _close(S.logits, logits, "logits")
    _close(S.loss, ce, "loss")
    for (name, _), g, want in zip(M.MNIST_CNN_VARIABLES, S.grads, grads):
        _close(g, want, name)
    # the model's own loss scaling agrees with `scale`
    loss, _, _ = M.reference_loss([torch.from_numpy(p) for p in params], torch.from_numpy(x), torch.from_numpy(y), R)
    _close(S.loss.sum() * scale, loss.item(), "scaled loss")


def test_stages_match_autograd_integer_coded():
    """On integer-coded data the pools tie and ReLUs sit at exact zeros: the explicit routing (first maximum,
    masks > 0) is the one autograd takes.  The unsaturated head is compared (in f64 e^-128 is not 0); the
    saturated one differs from it by less than e^-128."""
    c = MR.Coded(8)
    x, y = c.chunk(1)
    S, AB = MR.step_ref(c.params, x, y, c.scale)
    assert S.tie1[:, :MR.LIVE, :MR.LIVE][S.P1[:, :MR.LIVE, :MR.LIVE] > 0].any() and S.tie2[S.P2 > 0].any()
    grads, logits, ce = _autograd(c.params, x, y, c.scale)
    assert np.array_equal(S.logits, logits)
    _close(S.loss, ce, "loss")
    for (name, _), g, want in zip(M.MNIST_CNN_VARIABLES, S.grads, grads):
        _close(g, want, name)
    Ss, _ = c.ref(1)
    assert np.abs(Ss.dL - S.dL).max() <= c.scale * np.exp(-128.0) * 10
    assert np.abs(Ss.loss - S.loss).max() <= np.exp(-128.0) * 10
    assert np.array_equal(Ss.correct, S.correct)


def test_abs_sums_dominate():
    params, x, y = _random_case(4, 5)
    S, AB = MR.step_ref(params, x, y, 0.25)
    for k in AB:
        if k == "grads":
            for g, a in zip(S.grads, AB.grads):
                assert (np.abs(g) <= a * (1 + 1e-12) + 1e-300).all()
        elif k in ("C1", "C2"):
            assert (np.abs(S[k]) <= AB[k] * (1 + 1e-12)).all(), k
        else:
            assert (np.abs(S[k]) <= AB[k] * (1 + 1e-12) + 1e-300).all(), k


def test_pool_first_maximum_and_routing():
    pre = np.zeros((1, 4, 4, 2))
    pre[0, :2, :2, 0] = [[5, 7], [7, 7]]   # first maximum: code 1
    pre[0, :2, 2:, 0] = [[1, 2], [3, 3]]   # code 2
    pre[0, 2:, :2, 0] = [[-4, -4], [-4, -4]]  # all equal: code 0
    pre[0, 2:, 2:, 0] = [[0, 1], [2, 9]]   # unique: code 3
    pre[0, :2, :2, 1] = [[-1, -3], [-1, -2]]  # negative tie: code 0
    mx, arg, tie = MR.pool_first_max(pre)
    assert arg[0, :, :, 0].tolist() == [[1, 2], [0, 3]] and mx[0, :, :, 0].tolist() == [[7, 3], [-4, 9]]
    assert tie[0, :, :, 0].tolist() == [[True, True], [True, False]]
    assert arg[0, 0, 0, 1] == 0 and tie[0, 0, 0, 1]
    # routing: the window's gradient lands on the cell dy*2 + dx names, and only there
    dP2 = np.zeros((1, 1600))
    A2 = np.zeros((1, 1600), np.uint8)
    for q, (ph, pw, c) in enumerate([(0, 0, 0), (1, 2, 5), (4, 4, 63), (2, 0, 17)]):
        f = (ph * 5 + pw) * 64 + c
        dP2[0, f], A2[0, f] = q + 1.0, q
    dC = MR.pool2_bwd(dP2, A2)
    assert dC.sum() == 10.0 and np.count_nonzero(dC) == 4
    assert dC[0, 0, 0, 0] == 1 and dC[0, 2, 5, 5] == 2 and dC[0, 9, 8, 63] == 3 and dC[0, 5, 1, 17] == 4
    dC1 = MR.pool1_bwd(np.full((1, 13, 13, 32), 2.0), np.ones((1, 13, 13, 32)), np.full((1, 13, 13, 32), 3, np.uint8))
    assert (dC1[0, 1::2, 1::2] == 2).all() and dC1.sum() == 2.0 * 169 * 32
    # closed ReLU masks pass nothing
    assert not MR.pool1_bwd(np.ones((1, 13, 13, 32)), np.zeros((1, 13, 13, 32)), np.zeros((1, 13, 13, 32), np.uint8)).any()


def test_quarter_map():
    f = np.arange(1600)
    q = MR.quarter_of_feature(f)
    assert all((q == c).sum() == 400 for c in range(4))
    assert (q == ((f % 64) // 16)).all() and q[15] == 0 and q[16] == 1 and q[63] == 3 and q[64] == 0
    rng = np.random.RandomState(0)
    P2, w3 = rng.rand(3, 1600), rng.randn(1600, 128)
    parts, ab = MR.dense1_parts(P2, w3)
    for c in range(4):
        ch = np.zeros((5, 5, 64))
        ch[:, :, 16 * c:16 * c + 16] = 1  # conv2 channels 16c .. 16c+15 of every window
        _close(parts[c], (P2 * ch.reshape(1600)) @ w3, f"quarter {c}")
    _close(parts.sum(0), P2 @ w3, "quarters add up")
    H, abH = MR.dense1(P2, w3, np.arange(128.0))
    _close(H, np.maximum(P2 @ w3 + np.arange(128.0), 0), "H")


def test_part_layouts():
    rng = np.random.RandomState(1)
    b = 3
    rows = rng.randint(-9, 10, (b, 289, 64)).astype(np.float32)
    plain = np.zeros(b * 73 * 256, np.float32)  # (the buffer is sized for the larger layout)
    plain[:rows.size] = rows.reshape(-1)
    assert np.array_equal(MR.part2_rows(plain, b, False), rows)
    quads = np.zeros((b, 292, 64), np.float32)
    quads[:, :289] = rows
    fused = quads.reshape(b, 73, 4, 64).transpose(0, 1, 3, 2).copy()  # [b][73][64][4]
    assert np.array_equal(MR.part2_rows(fused.reshape(-1), b, True), rows)
    fused[1, 72, 5, 2] = 1.0  # a padding row of the bias quad
    with pytest.raises(AssertionError):
        MR.part2_rows(fused.reshape(-1), b, True)
    p1 = rng.randint(-9, 10, (4 * b, 320)).astype(np.float32)
    assert np.array_equal(MR.part1_image(p1.reshape(-1), b, True), p1.reshape(b, 4, 320).sum(1))
    assert np.array_equal(MR.part1_image(p1.reshape(-1), b, False), p1[:2 * b].reshape(b, 2, 320).sum(1))


def test_argmax_checked():
    want = np.array([[0, 1, 2, 3]], np.uint8)
    pooled = np.array([[1.0, 0.0, 2.0, 0.0]])
    MR.argmax_checked(np.array([[0, 3, 2, 0]], np.uint8), want, pooled, "ok")  # free where the pooled value is 0
    with pytest.raises(AssertionError):
        MR.argmax_checked(np.array([[1, 1, 2, 3]], np.uint8), want, pooled, "wrong")
    with pytest.raises(AssertionError):
        MR.argmax_checked(np.array([[0, 4, 2, 3]], np.uint8), want, pooled, "range")


@pytest.mark.parametrize("b,R", MR.CODED_CASES)
def test_coded_inputs_meet_conditions(b, R):
    """(a) every abs sum (over the scale where dL enters) below 2^24, (b) logit gaps >= 128, (c) mispredicted
    images, (d) >= 5 % positive exact ties in both pools -- on every chunk the GPU tests use."""
    c = MR.coded(b, R)
    assert c.scale == 1.0 / c.global_batch and c.global_batch >= b * R and c.global_batch & (c.global_batch - 1) == 0
    assert set(np.unique(c.X)) == {0.0, 1.0, 2.0, 3.0} and (c.X == 0).mean() > 0.3
    w1, b1, w2, b2, w3, b3, w4, b4 = c.params
    assert np.abs(w1).max() == 2 and set(np.unique(w2)) == {-1.0, 0.0, 1.0} and set(np.unique(w3)) == {-1.0, 0.0, 1.0}
    assert len(np.unique(np.abs(w4))) == 1 and np.log2(np.abs(w4[0, 0])) % 1 == 0
    for bias in (b1, b2, b3, b4):
        assert bias.min() < 0 < bias.max() and (bias == np.round(bias)).all()
    assert len(set(c.idx.tolist())) == 3 * b
    for k in (range(3) if b <= 17 else (1,)):
        S, AB = MR.coded_ref(b, R, k)
        fig = c.check(S, AB)
        assert fig["fwd"] < 2 ** 24 and fig["bwd"] < 2 ** 24 and fig["gap"] >= 128
