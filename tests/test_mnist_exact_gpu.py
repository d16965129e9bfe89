"""The fused MNIST-CNN train step (csrc/kernels/mnist_cnn.hip) against the explicit f64 reference of every
stage (mnist_refs.py): saved state, per-image partial slabs, gradients, SGD update and metrics.

Two kinds of test, neither with a measured tolerance:

* Integer-coded ("saturated") steps: pixels, weights and biases are small integers, lr and the loss scale
  powers of two, and every row's top logit leads by >= 128, so that the f32 softmax is exactly one-hot.
  Every sum the step can form, in any order, is then an integer multiple of the scale below 2^24 times it,
  and everything the kernels store must EQUAL the f64 reference (mnist_refs.Coded states the conditions
  (a) - (d); they are asserted on the host for every case before the comparison).

* Random real-valued data: each stage's output is compared element by element with the f64 reference of
  that stage computed from the KERNEL'S OWN stored input of the stage, within
  conv_refs.error_bound_f32(abs sum, terms of the reduction); the softmax stage's bound is derived in
  `softmax_bounds`.

Single process; the xGMI exchange finalize and non-finite inputs are not covered here."""
import numpy as np
import pytest
import torch

import conv_refs as CR
import f32_edge_helpers as FE
import mnist_refs as MR
import test_mnist_fused_gpu as TF
from tensorflow_distributed_learning_amd.models import mnist_cnn as M

pytestmark = pytest.mark.gpu

# (TDL_MNIST_DP2_FWD, TDL_MNIST_FUSED_BWD): one launch for forward + loss + backward; dP2 in the forward
# kernel and k_conv_bwd; the K5 launch for dP2 and k_conv_bwd
MODES = {"fused": ("1", "1"), "dp2fwd": ("1", "0"), "k5": ("0", "1")}


def _env(monkeypatch, mode, variant=None):
    monkeypatch.setenv("TDL_MNIST_DP2_FWD", MODES[mode][0])
    monkeypatch.setenv("TDL_MNIST_FUSED_BWD", MODES[mode][1])
    monkeypatch.delenv("TDL_SHARE_GPU", raising=False)
    monkeypatch.delenv("TDL_FX_GRID", raising=False)
    if variant is None:
        monkeypatch.delenv("TDL_MNIST_VARIANT", raising=False)
    else:
        monkeypatch.setenv("TDL_MNIST_VARIANT", str(variant))


def _named_mode(cuda, step, mode, b):
    """The step runs what the case names (dP2 in the forward needs all 4b workgroups resident at once)."""
    fits = 4 * b <= torch.cuda.get_device_properties(cuda).multi_processor_count
    assert step.dp2_in_forward == (MODES[mode][0] == "1" and fits), (mode, b)
    assert step.fused_bwd == (mode == "fused" and fits), (mode, b)


def _coded_step(cuda, monkeypatch, b, R, mode, variant=None):
    _env(monkeypatch, mode, variant)
    c = MR.coded(b, R)
    layout = M.mnist_layout()
    params = [torch.from_numpy(p).float() for p in c.params]
    W = layout.pack(params, device=cuda)
    G = torch.zeros_like(W)
    lr = torch.tensor([c.lr], device=cuda)
    X = torch.from_numpy(c.X).float().to(cuda)
    Y = torch.from_numpy(c.Y).to(cuda)
    step = M.FusedMnistTrainStep(X, Y, torch.from_numpy(c.idx).to(cuda), W, G, layout, b, R, lr,
                                 global_batch=c.global_batch)
    _named_mode(cuda, step, mode, b)
    return c, layout, W, G, step


def _poison(step, names):
    bufs = step.buffers()
    for n in names:
        t = bufs[n]
        t.fill_(0xFF if t.dtype == torch.uint8 else float("nan"))


def _views(step, b):
    B = {k: v.cpu() for k, v in step.buffers().items()}
    return dict(P1=B["P1"].view(b, 13, 13, 32)[:, :MR.LIVE, :MR.LIVE], A1=B["A1"].view(b, 13, 13, 32)[:, :MR.LIVE, :MR.LIVE],
                P2=B["P2"].view(b, 1600), A2=B["A2"].view(b, 1600), H=B["H"].view(b, 128), dH=B["dH"].view(b, 128),
                dP2=B["dP2"].view(b, 1600), dL=B["dL"].view(b, 32), part3=B["part3"].view(4, b, 128),
                part2=B["part2"], part1=B["part1"])


def _exact_saved(step, S, b, fused, what):
    """The saved state and per-image partials of a training step, bit for bit."""
    V = _views(step, b)
    live = (slice(None), slice(0, MR.LIVE), slice(0, MR.LIVE))
    FE.same_bits(V["P2"], S.P2, what + " P2")
    FE.same_bits(V["H"], S.H, what + " H")
    FE.same_bits(V["dL"][:, :10], S.dL, what + " dL")
    assert not V["dL"][:, 10:].any(), what + ": dL row padding written"
    FE.same_bits(V["dH"], S.dH, what + " dH")
    if not fused:  # the fused backward keeps these in LDS
        FE.same_bits(V["P1"], S.P1[live], what + " P1")
        MR.argmax_checked(V["A1"].numpy(), S.A1[live], S.P1[live], what + " A1")
        MR.argmax_checked(V["A2"].numpy(), S.A2, S.P2, what + " A2")
        FE.same_bits(V["dP2"], S.dP2, what + " dP2")
    p2 = MR.part2_rows(V["part2"], b, fused)
    assert np.array_equal(p2, S.part2), f"{what} part2: images {sorted(set(np.argwhere(p2 != S.part2)[:, 0].tolist()))[:8]}, " \
                                        f"first at (image, row, column) {np.argwhere(p2 != S.part2)[0].tolist()}"
    p1 = MR.part1_image(V["part1"], b, fused)
    assert np.array_equal(p1, S.part1), f"{what} part1: first at (image, column) {np.argwhere(p1 != S.part1)[0].tolist()}"


def _exact_grads(layout, G, S, what):
    for (name, _), got, want in zip(M.MNIST_CNN_VARIABLES, layout.views(G.cpu()), S.grads):
        FE.same_bits(got, want, f"{what} {name}")


def _exact_metrics(step, S, b, what):
    m = step.metrics.cpu().double().numpy()
    assert S.loss.sum() < 2 ** 24  # integers: the order of the atomic adds does not matter
    assert m[0] == S.loss.sum() and m[1] == S.correct.sum() and m[2] == b, (what, m, S.loss.sum(), S.correct.sum())


def _run_exact(cuda, monkeypatch, b, R, mode, split=False, variant=None):
    c, layout, W, G, step = _coded_step(cuda, monkeypatch, b, R, mode, variant)
    S, AB = MR.coded_ref(b, R, 1)  # asserts the conditions (a) - (d)
    fused = step.fused_bwd and not split
    what = f"b={b} R={R} {mode}{' split' if split else ''}{'' if variant is None else f' variant {variant}'}"
    W0 = W.clone()
    _poison(step, ["P2", "H", "dH", "part1", "part2"] + ([] if fused else ["P1", "A1", "A2", "dP2"]))
    off = b  # chunk 1
    if split:
        step.forward_dense(off)
        _exact_grads_dense = [g.clone() for g in layout.views(G)[4:]]  # final before the conv backward
        step.backward_conv()
    else:
        step.forward_backward(off)
    step.finalize(False)
    torch.cuda.synchronize()
    step.check()
    assert torch.equal(W, W0), what + ": finalize(False) changed W"
    _exact_saved(step, S, b, fused, what)
    _exact_grads(layout, G, S, what)
    _exact_metrics(step, S, b, what)
    if split:
        for (name, _), got, want in zip(M.MNIST_CNN_VARIABLES[4:], _exact_grads_dense, S.grads[4:]):
            FE.same_bits(got, want, f"{what} {name} after forward_dense")

    # ---- the SGD update from the same partials, with and without the gradient store
    want_W = [p - c.lr * g for p, g in zip(c.params, S.grads)]
    for keep in (True, False):
        # (the fused finalize of a single replica skips the gradient store; with R > 1 and no exchange the
        # all-reduce still reads G, and k_finalize always writes it)
        skip_g = fused and R == 1 and not keep
        W.copy_(W0)
        if skip_g:
            G.fill_(123.0)
        step.finalize(True, keep_grad=keep)
        torch.cuda.synchronize()
        for (name, _), got, want in zip(M.MNIST_CNN_VARIABLES, layout.views(W.cpu()), want_W):
            FE.same_bits(got, want, f"{what} SGD keep_grad={keep} {name}")
        if skip_g:
            assert bool((G == 123.0).all()), what + ": keep_grad=False wrote G"
        else:
            _exact_grads(layout, G, S, what + f" keep_grad={keep}")
    W.copy_(W0)

    # ---- forward only: features (part3, saved activations) and evaluation (logits, metrics)
    _poison(step, ["P1", "A1", "P2", "A2", "part3"])
    step._impl.forward_features(off)
    torch.cuda.synchronize()
    V = _views(step, b)
    live = (slice(None), slice(0, MR.LIVE), slice(0, MR.LIVE))
    FE.same_bits(V["part3"], S.part3, what + " part3 (features)")
    FE.same_bits(V["P1"], S.P1[live], what + " P1 (features)")
    MR.argmax_checked(V["A1"].numpy(), S.A1[live], S.P1[live], what + " A1 (features)")
    FE.same_bits(V["P2"], S.P2, what + " P2 (features)")
    MR.argmax_checked(V["A2"].numpy(), S.A2, S.P2, what + " A2 (features)")
    step.metrics.zero_()
    logits = torch.full((b * 10,), float("nan"), device=cuda)
    step.forward_eval(off, logits)
    torch.cuda.synchronize()
    FE.same_bits(logits.view(b, 10), S.logits, what + " logits (eval)")
    _exact_metrics(step, S, b, what + " eval")
    step.check()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("b", [1, 8, 16, 17, 64])
def test_exact_step(cuda, monkeypatch, b, mode):
    _run_exact(cuda, monkeypatch, b, 1, mode)


@pytest.mark.parametrize("b", [65, 128, 129, 256])
def test_exact_step_large_batch(cuda, monkeypatch, b):
    """Past 4b = CUs dP2 cannot run in the forward kernel (whatever TDL_MNIST_DP2_FWD asks for): K5 and
    k_conv_bwd, and k_finalize's second and later trips over the partial slabs (64 images / 128 part1 rows
    a trip; b = 65: a trip of a single image; b = 256: the binding's maximum)."""
    _run_exact(cuda, monkeypatch, b, 1, "fused")


@pytest.mark.parametrize("mode", sorted(MODES))
def test_exact_step_two_replicas(cuda, monkeypatch, mode):
    _run_exact(cuda, monkeypatch, 8, 2, mode)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("b", [17, 64])
def test_exact_step_split(cuda, monkeypatch, b, mode):
    """forward_dense / backward_conv (the R > 1 engine path): the dense gradients are final in G before
    the conv backward runs, the conv backward is k_conv_bwd in every mode."""
    _run_exact(cuda, monkeypatch, b, 2, mode, split=True)


@pytest.mark.parametrize("mode", ["fused", "dp2fwd"])
def test_exact_step_consecutive_block_map(cuda, monkeypatch, mode):
    """TDL_MNIST_VARIANT=0: workgroup -> (image, quarter) by consecutive block ids instead of the default
    XCD-aware map (which b % 8 == 0 enables; the b = 8 / 16 / 64 cases above run it)."""
    _run_exact(cuda, monkeypatch, 8, 1, mode, variant=0)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_exact_consecutive_steps(cuda, monkeypatch, mode):
    """Three forward_backward + finalize(False) on ONE step object at different idx offsets: the hand-off
    tags advance, the partial slabs hold the previous step's values, and each step is still exact."""
    b = 8
    c, layout, W, G, step = _coded_step(cuda, monkeypatch, b, 1, mode)
    for k in (2, 0, 1):
        S, AB = MR.coded_ref(b, 1, k)
        step.metrics.zero_()
        step.forward_backward(k * b)
        step.finalize(False)
        torch.cuda.synchronize()
        what = f"{mode} chunk {k}"
        _exact_saved(step, S, b, step.fused_bwd, what)
        _exact_grads(layout, G, S, what)
        _exact_metrics(step, S, b, what)
    step.check()


# ------------------------------------------------------------------------------------------- random data, stage by stage
def _within(got, want, bound, what):
    g = got.detach().cpu().double().numpy() if hasattr(got, "detach") else np.asarray(got, np.float64)
    want, bound = np.asarray(want, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(want))
    assert g.shape == want.shape, (what, g.shape, want.shape)
    err = np.abs(g - want)
    bad = np.argwhere(~(err <= bound))
    assert len(bad) == 0, f"{what}: {len(bad)} of {g.size} outside the bound, first at {tuple(bad[0])}: got " \
                          f"{g[tuple(bad[0])]}, want {want[tuple(bad[0])]}, bound {bound[tuple(bad[0])]}"
    return float((err / np.maximum(bound, 1e-300)).max())


def _window_max(e):
    """The largest of a per-cell bound over each 2 x 2 pool window: |max a - max b| <= max |a - b|."""
    b, H, W, C = e.shape
    return np.stack([e[:, dy:2 * (H // 2):2, dx:2 * (W // 2):2] for dy in (0, 1) for dx in (0, 1)]).max(0)


def _pool_stage(got_P, got_A, pre, P, A, ab, terms, what):
    """A conv + pool stage: the pooled value within the window's bound (the ReLU and the maximum are
    1-Lipschitz); the argmax equal where the reference's maximum is unique and positive by more than twice
    that bound."""
    e = _window_max(CR.error_bound_f32(ab, terms))
    e = e.reshape(P.shape)
    _within(got_P, P, e, what)
    b, H, W, C = pre.shape
    win = np.sort(np.stack([pre[:, dy:2 * (H // 2):2, dx:2 * (W // 2):2] for dy in (0, 1) for dx in (0, 1)]), axis=0)
    sure = ((win[3] - win[2]).reshape(P.shape) > 2 * e) & (P > 2 * e)
    assert sure.mean() > 0.3, what  # (the comparison is not vacuous)
    ga = got_A.numpy() if hasattr(got_A, "numpy") else got_A
    assert (ga < 4).all() and np.array_equal(ga[sure], A[sure]), f"{what}: argmax differs in a decided window"


def softmax_bounds(H, w4, b4, y, scale):
    """Bounds of the loss head's outputs given its stored input H (f64 view of the kernel's f32 values):
    (reference loss [b], its bound [b], reference dL [b,10], its bound [b,10], e_lg [b,10]).

    With u = 2^-24 (an f32 rounding is relative u; a "1 ulp" instruction relative 2u):

    * logits: lg' = lg + a, |a| <= e_lg = error_bound_f32(sum |H||w4| + |b4|, 129); the row maximum moves by
      at most E = max_c e_lg.
    * t' = fl(lg'_c - m'): |t' - t| <= d = e_lg + E + u (|t| + e_lg + E).
    * __expf(t') = v_exp_f32(fl(t' * fl(log2 e))): the constant and the product are rounded once each, so the
      exponent is t' (1 + th), |th| <= 2u (1 + u): PROPORTIONAL TO |t'|; v_exp_f32 is 1 ulp (ISA guide) and
      flushes results below 2^-126.  e' = exp(t + eta) (1 + 2u') + 2^-126 with |eta| <= d + (|t| + d) 2u(1 + u),
      i.e. relative rho_c = expm1(eta) (1 + 2u) + 2u.
    * se' = the f32 sum of ten non-negative terms: |se' - se| <= D + 10 u (se + D), D = sum e_c rho_c + 10 * 2^-126;
      rho_se = that / se.
    * inv' = fl(1 / se') (correctly rounded by default; 1 ulp granted): relative rho_inv = rho_se / (1 - rho_se) + 2u.
    * p' = fl(e' inv'): |p' - p| <= dp = p ((1 + rho_c)(1 + rho_inv)(1 + u) - 1) + 2^-126.
    * dL' = fl(fl(p' - 1hot) scale): <= scale (dp + 2u (|p - 1hot| + dp)) + 2^-149 (a denormal product).
    * loss' = fl(fl(m' + fl(v_log_f32(se') fl(ln 2))) - lg'_y): |m' - m| <= E; ln se' - ln se <= rho_se / (1 - rho_se);
      v_log_f32 1 ulp and the ln 2 constant and product: 4u |ln se'|; lg'_y: e_lg[y]; the two roundings
      u (|lse| + |loss|), doubled for the perturbed operands.
    Nothing here is fitted to an observed error."""
    u = 2.0 ** -24
    lg, ab = MR.dense2(H, w4, b4)
    e_lg = CR.error_bound_f32(ab, 129)
    loss, correct, dL = MR.softmax_xent(lg, y, scale)
    rows = np.arange(lg.shape[0])
    E = e_lg.max(1, keepdims=True)
    m = lg.max(1, keepdims=True)
    t = lg - m
    d = e_lg + E + u * (np.abs(t) + e_lg + E)
    eta = d + (np.abs(t) + d) * 2 * u * (1 + u)
    rho = np.expm1(eta) * (1 + 2 * u) + 2 * u
    e = np.exp(t)
    se = e.sum(1, keepdims=True)
    D = (e * rho).sum(1, keepdims=True) + 10 * 2.0 ** -126
    rho_se = (D + 10 * u * (se + D)) / se
    assert (rho_se < 0.01).all()
    rho_inv = rho_se / (1 - rho_se) + 2 * u
    p = e / se
    dp = p * ((1 + rho) * (1 + rho_inv) * (1 + u) - 1) + 2.0 ** -126
    onehot = np.zeros_like(lg)
    onehot[rows, np.asarray(y).astype(np.int64)] = 1.0
    e_dL = scale * (dp + 2 * u * (np.abs(p - onehot) + dp)) + 2.0 ** -149
    lnse = np.log(se)[:, 0]
    e_loss = (E[:, 0] + (rho_se / (1 - rho_se))[:, 0] + 4 * u * (lnse + 0.01) + e_lg[rows, np.asarray(y).astype(np.int64)]
              + 2 * u * (np.abs(m[:, 0]) + lnse + np.abs(loss) + 1.0))
    return loss, e_loss, dL, e_dL, e_lg


def _stage_checks(cuda, step, X, Y, params, layout, G, idx, off, b, R, P1_in, A1_in):
    """The stage-wise bounds on what a training step stored.  P1_in / A1_in: the kernel's own P1 / A1 (stored
    by the step without the fused backward, by a forward_features launch of the same rows with it)."""
    ids = idx[off:off + b].long()
    x, y = X[ids].double().numpy(), Y[ids].numpy()
    w1, b1, w2, b2, w3, b3, w4, b4 = [MR.f64(p) for p in params]
    scale = float(np.float32(1.0 / (b * R)))  # (the step holds 1 / global batch as an f32)
    B = {k: v.cpu() for k, v in step.buffers().items()}
    fused = step.fused_bwd
    P1, A1 = P1_in.double().numpy(), A1_in.numpy()
    P2 = B["P2"].view(b, 1600).double().numpy()
    H = B["H"].view(b, 128).double().numpy()
    dH = B["dH"].view(b, 128).double().numpy()
    dLk = B["dL"].view(b, 32)[:, :10].double().numpy()

    # conv1 + pool 1 from X (9 products + the bias) over the live windows; the dead border holds zeros
    live = (slice(None), slice(0, MR.LIVE), slice(0, MR.LIVE))
    pre1, P1r, A1r, ab1, _ = MR.conv1_pool(x, w1, b1)
    _pool_stage(P1[live], A1[live], pre1[:, :24, :24], P1r[live], A1r[live], ab1[:, :24, :24], 10, "P1 / A1 from X")
    assert not P1[:, 12].any() and not P1[:, :, 12].any() and not A1[:, 12].any() and not A1[:, :, 12].any()
    # conv2 + pool 2 from the stored P1 (288 products + the bias)
    pre, P2r, A2r, ab, _ = MR.conv2_pool(P1, w2, b2)
    e2 = _window_max(CR.error_bound_f32(ab, 289)).reshape(b, 1600)
    _within(P2, P2r, e2, "P2 from P1")
    # dense1 from the stored P2 (1600 products + the bias), the loss head from the stored H
    Hr, abH = MR.dense1(P2, w3, b3)
    _within(H, Hr, CR.error_bound_f32(abH, 1601), "H from P2")
    loss, e_loss, dLr, e_dL, e_lg = softmax_bounds(H, w4, b4, y, scale)
    _within(dLk, dLr, e_dL, "dL from H")
    m = step.metrics.cpu().double().numpy()
    e_sum = e_loss.sum() + b * 2.0 ** -24 * (loss.sum() + e_loss.sum())  # + the b atomic adds
    print(f"loss sum {m[0]!r} vs {loss.sum()!r}: error {abs(m[0] - loss.sum()):.3e}, bound {e_sum:.3e}")
    assert abs(m[0] - loss.sum()) <= e_sum, (m[0], loss.sum(), e_sum)
    lg, _ = MR.dense2(H, w4, b4)
    top2 = np.sort(lg, 1)[:, -2:]
    decided = (top2[:, 1] - top2[:, 0]) > 2 * e_lg.max(1)
    hit = lg.argmax(1) == y
    assert (hit & decided).sum() <= m[1] <= (hit & decided).sum() + (~decided).sum() and m[2] == b
    # dense2 / dense1 backward from the stored dL, H, dH, P2
    dHr, abd = MR.dense2_bwd(dLk, H, w4)
    _within(dH, dHr, CR.error_bound_f32(abd, 10), "dH from dL, H")
    (dW3, db3, dW4, db4), (a3, ab3, a4, ab4) = MR.dense_wgrads(P2, H, dH, dLk)
    got = layout.views(G.cpu())
    for name, g, want, a in (("dW3", got[4], dW3, a3), ("db3", got[5], db3, ab3), ("dW4", got[6], dW4, a4),
                             ("db4", got[7], db4, ab4)):
        _within(g, want, CR.error_bound_f32(a, b), f"{name} from the stored P2 / H / dH / dL")
    if fused:
        return
    # ---- without the fused backward every stage's input is stored
    A2 = B["A2"].view(b, 1600).numpy()
    dP2 = B["dP2"].view(b, 1600).double().numpy()
    _pool_stage(P2.reshape(b, 5, 5, 64), A2.reshape(b, 5, 5, 64), pre, P2r.reshape(b, 5, 5, 64),
                A2r.reshape(b, 5, 5, 64), ab, 289, "P2 / A2 from P1")
    dP2r, abp = MR.dense1_bwd(dH, P2, w3)
    _within(dP2, dP2r, CR.error_bound_f32(abp, 128), "dP2 from dH, P2")
    # conv backward from the stored dP2 / A2 / P1 / A1: dW2 over the 100 positions
    dC2 = MR.pool2_bwd(dP2, A2)
    p2r, abw2 = MR.conv2_wgrad(P1, dC2)
    _within(MR.part2_rows(B["part2"], b, False), p2r, CR.error_bound_f32(abw2, 100), "part2 from dP2, A2, P1")
    # dW1: dP1 (9 taps x 64 channels) carries its own error e_v into the sum over the 144 live pixels:
    # |dw' - dw| <= sum |x| e_v + error_bound_f32(sum |x| (|v| + e_v), 144)
    dP1, abp1 = MR.conv2_dgrad(dC2, w2)
    e_v = CR.error_bound_f32(abp1, 576)
    p1r, abw1, thru = MR.conv1_wgrad(x, MR.pool1_bwd(dP1, P1, A1), MR.pool1_bwd(e_v, P1, A1))
    _within(MR.part1_image(B["part1"], b, False), p1r, thru + CR.error_bound_f32(abw1 + thru, 144),
            "part1 from dP2, A2, P1, A1, X")
    # the finalize's sums over the images, from the stored partials
    s2 = MR.part2_rows(B["part2"], b, False)
    s1 = MR.f64(B["part1"]).reshape(-1)[:2 * b * 320].reshape(2 * b, 320)
    _within(torch.cat([got[2].reshape(288, 64), got[3].reshape(1, 64)]), s2.sum(0),
            CR.error_bound_f32(np.abs(s2).sum(0), b), "dW2 / db2 from part2")
    _within(torch.cat([got[0].reshape(288), got[1]]), s1.sum(0), CR.error_bound_f32(np.abs(s1).sum(0), 2 * b),
            "dW1 / db1 from part1")


@pytest.mark.parametrize("mode", ["dp2fwd", "k5"])
@pytest.mark.parametrize("b,R", [(8, 1), (17, 2)])
def test_stages_random_unfused(cuda, monkeypatch, b, R, mode):
    _env(monkeypatch, mode)
    X, Y, params, layout, W, G, idx, lr, step = TF._setup(cuda, b, R)
    _named_mode(cuda, step, mode, b)
    off = b
    step.forward_backward(off)
    step.finalize(False)
    torch.cuda.synchronize()
    step.check()
    P1 = step.buffers()["P1"].cpu().view(b, 13, 13, 32)
    A1 = step.buffers()["A1"].cpu().view(b, 13, 13, 32)
    _stage_checks(cuda, step, X, Y, params, layout, G, idx, off, b, R, P1, A1)
    # part3 (stored by a forward-only launch) from the stored P2: 400 products per quarter
    P2 = step.buffers()["P2"].cpu().view(b, 1600).double().numpy()
    step._impl.forward_features(off)
    torch.cuda.synchronize()
    assert np.array_equal(step.buffers()["P2"].cpu().view(b, 1600).double().numpy(), P2)  # (the same forward)
    parts, abq = MR.dense1_parts(P2, params[4])
    _within(step.buffers()["part3"].cpu().view(4, b, 128), parts, CR.error_bound_f32(abq, 400), "part3 from P2")


@pytest.mark.parametrize("b,R", [(8, 1), (17, 2)])
def test_stages_random_fused(cuda, monkeypatch, b, R):
    """The fused step stores P2, H, dH, dL and the dense gradients (its conv gradients are covered by the
    exact test and the golden file).  Its conv1 output stays in LDS: P1 / A1 are those a
    forward_features launch of the same rows stored (the same conv1 code on the same inputs), checked against X,
    and P2 is checked against that P1."""
    _env(monkeypatch, "fused")
    X, Y, params, layout, W, G, idx, lr, step = TF._setup(cuda, b, R)
    _named_mode(cuda, step, "fused", b)
    off = b
    step._impl.forward_features(off)
    torch.cuda.synchronize()
    P1 = step.buffers()["P1"].cpu().view(b, 13, 13, 32).clone()
    A1 = step.buffers()["A1"].cpu().view(b, 13, 13, 32).clone()
    _poison(step, ["P2", "H", "dH"])
    step.forward_backward(off)
    step.finalize(False)
    torch.cuda.synchronize()
    step.check()
    _stage_checks(cuda, step, X, Y, params, layout, G, idx, off, b, R, P1, A1)
