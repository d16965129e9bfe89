"""The references of tests/kernel_refs.py against independent implementations (no GPU): bf16_rne bit for
bit against torch's f32 -> bf16 conversion, the f64 optimizer updates against the optimizers' torch
formulas (keras/optimizers.py on CPU tensors), the cross-entropy references against torch in f64."""
import numpy as np
import pytest
import torch

import kernel_refs as R
from tensorflow_distributed_learning_amd.engine.slab import SlabLayout, VarSpec, transpose_tables
from tensorflow_distributed_learning_amd.keras import optimizers as O


def _torch_bf16_bits(x: np.ndarray) -> np.ndarray:
    return torch.from_numpy(x.copy()).bfloat16().view(torch.int16).numpy().view(np.uint16)


def test_bf16_rne_random_finite_bitwise():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(100000) * 2.0 ** rng.integers(-60, 60, 100000)).astype(np.float32)
    assert np.isfinite(x).all()
    np.testing.assert_array_equal(R.bf16_rne(x), _torch_bf16_bits(x))


def test_bf16_rne_special_values_bitwise():
    x = R.SPECIALS_F32
    got = R.bf16_rne(x)
    np.testing.assert_array_equal(got, _torch_bf16_bits(x))
    u = x.view(np.uint32)
    # the halfway cases by hand: ties go to the even bf16, in both directions and both signs
    for bits, want in [(0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0xBF808000, 0xBF80), (0xBF818000, 0xBF82),
                       (0x3F808001, 0x3F81), (0x3F807FFF, 0x3F80), (0x7F7F8000, 0x7F80), (0x7F7F7FFF, 0x7F7F),
                       (0x00000001, 0x0000), (0x80000001, 0x8000), (0x00008000, 0x0000), (0x00018000, 0x0002)]:
        assert got[np.nonzero(u == bits)[0][0]] == want, hex(bits)


def test_bf16_rne_keeps_nan():
    got = R.bf16_rne(R.NAN_PAYLOADS_F32)
    assert R.bf16_is_nan(got).all(), [hex(v) for v in got]
    assert np.isnan(R.bf16_bits_to_f64(got)).all()
    assert torch.from_numpy(R.NAN_PAYLOADS_F32.copy()).bfloat16().isnan().all()
    # the sign survives
    assert (got >> 15).tolist() == [0, 0, 1]


def _run_both(opt, step_ref, state0, n=4099, steps=3, lr_change=None):
    """opt: a keras optimizer run on CPU tensors (its torch formulas); step_ref(w, g, state, t) -> (w, state)."""
    rng = np.random.default_rng(1)
    w0 = rng.standard_normal(n).astype(np.float32)
    W = torch.from_numpy(w0.copy())
    w, state = w0.astype(np.float64), state0(n)
    for t in range(1, steps + 1):
        g = (rng.standard_normal(n) * 0.1).astype(np.float32)
        opt.apply_flat(W, torch.from_numpy(g.copy()))
        w, state = step_ref(w, g.astype(np.float64), state, t)
    np.testing.assert_allclose(W.numpy(), w, rtol=1e-4, atol=1e-6)
    return opt, state


@pytest.mark.parametrize("momentum,nesterov", [(0.0, False), (0.9, False), (0.9, True)])
def test_sgd_ref_matches_torch_formulas(momentum, nesterov):
    opt = O.SGD(0.05, momentum=momentum, nesterov=nesterov)

    def step(w, g, v, t):
        return R.sgd_ref(w, g, 0.05, v, momentum, nesterov)

    opt, v = _run_both(opt, step, lambda n: np.zeros(n) if momentum > 0 else None)
    if momentum > 0:
        np.testing.assert_allclose(opt.slots()["momentum"].numpy(), v, rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_ref_matches_torch_formulas(amsgrad, wd):
    opt = O.AdamW(0.01, weight_decay=wd, amsgrad=amsgrad) if wd else O.Adam(0.01, amsgrad=amsgrad)

    def step(w, g, st, t):
        w, m, v, vh = R.adam_ref(w, g, st[0], st[1], st[2], 0.01, t, 0.9, 0.999, 1e-7, wd)
        return w, (m, v, vh)

    opt, (m, v, vh) = _run_both(opt, step, lambda n: (np.zeros(n), np.zeros(n), np.zeros(n) if amsgrad else None))
    np.testing.assert_allclose(opt.slots()["m"].numpy(), m, rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(opt.slots()["v"].numpy(), v, rtol=1e-4, atol=1e-10)
    if amsgrad:
        np.testing.assert_allclose(opt.slots()["vhat"].numpy(), vh, rtol=1e-4, atol=1e-10)


@pytest.mark.parametrize("momentum", [0.0, 0.8])
@pytest.mark.parametrize("centered", [False, True])
def test_rmsprop_ref_matches_torch_formulas(momentum, centered):
    opt = O.RMSprop(0.01, rho=0.9, momentum=momentum, epsilon=1e-7, centered=centered)

    def step(w, g, st, t):
        w, rms, mom, mg, _ = R.rmsprop_ref(w, g, st[0], st[1], st[2], 0.01, 0.9, momentum, 1e-7)
        return w, (rms, mom, mg)

    opt, (rms, mom, mg) = _run_both(
        opt, step, lambda n: (np.zeros(n), np.zeros(n) if momentum > 0 else None, np.zeros(n) if centered else None))
    np.testing.assert_allclose(opt.slots()["rms"].numpy(), rms, rtol=1e-4, atol=1e-10)
    if momentum > 0:
        np.testing.assert_allclose(opt.slots()["mom"].numpy(), mom, rtol=1e-4, atol=1e-7)
    if centered:
        np.testing.assert_allclose(opt.slots()["mg"].numpy(), mg, rtol=1e-4, atol=1e-8)


def test_adagrad_ref_matches_torch_formulas():
    opt = O.Adagrad(0.05, initial_accumulator_value=0.1, epsilon=1e-7)

    def step(w, g, acc, t):
        return R.adagrad_ref(w, g, acc, 0.05, 1e-7)

    opt, acc = _run_both(opt, step, lambda n: np.full(n, R.f32(0.1)))
    np.testing.assert_allclose(opt.slots()["acc"].numpy(), acc, rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("scale,offset", [(3.0, 0.0), (30.0, 0.0), (1.0, 1e4)])
def test_xent_refs_match_torch_f64(scale, offset):
    rng = np.random.default_rng(2)
    N, K = 37, 65
    z = (rng.standard_normal((N, K)) * scale + offset).astype(np.float32)
    y = rng.integers(0, K, N)
    y[3], y[5] = -1, K  # out of range: no loss, no one-hot term
    loss, lse, p, dz = R.xent_ref(z, y)
    zt = torch.from_numpy(z).double().requires_grad_(True)
    ok = torch.from_numpy((y >= 0) & (y < K))
    yt = torch.from_numpy(np.where((y >= 0) & (y < K), y, 0))
    lt = torch.nn.functional.cross_entropy(zt, yt, reduction="none") * ok
    np.testing.assert_allclose(loss, lt.detach().numpy(), rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(lse, torch.logsumexp(zt, 1).detach().numpy(), rtol=1e-13)
    lt.sum().backward()
    want = zt.grad.numpy().copy()
    sm = torch.softmax(zt.detach(), 1).numpy()
    want[~ok.numpy()] = sm[~ok.numpy()]
    np.testing.assert_allclose(dz, want, rtol=1e-10, atol=1e-15)
    # the f32 emulation is the same function at f32 precision: errors of a few ulp of |z|
    el, elg, edz = R.xent_emul_f32(z, y)
    bound = 8 * R.ulp32(np.abs(z).max()) + 1e-6
    assert np.abs(elg - lse).max() <= bound and np.abs(el - loss).max() <= bound
    assert np.abs(edz - dz).max() <= 64 * R.ulp32(np.abs(z).max()) + 1e-6


def test_transpose_tables_cover_every_conv_kernel_once():
    specs = [VarSpec("k1", (3, 3, 1, 32)), VarSpec("b1", (32,)), VarSpec("k2", (7, 7, 3, 64)), VarSpec("d", (5, 3)),
             VarSpec("k3", (1, 1, 64, 256))]
    layout = SlabLayout(specs, align=1)
    entries, tiles = transpose_tables(layout.specs, layout.offsets)
    assert entries == [[0, 0, 9, 32], [320, 320, 147, 64], [320 + 9408 + 15, 320 + 9408 + 15, 64, 256]]
    for e, (_, _, r, k) in enumerate(entries):
        mine = sorted((a, b) for ee, a, b, z in tiles if ee == e and z == 0)
        assert mine == [(a, b) for a in range((r + 63) // 64) for b in range((k + 63) // 64)]
    assert len(tiles) == 1 + 3 + 4


# ------------------------------------------------------------------------------------- batch norm
def _bn_case(M, C, seed=0, mean=0.5, std=2.0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((M, C)) * std + mean).astype(np.float32)
    dy = rng.standard_normal((M, C)).astype(np.float32)
    res = rng.standard_normal((M, C)).astype(np.float32)
    g = (rng.random(C) + 0.5).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    mm, mv = rng.standard_normal(C).astype(np.float32), (rng.random(C) + 0.5).astype(np.float32)
    off = rng.standard_normal(C).astype(np.float32)
    return x, dy, res, g, b, mm, mv, off


@pytest.mark.parametrize("M", [1, 2, 37])
@pytest.mark.parametrize("residual,relu", [(False, False), (False, True), (True, True)])
def test_bn_refs_match_torch_f64(M, residual, relu):
    """Forward and backward references against torch.nn.functional.batch_norm and autograd in f64."""
    import torch.nn.functional as F

    C = 8
    x, dy, res, g, b, mm, mv, off = _bn_case(M, C, seed=M)
    f = R.bn_fwd_ref(x, g, b, mm, mv, 0.9, 1e-3, res if residual else None, off, relu)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    g64 = torch.from_numpy(g).double().requires_grad_(True)
    b64 = torch.from_numpy(b).double().requires_grad_(True)
    tm, tv = torch.from_numpy(mm).double(), torch.from_numpy(mv).double()
    mu = x64.mean(0)
    var = ((x64 - mu) ** 2).mean(0)
    y = (x64 - mu) / torch.sqrt(var + R.f32(1e-3)) * g64 + b64
    if M > 1:  # (torch refuses one value per channel in training mode)
        yt = F.batch_norm(x64, tm, tv, g64, b64, training=True, momentum=1 - R.f32(0.9), eps=R.f32(1e-3))
        torch.testing.assert_close(yt, y, atol=1e-12, rtol=1e-12)
        # torch's moving mean has no mean_off; its moving variance is the unbiased one
        np.testing.assert_allclose(f["moving_mean"] - off.astype(np.float64) * (1 - R.f32(0.9)), tm.numpy(), atol=1e-12)
        np.testing.assert_allclose(f["moving_var"], tv.numpy(), atol=1e-12)
    else:
        np.testing.assert_allclose(f["moving_var"], mv.astype(np.float64) * R.f32(0.9), atol=1e-12)  # var == 0, as computed
    if residual:
        y = y + torch.from_numpy(res).double()
    if relu:
        y = torch.relu(y)
    np.testing.assert_allclose(f["y"], y.detach().numpy(), atol=1e-12)
    y.backward(torch.from_numpy(dy).double())
    mode = 2 if residual else (1 if relu else 0)
    bw = R.bn_bwd_ref(dy, x, g, f["mean"], f["invstd"], mode, f["scale"], f["shift"], f["y"],
                      dgamma0=np.full(C, 2.0), dbeta0=None)
    np.testing.assert_allclose(bw["dx"], x64.grad.numpy(), atol=1e-10)
    np.testing.assert_allclose(bw["dgamma"] - 2.0, g64.grad.numpy(), atol=1e-10)
    np.testing.assert_allclose(bw["dbeta"], b64.grad.numpy(), atol=1e-10)


def test_bn_ref_mean_of_output_is_beta():
    x, _, _, g, b, *_ = _bn_case(301, 24, seed=5, mean=8.0, std=0.5)
    f = R.bn_fwd_ref(x, g, b, None, None, 0.9, 1e-3)
    np.testing.assert_allclose(f["y"].mean(axis=0), b.astype(np.float64), atol=1e-12)
    assert f["moving_mean"] is None and f["moving_var"] is None
    # and the normalised variance is var / (var + eps)
    np.testing.assert_allclose(f["y"].var(axis=0), g.astype(np.float64) ** 2 * f["var"] / (f["var"] + R.f32(1e-3)),
                               rtol=1e-12)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_bn_emulations_close_to_f64_on_easy_data(mode, bf16):
    """The f32 emulations are the same formulas: on randn data they agree with f64 to f32 (bf16) rounding."""
    M, C = 200, 16
    x, dy, res, g, b, mm, mv, off = _bn_case(M, C, seed=11)
    if bf16:
        x, dy, res = (R.bf16_bits_to_f64(R.bf16_rne(t)).astype(np.float32) for t in (x, dy, res))
    kw = dict(residual=res if mode == 2 else None, mean_off=off, relu=mode != 0)
    f = R.bn_fwd_ref(x, g, b, mm, mv, 0.99, 1e-3, **kw)
    e = R.bn_fwd_emul_f32(x, g, b, mm, mv, 0.99, 1e-3, bf16=bf16, **kw)
    for k in ("mean", "invstd", "scale", "shift", "moving_mean", "moving_var"):
        np.testing.assert_allclose(e[k], f[k], rtol=2e-6, atol=2e-6, err_msg=k)
    ytol = 2.0 ** -8 if bf16 else 1e-6
    np.testing.assert_allclose(e["y"], f["y"], rtol=ytol, atol=ytol)
    bw = R.bn_bwd_ref(dy, x, g, f["mean"], f["invstd"], mode, f["scale"], f["shift"], e["y"])
    be = R.bn_bwd_emul_f32(dy, x, g, e["mean"], e["invstd"], mode, e["scale"], e["shift"], e["y"], bf16=bf16)
    same = (bw["dz"] == be["dz"]).all(axis=0)  # (mode 1: a mask decision may differ at a pre-activation near 0)
    assert same.mean() > 0.8
    np.testing.assert_allclose(be["dgamma"][same], bw["dgamma"][same], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(be["dbeta"][same], bw["dbeta"][same], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(be["dx"][:, same], bw["dx"][:, same], rtol=ytol, atol=ytol)


def test_bn_emulation_loses_the_variance_at_a_large_mean():
    """What the emulation is for: Q/M - mean^2 from f32 sums degrades with (mean/std)^2 (csrc/kernels/bn.h)."""
    errs = []
    for mean, std in ((0.5, 2.0), (8.0, 0.5), (30.0, 0.25)):
        x = _bn_case(3000, 8, seed=3, mean=mean, std=std)[0]
        f = R.bn_fwd_ref(x, None, None, None, None, 0.9, 1e-3)
        e = R.bn_fwd_emul_f32(x, None, None, None, None, 0.9, 1e-3)
        errs.append(np.abs(e["invstd"] / f["invstd"] - 1).max())
    # a sequential f32 sum of 3000 terms carries ~sqrt(3000) * 2^-24 = 3e-6; times (mean/std)^2 + 1 for the variance
    assert errs[0] < 1e-5 and errs[1] < 1e-3 and errs[2] < 5e-2 and errs[0] < errs[1] < errs[2], errs


# ------------------------------------------------------------------------------------- max pool
POOL_GEOMS = [(3, 3, 2, 2, 1, 1, 1, 1), (3, 3, 2, 2, 0, 1, 0, 1), (2, 2, 2, 2, 0, 0, 0, 0), (2, 3, 1, 2, 0, 0, 1, 1),
              (1, 1, 2, 2, 0, 0, 0, 0), (2, 2, 3, 3, 0, 0, 0, 0), (5, 5, 1, 1, 2, 2, 2, 2)]


def _torch_pool(x, geom, pad_zero):
    import torch.nn.functional as F

    kh, kw, sh, sw, pt, pb, pl, pr = geom
    h = torch.from_numpy(x).permute(0, 3, 1, 2)
    h = F.pad(h, (pl, pr, pt, pb), value=0.0 if pad_zero else float("-inf"))
    return F.max_pool2d(h, (kh, kw), (sh, sw)).permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("geom", POOL_GEOMS + [(3, 3, 3, 3, 0, 0, 0, 0)])
@pytest.mark.parametrize("pad_zero", [False, True])
def test_maxpool_ref_matches_torch(geom, pad_zero):
    kh, kw, sh, sw, pt, pb, pl, pr = geom
    rng = np.random.default_rng(sum(geom))
    H, W = (3, 3) if geom == (3, 3, 3, 3, 0, 0, 0, 0) else (7, 9)
    x = (rng.standard_normal((2, H, W, 8)) - (1.0 if pad_zero else 0.0)).astype(np.float32)
    y, arg = R.maxpool_fwd_ref(x, *geom, pad_zero)
    np.testing.assert_array_equal(y, _torch_pool(x, geom, pad_zero))
    assert set(np.unique(arg)) <= set(range(kh * kw)) | {255}
    assert pad_zero or (arg != 255).all()
    # the argmax points at the maximum, and autograd routes the gradient the same way (no ties in randn)
    dy = rng.standard_normal(y.shape).astype(np.float32)
    dx = R.maxpool_bwd_ref(dy, arg, x.shape, kh, kw, sh, sw, pt, pl)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    h = torch.nn.functional.pad(xt.permute(0, 3, 1, 2), (pl, pr, pt, pb), value=0.0 if pad_zero else float("-inf"))
    torch.nn.functional.max_pool2d(h, (kh, kw), (sh, sw)).permute(0, 2, 3, 1).backward(torch.from_numpy(dy).double())
    np.testing.assert_allclose(dx, xt.grad.numpy(), atol=1e-12)
    # sum(dx) == sum of dy over the windows whose argmax is a real element
    np.testing.assert_allclose(dx.sum(), dy.astype(np.float64)[arg != 255].sum(), atol=1e-9)


def test_maxpool_ref_ties_nan_and_inf():
    geom = (3, 3, 2, 2, 1, 1, 1, 1)
    x = np.full((1, 5, 5, 8), 2.0, dtype=np.float32)
    y, arg = R.maxpool_fwd_ref(x, *geom, False)
    assert (y == 2.0).all()
    # the first in-range window position: 4 in the corner (row 0 and column 0 are padding), 3 / 1 on the edges
    assert arg[0, 0, 0, 0] == 4 and arg[0, 0, 1, 0] == 3 and arg[0, 1, 0, 0] == 1 and arg[0, 1, 1, 0] == 0
    x[0, 2, 2, 0] = np.nan
    x[0, :, :, 1] = -np.inf
    y, arg = R.maxpool_fwd_ref(x, *geom, False)
    assert (y[..., 0] == 2.0).all() and (arg[..., 0] != 255).all()  # the NaN never wins
    assert (y[..., 1] == -np.inf).all() and (arg[..., 1] == 255).all()  # -inf never beats the initial -inf
    y0, arg0 = R.maxpool_fwd_ref(-np.abs(x[..., 2:]) - 1, *geom, True)
    assert (y0[0, 0] == 0).all() and (arg0[0, 0] == 255).all() and (arg0[0, 1, 1] != 255).all()
    dx = R.maxpool_bwd_ref(np.ones_like(y0), arg0, (1, 5, 5, 6), 3, 3, 2, 2, 1, 1)
    assert dx.sum() == (arg0 != 255).sum()
