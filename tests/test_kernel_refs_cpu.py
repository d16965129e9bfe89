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
