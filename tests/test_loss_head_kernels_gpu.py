"""The weighted / smoothed loss head ``xent_head_w`` and the three-column gather ``gather_xyw``
(csrc/kernels/loss_head.hip) against the f64 oracle of tests/loss_head_refs.py, at shapes on both sides of the
K <= 64 path and of the switch from one workgroup to rows + finish (65536 logits), for three logit families,
sparse and dense targets, every combination of sample / class weights and label smoothing 0 and 0.1.

Tolerances follow tests/test_head_gpu.py: 4 E + one f32 ulp, E the largest error of the f32 emulation
(loss_head_refs.head_emul_f32) over at least 64 drawn rows, from the CPU alone.  The emulation includes the
weights and the 1 / gn scaling, so E (taken per unit of row scale w / gn) covers their roundings.
"""
import functools

import numpy as np
import pytest
import torch

import kernel_refs as R
import loss_head_refs as LR

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 2), (5, 64), (4, 65), (9, 129), (7, 1000), (1024, 64), (1025, 64)]
FAMILIES = ["randn3", "offset1e4", "dupmax"]
WEIGHTS = ["none", "sw", "cw", "swcw"]
EPS = [0.0, 0.1]
GUARD = 16
GUARD_BITS = 0x4B1D5EED


def _hip():
    from tensorflow_distributed_learning_amd.ops import hip

    return hip()


@functools.lru_cache(maxsize=None)
def _inputs(N, K, family, dense):
    """Logits, target and weights of a shape: max(N, 64) rows are drawn, the kernels get the first N.  Weights in
    [0.25, 4]; with N >= 4 rows 1 and 2 carry the labels -1 and K (sparse) and row 3 weighs 0; with K >= 2 the
    last class weighs 0 (at N < 4 or K = 1 a zero would leave nothing else to check)."""
    rng = np.random.default_rng(1000 * N + K + (7 if dense else 0))
    Mr = max(N, 64)
    z = rng.standard_normal((Mr, K))
    z = {"randn3": z * 3, "offset1e4": z + 1e4, "dupmax": z * 3}[family].astype(np.float32)
    y = rng.integers(0, K, Mr)
    if family == "dupmax" and K >= 2:
        for r in range(Mr):  # the row's maximum at two indices i < j; the label on either
            i, j = sorted(rng.choice(K, 2, replace=False))
            z[r, i] = z[r, j] = z[r].max() + np.float32(1.0)
            y[r] = i if r % 2 == 0 else j
    if dense:
        t = np.zeros((Mr, K), dtype=np.float32)
        t[np.arange(Mr), y] = 1.0
        soft = rng.random((Mr, K)).astype(np.float32)  # every other row a soft target (rows need not sum to 1)
        t[1::2] = (0.5 * t[1::2] + 0.5 * soft[1::2] / soft[1::2].sum(axis=1, keepdims=True)).astype(np.float32)
        if family == "dupmax" and K >= 2:
            t[4::8] = 0.0  # ... and some with the target's maximum twice (class = the first index)
            t[4::8, 0] = t[4::8, K - 1] = 0.5
        target = t
    else:
        if N >= 4:
            y[1], y[2] = -1, K
        target = y
    sw = rng.uniform(0.25, 4.0, Mr).astype(np.float32)
    cw = rng.uniform(0.25, 4.0, K).astype(np.float32)
    if N >= 4:
        sw[3] = 0.0
    if K >= 2:
        cw[K - 1] = 0.0
    return z, target, sw, cw


@functools.lru_cache(maxsize=None)
def _case(N, K, family, dense, weights, eps):
    """(inputs of the first N rows, f64 reference, tolerances) of one case."""
    z, target, sw, cw = _inputs(N, K, family, dense)
    sw = sw if "sw" in weights else None
    cw = cw if "cw" in weights else None
    gn = float(2 * N + 3)
    ref = LR.head_ref(z, target, sw, cw, eps, gn)
    e_wl, e_dz, e_w = LR.head_emul_f32(z, target, sw, cw, eps, gn)
    live = ref["w"] > 0  # (a row of weight 0 is exactly 0 in the kernel, the emulation and the oracle)
    scale = ref["w"] / gn
    # errors per unit of the row's weight / scale, over all drawn rows
    e_loss = float(np.abs(e_wl[live] / ref["w"][live] - ref["loss"][live]).max()) if live.any() else 0.0
    e_dzu = float(np.abs(e_dz[live] / scale[live, None] - ref["dzu"][live]).max()) if live.any() else 0.0
    tol_loss = 4 * e_loss + R.ulp32(ref["mag"])                                            # per unit of w
    tol_dzu = 4 * e_dzu + R.ulp32(np.maximum(ref["p"] * ref["S"][:, None], np.abs(ref["dzu"])))  # per unit of scale
    both = sw is not None and cw is not None  # (then w = f32(sw cw) is rounded: half an ulp; else it is exact)
    tol_w = 0.5 * R.ulp32(ref["w"]) * both
    cut = lambda a: a[:N]  # noqa: E731
    return ({"z": z[:N], "target": target[:N], "sw": None if sw is None else sw[:N], "cw": cw, "gn": gn},
            {k: cut(v) for k, v in ref.items()},
            {"loss": cut(tol_loss), "dzu": cut(tol_dzu), "w": cut(tol_w)}, (e_loss, e_dzu))


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n, dtype=torch.float32):
    """(view of n elements, whole buffer) with GUARD words of a bit pattern on either side."""
    whole = torch.full((n + 2 * GUARD,), GUARD_BITS, dtype=torch.int32, device="cuda")
    return whole.view(dtype)[GUARD:GUARD + n] if dtype != torch.int32 else whole[GUARD:GUARD + n], whole


def _guards_intact(whole, n) -> bool:
    return bool((whole[:GUARD] == GUARD_BITS).all() and (whole[GUARD + n:] == GUARD_BITS).all())


def _run(inp, eps, accs0=(10.0, 3.0, 1.0, 2.0), guard=False, cw_t=None):
    z, target = _cuda(inp["z"]), _cuda(inp["target"])
    accs = [torch.tensor([v], dtype=torch.float64, device="cuda") for v in accs0]
    N, K = inp["z"].shape
    kw = {}
    if guard:
        dz_v, dz_w = _guarded(N * K)
        ws_v, ws_w = _guarded(3 * N)
        ws_w.view(torch.float32)[GUARD:GUARD + 3 * N] = float("nan")
        kw = dict(dz_out=dz_v.view(N, K), rows_ws=ws_v)
    cw = cw_t if cw_t is not None else _cuda(inp["cw"])
    loss, dz = _hip().xent_head_w(z, target, inp["gn"], _cuda(inp["sw"]), cw, eps, *accs, **kw)
    out = (loss.item(), dz.cpu().numpy().astype(np.float64), [a.item() for a in accs])
    if guard:
        assert _guards_intact(dz_w, N * K), "xent_head_w wrote outside dz"
        assert _guards_intact(ws_w, 3 * N), "xent_head_w wrote outside the row workspace"
    return out


def _within(got, ref, bound, what):
    err = np.abs(got - ref)
    bad = ~(err <= bound)  # (a NaN is bad)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the bound, first at {i}: got "
                             f"{got[i]!r}, f64 reference {ref[i]!r}, bound {bound[i]:.3e}")


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("nk", SHAPES, ids=str)
def test_head_against_f64(nk, family, dense):
    N, K = nk
    for weights in WEIGHTS:
        for eps in EPS:
            inp, ref, tol, emax = _case(N, K, family, dense, weights, eps)
            what = f"{nk} {family} {'dense' if dense else 'sparse'} {weights} eps={eps}"
            print(f"{what}: emulation max err per unit weight: loss {emax[0]:.3e} dz {emax[1]:.3e}")
            loss, dz, accs = _run(inp, eps, guard=True)
            gn, w = inp["gn"], ref["w"]
            total, total_tol = float((w * ref["loss"]).sum()), float((w * tol["loss"]).sum())
            # rows are summed in f64; the result is rounded to f32 once
            assert abs(loss - total / gn) <= total_tol / gn + R.ulp32(total / gn), (what, loss, total / gn)
            assert abs(accs[0] - (10.0 + total)) <= total_tol, (what, accs[0], 10.0 + total)
            assert accs[1] == 3.0 + N, what  # the loss tracker counts rows
            cor, cnt = float((w * ref["correct"]).sum()), float(w.sum())
            if weights == "none":
                assert accs[2] == 1.0 + cor and accs[3] == 2.0 + N, (what, accs)
            else:
                # f32 weights and their sums over <= 1025 rows are exact in f64; w = f32(sw cw) is half an ulp off
                assert abs(accs[2] - (1.0 + cor)) <= float((tol["w"] * ref["correct"]).sum()), (what, accs[2], cor)
                assert abs(accs[3] - (2.0 + cnt)) <= float(tol["w"].sum()), (what, accs[3], cnt)
            scale = (w / gn)[:, None]
            want = ref["dz"]
            _within(dz, want, tol["dzu"] * scale + R.ulp32(want), what + " dz")
            zero = w == 0
            assert (dz[zero] == 0).all(), what + ": a row of weight 0 must have dz == 0"
            if not dense:
                bad = ref["cls"] < 0
                # a label outside [0, K): no loss, no one-hot or smoothing term, the row still weighs sw
                _within(dz[bad], ref["p"][bad] * scale[bad], tol["dzu"][bad] * scale[bad] + R.ulp32(want[bad]),
                        what + " dz of invalid labels")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("nk", SHAPES, ids=str)
def test_unsmoothed_sparse_head_has_xent_heads_bits(nk, family):
    """eps = 0 and sparse labels: no weights, and weights that are all 1, give ``xent_head``'s loss, dz and four
    accumulators bit for bit."""
    N, K = nk
    inp = _case(N, K, family, False, "none", 0.0)[0]
    z, y = _cuda(inp["z"]), _cuda(inp["target"])
    accs0 = (10.0, 3.0, 1.0, 2.0)

    def fresh():
        return [torch.tensor([v], dtype=torch.float64, device="cuda") for v in accs0]

    a = fresh()
    loss0, dz0 = _hip().xent_head(z, y, inp["gn"], *a)
    ones_n, ones_k = torch.ones(N, device="cuda"), torch.ones(K, device="cuda")
    for sw, cw in ((None, None), (ones_n, None), (None, ones_k), (ones_n, ones_k)):
        b = fresh()
        loss1, dz1 = _hip().xent_head_w(z, y, inp["gn"], sw, cw, 0.0, *b)
        what = f"{nk} {family} sw={sw is not None} cw={cw is not None}"
        assert torch.equal(loss0.view(torch.int32), loss1.view(torch.int32)), what
        assert torch.equal(dz0.view(torch.int32), dz1.view(torch.int32)), what
        for p, q in zip(a, b):
            assert torch.equal(p.view(torch.int64), q.view(torch.int64)), what


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
@pytest.mark.parametrize("nk", [(5, 64), (9, 129), (1025, 64)], ids=str)
def test_zero_weight_rows_add_nothing(nk, dense):
    """All weights 0 (through sw, through cw, through both): dz == 0 everywhere, the loss is 0, the loss total and
    both accuracy sums stay, the loss count advances by N."""
    N, K = nk
    inp = dict(_case(N, K, "randn3", dense, "swcw", 0.1)[0])
    if not dense:
        inp["target"] = np.clip(inp["target"], 0, K - 1)  # (an invalid label takes class weight 1, not cw's 0)
    zeros_n, zeros_k = np.zeros(N, dtype=np.float32), np.zeros(K, dtype=np.float32)
    for sw, cw in ((zeros_n, None), (None, zeros_k), (zeros_n, inp["cw"]), (inp["sw"], zeros_k)):
        loss, dz, accs = _run(dict(inp, sw=sw, cw=cw), 0.1)
        assert loss == 0.0 and (dz == 0).all(), (nk, sw is None, cw is None)
        assert accs == [10.0, 3.0 + N, 1.0, 2.0]


@pytest.mark.parametrize("nk", [(5, 64), (4, 65), (1025, 64)], ids=str)
def test_out_of_range_labels_never_index_the_class_weights(nk):
    """The class-weight table sits between NaN guard words: a label of -1, K, a far negative or a far positive one
    that indexed it would read a NaN (or fault), and the NaN would show in the loss, dz and the sums."""
    N, K = nk
    inp = dict(_case(N, K, "randn3", False, "cw", 0.1)[0])
    y = inp["target"].copy()
    y[0], y[1], y[2], y[3] = -1, K, -(2 ** 40), 2 ** 40 + 3
    inp["target"] = y
    whole = torch.full((K + 2 * GUARD,), float("nan"), device="cuda")
    whole[GUARD:GUARD + K] = torch.from_numpy(inp["cw"]).cuda()
    for eps in EPS:
        loss, dz, accs = _run(inp, eps, cw_t=whole[GUARD:GUARD + K])
        assert np.isfinite(loss) and np.isfinite(dz).all() and np.isfinite(accs).all()
        ref = LR.head_ref(inp["z"], y, None, inp["cw"], eps, inp["gn"])
        assert (ref["w"][:4] == 1.0).all() and (ref["loss"][:4] == 0.0).all()
        np.testing.assert_allclose(dz[:4] * inp["gn"], ref["p"][:4], rtol=1e-5, atol=1e-7)  # plain softmax, weight 1
    assert torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[GUARD + K:]).all()


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
def test_empty_batch(dense):
    K = 10
    z = torch.zeros(0, K, device="cuda")
    target = torch.zeros(0, K, device="cuda") if dense else torch.zeros(0, dtype=torch.int64, device="cuda")
    for sw, cw in ((None, None), (torch.zeros(0, device="cuda"), torch.ones(K, device="cuda"))):
        accs = [torch.tensor([v], dtype=torch.float64, device="cuda") for v in (10.0, 3.0, 1.0, 2.0)]
        loss, dz = _hip().xent_head_w(z, target, 8.0, sw, cw, 0.1, *accs)
        torch.cuda.synchronize()
        assert loss.item() == 0.0 and dz.shape == (0, K)
        assert [a.item() for a in accs] == [10.0, 3.0, 1.0, 2.0]


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
@pytest.mark.parametrize("nk", [(5, 64), (9, 129), (1025, 64)], ids=str)
def test_two_runs_give_the_same_bits(nk, dense):
    N, K = nk
    inp = _case(N, K, "randn3", dense, "swcw", 0.1)[0]
    a, b = _run(inp, 0.1), _run(inp, 0.1)
    assert np.float32(a[0]).view(np.int32) == np.float32(b[0]).view(np.int32)
    assert np.array_equal(a[1].view(np.int64), b[1].view(np.int64))
    assert np.array_equal(np.array(a[2]).view(np.int64), np.array(b[2]).view(np.int64))


def test_bad_arguments_are_rejected():
    z = torch.zeros(4, 10, device="cuda")
    y = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="sw"):
        _hip().xent_head_w(z, y, 4.0, torch.ones(5, device="cuda"), None, 0.0)
    with pytest.raises(RuntimeError, match="cw"):
        _hip().xent_head_w(z, y, 4.0, None, torch.ones(9, device="cuda"), 0.0)
    with pytest.raises(RuntimeError, match="targets"):
        _hip().xent_head_w(z, torch.zeros(4, 9, device="cuda"), 4.0, None, None, 0.0)
    with pytest.raises(RuntimeError, match="smoothing"):
        _hip().xent_head_w(z, y, 4.0, None, None, 1.5)
    with pytest.raises(RuntimeError, match="labels"):
        _hip().xent_head_w(z, y.int(), 4.0, None, None, 0.0)


# ------------------------------------------------------------------------------------- the three-column gather
@pytest.mark.parametrize("lab", [torch.int64, torch.int32], ids=["int64", "int32"])
@pytest.mark.parametrize("shape", [(784,), (28, 28, 1), (5,), (3, 2)], ids=str)
def test_gather_xyw_is_numpy_indexing(shape, lab):
    n = 37
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n,) + shape).astype(np.float32)
    Y = rng.integers(-5, 1000, n)
    W = rng.uniform(0, 4, n).astype(np.float32)
    idx = np.concatenate([rng.integers(0, n, 21), [0, n - 1, n - 1]]).astype(np.int32)
    Xd, Yd, Wd = _cuda(X), torch.from_numpy(Y).to(lab).cuda(), _cuda(W)
    x, y, w = _hip().gather_xyw(Xd, Yd, Wd, _cuda(idx))
    assert x.shape == (len(idx),) + shape and y.dtype == lab and w.dtype == torch.float32
    assert np.array_equal(x.cpu().numpy().view(np.int32), X[idx].view(np.int32))
    assert np.array_equal(y.cpu().numpy(), Y[idx]) and np.array_equal(w.cpu().numpy().view(np.int32), W[idx].view(np.int32))
    # into guarded outputs: nothing is written outside the three columns
    row = int(np.prod(shape))
    xo, xw = _guarded(len(idx) * row)
    wo, ww = _guarded(len(idx))
    words = 2 if lab == torch.int64 else 1
    yo_i32, yw = _guarded(len(idx) * words, torch.int32)
    yo = yo_i32.view(lab)
    x2, y2, w2 = _hip().gather_xyw(Xd, Yd, Wd, _cuda(idx), out_x=xo.view((len(idx),) + shape), out_y=yo, out_w=wo)
    assert torch.equal(x2, x) and torch.equal(y2, y) and torch.equal(w2, w)
    assert _guards_intact(xw, len(idx) * row) and _guards_intact(ww, len(idx)) and _guards_intact(yw, len(idx) * words)
    # and gather_xy's first two columns
    gx, gy = _hip().gather_xy(Xd, Yd, _cuda(idx))
    assert torch.equal(gx, x) and torch.equal(gy, y)


def test_gather_xyw_empty_batch():
    X, Y, W = torch.zeros(4, 8, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"), torch.ones(4, device="cuda")
    x, y, w = _hip().gather_xyw(X, Y, W, torch.zeros(0, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert x.shape == (0, 8) and y.shape == (0,) and w.shape == (0,) and w.dtype == torch.float32
    assert (torch.ones(4, device="cuda") + 1).sum().item() == 8.0
