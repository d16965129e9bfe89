"""The group-normalisation kernels of csrc/kernels/groupnorm.hip, called through the bindings and compared
with the f64 references of tests/groupnorm_refs.py: one value per group (m = 1), a 2-D input, several
group sizes down to one channel, more pixels than one workgroup's share with a short last part, the
per-element path (C * sizeof(elem) not a multiple of 16), several column blocks (C = 2048) and a short last
one (C = 320 f32), with and without
gamma / beta, dgamma / dbeta returned or added into prefilled targets, data with a large mean, constant
groups, NaN / Inf confined to their (sample, group), per-sample independence, run-to-run identity, and
what supported() refuses.

Every operand is a view into the middle of a NaN-filled buffer, 16-byte aligned: a read outside the
operand poisons a sum.

Tolerances come from the references alone: E = max |emulation - f64 reference| on the case's own inputs
(groupnorm_refs.gn_*_emul: the kernels' formulas -- sequential f64 sums, f32 coefficient tables, one f32 fma
per element), and every compared element must lie within 4 E + 1 ulp of the output dtype at the reference's
magnitude.  test_large_mean also shows that the same formulas with f32 sums miss that bound.
"""
import numpy as np
import pytest
import torch

import groupnorm_refs as GR
import kernel_refs as R

pytestmark = pytest.mark.gpu

EPS = 1e-3
DTYPES = [torch.float32, torch.bfloat16]
# [N, P = H x W, C], G (-1: one group per channel)
SHAPES = [((1, 1, 8), 1), ((1, 1, 8), 8), ((3, 1, 24), 3), ((2, 49, 16), 1), ((2, 49, 16), 4), ((2, 49, 16), 16),
          ((2, 49, 16), -1), ((2, 37 * 41, 8), 2), ((5, 9, 6), 3), ((2, 25, 3), 1), ((2, 16, 2048), 32),
          ((2, 9, 320), 5)]  # (the last: 80 f32 columns, a short second column block)
IDS = [f"{s[0]}x{s[1]}x{s[2]}-G{g}" for s, g in SHAPES]
REPORT = {}  # quantity -> [largest E, largest kernel error] over the module (printed at the end, for the record)


def _C():
    from tensorflow_distributed_learning_amd.ops import hip

    return hip()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(REPORT):
        print(f"\n[gn kernels] {k}: largest E {REPORT[k][0]:.3g}, largest kernel error {REPORT[k][1]:.3g}", end="")
    print()


def _bf(v):
    return R.bf16_bits_to_f64(R.bf16_rne(v)).astype(np.float32)


def _dev(vals, dtype, shape=None):
    """vals as a 16-byte-aligned view with 16 NaN elements in front of and behind it."""
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    n = vals.size
    buf = torch.full((n + 32,), float("nan"), dtype=dtype, device="cuda")
    v = buf[16:16 + n].view(tuple(shape or vals.shape))
    v.copy_(torch.from_numpy(vals).to(dtype).reshape(v.shape))
    assert v.data_ptr() % 16 == 0 and v.is_contiguous()
    return v


def _vec(vals):
    return _dev(vals, torch.float32)


def _np(t):
    return t.detach().double().cpu().numpy()


def _inputs(shape, bf16, seed, mean=0.5, std=2.0):
    rng = np.random.default_rng(seed)
    C = shape[-1]
    x = (rng.standard_normal(shape) * std + mean).astype(np.float32)
    dy = rng.standard_normal(shape).astype(np.float32)
    if bf16:
        x, dy = _bf(x), _bf(dy)
    rng = np.random.default_rng(seed + 1000)  # the parameters depend on (seed, C) alone, not on N or P
    p = dict(g=(rng.random(C) + 0.5).astype(np.float32), b=rng.standard_normal(C).astype(np.float32),
             dg0=rng.standard_normal(C).astype(np.float32), db0=rng.standard_normal(C).astype(np.float32))
    return x, dy, p


def _cmp(name, got, ref, emu, ulp, sel=None):
    """got within 4 E + 1 ulp of ref on the elements `sel` (a boolean mask; all by default)."""
    with np.errstate(invalid="ignore"):
        d = np.abs(emu - ref)
        err = np.abs(got - ref)
    tol_ulp = ulp(ref)
    if sel is not None:
        d, err, tol_ulp = d[sel], err[sel], tol_ulp[sel]
    E = float(d.max()) if d.size else 0.0
    assert np.isfinite(E), f"{name}: the references are not finite where they are compared"
    tol = 4.0 * E + tol_ulp
    assert np.isfinite(err).all(), f"{name}: non-finite output"
    rec = REPORT.setdefault(name, [0.0, 0.0])
    rec[0], rec[1] = max(rec[0], E), max(rec[1], float(err.max()) if err.size else 0.0)
    bad = err > tol
    assert not bad.any(), (f"{name}: {int(bad.sum())} elements off, worst error {err.max():.3g} "
                           f"(E {E:.3g}, tolerance there {tol.flat[err.argmax()]:.3g})")


def _run(shape, G, dtype, seed=0, mean=0.5, std=2.0, gamma=True, beta=True, acc=0, edit=None, x_dy=None):
    """One forward + backward through the bindings.  Returns the inputs and the outputs (torch tensors)."""
    Ck = _C()
    bf16 = dtype == torch.bfloat16
    x, dy, p = _inputs(shape, bf16, seed, mean, std)
    if x_dy is not None:
        x, dy = x_dy
    if edit is not None:
        edit(x)
    G = GR.groups_of(shape[-1], G)
    g, b = (p["g"] if gamma else None), (p["b"] if beta else None)
    dg0, db0 = (p["dg0"] if acc & 1 else None), (p["db0"] if acc & 2 else None)
    dev_shape = (shape[0], shape[2]) if shape[1] == 1 and shape[0] > 1 else shape  # [3, 1, 24]: a 2-D input
    tx, tdy = _dev(x, dtype, dev_shape), _dev(dy, dtype, dev_shape)
    tg, tb = (_vec(g) if gamma else None), (_vec(b) if beta else None)
    tdg, tdb = (_vec(dg0) if acc & 1 else None), (_vec(db0) if acc & 2 else None)
    y, st = Ck.gn_forward(tx, G, tg, tb, EPS)[:2]
    dx, dg, db = Ck.gn_backward(tdy, tx, G, tg, st, tdg, tdb)[:3]
    if acc & 1:
        assert dg.data_ptr() == tdg.data_ptr()
    if acc & 2:
        assert db.data_ptr() == tdb.data_ptr()
    torch.cuda.synchronize()
    return dict(x=x, dy=dy, g=g, b=b, dg0=dg0, db0=db0, G=G, bf16=bf16, y=y.reshape(shape), st=st,
                dx=dx.reshape(shape), dg=dg, db=db)


def _check(shape, G, dtype, label="", sel_ng=None, **kw):
    """_run against the references.  sel_ng: boolean [N, G] of the (sample, group) pairs to compare (the
    others are the caller's); dgamma / dbeta are then compared on the channels whose every sample is."""
    o = _run(shape, G, dtype, **kw)
    N, P, C = shape
    G_, bf16 = o["G"], o["bf16"]
    ulp_out = R.ulp_bf16 if bf16 else R.ulp32
    tag = "bf16" if bf16 else "f32"
    with np.errstate(all="ignore"):
        f = GR.gn_fwd_ref(o["x"], G_, o["g"], o["b"], EPS)
        e = GR.gn_fwd_emul(o["x"], G_, o["g"], o["b"], EPS, bf16=bf16)
        bw = GR.gn_bwd_ref(o["dy"], o["x"], G_, o["g"], EPS, o["dg0"], o["db0"])
        be = GR.gn_bwd_emul(o["dy"], o["x"], G_, o["g"], e["mean"], e["r"], o["dg0"], o["db0"], bf16=bf16)
    sel = sel_c = None
    if sel_ng is not None:
        sel = np.broadcast_to(np.repeat(sel_ng, C // G_, axis=1)[:, None, :], shape)
        sel_c = np.repeat(sel_ng.all(axis=0), C // G_)
    st = _np(o["st"])
    # the saved statistics are f64: within 4 E + 1 f32 ulp like everything else (they are far closer)
    _cmp(label + "mean", st[..., 0], f["mean"], e["mean"], R.ulp32, sel_ng)
    _cmp(label + "r", st[..., 1], f["r"], e["r"], R.ulp32, sel_ng)
    _cmp(label + f"y {tag}", _np(o["y"]), f["y"], e["y"], ulp_out, sel)
    _cmp(label + f"dx {tag}", _np(o["dx"]), bw["dx"], be["dx"], ulp_out, sel)
    _cmp(label + f"dgamma {tag}", _np(o["dg"]), bw["dgamma"], be["dgamma"], R.ulp32, sel_c)
    _cmp(label + f"dbeta {tag}", _np(o["db"]), bw["dbeta"], be["dbeta"], R.ulp32, sel_c)
    return o, f, e


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape,G", SHAPES, ids=IDS)
def test_shapes_against_f64(shape, G, dtype):
    _check(shape, G, dtype, seed=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("gamma,beta", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("shape,G", [((2, 49, 16), 4), ((5, 9, 6), 3)], ids=["vector", "per-element"])
def test_without_gamma_or_beta(shape, G, gamma, beta, dtype):
    _check(shape, G, dtype, seed=2, gamma=gamma, beta=beta)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("acc", [1, 2, 3])
@pytest.mark.parametrize("shape,G", [((2, 49, 16), 4), ((2, 25, 3), 1), ((2, 16, 2048), 32)],
                         ids=["vector", "per-element", "column-blocks"])
def test_gradients_added_into_targets(shape, G, acc, dtype):
    o, _, _ = _check(shape, G, dtype, seed=3, acc=acc, label="acc ")
    # the target that was not given is returned fresh, the given one holds prefill + gradient
    plain = _run(shape, G, dtype, seed=3)
    for bit, k, k0 in ((1, "dg", "dg0"), (2, "db", "db0")):
        if acc & bit:
            want = torch.from_numpy(o[k0]).cuda() + plain[k]
            assert torch.equal(o[k], want)
        else:
            assert torch.equal(o[k], plain[k])


def test_plan_splits_the_pixels():
    """The shapes above exercise what they claim: several chunks with a short last one, the per-element
    path, several column blocks."""
    Ck = _C()
    for bf16 in (False, True):
        vec, cols, tc, rl, colblocks, rows_wg, chunks = Ck.gn_plan(37 * 41, 8, bf16)
        assert vec == (8 if bf16 else 4) and chunks >= 2 and (37 * 41) % rows_wg != 0
        assert Ck.gn_plan(9, 6, bf16)[0] == 1 and Ck.gn_plan(25, 3, bf16)[0] == 1
    assert Ck.gn_plan(16, 2048, False)[4] == 8 and Ck.gn_plan(16, 2048, True)[4] == 4
    vec, cols, tc, rl, colblocks, rows_wg, chunks = Ck.gn_plan(9, 320, False)
    assert cols == 80 and tc == 64 and colblocks == 2  # the second column block is 16 columns wide


# ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_large_mean(dtype):
    """mean 100, std 0.1: E[x^2] - mean^2 cancels 6 digits.  The f64 sums keep the bound; the same formulas
    with f32 sums would not (shown on the f32 data, where the output's own rounding does not hide it)."""
    shape, G = (2, 37 * 41, 8), 2
    o, f, e = _check(shape, G, dtype, seed=4, mean=100.0, std=0.1, label="mean100 ")
    if dtype == torch.float32:
        e32 = GR.gn_fwd_emul(o["x"], G, o["g"], o["b"], EPS, sums="f32")
        E = np.abs(e["y"] - f["y"]).max()
        assert (np.abs(e32["y"] - f["y"]) > 4 * E + R.ulp32(f["y"])).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_constant_group(dtype):
    """A constant group: var = 0, r = 1 / sqrt(eps), y = beta, and dx is finite."""
    shape, G = (2, 49, 16), 4

    def edit(x):
        x[1, :, 4:8] = 3.25

    o, f, e = _check(shape, G, dtype, seed=5, edit=edit, label="const ")
    st = _np(o["st"])
    assert abs(st[1, 1, 1] * np.sqrt(EPS) - 1.0) < 1e-12 and st[1, 1, 0] == 3.25
    assert torch.isfinite(o["dx"].float()).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("shape,G", [((2, 49, 16), 4), ((5, 9, 6), 3)], ids=["vector", "per-element"])
def test_non_finite_stays_in_its_group(shape, G, bad, dtype):
    N, P, C = shape
    cpg = C // G
    n0, g0 = 1, 1

    def edit(x):
        x[n0, P // 2, g0 * cpg] = bad

    sel_ng = np.ones((N, G), dtype=bool)
    sel_ng[n0, g0] = False
    o, _, _ = _check(shape, G, dtype, seed=6, edit=edit, sel_ng=sel_ng, label="nonfinite ")
    clean = _run(shape, G, dtype, seed=6)
    ch = slice(g0 * cpg, (g0 + 1) * cpg)
    for k in ("y", "dx"):
        got, want = o[k].clone(), clean[k].clone()
        assert not torch.isfinite(got[n0, :, ch].float()).any(), f"{k}: the poisoned group must not look finite"
        got[n0, :, ch] = 0
        want[n0, :, ch] = 0
        assert torch.isfinite(got.float()).all()
        assert torch.equal(got, want), f"{k}: another (sample, group) changed"
    for k in ("dg", "db"):
        got, want = o[k].clone(), clean[k].clone()
        if k == "dg":  # dbeta sums dy alone: it never sees x
            assert not torch.isfinite(got[ch]).any()
        got[ch] = 0
        want[ch] = 0
        assert torch.equal(got, want), f"{k}: a channel of another group changed"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape,G", [((3, 49, 16), 4), ((2, 37 * 41, 8), 2), ((5, 9, 6), 3), ((2, 16, 2048), 32)],
                         ids=["vector", "chunks", "per-element", "column-blocks"])
def test_per_sample_independence(shape, G, dtype):
    """y[i] and dx[i] of the batch are the bits of sample i run alone."""
    whole = _run(shape, G, dtype, seed=7)
    for i in range(shape[0]):
        one = _run((1,) + shape[1:], G, dtype, seed=7, x_dy=(whole["x"][i:i + 1], whole["dy"][i:i + 1]))
        assert torch.equal(one["y"][0], whole["y"][i]), f"y of sample {i}"
        assert torch.equal(one["dx"][0], whole["dx"][i]), f"dx of sample {i}"
        assert torch.equal(one["st"][0], whole["st"][i])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape,G", [((2, 37 * 41, 8), 2), ((5, 9, 6), 3), ((2, 16, 2048), 32)],
                         ids=["chunks", "per-element", "column-blocks"])
def test_two_runs_are_bit_identical(shape, G, dtype):
    a, b = _run(shape, G, dtype, seed=8), _run(shape, G, dtype, seed=8)
    for k in ("y", "st", "dx", "dg", "db"):
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ the op
def test_supported():
    from tensorflow_distributed_learning_amd.ops import groupnorm as gn

    x = torch.zeros(2, 4, 4, 8, device="cuda")
    assert gn.supported(x, 4) and gn.supported(x.bfloat16(), 8) and gn.supported(x[:, 0, 0], 2)
    assert not gn.supported(x, 3)  # groups does not divide C
    assert not gn.supported(x[:0], 4)  # empty batch
    assert not gn.supported(x.to(torch.int32), 4)
    assert not gn.supported(x.cpu(), 4)
    assert not gn.supported(x[0, 0, 0], 4)  # one dimension
    assert not gn.supported(torch.zeros(1, gn.MAX_C + 8, device="cuda"), 1)
    # 2^24 samples of one value: within the C and N * C limits, but one workgroup per sample is a grid of 2^32
    # threads, which does not launch -- refused by supported() and by the binding, run by the PyTorch ops
    wide = torch.ones(1 << 24, 1, device="cuda")
    assert gn.supported(wide[:-1], 1) and not gn.supported(wide, 1)
    with pytest.raises(RuntimeError):
        _C().gn_forward(wide, 1, None, None, EPS)
    before = gn.CALLS[0]
    assert float(gn.group_norm(wide, 1, None, None, EPS).abs().max()) == 0.0 and gn.CALLS[0] == before
    del wide
    with pytest.raises(RuntimeError):
        _C().gn_forward(x, 3, None, None, EPS)
    with pytest.raises(RuntimeError):
        _C().gn_forward(x[:0], 4, None, None, EPS)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.float64])
def test_op_autograd(dtype, monkeypatch):
    """ops.groupnorm.group_norm on the GPU: the kernels (f16 / f64 through f32), gradients by autograd,
    non-contiguous inputs; against the PyTorch-op path on the same device (TDL_GROUPNORM=torch)."""
    from tensorflow_distributed_learning_amd.ops import groupnorm as gn

    torch.manual_seed(0)
    x = torch.randn(3, 6, 16, 5, device="cuda").to(dtype).movedim(2, -1).requires_grad_(True)  # [3, 6, 5, 16] strided
    g = (torch.rand(16, device="cuda") + 0.5).requires_grad_(True)
    b = torch.randn(16, device="cuda").requires_grad_(True)
    dy = torch.randn(3, 6, 5, 16, device="cuda").to(dtype)
    before = gn.CALLS[0]
    y = gn.group_norm(x, 4, g, b, EPS)
    assert gn.CALLS[0] == before + 1 and y.dtype == dtype
    y.backward(dy)
    got = [y.detach(), x.grad.clone(), g.grad.clone(), b.grad.clone()]
    x.grad = g.grad = b.grad = None
    monkeypatch.setenv("TDL_GROUPNORM", "torch")
    y2 = gn.group_norm(x, 4, g, b, EPS)
    assert gn.CALLS[0] == before + 1
    y2.backward(dy)
    # both sides round their outputs to `dtype`; the sums of 120 terms differ by f32 rounding only
    tol = {torch.float32: 2e-5, torch.float64: 2e-5, torch.float16: 4e-3, torch.bfloat16: 3e-2}[dtype]
    for name, a, r in zip(("y", "dx", "dgamma", "dbeta"), got, (y2.detach(), x.grad, g.grad, b.grad)):
        scale = max(float(r.abs().max()), 1.0)
        assert float((a.double() - r.double()).abs().max()) <= tol * scale, name
