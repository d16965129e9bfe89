"""The batch-norm kernels of csrc/kernels/bn.hip at their edges, called through the bindings and compared with
the f64 references of tests/kernel_refs.py: row counts around the partial pass's chunk, several parts with a
short last one, the grid-stride elementwise kernels over many strides (channel advance, both unrolls),
partial rows given by a producer (the pre-reduction above 1024 rows), the options of the bindings, data with
a large mean, NaN / Inf / constant channels, NaN payloads in the bf16 stores, and the refused shapes.

Every operand is a view into the middle of a NaN-filled buffer (one row of NaN on each side, 16-byte
aligned): a read outside the operand poisons a sum.

Tolerances come from the references alone: E = max |f32 emulation - f64 reference| on the case's own inputs
(kernel_refs.bn_*_emul_f32: the kernels' formulas with a sequential f32 sum per channel), and every compared
element must lie within 4 E + 1 ulp of the output dtype at the reference's magnitude.

ReLU mask decisions (mode 1, recomputed by the kernel from x and its own f32 scale / shift): an element whose
reference pre-activation is within tau = |x| tol(scale) + tol(shift) of zero may legitimately fall on either
side.  Such elements get dy = 0, so that neither side's decision reaches a sum or dx; each case asserts that
they are at most 0.5 % of its elements (largest seen: 0.037 %).  Every other element's decision then shows in dx
(a wrong one is an error of |A dy|, far above the tolerance).  Mode 2 masks by the stored y, which the
reference reads too: nothing is excluded there.  Where tau would cover more than the cap (offset data, 1 to 3
rows) mode 1 takes the mask from the kernel's own f32 scale / shift instead (kernel_mask in _check).
"""
import contextlib

import numpy as np
import pytest
import torch

import kernel_refs as R

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-3, 0.9
DTYPES = [torch.float32, torch.bfloat16]
MAX_EXCLUDED = 0.005
REPORT = {}  # quantity -> [largest E, largest kernel error] over the module (printed at the end, for the record)


def _C():
    from tensorflow_distributed_learning_amd.ops import hip

    return hip()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(REPORT):
        print(f"\n[bn edges] {k}: largest E {REPORT[k][0]:.3g}, largest kernel error {REPORT[k][1]:.3g}", end="")
    print()


@contextlib.contextmanager
def _tuning(max_parts=0, elem_blocks=0, elem_unroll=0, grid_stride=False):
    """Sweep hooks set for one case and put back to the defaults of bn.hip (both grid caps)."""
    C = _C()
    try:
        C.bn_set_tuning(max_parts, elem_blocks, elem_unroll, 0)
        if grid_stride:
            C.bn_set_elementwise(0, 4)
        yield
    finally:
        C.bn_set_tuning(512, 4096, 1, 8192)
        C.bn_set_elementwise(1, 4)


def chunk_of(C):
    return (256 // (C // 8)) * 4


def _bf(v):
    return R.bf16_bits_to_f64(R.bf16_rne(v)).astype(np.float32)


def _dev(vals, dtype):
    """vals [M, C] as a 16-byte-aligned view with a row of NaN in front of and behind it."""
    M, C = vals.shape
    buf = torch.full((M + 2, C), float("nan"), dtype=dtype, device="cuda")
    v = buf[1:M + 1]
    v.copy_(torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float32)).to(dtype))
    assert v.data_ptr() % 16 == 0 and v.is_contiguous()
    return v


def _vec(vals):
    """An f32 [C] parameter between two NaN-filled 16-byte blocks."""
    buf = torch.full((len(vals) + 8,), float("nan"), dtype=torch.float32, device="cuda")
    v = buf[4:4 + len(vals)]
    v.copy_(torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float32)))
    return v


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _inputs(M, C, bf16, seed, mean=0.5, std=2.0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((M, C)) * std + mean).astype(np.float32)
    dy = rng.standard_normal((M, C)).astype(np.float32)
    res = rng.standard_normal((M, C)).astype(np.float32)
    if bf16:
        x, dy, res = _bf(x), _bf(dy), _bf(res)
    p = dict(g=(rng.random(C) + 0.5).astype(np.float32), b=rng.standard_normal(C).astype(np.float32),
             mm=rng.standard_normal(C).astype(np.float32), mv=(rng.random(C) + 0.5).astype(np.float32),
             off=rng.standard_normal(C).astype(np.float32), dg0=rng.standard_normal(C).astype(np.float32),
             db0=rng.standard_normal(C).astype(np.float32))
    return x, dy, res, p


def _tol(ref, emu, ulp, sel=None):
    with np.errstate(invalid="ignore"):
        d = np.abs(emu - ref)
    if sel is not None:
        d = d[..., sel]
    E = float(np.nanmax(d)) if d.size else 0.0
    return E, 4.0 * E + ulp(ref)


def _cmp(name, got, ref, emu, ulp, sel=None):
    """got within 4 E + 1 ulp of ref on the channels `sel` (all by default); name: the REPORT key."""
    E, tol = _tol(ref, emu, ulp, sel)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)
    if sel is not None:
        err, tol = err[..., sel], tol[..., sel]
    assert np.isfinite(err).all(), f"{name}: non-finite output"
    rec = REPORT.setdefault(name, [0.0, 0.0])
    rec[0], rec[1] = max(rec[0], E), max(rec[1], float(err.max()) if err.size else 0.0)
    bad = err > tol
    assert not bad.any(), (f"{name}: {int(bad.sum())} elements off, worst error {err.max():.3g} "
                           f"(E {E:.3g}, tolerance there {tol[np.unravel_index(err.argmax(), err.shape)]:.3g})")


def _check(M, C, dtype, mode, seed=0, mean=0.5, std=2.0, gamma=True, beta=True, moving=True, mean_off=False,
           momentum=MOM, acc=0, edit=None, good=None, label="", kernel_mask=False):
    """One forward + backward of [M, C] through the bindings against the references.  mode 0 plain, 1 relu,
    2 add + relu.  edit(x): changes the input in place (special values); good: channels to compare (the
    others are the caller's); label: prefix of the REPORT keys.  kernel_mask (mode 1): the references take the
    mask from the kernel's own returned f32 scale / shift through a CPU f32 fma, which is the kernel's decision
    bit for bit (the sign of an fma survives the f64 detour), so nothing is excluded and every other output is
    still checked against f64 -- for data on which tau would cover more than the cap.  Returns what the caller
    may want to look at."""
    Ck = _C()
    bf16 = dtype == torch.bfloat16
    ulp_out = R.ulp_bf16 if bf16 else R.ulp32
    x, dy, res, p = _inputs(M, C, bf16, seed, mean, std)
    if edit is not None:
        edit(x)
    g, b = (p["g"] if gamma else None), (p["b"] if beta else None)
    mm, mv = (p["mm"], p["mv"]) if moving else (None, None)
    off = p["off"] if mean_off else None
    relu, resid = mode != 0, (res if mode == 2 else None)
    with np.errstate(all="ignore"):
        f = R.bn_fwd_ref(x, g, b, mm, mv, momentum, EPS, resid, off, relu)
        e = R.bn_fwd_emul_f32(x, g, b, mm, mv, momentum, EPS, resid, off, relu, bf16=bf16)
    sel = None if good is None else np.asarray(good)

    tx, tdy = _dev(x, dtype), _dev(dy, dtype)
    tg, tb = (_vec(g) if gamma else None), (_vec(b) if beta else None)
    tmm, tmv = (_vec(mm), _vec(mv)) if moving else (None, None)
    y, st = Ck.bn_forward_train(tx, tg, tb, tmm, tmv, momentum, EPS, relu, _dev(res, dtype) if mode == 2 else None,
                                _vec(off) if mean_off else None, None)
    st_np, y_np = _np(st), _np(y)
    tag = "bf16" if bf16 else "f32"
    for i, k in enumerate(("mean", "invstd", "scale", "shift")):
        _cmp(label + k, st_np[i], f[k], e[k], R.ulp32, sel)
    if moving:
        _cmp(label + "moving_mean", _np(tmm), f["moving_mean"], e["moving_mean"], R.ulp32, sel)
        _cmp(label + "moving_var", _np(tmv), f["moving_var"], e["moving_var"], R.ulp32, sel)
    _cmp(label + f"y {tag}", y_np, f["y"], e["y"], ulp_out, sel)

    # backward: the kernel gets its own forward statistics (and, mode 2, its own stored y)
    excluded = 0.0
    ref_mode, y_mask = mode, y_np
    if mode == 1 and kernel_mask:
        ref_mode = 2  # (the references' mode 2 masks by y_mask > 0)
        y_mask = R._fma32(x, st_np[2].astype(np.float32), st_np[3].astype(np.float32)).astype(np.float64)
        assert ((y_np > 0) == (y_mask > 0)).all()  # the forward's ReLU decided the same way
    elif mode == 1:
        _, tol_sc = _tol(f["scale"], e["scale"], R.ulp32, sel)
        _, tol_sh = _tol(f["shift"], e["shift"], R.ulp32, sel)
        near = np.abs(f["pre"]) <= np.abs(x.astype(np.float64)) * tol_sc + tol_sh
        if sel is not None:
            near[:, np.setdiff1d(np.arange(C), sel)] = False
        excluded = float(near.mean())
        assert excluded <= MAX_EXCLUDED, f"{excluded:.4%} of the elements have an undecided mask"
        rec = REPORT.setdefault(label + "excluded mask share", [0.0, 0.0])
        rec[0] = rec[1] = max(rec[0], excluded)
        dy = np.where(near, np.float32(0), dy)
        tdy = _dev(dy, dtype)
        # outside the excluded set the forward's ReLU took the reference's side
        agree = ((y_np > 0) == (f["pre"] > 0)) | near
        assert (agree if sel is None else agree[:, sel]).all()
    dg0, db0 = (p["dg0"] if acc & 1 else None), (p["db0"] if acc & 2 else None)
    tdg, tdb = (_vec(dg0) if acc & 1 else None), (_vec(db0) if acc & 2 else None)
    with np.errstate(all="ignore"):
        bw = R.bn_bwd_ref(dy, x, g, f["mean"], f["invstd"], ref_mode, f["scale"], f["shift"], y_mask, dg0, db0)
        be = R.bn_bwd_emul_f32(dy, x, g, e["mean"], e["invstd"], ref_mode, e["scale"], e["shift"], y_mask, dg0, db0,
                               bf16=bf16)
    out = Ck.bn_backward(tdy, tx, y if mode == 2 else None, tg, st, mode, tdg, tdb, None)
    if acc & 1:
        assert out[1].data_ptr() == tdg.data_ptr()
    if acc & 2:
        assert out[2].data_ptr() == tdb.data_ptr()
    dx_np = _np(out[0])
    _cmp(label + "dgamma", _np(out[1]), bw["dgamma"], be["dgamma"], R.ulp32, sel)
    _cmp(label + "dbeta", _np(out[2]), bw["dbeta"], be["dbeta"], R.ulp32, sel)
    _cmp(label + f"dx {tag}", dx_np, bw["dx"], be["dx"], ulp_out, sel)
    if mode == 2:  # the residual's gradient: dy where the stored y is positive, bit for bit
        dz = _np(out[3])
        np.testing.assert_array_equal(dz if sel is None else dz[:, sel], bw["dz"] if sel is None else bw["dz"][:, sel])
    return dict(f=f, e=e, st=st_np, y=y_np, y_t=y, dx=dx_np, dgamma=_np(out[1]), dbeta=_np(out[2]), mv=_np(tmv) if moving else None,
                mm=_np(tmm) if moving else None, excluded=excluded)


# ------------------------------------------------------------------------------------- shapes
def _rows(C):
    c = chunk_of(C)
    return [1, 2, 3, c - 1, c, c + 1, 4 * c + 1]


SHAPES = [(M, C) for C in (8, 24, 96, 1000, 2048) for M in _rows(C)]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("M,C", SHAPES)
def test_bn_row_counts_around_the_chunk(M, C, dtype, mode):
    """k_bn_partial's unrolled loop, its tail and the `rr < R` guard (256 % (C/8) != 0 at C = 24, 96, 1000);
    M = 1 leaves the moving variance as computed.

    With 1 to 3 rows a channel's variance is zero or nearly so, and Q/M - mean^2 carries an absolute error of
    about x^2 2^-24 that is measured against eps: tau then covers 1 to 100 % of the elements, so mode 1 takes the
    mask from the kernel's own scale / shift there (kernel_mask, see _check).  The data are the common ones."""
    _check(M, C, dtype, mode, seed=M * 7 + C, kernel_mask=M <= 3)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [8, 24, 96, 1000, 2048])
def test_bn_several_parts_short_last(C, dtype, mode):
    """max_parts = 3: 8 chunks + 3 rows in parts of 3 chunks, the last one 2 chunks + 3 rows."""
    M = 8 * chunk_of(C) + 3
    with _tuning(max_parts=3):
        _check(M, C, dtype, mode, seed=C)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("unroll", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [24, 96, 1000, 64])
def test_bn_grid_stride_channel_advance(C, dtype, unroll, mode):
    """k_bn_apply / k_bn_dx with a grid of 2 blocks: 8 and more grid strides per tensor, so the incremental
    channel (cstep, adv and its wrap at C) is what addresses the LDS tables; elem_unroll 2 is the U = 2
    instantiation (bf16).  C = 64 takes these kernels through bn_set_elementwise(0, 4)."""
    M = 4 * chunk_of(C) + 1
    assert M * C // 8 > 7 * 512
    with _tuning(elem_blocks=2, elem_unroll=unroll, grid_stride=True):
        _check(M, C, dtype, mode, seed=C + unroll)


def test_bn_tuning_hook_sets_the_two_grid_caps_separately():
    """elem_blocks is the grid-stride kernels' grid cap alone and the fourth argument the blocked kernels'
    (bn_get_tuning reads them back); 0 keeps a value; a blocked case gives the same bits under caps 1, 2 and the
    default."""
    Ck = _C()
    assert Ck.bn_get_tuning() == (512, 4096, 1, 8192)  # the defaults, which every case here restores
    x, _, _, p = _inputs(4099, 64, True, 3)
    tx, tg, tb = _dev(x, torch.bfloat16), _vec(p["g"]), _vec(p["b"])
    outs = []
    try:
        for caps, want in (((0, 2, 0, 0), (512, 2, 1, 8192)), ((0, 0, 0, 1), (512, 2, 1, 1)), ((0, 0, 2, 2), (512, 2, 2, 2)),
                           ((7, 4096, 1, 8192), (7, 4096, 1, 8192))):
            Ck.bn_set_tuning(*caps)
            assert Ck.bn_get_tuning() == want
            outs.append(Ck.bn_forward_train(tx, tg, tb, None, None, MOM, EPS, True, None, None, None)[0])
    finally:
        Ck.bn_set_tuning(512, 4096, 1, 8192)
    assert Ck.bn_get_tuning() == (512, 4096, 1, 8192)
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16))


# ------------------------------------------------------------------------------------- given partials
PARTS = [1, 63, 64, 65, 1024, 1025, 1087, 1088, 1089, 4097]


def _synthetic_part(P, C, seed):
    """[P + ceil(P/64)][2][C]: random sums in the first P rows (s ~ N(0, 1) and s^2 + [0.5, 1.5): with M = P
    rows the variance sum q / M - (sum s / M)^2 is at least 0.5 by Cauchy-Schwarz), NaN behind them (the
    pre-reduction's output rows)."""
    rng = np.random.default_rng(seed)
    part = np.full((P + (P + 63) // 64, 2, C), np.nan, dtype=np.float32)
    part[:P, 0] = rng.standard_normal((P, C))
    part[:P, 1] = part[:P, 0] ** 2 + rng.random((P, C)).astype(np.float32) + 0.5
    return part


def _seq32(a):
    s = np.zeros(a.shape[1], dtype=np.float32)
    for r in range(a.shape[0]):
        s = s + a[r]
    return s.astype(np.float64)


@pytest.mark.parametrize("C", [8, 96, 256])
@pytest.mark.parametrize("P", PARTS)
def test_bn_stats_from_given_partials(P, C):
    """bn_stats_train(part=...): k_bn_fwd_finalize over P rows, through k_bn_prereduce above 1024."""
    Ck = _C()
    part = _synthetic_part(P, C, P + C)
    x, _, _, p = _inputs(P, C, True, 1)
    M = P
    S, Q = part[:P, 0].astype(np.float64).sum(0), part[:P, 1].astype(np.float64).sum(0)
    Se, Qe = _seq32(part[:P, 0]), _seq32(part[:P, 1])

    def stats(S, Q, f32):
        g, b = p["g"].astype(np.float64), p["b"].astype(np.float64)
        mu = S / M
        var = np.maximum(Q / M - mu * mu, 0.0)
        inv = 1.0 / np.sqrt(var + R.f32(EPS))
        if not f32:
            return mu, inv, g * inv, b - mu * g * inv, var
        mu, inv = mu.astype(np.float32), inv.astype(np.float32)
        sc = p["g"] * inv
        return mu.astype(np.float64), inv.astype(np.float64), sc.astype(np.float64), \
            (p["b"] - mu * p["g"] * inv).astype(np.float64), var

    ref, emu = stats(S, Q, False), stats(Se, Qe, True)
    assert (ref[4] > 0.4).all()
    tpart = torch.from_numpy(part).cuda()
    tmm, tmv = _vec(p["mm"]), _vec(p["mv"])
    st = _np(Ck.bn_stats_train(_dev(x, torch.bfloat16), _vec(p["g"]), _vec(p["b"]), tmm, tmv, MOM, EPS, None, tpart))
    for i, k in enumerate(("mean", "invstd", "scale", "shift")):
        _cmp(f"{k} (given partials)", st[i], ref[i], emu[i], R.ulp32)
    m = R.f32(MOM)
    unb = [v[4] * M / (M - 1) if M > 1 else v[4] for v in (ref, emu)]
    _cmp("moving_var (given partials)", _np(tmv), p["mv"].astype(np.float64) * m + unb[0] * (1 - m),
         (p["mv"] * np.float32(MOM) + unb[1].astype(np.float32) * (np.float32(1) - np.float32(MOM))).astype(np.float64), R.ulp32)
    # the rows a producer wrote are left alone
    np.testing.assert_array_equal(tpart[:P].cpu().numpy(), part[:P])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [8, 96, 256])
@pytest.mark.parametrize("P", PARTS)
def test_bn_backward_from_given_partials(P, C, dtype):
    """bn_backward(part=...): dgamma / dbeta / the dx coefficients from P given rows of (sum dz, sum dz*x)."""
    Ck = _C()
    bf16 = dtype == torch.bfloat16
    part = _synthetic_part(P, C, 2 * P + C)
    M = 37
    x, dz, _, p = _inputs(M, C, bf16, P)
    rng = np.random.default_rng(P)
    st = np.stack([rng.standard_normal(C), rng.random(C) + 0.5, np.ones(C), np.zeros(C)]).astype(np.float32)
    mu, inv, g = st[0].astype(np.float64), st[1].astype(np.float64), p["g"].astype(np.float64)

    def bwd(S, Q, f32):
        dg, db = (Q - mu * S) * inv, S
        A, B = g * inv, -g * inv * inv * dg / M
        D = -A * db / M - B * mu
        if not f32:
            return dg, db, A * dz + B * x + D
        dx = R._fma32(A, dz, R._fma32(B, x, D))
        return dg.astype(np.float32).astype(np.float64), db.astype(np.float32).astype(np.float64), R._store(dx, bf16)

    ref = bwd(part[:P, 0].astype(np.float64).sum(0), part[:P, 1].astype(np.float64).sum(0), False)
    emu = bwd(_seq32(part[:P, 0]), _seq32(part[:P, 1]), True)
    out = Ck.bn_backward(_dev(dz, dtype), _dev(x, dtype), None, _vec(p["g"]), torch.from_numpy(st).cuda(), 1, None, None,
                         torch.from_numpy(part).cuda())
    _cmp("dgamma (given partials)", _np(out[1]), ref[0], emu[0], R.ulp32)
    _cmp("dbeta (given partials)", _np(out[2]), ref[1], emu[1], R.ulp32)
    _cmp("dx (given partials) " + ("bf16" if bf16 else "f32"), _np(out[0]), ref[2], emu[2], R.ulp_bf16 if bf16 else R.ulp32)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_bn_own_pass_with_more_than_1024_parts(mode):
    """max_parts = 4096 at [4104, 2048] bf16: 1026 parts of one chunk (4 rows), pre-reduced by k_bn_prereduce."""
    with _tuning(max_parts=4096):
        _check(4104, 2048, torch.bfloat16, mode, seed=9)


# ------------------------------------------------------------------------------------- options
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("opt", [dict(mean_off=True), dict(gamma=False), dict(beta=False), dict(gamma=False, beta=False),
                                 dict(moving=False), dict(acc=1), dict(acc=2), dict(acc=3), dict(momentum=0.0),
                                 dict(momentum=1.0)],
                         ids=["mean_off", "no_gamma", "no_beta", "no_gamma_beta", "no_moving", "acc_dgamma", "acc_dbeta",
                              "acc_both", "momentum0", "momentum1"])
def test_bn_options(opt, dtype, mode):
    """[301, 24] (two parts' worth of rows for one, ragged): each option of the bindings; mode 2 is the residual."""
    r = _check(301, 24, dtype, mode, seed=5, **opt)
    if opt.get("momentum") == 1.0:  # the moving statistics are kept bit for bit
        _, _, _, p = _inputs(301, 24, dtype == torch.bfloat16, 5)
        np.testing.assert_array_equal(r["mm"], p["mm"].astype(np.float64))
        np.testing.assert_array_equal(r["mv"], p["mv"].astype(np.float64))


# ------------------------------------------------------------------------------------- offset data
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("mean,std", [(8.0, 0.5), (30.0, 0.25)])
def test_bn_offset_data_within_derived_tolerance(mean, std, mode):
    """f32 randn * std + mean, M = 3000: the variance Q/M - mean^2 from f32 sums loses (mean/std)^2 of accuracy, and
    so does the sequential emulation that sizes the tolerance.  scale and shift are large and nearly cancel in
    x*scale + shift; tau = |x| tol(scale) + tol(shift) does not see that their errors cancel too, and would hold
    1.95 % of the elements at (8, 0.5) and all of them at (30, 0.25).  So mode 1 decides the mask from the kernel's
    own f32 scale / shift with a CPU f32 fma (kernel_mask, see _check): bit-exact, nothing excluded, and the
    statistics, y, dgamma, dbeta and dx are still held to the f64 reference."""
    _check(3000, 8, torch.float32, mode, seed=3, mean=mean, std=std, label=f"offset ({mean:g}, {std:g}) ", kernel_mask=True)


def test_bn_offset_data_beyond_the_supported_range():
    """Characterisation (csrc/kernels/bn.h): mean 100, std 0.1 in f32, M = 3000.  Q/M - mean^2 from f32 sums has
    no correct digit left; the kernel stays finite and bounded.  Measured relative error of invstd: kernel
    0.244, the sequential emulation 2.37 (one f32 sum of 3000 terms instead of 256 short ones)."""
    Ck = _C()
    x, _, _, p = _inputs(3000, 8, False, 3, mean=100.0, std=0.1)
    tmm, tmv = _vec(p["mm"]), _vec(p["mv"])
    y, st = Ck.bn_forward_train(_dev(x, torch.float32), _vec(p["g"]), _vec(p["b"]), tmm, tmv, MOM, EPS, False, None, None,
                                None)
    f = R.bn_fwd_ref(x, p["g"], p["b"], p["mm"], p["mv"], MOM, EPS)
    e = R.bn_fwd_emul_f32(x, p["g"], p["b"], p["mm"], p["mv"], MOM, EPS)
    st = _np(st)
    print(f"\n[bn edges] mean 100 std 0.1: relative invstd error kernel {np.abs(st[1] / f['invstd'] - 1).max():.3g}, "
          f"emulation {np.abs(e['invstd'] / f['invstd'] - 1).max():.3g}")
    for t in (y, tmm, tmv):
        assert torch.isfinite(t).all()
    assert np.isfinite(st).all()
    assert (st[1] <= 1.0 / np.sqrt(R.f32(EPS)) * (1 + 2.0 ** -23)).all() and (st[1] > 0).all()


# ------------------------------------------------------------------------------------- special values
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_bn_nan_or_inf_in_one_channel(value, dtype, mode):
    """One element of channel 5 is NaN (Inf): that channel's statistics, moving variance, parameter gradients
    and dx are NaN wherever the f64 reference's are (the mean of an Inf channel is Inf in both).  Its y is NaN in
    the reference (np.maximum keeps a NaN) and in the kernel without the fused ReLU; with it the kernel deviates
    as csrc/kernels/bn.h documents: fmaxf stores a NaN pre-activation as 0, which is asserted exactly.  The
    other channels are within tolerance."""
    M, C, bad = 301, 24, 5

    def edit(x):
        x[17, bad] = value

    good = [c for c in range(C) if c != bad]
    r = _check(M, C, dtype, mode, seed=6, edit=edit, good=good)
    f, st = r["f"], r["st"]
    for i, k in enumerate(("mean", "invstd", "scale", "shift")):
        assert np.isnan(f[k][bad]) == np.isnan(st[i][bad]), (k, f[k][bad], st[i][bad])
        assert np.isnan(f[k][bad]) or f[k][bad] == st[i][bad]
    assert np.isnan(f["invstd"][bad]) and np.isnan(f["moving_var"][bad]) and np.isnan(r["mv"][bad])
    assert np.isfinite(r["mm"][bad]) == np.isfinite(f["moving_mean"][bad])
    assert np.isnan(r["dgamma"][bad]) and np.isnan(r["dx"][:, bad]).all()
    assert np.isnan(f["y"][:, bad]).all()
    if mode == 0:
        assert np.isnan(r["y"][:, bad]).all()
    else:  # the documented deviation (bn.h): fmaxf stores a NaN pre-activation as exactly 0
        assert (r["y"][:, bad] == 0).all()


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_bn_constant_channel(dtype, mode):
    """Channel 2 is the constant 1.5 (exact in bf16, sums exact in f32): var == 0, invstd = 1/sqrt(eps), y = beta
    (+ residual) within tolerance and dx finite."""
    def edit(x):
        x[:, 2] = 1.5

    r = _check(301, 24, dtype, mode, seed=8, edit=edit)
    assert r["f"]["var"][2] == 0.0 and r["st"][0][2] == 1.5
    assert abs(r["st"][1][2] * np.sqrt(R.f32(EPS)) - 1) < 2.0 ** -22
    assert np.isfinite(r["dx"][:, 2]).all()


def test_bn_bf16_stores_keep_nan_payloads():
    """An f32 gamma whose NaN payload the integer rounding `u + 0x7fff + lsb` carries out of (into Inf or +-0): the
    f32 product the kernels round has that payload, and every stored bf16 must be a NaN of the same sign --
    forward (apply), and dx through the coefficient A = gamma * invstd.  Grid-stride and blocked kernels."""
    Ck = _C()
    M = 37
    for C, grid_stride in ((24, False), (64, True), (64, False)):
        x, dy, _, p = _inputs(M, C, True, 2)
        g = p["g"].copy()
        g[1:4] = R.NAN_PAYLOADS_F32
        tx = _dev(x, torch.bfloat16)
        with _tuning(grid_stride=grid_stride):
            y, st = Ck.bn_forward_train(tx, _vec(g), _vec(p["b"]), None, None, MOM, EPS, False, None, None, None)
            dx = Ck.bn_backward(_dev(dy, torch.bfloat16), tx, None, _vec(g), st, 0, None, None, None)[0]
        for name, t in (("y", y), ("dx", dx)):
            bits = t.view(torch.int16).cpu().numpy().view(np.uint16)[:, 1:4]
            assert R.bf16_is_nan(bits).all(), (name, C, grid_stride, [hex(v) for v in bits[0]])
        # y = fma(x, scale, shift) returns the NaN operand, scale = gamma * invstd, with its sign: the store keeps it
        ybits = y.view(torch.int16).cpu().numpy().view(np.uint16)[:, 1:4]
        assert ((ybits >> 15) == (R.bf16_rne(st[2][1:4].cpu().numpy()) >> 15)).all()
        ok = torch.isfinite(y.float()[:, 4:]).all() and torch.isfinite(dx.float()[:, 4:]).all()
        assert ok, "a NaN gamma leaked into other channels"


# ------------------------------------------------------------------------------------- refused shapes
def test_bn_refuses_empty_and_malformed_inputs():
    Ck = _C()
    dev = "cuda"
    g = torch.ones(8, device=dev)
    st = torch.zeros(4, 8, device=dev)
    for shape in ((0, 8), (4, 0)):
        x = torch.empty(shape, device=dev)
        with pytest.raises(RuntimeError, match="batch_norm"):
            Ck.bn_forward_train(x, None, None, None, None, MOM, EPS, False, None, None, None)
        with pytest.raises(RuntimeError, match="batch_norm"):
            Ck.bn_stats_train(x, None, None, None, None, MOM, EPS, None, None)
        with pytest.raises(RuntimeError, match="batch_norm"):
            Ck.bn_backward(x, x, None, None, st, 0, None, None, None)
    x = torch.randn(16, 8, device=dev)
    with pytest.raises(RuntimeError, match="y/x mismatch"):  # a short y would be read out of range
        Ck.bn_backward(x, x, torch.randn(8, 8, device=dev), g, st, 2, None, None, None)
    with pytest.raises(RuntimeError, match="y/x mismatch"):
        Ck.bn_backward(x, x, torch.randn(16, 8, device=dev).bfloat16(), g, st, 2, None, None, None)
    with pytest.raises(RuntimeError, match="stats"):
        Ck.bn_backward(x, x, None, g, st.cpu(), 0, None, None, None)


def test_empty_batch_takes_the_pytorch_path():
    from tensorflow_distributed_learning_amd.ops import batchnorm, pooling

    x = torch.empty(0, 4, 4, 8, device="cuda")
    assert not batchnorm.supported(x) and not pooling.supported(x)
    assert not batchnorm.supported(torch.empty(4, 0, device="cuda"))
    assert batchnorm.supported(torch.empty(1, 8, device="cuda")) and pooling.supported(torch.empty(1, 2, 2, 8, device="cuda"))
    y = pooling.max_pool_nhwc(x, (2, 2), (2, 2))
    assert y.shape == (0, 2, 2, 8)
