"""The kernels of csrc/kernels/layernorm.hip through the bindings against the f64 references of layernorm_refs.py, at
the smallest shapes that cross each edge of ln_plan (widths read from the plan).  Operands are 16-byte-aligned views
inside NaN-filled buffers: a read outside the operand poisons a sum.  Tolerance, from the references alone:
E = max |emulation - f64 reference| on the case's own inputs, every element within 4 E + 1 ulp of the output dtype.
"""
import numpy as np
import pytest
import torch

import kernel_refs as R
import layernorm_refs as LR

pytestmark = pytest.mark.gpu
EPS = 1e-3
DT = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
RMS = pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
# name -> (R, C) from the plan's widths p and v = elements per 16 bytes; R = 0: rows_wg + 1 rows (two blocks)
SHAPES = {
    "c1": lambda p, v: (5, 1), "c3-per-element": lambda p, v: (5, 3), "one-vector": lambda p, v: (3, v),
    "idle-lanes": lambda p, v: (3, 5 * v), "one-row": lambda p, v: (1, 6 * v), "odd-1023": lambda p, v: (3, 1023),
    "sub-wave-widest": lambda p, v: (9, p["sub_wave_max_c"]), "sub-wave-plus": lambda p, v: (9, p["sub_wave_max_c"] + v),
    "sub-widest": lambda p, v: (5, p["sub_max_c"]), "sub-plus": lambda p, v: (5, p["sub_max_c"] + v),
    "wave-widest": lambda p, v: (5, p["wave_max_c"]), "wave-plus": lambda p, v: (5, p["wave_max_c"] + v),
    "per-element-widest": lambda p, v: (2, p["max_c_per_element"] - 1), "max-c": lambda p, v: (0, p["max_c"]),
    "two-blocks-sub": lambda p, v: (0, 2 * v),
}


def _C():
    from tensorflow_distributed_learning_amd.ops import hip

    return hip()


def _shape(name, dtype):
    bf16 = dtype == torch.bfloat16
    rows, C = SHAPES[name](_C().ln_plan(1, 1, bf16), 8 if bf16 else 4)
    if rows == 0:
        rows = _C().ln_plan(1, C, bf16)["rows_wg"] + 1
        assert _C().ln_plan(rows, C, bf16)["blocks"] == 2
    return rows, C


def _dev(vals, dtype):
    """vals as a 16-byte-aligned view with 16 NaN elements in front of and behind it."""
    if vals is None:
        return None
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    buf = torch.full((vals.size + 32,), float("nan"), dtype=dtype, device="cuda")
    v = buf[16:16 + vals.size].view(vals.shape)
    v.copy_(torch.from_numpy(vals).to(dtype))
    assert v.data_ptr() % 16 == 0
    return v


def _np(t):
    return t.detach().double().cpu().numpy()


def _run(shape, dtype, rms, seed=0, mean=0.5, std=2.0, gamma=True, beta=True, acc=0, edit=None, x_dy=None):
    """One forward + backward through the bindings: the inputs (numpy) and the outputs (torch)."""
    bf16 = dtype == torch.bfloat16
    rng = np.random.default_rng(seed)
    x, dy = rng.standard_normal(shape) * std + mean, rng.standard_normal(shape)
    x, dy = x_dy if x_dy is not None else (x.astype(np.float32), dy.astype(np.float32))
    if bf16:
        x, dy = (R.bf16_bits_to_f64(R.bf16_rne(v)).astype(np.float32) for v in (x, dy))
    if edit is not None:
        edit(x)
    rng, C = np.random.default_rng(seed + 1000), shape[1]  # the parameters depend on (seed, C) alone
    g, b, dg0, db0 = [(rng.random(C) + 0.5).astype(np.float32)] + [rng.standard_normal(C).astype(np.float32) for _ in "123"]
    g, b = (g if gamma else None), (b if beta and not rms else None)
    dg0, db0 = (dg0 if acc & 1 else None), (db0 if acc & 2 and not rms else None)
    tx, tdy = _dev(x, dtype), _dev(dy, dtype)
    tg, tb, tdg, tdb = (_dev(v, torch.float32) for v in (g, b, dg0, db0))
    y, st = _C().ln_forward(tx, tg, tb, EPS, rms)
    dx, dg, db = _C().ln_backward(tdy, tx, tg, st, rms, tdg, tdb)
    assert (tdg is None or dg.data_ptr() == tdg.data_ptr()) and (tdb is None or db.data_ptr() == tdb.data_ptr())
    assert (db is None) == rms
    torch.cuda.synchronize()
    return dict(x=x, dy=dy, g=g, b=b, dg0=dg0, db0=db0, y=y, st=st, dx=dx, dg=dg, db=db)


def _check(shape, dtype, rms, rows=None, **kw):
    """_run against the references.  rows: boolean [R] of the rows to compare (dgamma / dbeta are then left out)."""
    o = _run(shape, dtype, rms, **kw)
    bf16 = dtype == torch.bfloat16
    with np.errstate(all="ignore"):
        f = LR.ln_fwd_ref(o["x"], o["g"], o["b"], EPS, rms)
        e = LR.ln_fwd_emul(o["x"], o["g"], o["b"], EPS, rms, bf16=bf16)
        f.update(LR.ln_bwd_ref(o["dy"], o["x"], o["g"], EPS, rms, o["dg0"], o["db0"]))
        e.update(LR.ln_bwd_emul(o["dy"], o["x"], o["g"], e["mean"], e["r"], rms, o["dg0"], o["db0"], bf16=bf16))
    st = _np(o["st"])
    got = dict(mean=st[:, 0], r=st[:, 1], y=_np(o["y"]), dx=_np(o["dx"]))
    if rows is None:
        got.update(dgamma=_np(o["dg"]), **({} if rms else dict(dbeta=_np(o["db"]))))
    for k, v in got.items():  # (the f64 statistics are held to f32 ulps like the f32 outputs; they are far closer)
        sel = rows if rows is not None and k not in ("dgamma", "dbeta") else slice(None)
        with np.errstate(invalid="ignore"):
            E, err = np.abs(e[k] - f[k])[sel].max(), np.abs(v - f[k])[sel]
        tol = 4.0 * E + (R.ulp_bf16 if bf16 and k in ("y", "dx") else R.ulp32)(f[k])[sel]
        print(f"[ln kernels] {k}: E {E:.3g}, kernel error {err.max():.3g}")
        assert np.isfinite(E) and (err <= tol).all(), f"{k}: worst error {err.max():.3g}, E {E:.3g}"
    return o, f, e


@DT
@RMS
@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_against_f64(name, rms, dtype):
    _check(_shape(name, dtype), dtype, rms, seed=1)


@DT
def test_the_shapes_cross_the_plan_edges(dtype):
    bf16 = dtype == torch.bfloat16
    plan = lambda n: _C().ln_plan(*_shape(n, dtype), bf16)  # noqa: E731
    assert plan("c3-per-element")["vec"] == 1 and plan("odd-1023")["vec"] == 1 and plan("one-vector")["vec"] > 1
    assert plan("idle-lanes")["L"] == (8 if bf16 else 4) and plan("one-row")["rows_fwd"] > 1  # 5 columns
    assert plan("sub-wave-widest")["L"] == 32 and plan("sub-wave-plus")["L"] == 64
    assert [plan(n)["plan"] for n in ("sub-widest", "sub-plus", "wave-widest", "wave-plus", "max-c")] == [0, 1, 1, 2, 2]
    assert [plan(n)["L_bwd"] for n in ("sub-plus", "per-element-widest", "max-c")] == [128, 512, 1024]


@DT
@RMS
@pytest.mark.parametrize("gamma,beta,acc", [(False, False, 0), (True, False, 0), (False, True, 0), (True, True, 1),
                                            (True, True, 2), (True, True, 3)])
@pytest.mark.parametrize("name", ["idle-lanes", "c3-per-element", "sub-plus"])
def test_switches_and_gradients_added_into_targets(name, gamma, beta, acc, rms, dtype):
    shape = _shape(name, dtype)
    o, _, _ = _check(shape, dtype, rms, seed=3, gamma=gamma, beta=beta, acc=acc)
    plain = _run(shape, dtype, rms, seed=3) if acc else None
    for bit, k, k0 in ((1, "dg", "dg0"), (2, "db", "db0")) if acc else ():
        if o[k] is not None:  # the given target holds prefill + gradient, the other is returned fresh
            assert torch.equal(o[k], torch.from_numpy(o[k0]).cuda() + plain[k] if acc & bit else plain[k])


@DT
@pytest.mark.parametrize("C", [48, 1024])
def test_large_mean(C, dtype):
    """mean / std = 300: the centred f64 statistics keep the bound; the same formulas with an f32 uncentred
    variance do not (shown on the f32 data, where the output's own rounding does not hide it)."""
    o, f, e = _check((3, C), dtype, False, seed=4, mean=300.0, std=1.0)
    if dtype == torch.float32:
        e32 = LR.ln_fwd_emul(o["x"], o["g"], o["b"], EPS, var="f32-uncentred")
        assert (np.abs(e32["y"] - f["y"]) > 4 * np.abs(e["y"] - f["y"]).max() + R.ulp32(f["y"])).any()


@DT
@RMS
@pytest.mark.parametrize("name", ["idle-lanes", "odd-1023", "wave-plus"])
def test_rows_are_independent_and_runs_repeat(name, rms, dtype):
    """y[i] and dx[i] are the bits of row i run alone; two runs are bit-identical."""
    shape = _shape(name, dtype)
    whole, again = _run(shape, dtype, rms, seed=7), _run(shape, dtype, rms, seed=7)
    for k in ("y", "st", "dx", "dg", "db"):
        assert (whole[k] is None and again[k] is None) or torch.equal(whole[k], again[k]), k
    for i in (0, shape[0] - 1):
        one = _run((1, shape[1]), dtype, rms, seed=7, x_dy=(whole["x"][i:i + 1], whole["dy"][i:i + 1]))
        assert all(torch.equal(one[k][0], whole[k][i]) for k in ("y", "dx", "st")), f"row {i}"


@DT
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("name", ["idle-lanes", "c3-per-element", "sub-plus"])
def test_non_finite_stays_in_its_row(name, bad, dtype):
    shape = _shape(name, dtype)
    rows = np.arange(shape[0]) != 1
    o, _, _ = _check(shape, dtype, False, seed=6, edit=lambda x: x.__setitem__((1, shape[1] // 2), bad), rows=rows)
    clean = _run(shape, dtype, False, seed=6)
    for k in ("y", "dx"):
        assert not torch.isfinite(o[k][1].float()).any(), f"{k}: the poisoned row must not look finite"
        assert torch.equal(o[k][torch.from_numpy(rows)], clean[k][torch.from_numpy(rows)]), f"{k}: another row changed"
    assert torch.equal(o["db"], clean["db"])  # dbeta sums dy alone: it never sees x


def test_supported():
    from tensorflow_distributed_learning_amd.ops import layernorm as ln

    x = torch.randn(2, 5, 4, 8, device="cuda")
    assert ln.supported(x) and ln.supported(x.bfloat16(), 2) and ln.supported(x, 4)
    assert not ln.supported(x.cpu()) and not ln.supported(x[:0]) and not ln.supported(x.to(torch.int32))
    assert not ln.supported(x, (1,)) and not ln.supported(x, 5)  # a non-trailing axis is not the kernels'
    wide = torch.zeros(1, ln.MAX_C + 4, device="cuda")
    assert ln.supported(wide[:, :-4]) and not ln.supported(wide) and not ln.supported(wide[:, :ln.MAX_C_PER_ELEMENT + 1])
    with pytest.raises(RuntimeError):
        _C().ln_forward(wide, None, None, EPS)
