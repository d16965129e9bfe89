"""The scan kernels of csrc/kernels/gru.hip through the bindings against the f64 reference of gru_refs.py, at the
smallest shapes that cross each edge of gru_plan (widths read from the plan).  Operands are 16-byte-aligned views
inside NaN-filled buffers.  Tolerance, from the references alone (as tests/test_lstm_kernels_gpu.py): E = max
|emulation - f64 reference| on the case's own inputs, every element of hs, h_last, dzx, dzh and dh0 within
4 E + 1 ulp of its dtype."""
import numpy as np
import pytest
import torch

import gru_refs as GR
import kernel_refs as KR
from test_lstm_kernels_gpu import _C, _dev  # the extension; NaN-fenced aligned device views

pytestmark = pytest.mark.gpu
DT = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
BASE = dict(B=3, T=3, U=32, state=False, dhs=True, last=False, rev=False, bias=True)
# name -> what differs from BASE; U may be a function of the plan.  state: h0 given, dh0 returned; dhs: a gradient
# for every step; last: dh_last given; bias: b_rec given
CASES = {
    "b1-idle-rows": dict(B=1), "b17-two-workgroups": dict(B=17), "t1-no-recurrence": dict(T=1, state=True),
    "t2": dict(T=2), "t5": dict(T=5), "u16-one-tile": dict(U=16), "u48-k-padding": dict(U=48),
    "resident-widest": dict(U=lambda p: p["resident_max_u"]),
    "first-streamed": dict(U=lambda p: p["resident_max_u"] + 16), "max-u": dict(B=1, T=2, U=lambda p: p["max_u"]),
    "dh-last-only": dict(dhs=False, last=True), "go-backwards": dict(T=4, rev=True, state=True, last=True),
    "no-recurrent-bias": dict(bias=False),
    "streamed-state": dict(U=lambda p: p["resident_max_u"] + 32, B=2, T=2, state=True, last=True),
}


def _case(name, dtype):
    c = dict(BASE, **CASES[name])
    if callable(c["U"]):
        c["U"] = c["U"](_C().gru_plan(1, 1, 16, dtype == torch.bfloat16))
    return c


def _inputs(c, dtype, seed=0):
    rng, (B, T, U) = np.random.default_rng(seed), (c["B"], c["T"], c["U"])
    f = lambda *s, k=1.0: (rng.standard_normal(s) * k).astype(np.float32)  # noqa: E731
    v = dict(zx=f(B, T, 3 * U), R=f(U, 3 * U, k=U ** -0.5), b_rec=f(3 * U, k=0.5), h0=f(B, U, k=0.5), dhs=f(B, T, U),
             dh_last=f(B, U))
    if dtype == torch.bfloat16:  # (b_rec is f32 in both)
        v.update({k: KR.bf16_bits_to_f64(KR.bf16_rne(v[k])).astype(np.float32) for k in v if k != "b_rec"})
    for k, on in (("b_rec", c["bias"]), ("h0", c["state"]), ("dhs", c["dhs"]), ("dh_last", c["last"])):
        v[k] = v[k] if on else None
    return v


def _run(c, dtype, v):
    K = _C()
    zx, R, h0, dhs, dhl = (_dev(v[k], dtype) for k in ("zx", "R", "h0", "dhs", "dh_last"))
    hs, hl, saved = K.gru_forward(zx, R, _dev(v["b_rec"], torch.float32), h0, c["rev"], True)
    dzx, dzh, dh0 = K.gru_backward(saved, hs, R, h0, dhs, dhl, c["rev"], c["state"])
    torch.cuda.synchronize()
    out = dict(hs=hs, h_last=hl, dzx=dzx, dzh=dzh)
    if c["state"]:
        out.update(dh0=dh0)
    return out


@DT
@pytest.mark.parametrize("name", list(CASES))
def test_cases_against_f64(name, dtype):
    c, bf16 = _case(name, dtype), dtype == torch.bfloat16
    v = _inputs(c, dtype)
    got = _run(c, dtype, v)
    kw = dict(b_rec=v["b_rec"], h0=v["h0"], dhs=v["dhs"], dh_last=v["dh_last"], rev=c["rev"])
    ref = GR.gru_scan_ref(v["zx"], v["R"], mode="f64", **kw)
    emu = GR.gru_scan_ref(v["zx"], v["R"], mode="bf16" if bf16 else "f32", **kw)
    for k, t in got.items():
        E = np.abs(emu[k] - ref[k]).max()
        err = np.abs(t.double().cpu().numpy() - ref[k])
        print(f"[gru kernels] {name} {k}: E {E:.3g}, kernel error {err.max():.3g}")
        tol = 4.0 * E + (KR.ulp_bf16 if bf16 else KR.ulp32)(ref[k])
        assert np.isfinite(E) and (err <= tol).all(), f"{k}: worst error {err.max():.3g}, E {E:.3g}"


@DT
def test_plan_and_bias_gradient(dtype):
    K, bf16 = _C(), dtype == torch.bfloat16
    u = K.gru_plan(1, 1, 16, bf16)["resident_max_u"]
    assert K.gru_plan(3, 3, u, bf16)["resident"] and not K.gru_plan(3, 3, u + 16, bf16)["resident"]
    assert K.gru_plan(17, 3, u, bf16)["workgroups"] == 2 and u > K.lstm_plan(1, 1, 16, bf16)["resident_max_u"]
    # db_rec: column sums over B T = 5 * 13 rows (more than the kernel's 32 row lanes), 48 columns (1.5 blocks),
    # added into a target; exact in f64 up to the one f32 rounding of the sum and of the add
    x = _dev(np.random.default_rng(1).standard_normal((5, 13, 48)).astype(np.float32), dtype)
    want = x.double().sum((0, 1))
    tgt = torch.ones(48, device="cuda")
    assert K.gru_bias_grad(x, tgt) is tgt and torch.equal(K.gru_bias_grad(x), want.float())
    assert torch.equal(tgt, 1 + want.float())


@DT
def test_nan_stays_in_its_row_and_runs_are_identical(dtype):
    c = dict(BASE, B=18, state=True, last=True)
    v = _inputs(c, dtype)
    a, b = _run(c, dtype, v), _run(c, dtype, v)
    assert all(torch.equal(a[k], b[k]) for k in a)
    v["zx"][4, 1, 7] = np.nan
    n = _run(c, dtype, v)
    rows = torch.arange(c["B"], device="cuda") != 4
    for k in a:
        assert torch.equal(n[k][rows], a[k][rows]), k
    assert n["hs"][4].isnan().any() and n["dzx"][4].isnan().any()
