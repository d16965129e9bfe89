"""The scan kernels of csrc/kernels/lstm.hip through the bindings against the f64 reference of lstm_refs.py, at the
smallest shapes that cross each edge of lstm_plan (widths read from the plan).  Operands are 16-byte-aligned views
inside NaN-filled buffers.  Tolerance, from the references alone: E = max |emulation - f64 reference| on the case's
own inputs, every element of hs, c_last, dZ, dh0 and dc0 within 4 E + 1 ulp of its dtype."""
import numpy as np
import pytest
import torch

import kernel_refs as KR
import lstm_refs as LR

pytestmark = pytest.mark.gpu
DT = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
BASE = dict(B=3, T=3, U=32, state=False, dhs=True, last=False, rev=False)
# name -> what differs from BASE; U may be a function of the plan.  state: h0 / c0 given, dh0 / dc0 returned;
# dhs: a gradient for every step; last: dh_last / dc_last given
CASES = {
    "b1-idle-rows": dict(B=1), "b17-two-workgroups": dict(B=17), "t1-no-recurrence": dict(T=1, state=True),
    "t2": dict(T=2), "t5": dict(T=5), "u16-one-tile": dict(U=16), "u48-k-padding": dict(U=48),
    "u80-five-tiles": dict(U=80), "resident-widest": dict(U=lambda p: p["resident_max_u"]),
    "first-streamed": dict(U=lambda p: p["resident_max_u"] + 16), "max-u": dict(B=1, T=2, U=lambda p: p["max_u"]),
    "last-step-dhs-only": dict(dhs=False, last=True), "go-backwards": dict(T=4, rev=True, state=True),
    "state-in-and-out": dict(state=True, last=True), "streamed-state": dict(U=lambda p: p["max_u"] // 2 + 16,
                                                                            B=2, T=2, state=True, last=True),
}


def _C():
    from tensorflow_distributed_learning_amd.ops import hip

    return hip()


def _case(name, dtype):
    c = dict(BASE, **CASES[name])
    if callable(c["U"]):
        c["U"] = c["U"](_C().lstm_plan(1, 1, 16, dtype == torch.bfloat16))
    return c


def _dev(vals, dtype):
    """vals as a 16-byte-aligned view with 16 NaN elements in front of and behind it."""
    if vals is None:
        return None
    buf = torch.full((vals.size + 32,), float("nan"), dtype=dtype, device="cuda")
    v = buf[16:16 + vals.size].view(vals.shape)
    v.copy_(torch.from_numpy(vals).to(dtype))
    assert v.data_ptr() % 16 == 0
    return v


def _inputs(c, dtype, seed=0):
    rng, (B, T, U) = np.random.default_rng(seed), (c["B"], c["T"], c["U"])
    f = lambda *s, k=1.0: (rng.standard_normal(s) * k).astype(np.float32)  # noqa: E731
    v = dict(zx=f(B, T, 4 * U), R=f(U, 4 * U, k=U ** -0.5), h0=f(B, U, k=0.5), c0=f(B, U), dhs=f(B, T, U),
             dh_last=f(B, U), dc_last=f(B, U))
    if dtype == torch.bfloat16:  # (c0 / dc_last are f32 in both)
        v.update({k: KR.bf16_bits_to_f64(KR.bf16_rne(v[k])).astype(np.float32) for k in v if k not in ("c0", "dc_last")})
    for k, on in (("h0", c["state"]), ("c0", c["state"]), ("dhs", c["dhs"]), ("dh_last", c["last"]), ("dc_last", c["last"])):
        v[k] = v[k] if on else None
    return v


def _run(c, dtype, v):
    K, f32 = _C(), torch.float32
    zx, R, h0, dhs, dhl = (_dev(v[k], dtype) for k in ("zx", "R", "h0", "dhs", "dh_last"))
    c0, dcl = _dev(v["c0"], f32), _dev(v["dc_last"], f32)
    hs, hl, cl, gates, cs = K.lstm_forward(zx, R, h0, c0, c["rev"], True)
    dz, dh0, dc0 = K.lstm_backward(gates, cs, R, c0, dhs, dhl, dcl, c["rev"], c["state"])
    torch.cuda.synchronize()
    out = dict(hs=hs, h_last=hl, c_last=cl, dz=dz)
    if c["state"]:
        out.update(dh0=dh0, dc0=dc0)
    return out


@DT
@pytest.mark.parametrize("name", list(CASES))
def test_cases_against_f64(name, dtype):
    c, bf16 = _case(name, dtype), dtype == torch.bfloat16
    v = _inputs(c, dtype)
    got = _run(c, dtype, v)
    kw = dict(h0=v["h0"], c0=v["c0"], dhs=v["dhs"], dh_last=v["dh_last"], dc_last=v["dc_last"], rev=c["rev"])
    ref = LR.lstm_scan_ref(v["zx"], v["R"], mode="f64", **kw)
    emu = LR.lstm_scan_ref(v["zx"], v["R"], mode="bf16" if bf16 else "f32", **kw)
    for k, t in got.items():
        lowp = bf16 and k not in ("c_last", "dc0")
        E = np.abs(emu[k] - ref[k]).max()
        err = np.abs(t.double().cpu().numpy() - ref[k])
        print(f"[lstm kernels] {name} {k}: E {E:.3g}, kernel error {err.max():.3g}")
        tol = 4.0 * E + (KR.ulp_bf16 if lowp else KR.ulp32)(ref[k])
        assert np.isfinite(E) and (err <= tol).all(), f"{k}: worst error {err.max():.3g}, E {E:.3g}"


@DT
def test_plan_tells_resident_from_streamed(dtype):
    bf16 = dtype == torch.bfloat16
    u = _C().lstm_plan(1, 1, 16, bf16)["resident_max_u"]
    assert _C().lstm_plan(3, 3, u, bf16)["resident"] and not _C().lstm_plan(3, 3, u + 16, bf16)["resident"]
    assert _C().lstm_plan(17, 3, u, bf16)["workgroups"] == 2


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
    assert n["hs"][4].isnan().any() and n["dz"][4].isnan().any()
