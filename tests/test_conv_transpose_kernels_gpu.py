"""The transposed-convolution kernels of csrc/kernels/conv_transpose.hip, called through the bindings and compared
with the float64 scatter-form references of tests/convt_refs.py on the same (bf16: pre-rounded, the weight too)
inputs.

Every operand is a view into the middle of a NaN-filled buffer, 16-byte aligned: a read outside the operand
poisons a result.  The bounds follow from the arithmetic contract (f32 accumulation on the MFMA, one rounding to
the output dtype), with u = 2^-24 for f32 output and 2^-8 for bf16 output, mag = the sum of the absolute values
of the terms:

  forward         |got - ref| <= (kh kw C + 2) 2^-23 mag + u |ref|        (dgrad: kh kw F)
  wgrad, db       |got - ref| <= (n + S + 1) 2^-23 mag + 2^-23 (|target0| + |ref|)    (n pixels, S plan splits)

With ReLU fused no pre-activation of the reference lies within the forward bound of zero (asserted: the seed).
"""
import numpy as np
import pytest
import torch

import convt_refs as TR
import kernel_refs as R

pytestmark = pytest.mark.gpu


def _C():
    from tensorflow_distributed_learning_amd.ops import hip

    return hip()


def _dev(vals, dtype):
    """vals as a 16-byte-aligned view with 16 NaN elements in front of and behind it."""
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    buf = torch.full((vals.size + 32,), float("nan"), dtype=dtype, device="cuda")
    v = buf[16:16 + vals.size].view(vals.shape)
    v.copy_(torch.from_numpy(vals).to(dtype))
    assert v.data_ptr() % 16 == 0 and v.is_contiguous()
    return v


def _np(t):
    return t.detach().double().cpu().numpy()


def _check(name, got, ref, tol):
    err = np.abs(_np(got).reshape(ref.shape) - ref)
    i = int(np.argmax(err - tol))
    print(f"[convt kernels] {name}: error {err.flat[i]:.3g} where it comes closest to its bound {tol.flat[i]:.3g}")
    assert np.isfinite(err).all(), f"{name}: non-finite output"
    assert (err <= tol).all(), f"{name}: {int((err > tol).sum())} elements off, worst {err.max():.3g}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", TR.CASES, ids=TR.IDS)
def test_kernels_against_f64(case, dtype):
    Ck = _C()
    shape, F, k, s, d, padding, op, act = case
    bf16 = dtype == torch.bfloat16
    N, H, W, C = shape
    geo4 = TR.geometry(shape, k, s, d, padding, op)
    oh, ow, pt, pl = geo4
    rng = np.random.default_rng(23)  # (a seed whose ReLU cases keep every pre-activation clear of zero)
    x = rng.standard_normal(shape).astype(np.float32)
    dy = rng.standard_normal((N, oh, ow, F)).astype(np.float32)
    w = rng.standard_normal(k + (F, C)).astype(np.float32)
    b = rng.standard_normal(F).astype(np.float32)
    if bf16:
        x, dy, w = (R.bf16_bits_to_f64(R.bf16_rne(v)).astype(np.float32) for v in (x, dy, w))
    geo = [s[0], s[1], d[0], d[1], pt, pl]

    # the plan shows that the case hits what it is there for
    plan = Ck.convt_plan(list(shape), F, k[0], k[1], oh, ow, geo)
    assert plan["phases"] == s[0] * s[1] and len(plan["phase_taps"]) == plan["phases"]
    assert sum(plan["phase_taps"]) == k[0] * k[1]
    empty = {((2, 2), (3, 3), (1, 1)): 5, ((3, 3), (2, 2), (2, 2)): 3}.get((k, s, d), 0)  # ke < s; odd phases
    assert plan["empty_phases"] == empty == sum(t == 0 for t in plan["phase_taps"])
    if k == (4, 4):
        assert plan["phase_taps"] == [4, 4, 4, 4]
    if k == (3, 3) and s == (2, 2) and d == (1, 1):
        assert sorted(plan["phase_taps"]) == [1, 2, 2, 4]
    if C == 40:
        assert plan["fwd_kchunks"] > 1 and plan["dgrad_kchunks"] > 1 and plan["fwd_colblocks"] == 2 and F % 16 == 8
    if C == 6:
        assert plan["fwd_vec"] == 0 and plan["dgrad_vec"] == 0
    if W == 37:
        assert plan["fwd_pixel_tiles"] > 1 and (N * H * W) % plan["fwd_pixels_per_tile"] not in (0, 1)
    if N == 4:
        assert plan["wgrad_splits"] > 1
    S = plan["wgrad_splits"]
    u = 2.0 ** -8 if bf16 else 2.0 ** -24
    xd, dyd, wd, bd = _dev(x, dtype), _dev(dy, dtype), _dev(w, torch.float32), _dev(b, torch.float32)

    # forward, with and without the bias
    mask = None
    for bias in (b, None):
        ref, mag = TR.forward(x, w, bias, s, d, geo4)
        tol = (k[0] * k[1] * C + 2) * 2.0 ** -23 * mag + u * np.abs(ref)
        if act:
            assert (np.abs(ref) > tol).all(), "the seed leaves a pre-activation within the bound of zero"
            if bias is not None:
                mask = ref > 0
            ref = np.maximum(ref, 0.0)
        y = Ck.convt_forward(xd, wd, bd if bias is not None else None, geo, oh, ow, act=act)
        _check("forward" + (" + bias" if bias is not None else ""), y, ref, tol)
        if bias is not None:
            y_saved = y
    if act:  # the backward kernels select dy by the saved output
        assert np.array_equal(_np(y_saved) > 0, mask)
        dy_eff, ym = dy * mask, y_saved
    else:
        dy_eff, ym = dy, None

    ref, mag = TR.dgrad(dy_eff, w, shape, s, d, geo4)
    dx = Ck.convt_dgrad(dyd, wd, H, W, geo, dy_mask=ym)
    _check("dgrad", dx, ref, (k[0] * k[1] * F + 2) * 2.0 ** -23 * mag + u * np.abs(ref))

    rw, mw, rb, mb = TR.wgrad(x, dy_eff, k, s, d, geo4)
    nw, nb = N * H * W, N * oh * ow  # pixels reduced
    gb = torch.full((F,), float("nan"), device="cuda")
    gw = Ck.convt_wgrad(xd, dyd, k[0], k[1], geo, dy_mask=ym, dbias=gb)
    _check("wgrad", gw, rw, (nw + S + 1) * 2.0 ** -23 * mw + 2.0 ** -23 * np.abs(rw))
    _check("db", gb, rb, (nb + S + 1) * 2.0 ** -23 * mb + 2.0 ** -23 * np.abs(rb))
    w0, b0 = rng.standard_normal(rw.shape).astype(np.float32), rng.standard_normal(rb.shape).astype(np.float32)
    tw, tb = _dev(w0, torch.float32), _dev(b0, torch.float32)
    Ck.convt_wgrad(xd, dyd, k[0], k[1], geo, dy_mask=ym, out=tw, accumulate=True, dbias=tb)
    _check("wgrad added", tw, w0 + rw, (nw + S + 1) * 2.0 ** -23 * mw + 2.0 ** -23 * (np.abs(w0) + np.abs(rw)))
    _check("db added", tb, b0 + rb, (nb + S + 1) * 2.0 ** -23 * mb + 2.0 ** -23 * (np.abs(b0) + np.abs(rb)))

    # a second run gives the same bits
    gb2 = torch.empty_like(gb)
    again = (Ck.convt_forward(xd, wd, bd, geo, oh, ow, act=act), Ck.convt_dgrad(dyd, wd, H, W, geo, dy_mask=ym),
             Ck.convt_wgrad(xd, dyd, k[0], k[1], geo, dy_mask=ym, dbias=gb2), gb2)
    for a, o in zip(again, (y_saved, dx, gw, gb)):
        assert torch.equal(a.contiguous().view(torch.uint8), o.contiguous().view(torch.uint8))


def test_supported_refuses_and_the_function_falls_back(monkeypatch):
    from tensorflow_distributed_learning_amd.ops import conv_transpose as CT

    gen = torch.Generator().manual_seed(0)
    x, w = torch.randn(1, 5, 5, 8, generator=gen).cuda(), torch.randn(3, 3, 6, 8, generator=gen).cuda()
    assert CT.supported(x, w, (2, 2))
    assert not CT.supported(x.cpu(), w.cpu(), (2, 2))
    assert not CT.supported(x.to(torch.int32), w, (2, 2))
    assert not CT.supported(x[..., :6], w, (2, 2))                                              # C does not match
    assert not CT.supported(x, torch.empty(1, 1, CT.MAX_RED + 1, 8, device="meta"), (1, 1))     # the reduction limit
    assert not CT.supported(x, w, (9, 1))                                                       # the stride limit
    ref = CT.conv2d_transpose_torch(x.cpu(), w.cpu(), None, (2, 2), "same")
    before = dict(CT.CALLS)
    torch.testing.assert_close(CT.conv2d_transpose(x.cpu(), w.cpu(), None, (2, 2), "same"), ref)
    monkeypatch.setenv("TDL_CONV_TRANSPOSE", "torch")
    torch.testing.assert_close(CT.conv2d_transpose(x, w, None, (2, 2), "same").cpu(), ref, rtol=1e-4, atol=1e-4)
    assert CT.CALLS == before
    monkeypatch.delenv("TDL_CONV_TRANSPOSE")
    torch.testing.assert_close(CT.conv2d_transpose(x, w, None, (2, 2), "same").cpu(), ref, rtol=1e-4, atol=1e-4)
    assert CT.CALLS["forward"] == before["forward"] + 1
