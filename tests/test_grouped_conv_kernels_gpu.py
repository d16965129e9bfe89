"""The grouped-convolution kernels of csrc/kernels/grouped_conv.hip, called through the bindings and compared with
the float64 loops of tests/grouped_conv_refs.py on the same (bf16: pre-rounded, the weight too) inputs.

Every operand is a view into the middle of a NaN-filled buffer, 16-byte aligned: a read outside the operand
poisons a result.  The bounds follow from the arithmetic contract (f32 accumulation on the MFMA, rounding to
nearest or truncating, one rounding to the output dtype), with T = kh kw Cg (dgrad: kh kw Kg), u = 2^-24 for f32
output and 2^-8 for bf16 output, mag = the sum of the absolute values of the terms:

  forward, dgrad  |got - ref| <= (T + 2) 2^-23 mag + u |ref|
  wgrad, db       |got - ref| <= (n + S + 1) 2^-23 mag + 2^-23 (|target0| + |ref|)    (n pixels, S plan splits)

With ReLU fused no pre-activation of the reference lies within the forward bound of zero (asserted: the seed).
"""
import numpy as np
import pytest
import torch

import grouped_conv_refs as GR
import kernel_refs as R

pytestmark = pytest.mark.gpu

# x [N,H,W,C], F, groups, kernel, strides, dilation, padding, fused ReLU
CASES = [
    ((1, 1, 1, 8), 8, 2, (1, 1), (1, 1), (1, 1), "valid", 0),     # one pixel, Cg = Kg = 4
    ((1, 1, 2, 8), 8, 2, (3, 3), (1, 1), (1, 1), "same", 0),      # kernel larger than the image
    ((2, 5, 7, 8), 16, 2, (3, 3), (1, 1), (1, 1), "same", 0),     # Kg = 8: two groups in one column tile
    ((2, 5, 7, 8), 16, 2, (3, 3), (1, 1), (1, 1), "same", 1),
    ((2, 6, 6, 12), 6, 3, (3, 3), (2, 2), (1, 1), "same", 0),     # Kg = 2, asymmetric pads, strided dgrad
    ((2, 6, 6, 12), 6, 3, (3, 3), (2, 2), (1, 1), "same", 1),
    ((1, 9, 11, 6), 9, 3, (3, 3), (1, 1), (2, 2), "valid", 0),    # Cg = 2, Kg = 3: per-element loads
    ((3, 4, 6, 8), 8, 8, (1, 3), (2, 1), (1, 1), "same", 0),      # Cg = Kg = 1, non-square kernel
    ((1, 8, 8, 8), 8, 2, (5, 5), (1, 1), (1, 1), "same", 0),      # reduction of 100: two k-chunks
    ((1, 37, 70, 32), 32, 8, (3, 3), (1, 1), (1, 1), "same", 0),  # several pixel tiles, a short last one
    ((2, 7, 7, 64), 64, 2, (3, 3), (1, 1), (1, 1), "same", 0),    # Cg = Kg = 32: two column tiles per group
    ((1, 8, 8, 40), 80, 2, (3, 3), (1, 1), (1, 1), "same", 0),    # Kg = 40: a short tile at a group boundary
    ((4, 20, 20, 16), 16, 4, (3, 3), (1, 1), (1, 1), "valid", 0), # 1296-pixel wgrad reduction, split
]
IDS = [f"{'x'.join(map(str, c[0]))}-F{c[1]}-g{c[2]}-k{c[3][0]}x{c[3][1]}-s{c[4][0]}{c[4][1]}-d{c[5][0]}-{c[6]}-act{c[7]}"
       for c in CASES]


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
    print(f"[gconv kernels] {name}: error {err.flat[i]:.3g} where it comes closest to its bound {tol.flat[i]:.3g}")
    assert np.isfinite(err).all(), f"{name}: non-finite output"
    assert (err <= tol).all(), f"{name}: {int((err > tol).sum())} elements off, worst {err.max():.3g}"


def _inputs(case, bf16, seed=7):
    shape, F, g, k, s, d, padding, act = case
    pads, oh, ow = GR.geometry(shape, k, s, d, padding)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    dy = rng.standard_normal((shape[0], oh, ow, F)).astype(np.float32)
    w = rng.standard_normal(k + (shape[3] // g, F)).astype(np.float32)
    b = rng.standard_normal(F).astype(np.float32)
    if bf16:
        x, dy, w = (R.bf16_bits_to_f64(R.bf16_rne(v)).astype(np.float32) for v in (x, dy, w))
    return x, dy, w, b, pads, oh, ow, rng


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernels_against_f64(case, dtype):
    Ck = _C()
    shape, F, g, k, s, d, padding, act = case
    bf16 = dtype == torch.bfloat16
    N, H, W, C = shape
    x, dy, w, b, pads, oh, ow, rng = _inputs(case, bf16)
    geo = [s[0], s[1], d[0], d[1], pads[0], pads[2]]
    plan = Ck.gconv_plan(list(shape), F, g, k[0], k[1], oh, ow, geo)
    if shape[1] == 37:
        assert plan["fwd_pixel_tiles"] > 1 and (N * oh * ow) % plan["fwd_pixels_per_tile"] not in (0, 1)
    if k == (5, 5):
        assert plan["fwd_kchunks"] == 2
    if C // g == 32:
        assert plan["fwd_tiles_per_group"] == 2 and plan["fwd_kchunks"] > 1
    if F // g == 40:
        assert plan["fwd_tiles_per_group"] == 3
    if F // g < 16:
        assert plan["fwd_groups_per_tile"] == 16 // (F // g)
    if shape[0] == 4:
        assert plan["wgrad_splits"] > 1
    Cg, Kg, S = C // g, F // g, plan["wgrad_splits"]
    u = 2.0 ** -8 if bf16 else 2.0 ** -24
    xd, dyd, wd, bd = _dev(x, dtype), _dev(dy, dtype), _dev(w, torch.float32), _dev(b, torch.float32)

    # forward, with and without the bias
    mask = None
    T = k[0] * k[1] * Cg
    for bias in (b, None):
        ref, mag = GR.forward(x, w, bias, g, s, d, pads, oh, ow)
        tol = (T + 2) * 2.0 ** -23 * mag + u * np.abs(ref)
        if act:
            assert (np.abs(ref) > tol).all(), "the seed leaves a pre-activation within the bound of zero"
            if bias is not None:
                mask = ref > 0
            ref = np.maximum(ref, 0.0)
        y = Ck.gconv_forward(xd, wd, bd if bias is not None else None, g, geo, oh, ow, act=act)
        _check("forward" + (" + bias" if bias is not None else ""), y, ref, tol)
        if bias is not None:
            y_saved = y
    if act:  # both backward kernels select dy by the saved output
        assert np.array_equal(_np(y_saved) > 0, mask)
        dy_eff, ym = dy * mask, y_saved
    else:
        dy_eff, ym = dy, None

    ref, mag = GR.dgrad(dy_eff, w, g, shape, s, d, pads)
    dx = Ck.gconv_dgrad(dyd, wd, g, H, W, geo, dy_mask=ym)
    _check("dgrad", dx, ref, (k[0] * k[1] * Kg + 2) * 2.0 ** -23 * mag + u * np.abs(ref))

    rw, mw, rb, mb = GR.wgrad(x, dy_eff, k, g, s, d, pads)
    n = N * oh * ow
    gb = torch.full((F,), float("nan"), device="cuda")
    gw = Ck.gconv_wgrad(xd, dyd, k[0], k[1], g, geo, dy_mask=ym, dbias=gb)
    _check("wgrad", gw, rw, (n + S + 1) * 2.0 ** -23 * mw + 2.0 ** -23 * np.abs(rw))
    _check("db", gb, rb, (n + S + 1) * 2.0 ** -23 * mb + 2.0 ** -23 * np.abs(rb))
    w0, b0 = rng.standard_normal(rw.shape).astype(np.float32), rng.standard_normal(rb.shape).astype(np.float32)
    tw, tb = _dev(w0, torch.float32), _dev(b0, torch.float32)
    Ck.gconv_wgrad(xd, dyd, k[0], k[1], g, geo, dy_mask=ym, out=tw, accumulate=True, dbias=tb)
    _check("wgrad added", tw, w0 + rw, (n + S + 1) * 2.0 ** -23 * mw + 2.0 ** -23 * (np.abs(w0) + np.abs(rw)))
    _check("db added", tb, b0 + rb, (n + S + 1) * 2.0 ** -23 * mb + 2.0 ** -23 * (np.abs(b0) + np.abs(rb)))

    # a second run gives the same bits
    gb2 = torch.empty_like(gb)
    again = (Ck.gconv_forward(xd, wd, bd, g, geo, oh, ow, act=act), Ck.gconv_dgrad(dyd, wd, g, H, W, geo, dy_mask=ym),
             Ck.gconv_wgrad(xd, dyd, k[0], k[1], g, geo, dy_mask=ym, dbias=gb2), gb2)
    for a, o in zip(again, (y_saved, dx, gw, gb)):
        assert torch.equal(a.contiguous().view(torch.uint8), o.contiguous().view(torch.uint8))


def test_supported_refuses_and_the_function_falls_back(monkeypatch):
    import torch.nn.functional as F

    from tensorflow_distributed_learning_amd.ops import grouped_conv as GC

    gen = torch.Generator().manual_seed(0)
    x, w = torch.randn(1, 6, 6, 8, generator=gen).cuda(), torch.randn(3, 3, 4, 6, generator=gen).cuda()
    assert GC.supported(x, w, 2)
    assert not GC.supported(x.cpu(), w.cpu(), 2)
    assert not GC.supported(x.to(torch.int32), w, 2)
    assert not GC.supported(x[..., :6], w, 2)                       # C / g does not match the kernel
    assert not GC.supported(x, torch.randn(3, 3, 2, 6).cuda(), 4)   # F % g != 0
    assert not GC.supported(x[..., :6].contiguous(), torch.randn(3, 3, 2, 6).cuda(), 4)  # C % g != 0
    assert not GC.supported(x, torch.empty(1, 1, 4, 2 * (GC.MAX_RED + 1), device="meta"), 2)  # the reduction limit
    ref = F.conv2d(x.cpu().permute(0, 3, 1, 2), w.cpu().permute(3, 2, 0, 1), groups=2).permute(0, 2, 3, 1)
    before = dict(GC.CALLS)
    torch.testing.assert_close(GC.conv2d(x.cpu(), w.cpu(), None, 2), ref)
    monkeypatch.setenv("TDL_GROUPED_CONV", "torch")
    torch.testing.assert_close(GC.conv2d(x, w, None, 2).cpu(), ref, rtol=1e-4, atol=1e-4)
    assert GC.CALLS == before
    monkeypatch.delenv("TDL_GROUPED_CONV")
    torch.testing.assert_close(GC.conv2d(x, w, None, 2).cpu(), ref, rtol=1e-4, atol=1e-4)
    assert GC.CALLS["forward"] == before["forward"] + 1
