"""The depthwise-convolution kernels of csrc/kernels/depthwise.hip, called through the bindings and compared
with the float64 loops of tests/depthwise_refs.py on the same (bf16: pre-rounded) inputs.

Every operand is a view into the middle of a NaN-filled buffer, 16-byte aligned: a read outside the operand
poisons a result.  The bounds follow from the kernels' arithmetic contract alone (T = kh kw taps; u = 2^-24 for
f32 output, 2^-8 for bf16 output):

  forward  |got - ref| <= (T + 2) 2^-24 (sum |x w| + |b|) + u |ref|      (T fmaf, the bias add, one rounding)
  dgrad    |got - ref| <= (T dm + 1) 2^-24 sum |dy w| + u |ref|
  wgrad/db |got - ref| <= 2^-23 (|target0| + |ref|) + n 2^-52 sum |dy x|  (n terms in f64, one f32 rounding, one add)

With ReLU fused, an element whose pre-activation reference lies within the forward bound of zero would be
excluded; the seeds are such that the reference excludes none (asserted).
"""
import numpy as np
import pytest
import torch

import depthwise_refs as DR
import kernel_refs as R

pytestmark = pytest.mark.gpu

# x [N,H,W,C] (C None: one full column block and a short one), kernel, strides, dilation, dm, padding, fused ReLU
CASES = [
    ((1, 1, 1, 8), (1, 1), (1, 1), (1, 1), 1, "valid", 0),     # one tap, one pixel
    ((1, 1, 2, 8), (3, 3), (1, 1), (1, 1), 1, "same", 0),      # kernel larger than the image
    ((2, 5, 7, 8), (3, 3), (1, 1), (1, 1), 1, "same", 0),      # halo on all sides, less than one tile
    ((2, 5, 7, 8), (3, 3), (1, 1), (1, 1), 1, "same", 1),      # ... with ReLU fused
    ((2, 6, 6, 16), (3, 3), (2, 2), (1, 1), 1, "same", 0),     # asymmetric 'same', strided dgrad phases
    ((2, 6, 6, 16), (3, 3), (2, 2), (1, 1), 1, "same", 1),     # ... with ReLU fused
    ((1, 9, 11, 8), (3, 3), (1, 1), (2, 2), 1, "valid", 0),    # dilation
    ((3, 4, 6, 8), (1, 3), (2, 1), (1, 1), 1, "same", 0),      # non-square kernel and strides
    ((1, 37, 70, 8), (3, 3), (1, 1), (1, 1), 1, "same", 0),    # several tiles, short last ones, several chunks
    ((2, 7, 7, 6), (3, 3), (1, 1), (1, 1), 1, "same", 0),      # per-element path
    ((2, 7, 7, 4), (3, 3), (1, 1), (1, 1), 2, "valid", 0),     # depth multiplier
    ((1, 8, 8, None), (5, 5), (1, 1), (1, 1), 1, "same", 0),   # a second, short column block; two tap rounds
    ((1, 12, 12, 8), (7, 7), (2, 2), (1, 1), 1, "same", 0),    # largest kernel, shrunken tile
]
IDS = [f"{'x'.join(map(str, c[0]))}-k{c[1][0]}x{c[1][1]}-s{c[2][0]}{c[2][1]}-d{c[3][0]}-dm{c[4]}-{c[5]}-act{c[6]}"
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
    print(f"[dw kernels] {name}: error {err.flat[i]:.3g} where it comes closest to its bound {tol.flat[i]:.3g}")
    assert np.isfinite(err).all(), f"{name}: non-finite output"
    assert (err <= tol).all(), f"{name}: {int((err > tol).sum())} elements off, worst {err.max():.3g}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernels_against_f64(case, dtype):
    Ck = _C()
    shape, k, s, d, dm, padding, act = case
    bf16 = dtype == torch.bfloat16
    if shape[3] is None:
        shape = shape[:3] + (72 if bf16 else 36,)
    N, H, W, C = shape
    pads, oh, ow = DR.geometry(shape, k, s, d, padding)
    geo = [s[0], s[1], d[0], d[1], pads[0], pads[2]]
    plan = Ck.dw_plan(list(shape), k[0], k[1], dm, oh, ow, geo, bf16)  # vec, cols, tc, colblocks, toh, tow, ...
    if case[0][3] is None:
        assert plan[3] == 2 and plan[1] % plan[2] != 0
    if shape[1] == 37:
        assert oh % plan[4] > 1 and ow % plan[5] > 1 and oh > plan[4] and ow > plan[5]
    rng = np.random.default_rng(7)
    x = rng.standard_normal(shape).astype(np.float32)
    dy = rng.standard_normal((N, oh, ow, C * dm)).astype(np.float32)
    if bf16:
        x, dy = (R.bf16_bits_to_f64(R.bf16_rne(v)).astype(np.float32) for v in (x, dy))
    w = rng.standard_normal(k + (C, dm)).astype(np.float32)
    b = rng.standard_normal(C * dm).astype(np.float32)
    T, u = k[0] * k[1], 2.0 ** -8 if bf16 else 2.0 ** -24
    xd, dyd, wd, bd = _dev(x, dtype), _dev(dy, dtype), _dev(w, torch.float32), _dev(b, torch.float32)

    # forward, with and without the bias
    mask = None
    for bias in (b, None):
        ref, mag = DR.forward(x, w, bias, s, d, pads, oh, ow)
        tol = (T + 2) * 2.0 ** -24 * mag + u * np.abs(ref)
        if act:
            assert (np.abs(ref) > tol).all(), "the seed leaves a pre-activation within the bound of zero"
            if bias is not None:
                mask = ref > 0
            ref = np.maximum(ref, 0.0)
        y = Ck.dw_forward(xd, wd, bd if bias is not None else None, geo, oh, ow, act=act)
        _check("forward" + (" + bias" if bias is not None else ""), y, ref, tol)
        if bias is not None:
            y_saved = y
    if act:  # both backward kernels mask dy by the saved output
        assert np.array_equal(_np(y_saved) > 0, mask)
        dy_eff, ym = dy * mask, y_saved
    else:
        dy_eff, ym = dy, None

    ref, mag = DR.dgrad(dy_eff, w, shape, s, d, pads)
    dx = Ck.dw_dgrad(dyd, wd, H, W, geo, dy_mask=ym)
    _check("dgrad", dx, ref, (T * dm + 1) * 2.0 ** -24 * mag + u * np.abs(ref))

    rw, mw, rb, mb = DR.wgrad(x, dy_eff, k, dm, s, d, pads)
    n = N * oh * ow
    gw, gb = Ck.dw_wgrad(xd, dyd, k[0], k[1], geo, dy_mask=ym)[:2]
    _check("wgrad", gw, rw, 2.0 ** -23 * np.abs(rw) + n * 2.0 ** -52 * mw)
    _check("db", gb, rb, 2.0 ** -23 * np.abs(rb) + n * 2.0 ** -52 * mb)
    w0, b0 = rng.standard_normal(rw.shape).astype(np.float32), rng.standard_normal(rb.shape).astype(np.float32)
    tw, tb = _dev(w0, torch.float32), _dev(b0, torch.float32)
    Ck.dw_wgrad(xd, dyd, k[0], k[1], geo, dy_mask=ym, dw_out=tw, db_out=tb)
    _check("wgrad added", tw, w0 + rw, 2.0 ** -23 * (np.abs(w0) + np.abs(rw)) + n * 2.0 ** -52 * mw)
    _check("db added", tb, b0 + rb, 2.0 ** -23 * (np.abs(b0) + np.abs(rb)) + n * 2.0 ** -52 * mb)

    # a second run gives the same bits
    again = (Ck.dw_forward(xd, wd, bd, geo, oh, ow, act=act), Ck.dw_dgrad(dyd, wd, H, W, geo, dy_mask=ym),
             *Ck.dw_wgrad(xd, dyd, k[0], k[1], geo, dy_mask=ym)[:2])
    for a, o in zip(again, (y_saved, dx, gw, gb)):
        assert torch.equal(a.contiguous().view(torch.uint8), o.contiguous().view(torch.uint8))


def test_supported_refuses_and_the_function_falls_back():
    from tensorflow_distributed_learning_amd.ops import depthwise as DW

    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 9, 9, 4, generator=g).cuda()
    ok = torch.randn(3, 3, 4, 1, generator=g).cuda()
    assert DW.supported(x, ok)
    assert not DW.supported(x.cpu(), ok.cpu())
    assert not DW.supported(x.to(torch.int32), ok)
    before = dict(DW.CALLS)
    for xx, ww in ((x, torch.randn(8, 8, 4, 1, generator=g).cuda()), (x, torch.randn(3, 3, 4, 9, generator=g).cuda()),
                   (x.cpu(), ok.cpu())):
        assert not DW.supported(xx, ww)
        y = DW.depthwise_conv2d(xx, ww, None, (1, 1), (0, 0, 0, 0), (1, 1))
        oh, ow = 9 - ww.shape[0] + 1, 9 - ww.shape[1] + 1
        ref, _ = DR.forward(_np(xx), _np(ww), None, (1, 1), (1, 1), (0, 0, 0, 0), oh, ow)
        np.testing.assert_allclose(_np(y), ref, rtol=1e-4, atol=1e-4)
    assert DW.CALLS == before
