"""The NHWC max-pool kernels of csrc/kernels/pool.hip against the explicit-loop numpy references of
tests/kernel_refs.py: every geometry class (rectangular windows and strides, a stride larger than the window,
padding on one side only, a 1x1 output), C = 8 / 64 / 2048, both dtypes, both padding kinds, the generic, the
unrolled 3x3 stride-2 and the 2x2 scatter kernels, ties, zero padding that wins, -inf and NaN inputs, and the
BN-fused forward / backward (with more than 1024 blocks, whose partial rows bn_backward pre-reduces).

y and the argmax bytes must match exactly; dx exactly in f32 (the reference adds the windows in the kernel's
order in f32) and to 1 bf16 ulp of the f64 sum of the contributing dy in bf16.  Every operand is a view into a
NaN-filled buffer, and (best effort) the block a result is likely to be allocated in is filled with NaN first, so
an element a kernel does not write is likely to show.
"""
import contextlib

import numpy as np
import pytest
import torch

import kernel_refs as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
# (kh, kw, sh, sw, pt, pb, pl, pr)
GEOMS = [(3, 3, 2, 2, 1, 1, 1, 1), (3, 3, 2, 2, 0, 1, 0, 1), (2, 2, 2, 2, 0, 0, 0, 0), (2, 3, 1, 2, 0, 0, 1, 1),
         (1, 1, 2, 2, 0, 0, 0, 0), (2, 2, 3, 3, 0, 0, 0, 0), (5, 5, 1, 1, 2, 2, 2, 2), (3, 3, 3, 3, 0, 0, 0, 0)]
ONE_BY_ONE = (3, 3, 3, 3, 0, 0, 0, 0)  # on a 3x3 image: a 1x1 output
BOTTOM_RIGHT = (3, 3, 2, 2, 0, 1, 0, 1)  # its padding is reached on an 8x10 image, not on 7x9


def _sizes(geom):
    return [(3, 3)] if geom == ONE_BY_ONE else [(7, 9), (8, 10)] if geom == BOTTOM_RIGHT else [(7, 9)]


def _C():
    from tensorflow_distributed_learning_amd.ops import hip

    return hip()


def _kernels(geom):
    """The kernel families a geometry can take: generic always; the unrolled 3x3 stride-2; the 2x2 scatter backward."""
    kh, kw, sh, sw, pt, pb, pl, pr = geom
    ks = ["generic"]
    if (kh, kw, sh, sw) == (3, 3, 2, 2):
        ks.append("k3s2")
    if (kh, kw, sh, sw, pt, pl) == (2, 2, 2, 2, 0, 0):
        ks.append("w2")
    return ks


@contextlib.contextmanager
def _kernel(kind):
    C = _C()
    try:
        C.maxpool_force_generic(kind != "k3s2")
        C.maxpool_w2(kind == "w2")
        yield
    finally:
        C.maxpool_force_generic(True)
        C.maxpool_w2(True)


def _bf(v):
    return R.bf16_bits_to_f64(R.bf16_rne(v)).astype(np.float32)


def _dev(vals, dtype):
    """vals [N, H, W, C] as a 16-byte-aligned view with a pixel row of NaN in front of and behind it."""
    C = vals.shape[-1]
    rows = vals.size // C
    buf = torch.full((rows + 2, C), float("nan"), dtype=dtype, device="cuda")
    v = buf[1:rows + 1].view(vals.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float32)).to(dtype))
    assert v.data_ptr() % 16 == 0 and v.is_contiguous()
    return v


def _poison_next(shape, dtype):
    """Best effort: fill the block the caching allocator will most likely hand to the next result of this shape
    with NaN (it usually reuses the block just freed; nothing guarantees it).  The exact comparison with the
    reference is the check; this only makes an unwritten element more likely to show."""
    t = torch.full(tuple(shape), float("nan"), dtype=dtype, device="cuda")
    del t


def _np32(t):
    return t.detach().float().cpu().numpy()


def _run(x, dy_of, geom, pad_zero, dtype, kind):
    """Forward and backward of x through the kernels and the references; dy_of(y_shape) -> dy.  Asserts the
    match and returns (y, arg, dx, dy) as numpy."""
    Ck = _C()
    kh, kw, sh, sw, pt, pb, pl, pr = geom
    bf16 = dtype == torch.bfloat16
    N, H, W, C = x.shape
    OH, OW = R.pool_out(H, kh, sh, pt, pb), R.pool_out(W, kw, sw, pl, pr)
    with np.errstate(invalid="ignore"):
        y_ref, arg_ref = R.maxpool_fwd_ref(x, *geom, pad_zero)
    dy = dy_of(y_ref.shape)
    tx, tdy = _dev(x, dtype), _dev(dy, dtype)
    with _kernel(kind):
        _poison_next(y_ref.shape, dtype)
        y, arg = Ck.maxpool_fwd(tx, kh, kw, sh, sw, pt, pl, OH, OW, pad_zero)
        _poison_next(x.shape, dtype)
        dx = Ck.maxpool_bwd(tdy, arg, list(x.shape), kh, kw, sh, sw, pt, pl)
    y, arg, dx = _np32(y), arg.cpu().numpy(), _np32(dx)
    np.testing.assert_array_equal(y, y_ref)
    np.testing.assert_array_equal(arg, arg_ref)
    assert set(np.unique(arg).tolist()) <= set(range(kh * kw)) | {255}
    if bf16:
        ref = R.maxpool_bwd_ref(dy, arg_ref, x.shape, kh, kw, sh, sw, pt, pl)
        assert np.isfinite(dx).all() and (np.abs(dx - ref) <= R.ulp_bf16(ref)).all()
        assert ((dx == 0) == (ref == 0)).all()  # no contributing window: exactly zero
    else:
        np.testing.assert_array_equal(dx, R.maxpool_bwd_ref(dy, arg_ref, x.shape, kh, kw, sh, sw, pt, pl, dtype=np.float32))
    return y, arg, dx, dy


def _randn_dy(seed, bf16):
    def dy_of(shape):
        v = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
        return _bf(v) if bf16 else v
    return dy_of


def _cases():
    out = []
    for geom in GEOMS:
        padded = any(geom[4:])
        for pad_zero in ((False, True) if padded else (False,)):
            for kind in _kernels(geom):
                out.append(pytest.param(geom, pad_zero, kind, id=f"{'x'.join(map(str, geom))}-{'zero' if pad_zero else 'inf'}-{kind}"))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [8, 64, 2048])
@pytest.mark.parametrize("geom,pad_zero,kind", _cases())
def test_maxpool_geometries(geom, pad_zero, kind, C, dtype):
    """N = 1 and 3 on a 7x9 image (3x3 for the 1x1 output): odd sizes, uncovered edge pixels for the 2x2 scatter
    kernel, pixels in no window for the stride above the window (dx = 0 there)."""
    bf16 = dtype == torch.bfloat16
    for N, (H, W) in [(N, hw) for N in (1, 3) for hw in _sizes(geom)]:
        rng = np.random.default_rng(N * 1000 + C + sum(geom))
        # zero padding: mostly negative data, so that the padding wins some windows
        x = (rng.standard_normal((N, H, W, C)) - (0.8 if pad_zero else 0.0)).astype(np.float32)
        if bf16:
            x = _bf(x)
        y, arg, dx, dy = _run(x, _randn_dy(N + C, bf16), geom, pad_zero, dtype, kind)
        if geom == ONE_BY_ONE:
            assert y.shape == (N, 1, 1, C)
        if geom == (2, 2, 3, 3, 0, 0, 0, 0):  # rows / columns 2, 5, 8 lie in no window
            assert (dx[:, 2::3] == 0).all() and (dx[:, :, 2::3] == 0).all() and (dx != 0).any()
        if pad_zero:
            assert (y[arg == 255] == 0).all() and ((arg == 255).any() or (geom, H) == (BOTTOM_RIGHT, 7))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("geom,pad_zero,kind", [c for c in _cases() if not c.values[1]])
def test_maxpool_constant_image(geom, pad_zero, kind, dtype):
    """Every window is one big tie: the argmax is the first in-range position, and all of dy comes back
    (integer dy: the sums are exact)."""
    H, W = (3, 3) if geom == ONE_BY_ONE else (7, 9)
    x = np.full((3, H, W, 8), 0.75, dtype=np.float32)

    def dy_of(shape):
        return np.random.default_rng(1).integers(-8, 9, shape).astype(np.float32)

    y, arg, dx, dy = _run(x, dy_of, geom, pad_zero, dtype, kind)
    kh, kw, sh, sw, pt, pb, pl, pr = geom
    assert (y == 0.75).all() and (arg != 255).all()
    for oh in range(y.shape[1]):
        for ow in range(y.shape[2]):
            i0, k0 = max(0, pt - oh * sh), max(0, pl - ow * sw)
            assert (arg[:, oh, ow] == i0 * kw + k0).all()
    assert dx.astype(np.float64).sum() == dy.astype(np.float64).sum()


@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("geom,pad_zero,kind", _cases())
def test_maxpool_bf16_image_of_four_values(geom, pad_zero, kind, C):
    H, W = (3, 3) if geom == ONE_BY_ONE else (7, 9)
    rng = np.random.default_rng(C)
    x = np.array([-1.5, -0.5, 0.5, 2.0], dtype=np.float32)[rng.integers(0, 4, (3, H, W, C))]
    _run(x, _randn_dy(2, True), geom, pad_zero, torch.bfloat16, kind)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["generic", "k3s2"])
@pytest.mark.parametrize("geom", GEOMS[:2])
def test_maxpool_zero_padding_wins_on_a_negative_image(geom, kind, dtype):
    """All inputs negative, zero padding: a window that touches the padding gives 0 with argmax 255 and routes
    no gradient; sum(dx) is the sum of dy over the other windows."""
    rng = np.random.default_rng(4)
    H, W = 8, 10
    x = (-0.25 - rng.random((3, H, W, 64))).astype(np.float32)
    if dtype == torch.bfloat16:
        x = _bf(x)

    def dy_of(shape):
        return rng.integers(-8, 9, shape).astype(np.float32)

    y, arg, dx, dy = _run(x, dy_of, geom, True, dtype, kind)
    kh, kw, sh, sw, pt, pb, pl, pr = geom
    touches = np.zeros(y.shape[1:3], dtype=bool)
    for oh in range(y.shape[1]):
        for ow in range(y.shape[2]):
            touches[oh, ow] = oh * sh - pt < 0 or oh * sh - pt + kh > H or ow * sw - pl < 0 or ow * sw - pl + kw > W
    assert touches.any() and not touches.all()
    assert (y[:, touches] == 0).all() and (arg[:, touches] == 255).all() and (arg[:, ~touches] != 255).all()
    assert dx.astype(np.float64).sum() == dy.astype(np.float64)[:, ~touches].sum()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("geom,pad_zero,kind", [c for c in _cases() if not c.values[1] and c.values[0] != ONE_BY_ONE])
def test_maxpool_minus_inf_inputs(geom, pad_zero, kind, dtype):
    """Real -inf elements under -inf padding: a third of the elements, and channel 1 entirely (its windows give
    -inf with argmax 255, as pool.hip states)."""
    rng = np.random.default_rng(6)
    x = rng.standard_normal((3, 7, 9, 8)).astype(np.float32)
    if dtype == torch.bfloat16:
        x = _bf(x)
    x[rng.random(x.shape) < 0.33] = -np.inf
    x[..., 1] = -np.inf
    y, arg, dx, _ = _run(x, _randn_dy(3, dtype == torch.bfloat16), geom, False, dtype, kind)
    assert (y[..., 1] == -np.inf).all() and (arg[..., 1] == 255).all() and (dx[..., 1] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("geom,pad_zero,kind", [c for c in _cases() if c.values[0] != ONE_BY_ONE])
def test_maxpool_nan_inputs_never_win(geom, pad_zero, kind, dtype):
    """pool.hip's stated NaN behaviour: a NaN input never wins a window.  NaNs in channels 0-3 only (a tenth of
    their elements, and one whole pixel neighbourhood): argmax bytes stay in range, channels 4-7 equal the
    NaN-free run, channels 0-3 equal the reference's maximum of the non-NaN elements, and maxpool_bwd on that
    argmax writes every dx element (finite, and no gradient on a NaN element)."""
    bf16 = dtype == torch.bfloat16
    rng = np.random.default_rng(8)
    clean = (rng.standard_normal((3, 7, 9, 8)) - (0.8 if pad_zero else 0.0)).astype(np.float32)
    if bf16:
        clean = _bf(clean)
    x = clean.copy()
    hole = rng.random(x.shape) < 0.1
    hole[..., 4:] = False
    hole[1, 2:7, 2:8, :4] = True
    x[hole] = np.nan
    y, arg, dx, _ = _run(x, _randn_dy(5, bf16), geom, pad_zero, dtype, kind)
    yc, argc, dxc, _ = _run(clean, _randn_dy(5, bf16), geom, pad_zero, dtype, kind)
    assert not np.isnan(y).any() and np.isfinite(dx).all()
    np.testing.assert_array_equal(y[..., 4:], yc[..., 4:])
    np.testing.assert_array_equal(arg[..., 4:], argc[..., 4:])
    np.testing.assert_array_equal(dx[..., 4:], dxc[..., 4:])
    assert (dx[hole] == 0).all()


def test_maxpool_empty_batch_returns_empty_results():
    Ck = _C()
    for dtype in DTYPES:
        x = torch.empty(0, 7, 9, 8, dtype=dtype, device="cuda")
        y, arg = Ck.maxpool_fwd(x, 3, 3, 2, 2, 1, 1, 4, 5, False)
        assert y.shape == (0, 4, 5, 8) and arg.shape == (0, 4, 5, 8) and y.dtype == dtype and arg.dtype == torch.uint8
        dx = Ck.maxpool_bwd(y, arg, [0, 7, 9, 8], 3, 3, 2, 2, 1, 1)
        assert dx.shape == (0, 7, 9, 8) and dx.dtype == dtype
        st = torch.zeros(4, 8, device="cuda")
        y, arg = Ck.maxpool_fwd(x, 3, 3, 2, 2, 1, 1, 4, 5, True, st)
        dz, part = Ck.maxpool_bwd_bn(y, arg, [0, 7, 9, 8], 3, 3, 2, 2, 1, 1, x, st)
        assert dz.shape == (0, 7, 9, 8) and part.shape == (0, 2, 8)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- BN-fused pool
def _bn_pool_case(N, H, W, C, dtype, seed):
    """maxpool_fwd(bn_stats=...) and maxpool_bwd_bn against the composition of the references: the pooled
    values are relu(f32 fma(x, scale, shift)) as stored in the dtype; dz is the pool's input gradient (f32 sums
    in the kernel's order, stored in the dtype) masked by fma(x, scale, shift) > 0."""
    Ck = _C()
    bf16 = dtype == torch.bfloat16
    geom, pad_zero = (3, 3, 2, 2, 1, 1, 1, 1), True  # the ResNet stem: ZeroPadding2D(1) -> 3x3 stride 2
    kh, kw, sh, sw, pt, pb, pl, pr = geom
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    if bf16:
        x = _bf(x)
    g, b = (rng.random(C) + 0.5).astype(np.float32), (rng.standard_normal(C) * 0.5).astype(np.float32)
    g[::5] *= -1  # (a negative gamma: the mask is not the sign of x - mean)
    mean, inv = (rng.standard_normal(C) * 0.1).astype(np.float32), (rng.random(C) + 0.5).astype(np.float32)
    scale = g * inv
    shift = b - mean * scale
    st = np.stack([mean, inv, scale, shift])
    pre = R._fma32(x, scale, shift)
    v = np.where(pre > 0, pre, np.float32(0)).astype(np.float32)
    if bf16:
        v = _bf(v)
    y_ref, arg_ref = R.maxpool_fwd_ref(v, *geom, pad_zero)
    OH, OW = y_ref.shape[1:3]
    dy = rng.standard_normal(y_ref.shape).astype(np.float32)
    if bf16:
        dy = _bf(dy)
    tx, tst = _dev(x, dtype), torch.from_numpy(st).cuda()
    _poison_next(y_ref.shape, dtype)
    y, arg = Ck.maxpool_fwd(tx, kh, kw, sh, sw, pt, pl, OH, OW, pad_zero, tst)
    np.testing.assert_array_equal(_np32(y), y_ref)
    np.testing.assert_array_equal(arg.cpu().numpy(), arg_ref)
    tdy = _dev(dy, dtype)
    _poison_next(x.shape, dtype)
    dz, part = Ck.maxpool_bwd_bn(tdy, arg, list(x.shape), kh, kw, sh, sw, pt, pl, tx, tst)
    dpool = R.maxpool_bwd_ref(dy, arg_ref, x.shape, kh, kw, sh, sw, pt, pl, dtype=np.float32)
    if bf16:
        dpool = _bf(dpool)
    dz_ref = np.where(pre > 0, dpool, np.float32(0))
    np.testing.assert_array_equal(_np32(dz), dz_ref)
    # the partial rows: one per block, P + ceil(P/64) rows allocated; their column sums are the BN backward sums
    P = min((N * H * W * (C // 8) + 255) // 256, 8192)
    assert part.shape == (P + (P + 63) // 64, 2, C)
    dz2, x2 = dz_ref.reshape(-1, C), x.reshape(-1, C)
    S = dz2.astype(np.float64).sum(0)
    Q = (dz2.astype(np.float64) * x2.astype(np.float64)).sum(0)
    Se, Qe = R._seq_sums_f32(dz2, x2)
    got = part[:P].double().sum(0).cpu().numpy()
    for name, gk, rk, ek in (("sum dz", got[0], S, Se), ("sum dz*x", got[1], Q, Qe)):
        tol = 4 * np.abs(ek.astype(np.float64) - rk).max() + R.ulp32(rk)
        assert (np.abs(gk - rk) <= tol).all(), (name, np.abs(gk - rk).max(), tol.min())
    # and through bn_backward(part=...): dgamma, dbeta and dx from those rows (pre-reduced above 1024 of them)
    out = Ck.bn_backward(dz, tx, None, torch.from_numpy(g).cuda(), tst, 1, None, None, part)
    mu, iv, gg = mean.astype(np.float64), inv.astype(np.float64), g.astype(np.float64)
    M = dz2.shape[0]

    def bwd(S, Q, f32):
        dg, db = (Q - mu * S) * iv, S
        A, B = gg * iv, -gg * iv * iv * dg / M
        D = -A * db / M - B * mu
        if not f32:
            return dg, db, A * dz2 + B * x2 + D
        return dg.astype(np.float32).astype(np.float64), db.astype(np.float32).astype(np.float64), \
            R._store(R._fma32(A, dz2, R._fma32(B, x2, D)), bf16)

    ref, emu = bwd(S, Q, False), bwd(Se.astype(np.float64), Qe.astype(np.float64), True)
    got = (out[1].double().cpu().numpy(), out[2].double().cpu().numpy(), _np32(out[0]).reshape(-1, C).astype(np.float64))
    for name, gk, rk, ek, ulp in (("dgamma", got[0], ref[0], emu[0], R.ulp32), ("dbeta", got[1], ref[1], emu[1], R.ulp32),
                                  ("dx", got[2], ref[2], emu[2], R.ulp_bf16 if bf16 else R.ulp32)):
        E = np.abs(ek - rk).max()
        err = np.abs(gk - rk)
        print(f"\n[pool edges] bn-fused {name} C={C} {'bf16' if bf16 else 'f32'} P={P}: E {E:.3g}, kernel error {err.max():.3g}", end="")
        assert (err <= 4 * E + ulp(rk)).all(), (name, err.max(), E)
    return P


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [8, 64, 2048])
def test_maxpool_bn_fused_matches_composed_references(C, dtype):
    _bn_pool_case(3, 7, 9, C, dtype, seed=C)


def test_maxpool_bwd_bn_with_more_than_1024_blocks():
    """(2, 132, 132, 64) bf16: 1089 blocks, one partial row each -- above the 1024 rows from which bn_backward
    reduces them in two levels (k_bn_prereduce)."""
    assert _bn_pool_case(2, 132, 132, 64, torch.bfloat16, seed=1) == 1089
