"""tests/conv_refs.py against torch.nn.functional.conv2d / torch.nn.grad in float64 on the CPU: random
geometries (strides, rectangular filters, asymmetric padding built with F.pad, outputs that leave the last
input rows unused), and the epilogue references on hand-checked values.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_refs as CR
import kernel_refs as R


def _geoms():
    rng = np.random.RandomState(7)
    out = [(1, 1, 1, 2, 3, 1, 1, 1, 1, 0, 0, 0, 0),  # M = 1
           (2, 2, 5, 3, 2, 3, 3, 1, 1, 2, 2, 2, 2),  # H < KH, PT = KH - 1
           (2, 6, 6, 2, 3, 3, 3, 2, 2, 0, 1, 0, 1),  # stride 2 'same' on an even size: top 0, bottom 1
           (1, 7, 5, 2, 2, 1, 7, 1, 1, 0, 0, 3, 3), (1, 7, 5, 2, 2, 7, 1, 1, 1, 3, 3, 0, 0),
           (1, 6, 9, 2, 2, 4, 8, 1, 1, 1, 2, 3, 4), (2, 5, 5, 3, 2, 2, 2, 1, 1, 1, 0, 0, 1)]
    while len(out) < 40:
        N, H, W, C, K = rng.randint(1, 3), rng.randint(1, 9), rng.randint(1, 9), rng.randint(1, 4), rng.randint(1, 4)
        KH, KW, SH, SW = rng.randint(1, 5), rng.randint(1, 5), rng.randint(1, 3), rng.randint(1, 3)
        pt, pl = rng.randint(0, KH), rng.randint(0, KW)
        pb, pr = rng.randint(0, KH), rng.randint(0, KW)
        if H + pt + pb < KH or W + pl + pr < KW:
            continue
        out.append((N, H, W, C, K, KH, KW, SH, SW, pt, pb, pl, pr))
    return out


def _torch_case(g):
    N, H, W, C, K, KH, KW, SH, SW, pt, pb, pl, pr = g
    rng = np.random.RandomState(sum(g))
    x = rng.randn(N, H, W, C)
    w = rng.randn(KH, KW, C, K)  # HWIO
    xt = torch.tensor(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wt = torch.tensor(w).permute(3, 2, 0, 1).contiguous().requires_grad_(True)
    y = F.conv2d(F.pad(xt, (pl, pr, pt, pb)), wt, None, (SH, SW))
    return x, w, xt, wt, y


@pytest.mark.parametrize("g", _geoms())
def test_convolutions_match_torch_float64(g):
    N, H, W, C, K, KH, KW, SH, SW, pt, pb, pl, pr = g
    x, w, xt, wt, y = _torch_case(g)
    OH, OW = y.shape[2], y.shape[3]
    got, ab = CR.conv_fwd_ref(x, w.transpose(3, 0, 1, 2), OH, OW, SH, SW, pt, pl)
    np.testing.assert_allclose(got, y.detach().permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
    want_ab = F.conv2d(F.pad(xt.detach().abs(), (pl, pr, pt, pb)), wt.detach().abs(), None, (SH, SW))
    np.testing.assert_allclose(ab, want_ab.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
    dy = np.random.RandomState(1).randn(N, OH, OW, K)
    y.backward(torch.tensor(dy).permute(0, 3, 1, 2))
    dx, _ = CR.conv_dgrad_ref(dy, w, H, W, SH, SW, pt, pl)
    np.testing.assert_allclose(dx, xt.grad.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
    dw, _ = CR.conv_wgrad_ref(x, dy, KH, KW, SH, SW, pt, pl)
    np.testing.assert_allclose(dw, wt.grad.permute(2, 3, 1, 0).numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("hw", [(4, 4), (5, 4), (4, 5), (5, 5), (1, 1)])
def test_stride2_gradient_matches_torch_nn_grad(hw):
    H, W = hw
    OH, OW = (H + 1) // 2, (W + 1) // 2
    rng = np.random.RandomState(3)
    dy, w = rng.randn(2, OH, OW, 3), rng.randn(1, 1, 4, 3)
    want = torch.nn.grad.conv2d_input((2, 4, H, W), torch.tensor(w).permute(3, 2, 0, 1),
                                      torch.tensor(dy).permute(0, 3, 1, 2), stride=2)
    got, _ = CR.conv_dgrad_s2_ref(dy, w, H, W)
    np.testing.assert_allclose(got, want.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
    assert np.all(got[:, 1::2] == 0) and np.all(got[:, :, 1::2] == 0)


def test_unreached_rows_are_ignored():
    """Stride 2, 3x3, H = 6 unpadded: OH = 2 reads rows 0..4; row 5 takes no part in y and gets no gradient."""
    rng = np.random.RandomState(0)
    x, w = rng.randn(1, 6, 6, 2), rng.randn(3, 3, 3, 2)
    y, _ = CR.conv_fwd_ref(x, w, 2, 2, 2, 2, 0, 0)
    x2 = x.copy()
    x2[:, 5] = 99.0
    x2[:, :, 5] = -99.0
    assert np.array_equal(CR.conv_fwd_ref(x2, w, 2, 2, 2, 2, 0, 0)[0], y)
    dx, _ = CR.conv_dgrad_ref(y, w.transpose(1, 2, 3, 0), 6, 6, 2, 2, 0, 0)
    assert np.all(dx[:, 5] == 0) and np.all(dx[:, :, 5] == 0) and np.all(dx[:, :5, :5] != 0)


def _bits(v):
    return R.bf16_rne(np.asarray(v, np.float32))


def test_rounding_order_and_ties():
    # 257 is halfway between 256 and 258: to even (256); 259 between 258 and 260: to even (260)
    assert list(R.bf16_bits_to_f64(CR.round_bf16([257.0, 259.0, -257.0, -259.0]))) == [256.0, 260.0, -256.0, -260.0]
    assert CR.count_ties(np.array([257.0, 259.0, -259.0, 256.0, 3.0, 0.0])) == (1, 2, 1, 2)
    # bf16(bf16(acc) + res) rounds twice: 257 -> 256, + 1 = 257 -> 256; one rounding of 258 would give 258
    assert R.bf16_bits_to_f64(CR.add_residual(CR.round_bf16([257.0]), _bits([1.0])))[0] == 256.0
    # halfway to Inf rounds to Inf; just below stays finite
    top = 2.0 ** 127 + 255 * 2.0 ** 119
    assert CR.round_bf16([top])[0] == 0x7F80 and CR.round_bf16([-top])[0] == 0xFF80
    assert CR.round_bf16([np.float32(top) - np.float32(2.0 ** 104)])[0] == 0x7F7F
    for nan in (0x7FFF, 0xFFFF, 0x7F81):
        assert R.bf16_is_nan(CR.add_residual(_bits([3.0]), np.array([nan], np.uint16)))[0]


def test_masks_follow_the_bit_rule():
    by = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x3F80, 0xBF80], np.uint16)
    assert list(CR.mask_from_bits(by)) == [False, False, True, False, True, False, True, False, True, False]
    one = np.float32(1.0)
    # x * 2 - 6 at x = 3 is exactly 0 (masked); one ulp of the shift either side decides
    bx = _bits([3.0, 3.0, 3.0, np.nan])
    sh = np.array([-6.0, np.nextafter(np.float32(-6), np.float32(0)), np.nextafter(np.float32(-6), np.float32(-7)),
                   1.0], np.float32)
    assert list(CR.mask_from_stats(bx, np.array([2.0, 2.0, 2.0, 1.0], np.float32) * one, sh)) == [False, True, False, False]
    assert list(R.bf16_bits_to_f64(CR.in_bn_ref(_bits([3.0, -3.0, np.nan]), np.float32([2, 2, 1]), np.float32([1, 1, 1])))) == [7.0, 0.0, 0.0]


def test_tile_sums_use_the_stored_values_and_count_tail_rows_only():
    v = np.zeros((130, 2))
    v[:, 0] = 257.0  # stored as 256
    v[129, 1] = 3.0
    s = CR.tile_sums(CR.round_bf16(v), None, 128)
    assert s.shape == (2, 2, 2)
    assert s[0, 0, 0] == 128 * 256 and s[0, 1, 0] == 128 * 256 ** 2 and s[1, 0, 0] == 2 * 256
    assert s[1, 0, 1] == 3 and s[1, 1, 1] == 9 and s[0, 0, 1] == 0
    assert CR.part_rows(1) == 2 and CR.part_rows(64) == 65 and CR.part_rows(65) == 67
    with pytest.raises(AssertionError):
        CR.tile_sums(CR.round_bf16(np.full((128, 1), 512.0)), None, 128)  # 128 * 512^2 = 2^25


@pytest.mark.parametrize("hw", [(4, 4), (5, 3), (3, 6)])
def test_stride2_epilogue_covers_all_four_pixels(hw):
    H, W = hw
    OH, OW = (H + 1) // 2, (W + 1) // 2
    rng = np.random.RandomState(5)
    acc = rng.randint(-300, 300, (2, OH, OW, 2)).astype(np.float64)
    res = rng.randint(-5, 6, (2, H, W, 2)).astype(np.float64)
    by = rng.randint(-1, 2, (2, H, W, 2)).astype(np.float64)
    bx = rng.randint(-3, 4, (2, H, W, 2)).astype(np.float64)
    dz, part, part2 = CR.dgrad_s2_epilogue_ref(acc, H, W, 3, _bits(res), _bits(by), _bits(bx), None, _bits(by))
    want = res.copy()
    want[:, ::2, ::2] = R.bf16_bits_to_f64(CR.round_bf16(acc)) + res[:, ::2, ::2]
    want = R.bf16_bits_to_f64(_bits(want)) * (by > 0)
    assert np.array_equal(R.bf16_bits_to_f64(dz), want)
    assert part.shape == ((2 * OH * OW + 2) // 3, 2, 2)
    np.testing.assert_array_equal(part.sum(0)[0], want.sum((0, 1, 2)))
    np.testing.assert_array_equal(part.sum(0)[1], (want * bx).sum((0, 1, 2)))
    np.testing.assert_array_equal(part2.sum(0)[1], (want * by).sum((0, 1, 2)))
    # the first tile: dy pixels 0..2 of image 0 and their blocks
    blocks = [(0, i // OW, i % OW) for i in range(3)] if OH * OW >= 3 else None
    if blocks:
        t = sum(want[n, 2 * i:2 * i + 2, 2 * j:2 * j + 2].sum((0, 1)) for n, i, j in blocks)
        np.testing.assert_array_equal(part[0, 0], t)


def test_coded_data_is_position_coded_and_bounded():
    a = CR.coded_ints((2, 5, 6, 64), 9, 1)
    assert a.min() >= -9 and a.max() <= 9 and np.all(a == np.round(a))
    assert not np.array_equal(a[:, 1:], a[:, :-1]) and not np.array_equal(a[:, ::-1], a)
    assert not np.array_equal(a, CR.coded_ints((2, 5, 6, 64), 9, 2))
    z = CR.coded_ints((4, 8, 8, 64), 9, 1, zero_frac=0.9)
    assert 0.8 < (z == 0).mean() < 0.97
    assert CR.amp_for(64, 350) >= 8 and CR.amp_for(4608, 350) <= 4


def test_error_bound_is_the_derived_one():
    r, ab = np.array([1.0, 300.0]), np.array([10.0, 4000.0])
    e = 576 * 2.0 ** -23 * ab
    np.testing.assert_array_equal(CR.error_bound(r, ab, 576), 0.5 * R.ulp_bf16(np.abs(r) + e) + e)
    with pytest.raises(AssertionError):
        CR.assert_exact(np.array([2.0 ** 24]))


# ------------------------------------------------------------------------------------- stem references
def _stem_geoms():
    rng = np.random.RandomState(11)
    out = [(224, 224, 7, 7, 2, (3, 3, 3, 3)), (9, 9, 1, 1, 1, (0, 0, 0, 0)), (16, 37, 3, 5, 2, (0, 1, 2, 0)),
           (20, 23, 8, 8, 3, (1, 2, 0, 1)), (6, 6, 7, 7, 2, (0, 0, 0, 0)), (7, 7, 7, 8, 2, (0, 0, 0, 0))]
    while len(out) < 60:
        out.append((rng.randint(1, 20), rng.randint(1, 20), rng.randint(1, 9), rng.randint(1, 9), rng.randint(1, 4),
                    tuple(int(p) for p in rng.randint(0, 4, 4))))
    return out


@pytest.mark.parametrize("g", _stem_geoms())
def test_stem_geometry_counts_the_valid_window_positions(g):
    H, W, KH, KW, SH, pads = g
    OH, OW, HPp, WP = CR.stem_geometry(H, W, KH, KW, SH, pads)
    HP, WPv = H + pads[0] + pads[1], W + pads[2] + pads[3]
    # brute force: window positions at multiples of the stride that lie inside the padded image
    assert max(OH, 0) == sum(1 for t in range(0, HP, SH) if t + KH <= HP)
    assert max(OW, 0) == sum(1 for l in range(0, WPv, 2) if l + KW <= WPv)
    if OH <= 0 or OW <= 0:
        return
    # the packed image: the smallest that holds the padded image and every KH x 8 window the kernels read
    assert HPp == max(HP, max(oh * SH + KH for oh in range(OH)))
    assert WP == max(WPv, max(2 * ow + 8 for ow in range(OW)))
    assert HPp == HP  # (the last window lies inside the padded image: extra rows need a taller filter than image)


def test_stem_geometry_of_an_image_smaller_than_its_filter():
    assert CR.stem_geometry(6, 20, 7, 7, 2, (0, 0, 0, 0))[0] == 0   # (C division would give (6 - 7) / 2 + 1 = 1)
    assert CR.stem_geometry(20, 5, 7, 7, 2, (0, 0, 0, 1))[1] == 0


@pytest.mark.parametrize("is_f32", [True, False])
@pytest.mark.parametrize("g", [(2, 5, 6, 3, 7, 7, 2, (3, 3, 3, 3)), (1, 4, 9, 4, 2, 8, 1, (0, 1, 2, 0)),
                               (2, 3, 4, 1, 3, 3, 3, (1, 0, 0, 2)), (1, 6, 5, 2, 1, 1, 1, (0, 0, 0, 0))])
def test_stem_pack_ref_against_a_loop_per_pixel(g, is_f32):
    N, H, W, C, KH, KW, SH, pads = g
    rng = np.random.RandomState(H * W)
    xf = (rng.randn(N, H, W, C) * 3).astype(np.float32)
    x = xf if is_f32 else R.bf16_rne(xf)
    got = CR.stem_pack_ref(x, is_f32, KH, KW, SH, pads)
    OH, OW, HPp, WP = CR.stem_geometry(H, W, KH, KW, SH, pads)
    assert got.shape == (N, HPp, WP, 4) and got.dtype == np.uint16
    for n in range(N):
        for hp in range(HPp):
            for wp in range(WP):
                h, w = hp - pads[0], wp - pads[2]
                for c in range(4):
                    want = 0
                    if 0 <= h < H and 0 <= w < W and c < C:
                        want = int(R.bf16_rne(xf[n, h, w, c:c + 1])[0])
                    assert got[n, hp, wp, c] == want, (n, hp, wp, c)


def test_stem_pack_ref_keeps_nan_payloads_and_copies_bf16_bits():
    x = np.zeros((1, 1, 3, 2), np.float32)
    x[0, 0, :, 0], x[0, 0, :, 1] = R.NAN_PAYLOADS_F32, -R.NAN_PAYLOADS_F32
    xp = CR.stem_pack_ref(x, True, 1, 1, 1, (0, 0, 1, 0))
    assert list(xp[0, 0, 1:4, 0]) == [0x7FC0, 0x7FFF, 0xFFFF]  # quieted, sign kept: never Inf, -0 or +0
    assert R.bf16_is_nan(xp[0, 0, 1:4, :2]).all() and not xp[0, 0, 0].any() and not xp[..., 2:].any()
    assert list(xp[0, 0, 1:4, 1] >> 15) == [1, 1, 0]
    bits = np.array([0x7F81, 0xFFFF, 0x0001, 0x8000, 0x7F80], np.uint16).reshape(1, 1, 5, 1)  # signalling NaN, ...
    assert np.array_equal(CR.stem_pack_ref(bits, False, 1, 1, 1, (0, 0, 0, 0))[0, 0, :5, 0], bits.ravel())


# ------------------------------------------------------------------------------------- f32 GEMM / conv references
def _dilated_geoms():
    # (N, H, W, C, K, KH, KW, SH, SW, DH, DW, pt, pb, pl, pr): stride, dilation and asymmetric pads together
    rng = np.random.RandomState(23)
    out = [(1, 7, 9, 2, 3, 3, 3, 2, 1, 2, 3, 1, 2, 3, 0), (2, 5, 5, 1, 2, 3, 2, 1, 2, 3, 2, 4, 2, 0, 1),
           (1, 3, 4, 3, 2, 3, 3, 1, 1, 2, 2, 2, 2, 2, 2),  # the dilated filter (5x5) is larger than the image
           (1, 6, 6, 2, 2, 1, 1, 3, 3, 2, 2, 0, 0, 0, 0)]  # 1x1: dilation has nothing to act on
    while len(out) < 30:
        N, H, W, C, K = rng.randint(1, 3), rng.randint(1, 10), rng.randint(1, 10), rng.randint(1, 4), rng.randint(1, 4)
        KH, KW, SH, SW = rng.randint(1, 4), rng.randint(1, 4), rng.randint(1, 4), rng.randint(1, 4)
        DH, DW = rng.randint(1, 4), rng.randint(1, 4)
        pt, pb, pl, pr = (int(v) for v in rng.randint(0, 4, 4))
        if H + pt + pb < (KH - 1) * DH + 1 or W + pl + pr < (KW - 1) * DW + 1:
            continue
        out.append((N, H, W, C, K, KH, KW, SH, SW, DH, DW, pt, pb, pl, pr))
    return out


@pytest.mark.parametrize("g", _dilated_geoms())
def test_dilated_convolutions_match_torch_float64(g):
    N, H, W, C, K, KH, KW, SH, SW, DH, DW, pt, pb, pl, pr = g
    rng = np.random.RandomState(sum(g))
    x, w = rng.randn(N, H, W, C), rng.randn(KH, KW, C, K)
    xt = torch.tensor(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wt = torch.tensor(w).permute(3, 2, 0, 1).contiguous().requires_grad_(True)
    y = F.conv2d(F.pad(xt, (pl, pr, pt, pb)), wt, None, (SH, SW), 0, (DH, DW))
    OH, OW = y.shape[2], y.shape[3]
    got, ab = CR.conv_fwd_ref(x, w.transpose(3, 0, 1, 2), OH, OW, SH, SW, pt, pl, dh=DH, dw=DW)
    np.testing.assert_allclose(got, y.detach().permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
    want_ab = F.conv2d(F.pad(xt.detach().abs(), (pl, pr, pt, pb)), wt.detach().abs(), None, (SH, SW), 0, (DH, DW))
    np.testing.assert_allclose(ab, want_ab.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
    dy = np.random.RandomState(1).randn(N, OH, OW, K)
    y.backward(torch.tensor(dy).permute(0, 3, 1, 2))
    dx, _ = CR.conv_dgrad_ref(dy, w, H, W, SH, SW, pt, pl, dh=DH, dw=DW)
    np.testing.assert_allclose(dx, xt.grad.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
    gw, _ = CR.conv_wgrad_ref(x, dy, KH, KW, SH, SW, pt, pl, dh=DH, dw=DW)
    np.testing.assert_allclose(gw, wt.grad.permute(2, 3, 1, 0).numpy(), rtol=1e-12, atol=1e-12)


def test_dilation_defaults_leave_the_references_unchanged():
    rng = np.random.RandomState(2)
    x, w, dy = rng.randn(1, 6, 5, 2), rng.randn(3, 2, 2, 3), rng.randn(1, 3, 4, 3)
    for a, b in zip(CR.conv_fwd_ref(x, w.transpose(3, 0, 1, 2), 3, 4, 2, 1, 1, 0),
                    CR.conv_fwd_ref(x, w.transpose(3, 0, 1, 2), 3, 4, 2, 1, 1, 0, dh=1, dw=1)):
        assert np.array_equal(a, b)
    assert np.array_equal(CR.conv_dgrad_ref(dy, w, 6, 5, 2, 1, 1, 0)[0], CR.conv_dgrad_ref(dy, w, 6, 5, 2, 1, 1, 0, dh=1, dw=1)[0])
    assert np.array_equal(CR.conv_wgrad_ref(x, dy, 3, 2, 2, 1, 1, 0)[0], CR.conv_wgrad_ref(x, dy, 3, 2, 2, 1, 1, 0, dh=1, dw=1)[0])


def test_f32_fusion_references_on_hand_checked_values():
    nan, inf = np.nan, np.inf
    acc = np.array([[1.0, -2.0, nan], [-inf, 0.5, -1.0]])
    b = np.array([1.0, 1.0, 1.0])
    got = CR.bias_act_ref(acc, b, 1)
    assert np.array_equal(got, [[2.0, 0.0, 0.0], [0.0, 1.5, 0.0]])  # fmaxf: the NaN pre-activation is 0
    assert np.isnan(CR.bias_act_ref(acc, b, 1, fmaxf=False)[0, 2]) and np.isnan(CR.bias_act_ref(acc, b, 0)[0, 2])
    assert np.array_equal(CR.bias_act_ref(acc[1:], None, 0, prior=np.array([[inf, 1.0, 1.0]]))[0, 1:], [1.5, 0.0])
    assert np.isnan(CR.bias_act_ref(acc[1:], None, 0, prior=np.array([[inf, 1.0, 1.0]]))[0, 0])
    # the mask is a select: Inf and NaN under mask <= 0 or a NaN mask are exact zeros, and -0 does not pass
    a = np.array([inf, nan, 3.0, 4.0, -inf, 5.0])
    m = np.array([0.0, -1.0, nan, 1e-30, -0.0, inf])
    assert np.array_equal(CR.masked_ref(a, m), [0.0, 0.0, 0.0, 4.0, 0.0, 5.0])
    assert CR.masked_ref(a, None) is not None and np.isnan(CR.masked_ref(a, None)[1])
    db, ab = CR.bias_grad_ref(np.array([[[1.0, -2.0], [3.0, 4.0]], [[-5.0, 6.0], [inf, 8.0]]]),
                              np.array([[[1.0, 1.0], [0.0, 1.0]], [[1.0, -1.0], [0.0, 1.0]]]))
    assert list(db) == [-4.0, 10.0] and list(ab) == [6.0, 14.0]


def test_pooled_forward_reference_ties_nans_and_odd_sizes():
    # a 1x1 conv with weight 1 over a 3x5 image: y = relu(x); windows (0..1, 0..1) and (0..1, 2..3)
    x = np.zeros((1, 3, 5, 1))
    x[0, :2, :2, 0] = [[2.0, 7.0], [7.0, -1.0]]      # tie: the first maximum (position 1) wins
    x[0, :2, 2:4, 0] = [[-3.0, np.nan], [-1.0, -2.0]]  # all <= 0 or NaN: relu gives zeros, position 0 wins
    x[0, 2, :, 0] = 99.0  # the odd last row and column are in no window
    w = np.ones((1, 1, 1, 1))
    y, mx, arg, ab = CR.conv_pool_fwd_ref(x, w, None, 3, 5)
    assert mx.shape == (1, 1, 2, 1) and list(mx.ravel()) == [7.0, 0.0] and list(arg.ravel()) == [1, 0]
    assert y[0, 0, 3, 0] == 0.0 and y[0, 2, 0, 0] == 99.0
    # without the ReLU the NaN stays in y, never wins, and a window of NaNs gives -inf and 255
    x[0, :2, :2, 0] = np.nan
    y, mx, arg, _ = CR.conv_pool_fwd_ref(x, w, None, 3, 5, act=0)
    assert np.isnan(y[0, 0, 3, 0]) and list(mx.ravel()) == [-np.inf, -1.0] and list(arg.ravel()) == [255, 2]
    # the backward: routed by argmax, masked by maximum > 0, nothing for 255 and nothing outside the windows
    dy = CR.conv_pool_bwd_ref(np.array([5.0, 6.0, 7.0]).reshape(1, 1, 3, 1), np.array([1.0, 0.0, 2.0]).reshape(1, 1, 3, 1),
                              np.array([3, 1, 255], np.uint8).reshape(1, 1, 3, 1), 3, 7)
    want = np.zeros((1, 3, 7, 1))
    want[0, 1, 1, 0] = 5.0
    assert np.array_equal(dy, want)


@pytest.mark.parametrize("g", [(2, 7, 8, 3, 4, 3, 3, 1, 1, 1, 1, 0, 0), (1, 9, 9, 2, 3, 3, 2, 2, 1, 1, 2, 1, 2),
                               (2, 6, 6, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0), (1, 11, 7, 2, 2, 3, 3, 1, 2, 2, 1, 2, 1)])
def test_pooled_references_match_autograd_of_pool_relu_conv(g):
    N, H, W, C, K, KH, KW, SH, SW, DH, DW, pt, pl = g
    rng = np.random.RandomState(sum(g))
    x, w, b = rng.randn(N, H, W, C), rng.randn(KH, KW, C, K), rng.randn(K)  # (random f64: no ties)
    xt = torch.tensor(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wt = torch.tensor(w).permute(3, 2, 0, 1).contiguous().requires_grad_(True)
    bt = torch.tensor(b).requires_grad_(True)
    yt = F.conv2d(F.pad(xt, (pl, 0, pt, 0)), wt, bt, (SH, SW), 0, (DH, DW))
    OH, OW = yt.shape[2], yt.shape[3]
    pt_ = F.max_pool2d(torch.relu(yt), 2)
    y, mx, arg, _ = CR.conv_pool_fwd_ref(x, w.transpose(3, 0, 1, 2), b, OH, OW, SH, SW, pt, pl, dh=DH, dw=DW)
    np.testing.assert_allclose(y, torch.relu(yt).detach().permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(mx, pt_.detach().permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
    assert arg.max() <= 3
    dp = rng.randn(*mx.shape)
    pt_.backward(torch.tensor(dp).permute(0, 3, 1, 2))
    dy = CR.conv_pool_bwd_ref(dp, mx, arg, OH, OW)
    dx, _ = CR.conv_dgrad_ref(dy, w, H, W, SH, SW, pt, pl, dh=DH, dw=DW)
    gw, _ = CR.conv_wgrad_ref(x, dy, KH, KW, SH, SW, pt, pl, dh=DH, dw=DW)
    np.testing.assert_allclose(dx, xt.grad.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(gw, wt.grad.permute(2, 3, 1, 0).numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(CR.bias_grad_ref(dy)[0], bt.grad.numpy(), rtol=1e-12, atol=1e-12)


def _f32_plan():
    import glob
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not glob.glob(os.path.join(root, "tensorflow_distributed_learning_amd", "_C*.so")):
        pytest.skip("extension not built (python build_native.py)")
    from tensorflow_distributed_learning_amd.ops import hip

    return hip().f32_plan


def test_f32_split_plan_invariants(monkeypatch):
    monkeypatch.delenv("TDL_F32_SPLIT", raising=False)
    plan = _f32_plan()
    Ms = [1, 4, 36, 63, 64, 65, 100, 1024, 4096, 16384, 32704, 32768, 32769, 100000]
    Ns = [1, 8, 63, 64, 65, 289, 1024]
    Ks = [1, 9, 15, 16, 17, 255, 256, 257, 288, 513, 1008, 1025, 1152, 4481, 16384, 65535, 65537, 70000, 1 << 20]
    pooled_fallbacks = 0
    for M in Ms:
        for N in Ns:
            for K in Ks:
                s, c, u = plan(M, N, K)
                assert c % 16 == 0 and (s - 1) * c < K <= s * c and 1 <= s <= 1024 and u == s, (M, N, K, s, c)
                if K <= 256:
                    assert s == 1, (M, N, K, s)
                if M % 4 == 0:  # the pooled conv over M / 4 windows whose unfused conv has M .. rows
                    for pm in (M, M + M // 8 + 1):
                        sp, cp, up = plan(M, N, K, True, pm)
                        s0, c0, _ = plan(pm, N, K)
                        assert up == s0 and cp % 16 == 0 and (sp - 1) * cp < K <= sp * cp and sp < 16
                        assert (sp == up and cp == c0) == (up < 16), (M, N, K, pm, sp, up)
                        pooled_fallbacks += up >= 16
                        if up >= 16:
                            assert sp == 1
    assert pooled_fallbacks > 50
    # the shapes the GPU edge tests rely on
    assert plan(5, 5, 257)[0] == 5 and plan(5, 5, 513)[0] == 9 and plan(5, 5, 1025)[0] == 17
    assert plan(5, 5, 4481)[0] == 71 and plan(1, 1, 70000)[:2] == (875, 80) and plan(16384, 8, 260)[0] == 4
    assert plan(36, 64, 9 * 112, True, 36) == (1, 1008, 16)


def test_f32_hook_setters_return_the_value_they_replace():
    _f32_plan()  # (skips when the extension is not built)
    from tensorflow_distributed_learning_amd.ops import hip

    C = hip()
    for name in ("f32_buf", "f32_reduce_narrow", "f32_pool_hoist", "f32_reduce16"):
        f = getattr(C, name)
        start = f(False)
        try:
            assert f(True) is False and f(True) is True and f(False) is True
        finally:
            assert f(start) is False
        assert f(start) is start
