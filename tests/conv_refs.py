"""f64 references of the bf16 implicit-GEMM convolution family (csrc/kernels/conv.hip, conv_wgrad.hip,
wgrad3x3.hip, stem.hip) and of the generic f32 GEMM / convolution (gemm_f32.hip) with its fusions, shared
by test_conv_refs_cpu.py, test_conv_edges_gpu.py, test_conv_wgrad_edges_gpu.py, test_stem_edges_gpu.py,
test_gemm_f32_edges_gpu.py and test_conv_f32_edges_gpu.py.  numpy only; nothing here touches a GPU.

Tensors are NHWC; weights come in the kernels' own layouts (OHWI forward, HWIO gradients).  Every
convolution is a loop over filter taps with one einsum per tap, so the indexing is the definition:
output pixel (oh, ow) of tap (kh, kw) reads input pixel (oh*SH - PT + kh*DH, ow*SW - PL + kw*DW) when that
lies inside the image.  Bottom / right padding is implied by (OH, OW); rows and columns no output reaches are
ignored.  Each convolution also returns sum |a||b| per output, for the error bound of the random-data
tests and for the exactness precondition of the integer-data tests.

The epilogue references round where the kernels round (conv.hip conv_epilogue): the accumulator to bf16
first, then the f32 add of the residual and a second rounding, then the ReLU mask, then the per-row-tile
sums from the stored bf16 values.
"""
import numpy as np

from kernel_refs import _relu_fmaxf, bf16_bits_to_f64, bf16_rne, maxpool_fwd_ref, ulp_bf16

EXACT_LIMIT = 2.0 ** 24  # integers below it are exact in f32, and so is every f32 sum of them in any order


def _taps(H, OH, SH, PT, kh, D=1):
    """(output rows, input rows) of the outputs whose tap kh (dilation D) lies inside an image of H rows."""
    o = np.arange(OH)
    i = o * SH - PT + kh * D
    ok = (i >= 0) & (i < H)
    return o[ok], i[ok]


def conv_fwd_ref(x, w_ohwi, oh, ow, sh=1, sw=1, pt=0, pl=0, *, dh=1, dw=1):
    """y [N,OH,OW,K] = conv(x [N,H,W,C], w [K,KH,KW,C]) in f64, and sum |x||w| per output."""
    x, w = np.asarray(x, np.float64), np.asarray(w_ohwi, np.float64)
    N, H, W, C = x.shape
    K, KH, KW, _ = w.shape
    y = np.zeros((N, oh, ow, K))
    ab = np.zeros((N, oh, ow, K))
    with np.errstate(invalid="ignore", over="ignore"):
        for kh in range(KH):
            o_h, i_h = _taps(H, oh, sh, pt, kh, dh)
            for kw in range(KW):
                o_w, i_w = _taps(W, ow, sw, pl, kw, dw)
                if o_h.size == 0 or o_w.size == 0:
                    continue
                xs = x[:, i_h][:, :, i_w]
                y[np.ix_(np.arange(N), o_h, o_w)] += np.einsum("nhwc,kc->nhwk", xs, w[:, kh, kw, :])
                ab[np.ix_(np.arange(N), o_h, o_w)] += np.einsum("nhwc,kc->nhwk", np.abs(xs), np.abs(w[:, kh, kw, :]))
    return y, ab


def conv_dgrad_ref(dy, w_hwio, h, w, sh=1, sw=1, pt=0, pl=0, *, dh=1, dw=1):
    """dx [N,H,W,C] of a conv with output gradient dy [N,OH,OW,K] and weights [KH,KW,C,K] in f64: every
    output pixel's dy . w[kh, kw]^T added to the input pixel its tap (kh, kw) read.  And sum |dy||w|."""
    dy, wt = np.asarray(dy, np.float64), np.asarray(w_hwio, np.float64)
    N, OH, OW, K = dy.shape
    KH, KW, C, _ = wt.shape
    dx = np.zeros((N, h, w, C))
    ab = np.zeros((N, h, w, C))
    with np.errstate(invalid="ignore", over="ignore"):
        for kh in range(KH):
            o_h, i_h = _taps(h, OH, sh, pt, kh, dh)
            for kw in range(KW):
                o_w, i_w = _taps(w, OW, sw, pl, kw, dw)
                if o_h.size == 0 or o_w.size == 0:
                    continue
                ds = dy[:, o_h][:, :, o_w]  # (for one tap every output pixel reads a different input pixel)
                dx[np.ix_(np.arange(N), i_h, i_w)] += np.einsum("nhwk,ck->nhwc", ds, wt[kh, kw])
                ab[np.ix_(np.arange(N), i_h, i_w)] += np.einsum("nhwk,ck->nhwc", np.abs(ds), np.abs(wt[kh, kw]))
    return dx, ab


def conv_dgrad_s2_ref(dy, w_hwio, h, w):
    """Input gradient of a 1x1 stride-2 unpadded conv: dx[n, 2i, 2j] = dy[n, i, j] . w^T, zero elsewhere."""
    assert np.asarray(w_hwio).shape[:2] == (1, 1)
    return conv_dgrad_ref(dy, w_hwio, h, w, 2, 2, 0, 0)


def conv_wgrad_ref(x, dy, kh_, kw_, sh=1, sw=1, pt=0, pl=0, *, dh=1, dw=1):
    """dW [KH,KW,C,K] = sum over output pixels of x[tap pixel] (x) dy[pixel] in f64, and sum |x||dy|.
    (dh, dw: the filter's dilation.)"""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    N, H, W, C = x.shape
    _, OH, OW, K = dy.shape
    gw = np.zeros((kh_, kw_, C, K))
    ab = np.zeros((kh_, kw_, C, K))
    with np.errstate(invalid="ignore", over="ignore"):
        for kh in range(kh_):
            o_h, i_h = _taps(H, OH, sh, pt, kh, dh)
            for kw in range(kw_):
                o_w, i_w = _taps(W, OW, sw, pl, kw, dw)
                if o_h.size == 0 or o_w.size == 0:
                    continue
                xs, ds = x[:, i_h][:, :, i_w], dy[:, o_h][:, :, o_w]
                gw[kh, kw] = np.einsum("nhwc,nhwk->ck", xs, ds)
                ab[kh, kw] = np.einsum("nhwc,nhwk->ck", np.abs(xs), np.abs(ds))
    return gw, ab


def assert_exact(absum, what="product sums"):
    """Precondition of a bitwise test: every sum the kernel can form, in any order, is an integer below 2^24."""
    m = float(np.max(absum)) if np.size(absum) else 0.0
    assert m < EXACT_LIMIT, f"{what}: sum |a||b| reaches {m} >= 2^24; the data is not exact in f32"


# ------------------------------------------------------------------------------------- epilogues
def round_bf16(acc):
    """bf16 bits of the f32 accumulator: bf16(acc).  (acc f64 that is exact in f32, or the f32 itself.)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return bf16_rne(np.asarray(acc, np.float64).astype(np.float32))


def add_residual(bits, res_bits):
    """bf16(f32(bf16 value) + residual): the f32 sum of two bf16 values rounded once to f32, then to bf16."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = (bf16_bits_to_f64(bits) + bf16_bits_to_f64(res_bits)).astype(np.float32)  # (the f64 sum is exact)
    return bf16_rne(s)


def mask_from_bits(by_bits):
    """[by > 0] on bf16 bits (conv.hip relu_mask_bf16x8): sign clear and not +0 -- a positive subnormal
    passes, and so does a NaN with a clear sign (a NaN with the sign set does not)."""
    b = np.asarray(by_bits, np.uint16)
    return ((b & 0x8000) == 0) & ((b & 0x7FFF) != 0)


def mask_from_stats(bx_bits, scale, shift):
    """[fmaf(bx, scale, shift) > 0] in f32 (conv.hip relu_mask_affine_bf16x8).  bx * scale is exact in f64
    (8 x 24 significant bits); the sum is rounded to f64 and then to f32, which keeps its sign and zero."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = bf16_bits_to_f64(bx_bits) * np.asarray(scale, np.float32).astype(np.float64) + np.asarray(
            shift, np.float32).astype(np.float64)
        return v.astype(np.float32) > 0


def apply_mask(bits, mask):
    return np.where(mask, np.asarray(bits, np.uint16), np.uint16(0)).astype(np.uint16)


def in_bn_ref(x_bits, scale, shift):
    """bf16(max(fmaf(x, scale, shift), 0)) as bf16 bits: the input-side BN -> ReLU of the operand loader
    (fmaxf: a NaN pre-activation gives 0).  Exact when x * scale + shift is exact in f32."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = (bf16_bits_to_f64(x_bits) * np.asarray(scale, np.float32).astype(np.float64)
             + np.asarray(shift, np.float32).astype(np.float64)).astype(np.float32)
    return bf16_rne(np.where(v > 0, v, np.float32(0)))


def tile_sums(v_bits, other, bm, exact=True):
    """[ceil(M / bm)][2][K] f64: per row tile of the [M, K] stored bf16 values v the channel sums of v and
    of v * other (other: f64 [M, K]; None: v itself, the forward's sum of squares).  exact: asserts the
    sums of magnitudes stay below 2^24, so that any f32 summation order gives these values exactly."""
    v = bf16_bits_to_f64(v_bits)
    M, K = v.shape
    o = v if other is None else np.asarray(other, np.float64)
    P = (M + bm - 1) // bm
    out = np.zeros((P, 2, K))
    for p in range(P):
        r = slice(p * bm, min((p + 1) * bm, M))
        out[p, 0] = v[r].sum(0)
        out[p, 1] = (v[r] * o[r]).sum(0)
        if exact:
            assert_exact(np.abs(v[r]).sum(0), "tile sums")
            assert_exact(np.abs(v[r] * o[r]).sum(0), "tile product sums")
    return out


def part_rows(P):
    """Rows of a conv epilogue's partial-sum buffer for P row tiles: P data rows + ceil(P/64) scratch rows."""
    return P + (P + 63) // 64


def dgrad_epilogue_ref(acc, bm, res_bits=None, bn_y_bits=None, bn_x_bits=None, bn_ss=None, bn_x2_bits=None, exact=True):
    """Epilogue of the stride-1 input gradient on the f64 accumulator acc [N,H,W,C]: (dz bits, part, part2)
    with part / part2 None where the operands are absent.  Order: bf16(acc); + residual; mask (bn_y bits,
    or bn_ss = (scale, shift) on bn_x); sums of (dz, dz*bn_x) and (dz, dz*bn_x2) per tile of bm rows."""
    C = acc.shape[-1]
    v = round_bf16(acc)
    if res_bits is not None:
        v = add_residual(v, res_bits)
    part = part2 = None
    if bn_x_bits is not None:
        m = mask_from_stats(bn_x_bits, *bn_ss) if bn_ss is not None else mask_from_bits(bn_y_bits)
        v = apply_mask(v, m)
        part = tile_sums(v.reshape(-1, C), bf16_bits_to_f64(bn_x_bits).reshape(-1, C), bm, exact)
        if bn_x2_bits is not None:
            part2 = tile_sums(v.reshape(-1, C), bf16_bits_to_f64(bn_x2_bits).reshape(-1, C), bm, exact)
    return v, part, part2


def dgrad_s2_epilogue_ref(acc, h, w, bm, res_bits=None, bn_y_bits=None, bn_x_bits=None, bn_ss=None, bn_x2_bits=None,
                          exact=True):
    """Epilogue of the 1x1 stride-2 input gradient.  acc [N,OH,OW,C] f64 is the gradient of the even pixels;
    dx [N,h,w,C]: pixel (2i, 2j) gets bf16(acc) (+ residual), the other pixels of its 2x2 block (those
    inside h x w) the residual or zero; then the mask over all of them; the partial sums are per tile of
    bm dy pixels (n, i, j), each owning the pixels of its 2x2 block."""
    N, OH, OW, C = acc.shape
    v = np.zeros((N, h, w, C), np.uint16) if res_bits is None else np.array(res_bits, np.uint16)
    ev = round_bf16(acc)
    v[:, ::2, ::2] = ev if res_bits is None else add_residual(ev, np.asarray(res_bits, np.uint16)[:, ::2, ::2])
    part = part2 = None
    if bn_x_bits is not None:
        m = mask_from_stats(bn_x_bits, *bn_ss) if bn_ss is not None else mask_from_bits(bn_y_bits)
        v = apply_mask(v, m)

        def block_sums(other_bits):
            # the per-dy-pixel sums over its 2x2 block, then tiles of bm dy pixels
            vf, of = bf16_bits_to_f64(v), bf16_bits_to_f64(other_bits)
            s, q, sa, qa = (np.zeros((N, OH, OW, C)) for _ in range(4))
            for a in (0, 1):
                for b in (0, 1):
                    vv, oo = vf[:, a::2, b::2], of[:, a::2, b::2]
                    hh, ww = vv.shape[1], vv.shape[2]
                    s[:, :hh, :ww] += vv
                    q[:, :hh, :ww] += vv * oo
                    sa[:, :hh, :ww] += np.abs(vv)
                    qa[:, :hh, :ww] += np.abs(vv * oo)
            M = N * OH * OW
            P = (M + bm - 1) // bm
            out = np.zeros((P, 2, C))
            for p in range(P):
                r = slice(p * bm, min((p + 1) * bm, M))
                out[p, 0], out[p, 1] = s.reshape(M, C)[r].sum(0), q.reshape(M, C)[r].sum(0)
                if exact:
                    assert_exact(sa.reshape(M, C)[r].sum(0), "tile sums")
                    assert_exact(qa.reshape(M, C)[r].sum(0), "tile product sums")
            return out

        part = block_sums(bn_x_bits)
        if bn_x2_bits is not None:
            part2 = block_sums(bn_x2_bits)
    return v, part, part2


# ------------------------------------------------------------------------------------- f32 fusions (gemm_f32.hip)
def bias_act_ref(acc, bias=None, act=0, prior=None, fmaxf=True):
    """Epilogue of the f32 kernels on the f64 result acc [..., N]: + bias[N], + prior (the accumulated
    output), then the ReLU.  fmaxf: as the kernels take it (a NaN pre-activation gives 0); else max(v, 0),
    where a NaN stays."""
    v = np.asarray(acc, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if bias is not None:
            v = v + np.asarray(bias, np.float64)
        if prior is not None:
            v = v + np.asarray(prior, np.float64)
        if act:
            v = _relu_fmaxf(v) if fmaxf else np.maximum(v, 0.0)
    return v


def masked_ref(a, mask):
    """The masked operand of the f32 kernels: a select on mask > 0 (not a product): an Inf or NaN element
    under a mask <= 0 -- or under a NaN mask -- is an exact 0."""
    if mask is None:
        return np.asarray(a, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(mask) > 0, np.asarray(a, np.float64), 0.0)


def bias_grad_ref(dy, mask=None):
    """(db [K], sum |dy| [K]): the masked output gradient summed over every axis but the last."""
    g = masked_ref(dy, mask)
    g = g.reshape(-1, g.shape[-1])
    with np.errstate(invalid="ignore", over="ignore"):
        return g.sum(0), np.abs(g).sum(0)


def conv_pool_fwd_ref(x, w_ohwi, bias, oh, ow, sh=1, sw=1, pt=0, pl=0, *, dh=1, dw=1, act=1):
    """conv -> (+ bias) -> ReLU (fmaxf) -> 2x2 / stride-2 'valid' max pool: (y [N,OH,OW,K], maximum
    [N,OH/2,OW/2,K], argmax uint8, sum |x||w| + |bias|).  The pool is kernel_refs.maxpool_fwd_ref: the first
    maximum of the window in (dy, dx) order wins, a NaN never does, a window of NaNs gives -inf and 255."""
    acc, ab = conv_fwd_ref(x, w_ohwi, oh, ow, sh, sw, pt, pl, dh=dh, dw=dw)
    y = bias_act_ref(acc, bias, act)
    if bias is not None:
        ab = ab + np.abs(np.asarray(bias, np.float64))
    ph, pw = oh // 2, ow // 2
    mx, arg = maxpool_fwd_ref(y[:, :2 * ph, :2 * pw], 2, 2, 2, 2, 0, 0, 0, 0, False)
    return y, mx, arg, ab


def conv_pool_bwd_ref(dp, mx, arg, oh, ow):
    """The conv-output gradient [N,OH,OW,K] the pooled-gradient loaders form from the pool's output gradient
    dp [N,PH,PW,K]: dp at the window position its argmax names, where the pooled maximum is > 0 (the ReLU
    mask); nothing where the argmax is 255; zero at pixels of an odd last row / column (in no window)."""
    dp, mx, arg = np.asarray(dp, np.float64), np.asarray(mx), np.asarray(arg)
    N, PH, PW, K = dp.shape
    dy = np.zeros((N, oh, ow, K))
    g = masked_ref(dp, mx)
    for q in range(4):
        dy[:, q // 2:2 * PH:2, q % 2:2 * PW:2] = np.where(arg == q, g, 0.0)
    return dy


# ------------------------------------------------------------------------------------- stem (stem.hip)
def stem_geometry(H, W, KH, KW, SH, pads):
    """(OH, OW, HPp, WP) of the small-channel conv with column stride 2 and pads (top, bottom, left, right):
    the output size of the padded image, and the packed image's rows and columns.  Every output pixel's
    window is 8 columns wide whatever KW is, so the packed row reaches column 2 (OW - 1) + 7 at the least;
    the packed image has the rows the last output row reads.  (An image smaller than the filter: OH or
    OW <= 0 by the floor division.)"""
    pt, pb, pl, pr = pads
    OH = (H + pt + pb - KH) // SH + 1
    OW = (W + pl + pr - KW) // 2 + 1
    WP = max(W + pl + pr, 2 * (OW - 1) + 8)
    HPp = max(H + pt + pb, (OH - 1) * SH + KH)
    return OH, OW, HPp, WP


def stem_pack_ref(x, is_f32, KH, KW, SH, pads):
    """uint16 bits of the packed image xp [N][HPp][WP][4] of x [N,H,W,C] (is_f32: f32 values, rounded with
    bf16_rne -- a NaN of any payload stays a NaN; else bf16 bits, copied): pixel (h, w) at (h + pt, w + pl),
    zero bits in the border and in channels C..3."""
    x = np.asarray(x, np.float32 if is_f32 else np.uint16)
    N, H, W, C = x.shape
    _, _, HPp, WP = stem_geometry(H, W, KH, KW, SH, pads)
    xp = np.zeros((N, HPp, WP, 4), np.uint16)
    xp[:, pads[0]:pads[0] + H, pads[2]:pads[2] + W, :C] = bf16_rne(x) if is_f32 else x
    return xp


# ------------------------------------------------------------------------------------- data and bounds
def coded_ints(shape, amp, salt, zero_frac=0.0):
    """Position-coded integers in [-amp, amp] as f64: a fixed integer hash of the element's coordinates
    (the last coordinate enters both as itself and mod 13), so that a shifted, mirrored or transposed read
    sees different values.  zero_frac of the elements are zero."""
    idx = np.indices(shape, dtype=np.int64)
    mult = [1000003, 10007, 1009, 101, 31, 7]
    h = np.full(shape, 12345 + 7919 * salt, dtype=np.int64)
    for d in range(len(shape)):
        h = h * 31 + idx[d] * mult[d % len(mult)]
    h = h + (idx[-1] % 13) * 4099
    h = (h ^ (h >> 15)) * 2246822519 % (1 << 32)
    h = (h ^ (h >> 13)) * 3266489917 % (1 << 32)
    h = h ^ (h >> 16)
    v = (h % (2 * amp + 1)) - amp
    if zero_frac > 0:
        v = np.where((h >> 8) % 1000 < int(zero_frac * 1000), 0, v)
    return v.astype(np.float64)


def amp_for(reduction, target_std):
    """Amplitude a such that a sum of `reduction` products of two uniform integers in [-a, a] has about the
    standard deviation target_std (var of one factor a(a+1)/3)."""
    a = 1
    while np.sqrt(reduction) * (a + 1) * (a + 2) / 3.0 <= target_std and a < 127:
        a += 1
    return a


def count_ties(acc):
    """(down, up, negative, positive): accumulator values exactly halfway between two bf16 values, by whether
    round-to-nearest-even takes the magnitude down or up, and by sign."""
    a = np.asarray(acc, np.float64)
    a = a[np.isfinite(a) & (a != 0)]
    lo = bf16_bits_to_f64(bf16_rne(a.astype(np.float32)).astype(np.uint16))
    u = ulp_bf16(a)
    tie = np.abs(np.abs(a) - np.abs(lo)) == u / 2  # (after rounding, |a - bf16(a)| == half a spacing of a)
    # a value at a power of two's upper side: the spacing is taken at |a|, which is the finer one, fine
    down = tie & (np.abs(lo) < np.abs(a))
    up = tie & (np.abs(lo) > np.abs(a))
    return int(down.sum()), int(up.sum()), int((tie & (a < 0)).sum()), int((tie & (a > 0)).sum())


def error_bound(ref, absum, reduction):
    """|y - r| <= 1/2 ulp_bf16(|r| + e) + e with e = R 2^-23 sum |a||b|: the f32 accumulation error of an
    R-term dot product in any order (each of at most R roundings is relative 2^-24 of a partial sum bounded
    by sum |a||b|; 2^-23 leaves a factor two), then one rounding to bf16."""
    e = reduction * 2.0 ** -23 * np.asarray(absum, np.float64)
    return 0.5 * ulp_bf16(np.abs(ref) + e) + e


def error_bound_f32(absum, reduction):
    """Bound of an f32 output (the weight gradient's `out`): e alone, plus its final rounding."""
    e = reduction * 2.0 ** -23 * np.asarray(absum, np.float64)
    return e
