"""The small-channel stride-2 conv kernels (csrc/kernels/stem.hip: k_stem_pack, k_stem_wpack, k_stem_fwd with
its fused batch-norm partial sums, k_stem_wgrad, k_stem_wgrad_reduce) and their bindings' geometry against
the f64 references of tests/conv_refs.py.

Exact cases: position-coded small integers, every product sum below 2^24 (asserted by the reference), so any
MFMA order, any slice split and any reduce order is exact: y must equal bf16_rne of the f64 sum bit for bit,
the f32 `out` of the weight gradient the f64 value, accumulate=True an integer base plus it, the bf16 dw
bf16_rne of it.  With KW < 8 the taps kw >= KW of a packed window hold real neighbouring pixels (non-zero
coded integers): the exact comparison with the KW-wide reference also shows that the zero weights of the
forward and the dropped columns of the reduce let nothing of them through.  Random-data cases use the derived
bounds of conv_refs.error_bound (forward: R = KH * 32 taps; weight gradient: R = pixels + slices).

Every tensor goes to the device as bit patterns and every comparison is on the CPU in numpy.  The references
run on the explicitly padded image, which is conv_refs.stem_pack_ref's -- the pack kernel is compared with
that bitwise first.
"""
import numpy as np
import pytest
import torch

import conv_refs as CR
import kernel_refs as R

pytestmark = pytest.mark.gpu

PATHS = ("pack f32", "pack bf16", "forward", "forward stats", "wgrad bf16", "wgrad f32", "wgrad accumulate")
RAN = {}    # path -> [cases, ties down, ties up]
RATIO = {}  # path -> largest error / bound

ROWS = 256    # output pixels per forward workgroup: the row tile of the BN partial sums (stem.hip kRows)
SLICE = 4096  # output pixels per weight-gradient workgroup (stem.hip kWgPix)


@pytest.fixture(scope="module")
def C():
    from tensorflow_distributed_learning_amd.ops import hip

    return hip()


def _dev(bits):
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).view(torch.bfloat16).cuda()


def _dev32(v):
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()


def _bits(t):
    return t.contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def _f64(t):
    return t.cpu().numpy().astype(np.float64)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype == np.uint16:
        bad = (got != want) & ~(R.bf16_is_nan(got) & R.bf16_is_nan(want))
    else:
        bad = (got != want) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        i = np.argwhere(bad)
        show = [(tuple(j), got[tuple(j)], want[tuple(j)]) for j in i[:6]]
        raise AssertionError(f"{what}: {len(i)} of {got.size} values differ (index, got, want): {show}")


def _ran(path, dn=0, up=0):
    r = RAN.setdefault(path, [0, 0, 0])
    r[0] += 1
    r[1] += dn
    r[2] += up


def _ratio(path, v):
    RATIO[path] = max(RATIO.get(path, 0.0), float(v))


class Geo:
    """(N, H, W, C, K, KH, KW, SH, (pt, pb, pl, pr)); the column stride is 2."""

    def __init__(self, g):
        self.g = g
        self.N, self.H, self.W, self.C, self.K, self.KH, self.KW, self.SH, self.pads = g
        self.OH, self.OW, self.HPp, self.WP = CR.stem_geometry(self.H, self.W, self.KH, self.KW, self.SH, self.pads)
        assert self.OH > 0 and self.OW > 0
        self.M = self.N * self.OH * self.OW
        self.P = -(-self.M // ROWS)
        self.slices = -(-self.M // SLICE)

    def __repr__(self):
        return (f"stem N{self.N} {self.H}x{self.W}x{self.C} -> {self.OH}x{self.OW}x{self.K} f{self.KH}x{self.KW} "
                f"s{self.SH}2 p{self.pads} M{self.M} xp {self.HPp}x{self.WP}")

    def padded(self, x_bits):
        """The explicitly padded image as f64 [N, HPp, WP, C] (the reference's input) and the packed bits."""
        xp = CR.stem_pack_ref(x_bits, False, self.KH, self.KW, self.SH, self.pads)
        return R.bf16_bits_to_f64(xp)[..., :self.C], xp

    def fwd(self, c, x, w, stats=False):
        return c.stem_fwd(x, w, *self.pads, self.SH, 2, stats)


def _exact_bits(v):
    b = R.bf16_rne(np.asarray(v, np.float32))
    assert np.array_equal(R.bf16_bits_to_f64(b), np.asarray(v, np.float64)), "test data is not exact in bf16"
    return b


def _rand_bits(rng, shape, scale=1.0):
    return R.bf16_rne((rng.randn(*shape) * scale).astype(np.float32))


# ------------------------------------------------------------------------------------- pack
def _f32_pool():
    """f32 pixels: every special of kernel_refs (+-0, +-Inf, the largest finite -- rounds to Inf --, subnormals,
    exact ties both ways, neighbours of ties), the three NaN payloads the integer rounding carries out of in
    both signs, and values that are no bf16 values.  57 values: odd, so a cyclic fill puts every one of them
    into every channel of a 2- or 4-channel image."""
    rng = np.random.default_rng(7)
    rnd = (rng.standard_normal(31) * 2.0 ** rng.integers(-20, 20, 31)).astype(np.float32)
    assert np.all(R.bf16_bits_to_f64(R.bf16_rne(rnd)) != rnd.astype(np.float64))
    nan = np.concatenate([R.NAN_PAYLOADS_F32.view(np.uint32), R.NAN_PAYLOADS_F32.view(np.uint32) ^ 0x80000000])
    pool = np.concatenate([R.SPECIALS_F32, nan.astype(np.uint32).view(np.float32), rnd])
    assert pool.size == 57 and np.isnan(pool).sum() == 6
    return pool


def _bf16_pool():
    """bf16 pixels, copied bit for bit: +-0, +-Inf, subnormals, quiet and signalling NaNs, random bits."""
    rng = np.random.default_rng(8)
    sp = np.array([0x0000, 0x8000, 0x7F80, 0xFF80, 0x0001, 0x8001, 0x007F, 0x7F7F, 0xFF7F, 0x7FC0, 0xFFC0, 0x7F81, 0xFF81,
                   0x7FFF, 0xFFFF], np.uint16)
    return np.concatenate([sp, rng.integers(0, 1 << 16, 42).astype(np.uint16)])  # 57 values


# (N, H, W, KH, KW, SH, pads): each pad zero and non-zero; WP widened past the padded width (KW < 8 on a narrow
# image) and not widened; KW = 8 on an odd padded width (WP = 13: packed rows only 8-byte aligned); SH = 3
# with bottom rows no window reaches.  Every image has >= 57 * C elements for the pools above.
PACK_GEOMS = {
    "all_pads_7x7": (2, 6, 7, 7, 7, 2, (3, 2, 1, 4)),            # padded 11x12, OW 3: 2*2+8 = 12, not widened
    "no_pads_widened": (2, 6, 7, 3, 3, 2, (0, 0, 0, 0)),          # padded width 7, OW 3: WP = 12
    "top_right_only_widened": (2, 6, 7, 5, 2, 1, (2, 0, 0, 1)),   # padded width 8, OW 4: WP = 14
    "bottom_left_only": (2, 6, 7, 4, 7, 3, (0, 3, 2, 0)),         # padded 9x9, SH 3: OH 2 reads rows 0..6
    "kw8_odd_width": (2, 6, 8, 2, 8, 2, (0, 1, 3, 2)),            # padded width 13, OW 3: 12 < 13, WP = 13 odd
}


@pytest.mark.parametrize("Cin", [1, 2, 3, 4])
@pytest.mark.parametrize("f32", [True, False], ids=["f32", "bf16"])
def test_pack_is_bitwise_the_reference(C, f32, Cin):
    """xp as stem_fwd returns it against stem_pack_ref: rounding of f32 pixels (a NaN of any payload stays a
    NaN), bf16 pixels copied bit for bit (strictly: NaN payloads too), zero border and zero channels C..3.

    The packed image never has more rows than the padded one: (OH - 1) SH + KH <= HP whenever the padded
    image is at least as tall as the filter (test_conv_refs_cpu.py), and a shorter one is refused
    (test_refusals)."""
    widened = odd = False
    for name, (N, H, W, KH, KW, SH, pads) in PACK_GEOMS.items():
        g = Geo((N, H, W, Cin, 64, KH, KW, SH, pads))
        pool = _f32_pool() if f32 else _bf16_pool()
        x = np.resize(np.roll(pool, Cin), (N, H, W, Cin))
        assert x.size >= pool.size * Cin and g.HPp == H + pads[0] + pads[1]
        widened |= g.WP > W + pads[2] + pads[3]
        odd |= g.WP == W + pads[2] + pads[3] and g.WP % 2 == 1 and KW == 8
        want = CR.stem_pack_ref(x, f32, KH, KW, SH, pads)
        w = _dev(_exact_bits(CR.coded_ints((KH, KW, Cin, 64), 3, 5)))
        out = g.fwd(C, _dev32(x) if f32 else _dev(x), w)
        got = _bits(out[1])
        assert tuple(out[1].shape) == (N, g.HPp, g.WP, 4) and out[1].dtype == torch.bfloat16
        if f32:
            nan = R.bf16_is_nan(want)
            assert nan.sum() >= 6 * Cin
            assert R.bf16_is_nan(got[nan]).all(), (
                f"{g!r} {name}: an f32 NaN pixel must stay a NaN, got {sorted({hex(v) for v in got[nan]})}")
            _same(got, want, f"{g!r} {name} pack f32")
        else:
            assert np.array_equal(got, want), f"{g!r} {name} pack bf16: {(got != want).sum()} values differ"
    assert widened and odd
    _ran("pack f32" if f32 else "pack bf16")


# ------------------------------------------------------------------------------------- forward, exact
FWD_GEOMS = {
    "m1860_8_tiles": (2, 61, 60, 3, 64, 7, 7, 2, (3, 3, 3, 3)),   # last tile partial; images cross tile boundaries
    "m2244_9_tiles": (2, 67, 66, 3, 64, 7, 7, 2, (3, 3, 3, 3)),   # XCD remap with a remainder
    "m45_1x1_c1": (1, 9, 9, 1, 64, 1, 1, 1, (0, 0, 0, 0)),        # fewer rows than one wave's
    "f8x8_c4_s3_k128": (3, 20, 23, 4, 128, 8, 8, 3, (1, 2, 0, 1)),
    "k192_widened": (1, 16, 37, 2, 192, 3, 5, 2, (0, 1, 2, 0)),
    "s1_f2x8": (4, 16, 32, 3, 64, 2, 8, 1, (0, 0, 0, 0)),
    "m256_exactly": (1, 33, 33, 3, 64, 3, 3, 2, (0, 0, 0, 0)),    # 16 x 16 outputs: one full tile
    "m257_oh1_ow257": (1, 5, 516, 2, 64, 5, 4, 1, (0, 0, 0, 0)),  # one row into a second tile; OW >= 64, OH = 1
    "kw8_odd_width": (2, 10, 21, 3, 64, 4, 8, 2, (1, 1, 0, 0)),   # WP = 21: rows of xp 8-byte aligned
}
_fcache = {}


class FProb:
    def __init__(self, name, regime):
        self.g = g = Geo(FWD_GEOMS[name])
        self.regime = regime
        a = CR.amp_for(g.KH * g.KW * g.C, 40 if regime == "small" else 3000)
        x = CR.coded_ints((g.N, g.H, g.W, g.C), a, 1)
        w = CR.coded_ints((g.KH, g.KW, g.C, g.K), a, 2)
        self.x_bits, self.w_bits = _exact_bits(x), _exact_bits(w)
        xpad, self.xp_bits = g.padded(self.x_bits)
        self.ref, ab = CR.conv_fwd_ref(xpad, w.transpose(3, 0, 1, 2), g.OH, g.OW, g.SH, 2, 0, 0)
        CR.assert_exact(ab)
        self.y_bits = CR.round_bf16(self.ref)
        yb = self.y_bits.reshape(g.M, g.K)
        self.part = CR.tile_sums(yb, None, ROWS, exact=regime == "small")
        if regime == "large":  # the sums of y stay exact; the sums of squares may round
            v = np.abs(R.bf16_bits_to_f64(yb))
            for p in range(g.P):
                CR.assert_exact(v[p * ROWS:(p + 1) * ROWS].sum(0), "tile sums")
        self.ties = CR.count_ties(self.ref)[:2]


def fprob(name, regime):
    if (name, regime) not in _fcache:
        _fcache[name, regime] = FProb(name, regime)
    return _fcache[name, regime]


@pytest.mark.parametrize("regime", ["small", "large"])
@pytest.mark.parametrize("name", list(FWD_GEOMS))
def test_forward_is_bitwise_and_its_bn_sums_exact_per_tile(C, name, regime):
    """y = bf16_rne(f64 sum) bit for bit, from bf16 and from f32 images, with and without the BN partial sums;
    rows 0..P-1 of the partial buffer hold each 256-row tile's channel sums of the stored y and y^2 (the scratch
    rows after them are not read).  small: both sums exact.  large (about 80 % of the outputs are rounded,
    thousands are exact ties): the sum of y exact, the sum of y^2 within 256 * 2^-23 of itself."""
    p = fprob(name, regime)
    g = p.g
    w = _dev(p.w_bits)
    for f32 in (False, True):
        x = _dev32(R.bf16_bits_to_f64(p.x_bits)) if f32 else _dev(p.x_bits)
        for stats in (False, True):
            what = f"{g!r} {regime} {'f32' if f32 else 'bf16'} x{' stats' if stats else ''}"
            out = g.fwd(C, x, w, stats)
            assert len(out) == (3 if stats else 2) and tuple(out[0].shape) == (g.N, g.OH, g.OW, g.K)
            _same(_bits(out[1]), p.xp_bits, what + " xp")
            _same(_bits(out[0]), p.y_bits, what + " y")
            if not stats:
                continue
            part = _f64(out[2])
            assert part.shape == (CR.part_rows(g.P), 2, g.K), part.shape
            _same(part[:g.P, 0], p.part[:, 0], what + " sum y per tile")
            if regime == "small":
                _same(part[:g.P, 1], p.part[:, 1], what + " sum y^2 per tile")
            else:
                err, bound = np.abs(part[:g.P, 1] - p.part[:, 1]), ROWS * 2.0 ** -23 * p.part[:, 1]
                _ratio("forward stats", np.max(err / np.maximum(bound, 1e-300)))
                assert np.all(err <= bound), (what, float(np.max(err / np.maximum(bound, 1e-300))))
    dn, up = p.ties if regime == "large" else (0, 0)
    _ran("forward", dn, up)
    _ran("forward stats", dn, up)


# ------------------------------------------------------------------------------------- weight gradient, exact
WG_GEOMS = {
    "m45_1x1_c1": (1, 9, 9, 1, 64, 1, 1, 1, (0, 0, 0, 0)),            # one partial chunk; KH = 1: waves 2-3 idle
    "ow4_f8x8_c4_s3": (2, 40, 8, 4, 64, 8, 8, 3, (1, 2, 3, 3)),       # M = 96: many wraps per chunk, across images
    "ow128_m4096": (1, 70, 262, 3, 64, 7, 7, 2, (0, 0, 0, 0)),        # exactly one slice; chunks never wrap
    "ow67_2_slices": (1, 134, 134, 3, 64, 7, 7, 2, (3, 3, 3, 3)),     # M = 4489: the second slice of 393 pixels
    "5_slices_k128": (4, 134, 134, 3, 128, 7, 7, 2, (3, 3, 3, 3)),    # reduce phases uneven
    "9_slices": (8, 134, 134, 3, 64, 7, 7, 2, (3, 3, 3, 3)),          # slice remap with a remainder
    "ow1_m88": (4, 50, 8, 3, 64, 7, 8, 2, (0, 0, 0, 0)),              # a chunk wraps 64 rows
    "oh1_m216": (3, 7, 150, 3, 64, 7, 7, 2, (0, 0, 0, 0)),            # OW = 72: every row ends an image
    "m4097": (1, 19, 487, 3, 64, 3, 7, 1, (0, 0, 0, 0)),              # 17 x 241: the second slice holds one pixel
    "k192": (2, 20, 20, 3, 192, 5, 5, 2, (2, 2, 2, 2)),               # M = 200
    "m65": (1, 11, 27, 2, 64, 3, 3, 2, (0, 0, 0, 0)),                 # 5 x 13: M % 64 = 1
    "m127": (1, 3, 259, 3, 64, 3, 7, 1, (0, 0, 0, 0)),                # 1 x 127: M % 64 = 63
}
_wcache = {}


class WProb:
    def __init__(self, geo, random=False, salt=0):
        self.g = g = Geo(geo)
        self.random = random
        if random:
            rng = np.random.RandomState(60 + salt)
            self.x_bits = _rand_bits(rng, (g.N, g.H, g.W, g.C))
            self.dy_bits = _rand_bits(rng, (g.N, g.OH, g.OW, g.K), g.M ** -0.5)
        else:
            a = CR.amp_for(g.M, 350)
            self.x_bits = _exact_bits(CR.coded_ints((g.N, g.H, g.W, g.C), a, 1 + 10 * salt))
            self.dy_bits = _exact_bits(CR.coded_ints((g.N, g.OH, g.OW, g.K), a, 2 + 10 * salt))
        self.w_bits = _exact_bits(CR.coded_ints((g.KH, g.KW, g.C, g.K), 2, 3))
        self.reference()
        self._d = None

    def reference(self):
        g = self.g
        xpad, self.xp_bits = g.padded(self.x_bits)
        self.dw, self.ab = CR.conv_wgrad_ref(xpad, R.bf16_bits_to_f64(self.dy_bits), g.KH, g.KW, g.SH, 2, 0, 0)
        self.base = CR.coded_ints(self.dw.shape, 1000, 7)
        if not self.random:
            CR.assert_exact(self.ab + np.abs(self.base))

    def dev(self, c):
        """(xp as stem_fwd packed it, dy) on the device; xp is checked against the reference once."""
        if self._d is None:
            xp = self.g.fwd(c, _dev(self.x_bits), _dev(self.w_bits))[1]
            _same(_bits(xp), self.xp_bits, f"{self.g!r} xp")
            self._d = (xp, _dev(self.dy_bits))
        return self._d

    def call(self, c, out=None, accumulate=False):
        g = self.g
        xp, dy = self.dev(c)
        return c.stem_wgrad(xp, dy, g.KH, g.KW, g.C, g.SH, out, accumulate)


def wprob(name):
    if name not in _wcache:
        _wcache[name] = WProb(WG_GEOMS[name])
    return _wcache[name]


@pytest.mark.parametrize("name", list(WG_GEOMS))
def test_weight_gradient_is_exact_in_every_mode(C, name):
    """The bf16 dw bitwise, the f32 out exactly (over a sentinel), accumulate onto an integer base exactly."""
    p = wprob(name)
    g = p.g
    assert g.slices == {"ow128_m4096": 1, "ow67_2_slices": 2, "5_slices_k128": 5, "9_slices": 9, "m4097": 2}.get(name, 1)
    dn, up = CR.count_ties(p.dw)[:2]
    got = p.call(C)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == p.dw.shape
    _same(_bits(got), CR.round_bf16(p.dw), f"{g!r} bf16")
    _ran("wgrad bf16", dn, up)
    out = torch.full(p.dw.shape, 123.0, device="cuda")
    _same(_f64(p.call(C, out, False)), p.dw, f"{g!r} f32")
    _ran("wgrad f32")
    out = _dev32(p.base)
    _same(_f64(p.call(C, out, True)), p.base + p.dw, f"{g!r} accumulate")
    _ran("wgrad accumulate")
    if name == "9_slices":  # deterministic: the same bits on a second call
        assert np.array_equal(_bits(p.call(C)), _bits(got))
        out2 = torch.full(p.dw.shape, -7.0, device="cuda")
        assert np.array_equal(p.call(C, out2, False).cpu().numpy(), p.call(C, out, False).cpu().numpy())


# ------------------------------------------------------------------------------------- random data
@pytest.mark.parametrize("name", ["m2244_9_tiles", "f8x8_c4_s3_k128", "k192_widened"])
def test_forward_random_data_within_the_derived_bound(C, name):
    """|y - r| <= 1/2 ulp_bf16(|r| + e) + e, e = KH * 32 * 2^-23 sum |x||w| (every MFMA reduces 32 taps, zero
    weighted ones included); the BN sums of the stored y within 256 * 2^-23 of the sums of magnitudes."""
    g = Geo(FWD_GEOMS[name])
    rng = np.random.RandomState(70 + g.M % 50)
    x_bits, w_bits = _rand_bits(rng, (g.N, g.H, g.W, g.C)), _rand_bits(rng, (g.KH, g.KW, g.C, g.K), 0.1)
    xpad, _ = g.padded(x_bits)
    ref, ab = CR.conv_fwd_ref(xpad, R.bf16_bits_to_f64(w_bits).transpose(3, 0, 1, 2), g.OH, g.OW, g.SH, 2, 0, 0)
    for f32 in (False, True):
        x = _dev32(R.bf16_bits_to_f64(x_bits)) if f32 else _dev(x_bits)
        y, _, part = g.fwd(C, x, _dev(w_bits), True)
        yb = _bits(y)
        r = float(np.max(np.abs(R.bf16_bits_to_f64(yb) - ref) / CR.error_bound(ref, ab, g.KH * 32)))
        sums = CR.tile_sums(yb.reshape(g.M, g.K), None, ROWS, exact=False)
        mags = CR.tile_sums(yb.reshape(g.M, g.K) & 0x7FFF, None, ROWS, exact=False)  # sums of |y| and y^2
        rs = float(np.max(np.abs(_f64(part)[:g.P] - sums) / np.maximum(ROWS * 2.0 ** -23 * mags, 1e-300)))
        print(f"bound stem forward {name} {'f32' if f32 else 'bf16'} x: y error / bound = {r:.4f}, sums = {rs:.4f}")
        _ratio("forward", r)
        _ratio("forward stats", rs)
        assert r <= 1.0 and rs <= 1.0, (name, r, rs)


@pytest.mark.parametrize("name", ["ow67_2_slices", "ow4_f8x8_c4_s3", "k192", "m4097"])
def test_weight_gradient_random_data_within_the_derived_bound(C, name):
    """|dw - r| <= e for the f32 out (plus its final rounding) and <= 1/2 ulp_bf16(|r| + e) + e for the bf16
    dw, e = (M + slices) 2^-23 sum |x||dy|: derived, not tuned."""
    p = WProb(WG_GEOMS[name], random=True)
    red = p.g.M + p.g.slices
    f = _f64(p.call(C, torch.zeros(p.dw.shape, device="cuda"), False))
    b = R.bf16_bits_to_f64(_bits(p.call(C)))
    a = _f64(p.call(C, _dev32(p.base), True)) - p.base
    e = CR.error_bound_f32(p.ab, red)
    r32 = float(np.max(np.abs(f - p.dw) / np.maximum(e + 0.5 * R.ulp32(p.dw), 1e-300)))
    r16 = float(np.max(np.abs(b - p.dw) / CR.error_bound(p.dw, p.ab, red)))
    # base + dw is rounded once more, at the magnitude of the sum
    racc = float(np.max(np.abs(a - p.dw) / np.maximum(e + 0.5 * R.ulp32(np.abs(p.base) + np.abs(p.dw) + e), 1e-300)))
    print(f"bound stem wgrad {name}: f32 error / bound = {r32:.4f}, bf16 = {r16:.4f}, accumulate = {racc:.4f}")
    _ratio("wgrad f32", r32)
    _ratio("wgrad bf16", r16)
    _ratio("wgrad accumulate", racc)
    assert r32 <= 1.0 and r16 <= 1.0 and racc <= 1.0, (name, r32, r16, racc)


# ------------------------------------------------------------------------------------- non-finite data
NAN_GEO = (2, 12, 14, 3, 64, 7, 7, 2, (3, 3, 3, 0))  # padded 18 x 17, OW = 6: the last field ends at column 16 = x's last
# (h, w, c) of the NaN pixel of image 1: next to the left border; the last column any field reaches; an odd
# padded column (9 = 2 * 1 + 7), which output column 1 reads only through its zero-weighted eighth tap
NAN_PIXELS = {"left_border": (5, 0, 1), "last_column": (6, 13, 2), "eighth_tap": (0, 6, 0)}


def _nan_problem(pix):
    p = WProb(NAN_GEO)
    g = p.g
    assert 2 * (g.OW - 1) + g.KW - 1 - g.pads[2] == g.W - 1
    h, w, c = pix
    p.x_bits = p.x_bits.copy()
    p.x_bits[1, h, w, c] = 0x7FC0
    p.random = True  # (no exactness assertion on sums that hold a NaN)
    p.reference()
    return p, h + g.pads[0], w + g.pads[2]


@pytest.mark.parametrize("pix", list(NAN_PIXELS))
def test_forward_nan_pixel_reaches_its_fields_and_at_most_its_windows(C, pix):
    """One NaN pixel (bf16 x).  Every output whose true KH x KW field holds it is NaN; every output whose
    KH x 8-column window does not hold it is finite and bit-equal to the reference.  An output in between
    reads the pixel only through the zero-weighted eighth tap of its window (KW = 7): 0 * NaN is NaN in
    the MFMA, so such an output may be either NaN or the reference value.  That is a documented property of
    the 8-tap window of stem.hip, not a defect: this test pins down where it can happen and nowhere else."""
    p, hp, wp = _nan_problem(NAN_PIXELS[pix])
    g = p.g
    w = CR.coded_ints((g.KH, g.KW, g.C, g.K), 3, 2)
    xpad, xp_bits = g.padded(p.x_bits)
    ref, _ = CR.conv_fwd_ref(xpad, w.transpose(3, 0, 1, 2), g.OH, g.OW, g.SH, 2, 0, 0)
    oh, ow = np.arange(g.OH)[:, None], np.arange(g.OW)[None, :]
    rows = (oh * g.SH <= hp) & (hp < oh * g.SH + g.KH)
    field = np.zeros((g.N, g.OH, g.OW), bool)
    window = np.zeros((g.N, g.OH, g.OW), bool)
    field[1] = rows & (2 * ow <= wp) & (wp < 2 * ow + g.KW)
    window[1] = rows & (2 * ow <= wp) & (wp < 2 * ow + 8)
    assert field.any() and np.array_equal(np.isnan(ref).all(-1), field) and np.array_equal(np.isnan(ref).any(-1), field)
    assert (window & ~field).any() == (pix == "eighth_tap")
    for stats in (False, True):
        out = g.fwd(C, _dev(p.x_bits), _dev(_exact_bits(w)), stats)
        _same(_bits(out[1]), xp_bits, f"{g!r} NaN {pix} xp")
        got, want = _bits(out[0]), CR.round_bf16(ref)
        nan = R.bf16_is_nan(got)
        assert nan[field].all(), f"{pix}: {(~nan[field]).sum()} outputs whose field holds the NaN pixel are finite"
        assert not nan[~window].any(), f"{pix}: {nan[~window].sum()} outputs outside every window of the pixel are NaN"
        _same(got[~window], want[~window], f"{g!r} NaN {pix} outside the windows")
        between = window & ~field
        ok = nan[between] | (got[between] == want[between])
        assert ok.all(), f"{pix}: an eighth-tap output is neither NaN nor the reference"


@pytest.mark.parametrize("pix", list(NAN_PIXELS))
def test_weight_gradient_nan_pixel_reaches_exactly_the_taps_that_read_it(C, pix):
    """dw[kh, kw, c, :] is NaN for exactly the taps under which some output pixel reads the NaN pixel; every
    other entry equals the reference (f32 out exactly, bf16 dw bitwise)."""
    p, hp, wp = _nan_problem(NAN_PIXELS[pix])
    g = p.g
    c = NAN_PIXELS[pix][2]
    taps = np.array([[any(o * g.SH + kh == hp for o in range(g.OH)) and any(2 * o + kw == wp for o in range(g.OW))
                      for kw in range(g.KW)] for kh in range(g.KH)])
    nan = np.isnan(p.dw)
    assert taps.any() and not np.delete(nan, c, axis=2).any()
    assert np.array_equal(nan[:, :, c, :].all(-1), taps) and np.array_equal(nan[:, :, c, :].any(-1), taps)
    _same(_f64(p.call(C, torch.zeros(p.dw.shape, device="cuda"), False)), p.dw, f"{g!r} NaN {pix} f32")
    _same(_bits(p.call(C)), CR.round_bf16(p.dw), f"{g!r} NaN {pix} bf16")


# ------------------------------------------------------------------------------------- refusals
def test_refusals(C):
    def t(*s, dtype=torch.bfloat16):
        return torch.ones(*s, device="cuda", dtype=dtype)

    x, w = t(2, 12, 12, 3), t(7, 7, 3, 64)
    y, xp = C.stem_fwd(x, w, 3, 3, 3, 3, 2, 2)
    assert tuple(y.shape) == (2, 6, 6, 64) and tuple(xp.shape) == (2, 18, 18, 4)
    dy = t(2, 6, 6, 64)
    assert tuple(C.stem_wgrad(xp, dy, 7, 7, 3, 2).shape) == (7, 7, 3, 64)
    bad = [
        lambda: C.stem_fwd(t(2, 12, 12, 5), t(7, 7, 5, 64), 3, 3, 3, 3, 2, 2),  # C = 5
        lambda: C.stem_fwd(x, t(9, 7, 3, 64), 3, 3, 3, 3, 2, 2),                # KH = 9
        lambda: C.stem_fwd(x, t(7, 9, 3, 64), 3, 3, 3, 3, 2, 2),                # KW = 9
        lambda: C.stem_fwd(x, w, 3, 3, 3, 3, 2, 1),                             # column stride 1
        lambda: C.stem_fwd(x, t(7, 7, 3, 32), 3, 3, 3, 3, 2, 2),                # K = 32
        lambda: C.stem_fwd(x, w, -1, 3, 3, 3, 2, 2),                            # a negative pad, each side
        lambda: C.stem_fwd(x, w, 3, -1, 3, 3, 2, 2),
        lambda: C.stem_fwd(x, w, 3, 3, -1, 3, 2, 2),
        lambda: C.stem_fwd(x, w, 3, 3, 3, -1, 2, 2),
        lambda: C.stem_fwd(t(2, 4, 12, 3), w, 0, 0, 3, 3, 2, 2),                # empty output: 4 rows under 7
        lambda: C.stem_fwd(t(2, 12, 4, 3), w, 3, 3, 1, 1, 2, 2),                # 6 padded columns under 7
        # one row / column short of the filter: a division truncating toward zero counts (6 - 7) / 2 + 1 = 1
        lambda: C.stem_fwd(t(2, 6, 12, 3), w, 0, 0, 3, 3, 2, 2),
        lambda: C.stem_fwd(t(2, 12, 6, 3), w, 3, 3, 0, 0, 2, 2),
        lambda: C.stem_fwd(x, w, 3, 3, 3, 3, 0, 2),                             # row stride 0
        lambda: C.stem_wgrad(xp, t(2, 7, 6, 64), 7, 7, 3, 2),                   # dy: OH does not fit xp
        lambda: C.stem_wgrad(xp, t(2, 6, 7, 64), 7, 7, 3, 2),                   # OW does not fit
        lambda: C.stem_wgrad(xp, dy, 7, 7, 3, 3),                               # nor these rows at SH = 3
        lambda: C.stem_wgrad(xp, t(3, 6, 6, 64), 7, 7, 3, 2),                   # batch mismatch
        lambda: C.stem_wgrad(xp, t(2, 0, 6, 64), 7, 7, 3, 2),                   # empty dy
        lambda: C.stem_wgrad(xp, t(2, 6, 6, 32), 7, 7, 3, 2),                   # K = 32
        lambda: C.stem_wgrad(xp, dy, 7, 7, 5, 2),                               # C = 5
        lambda: C.stem_wgrad(xp, dy, 7, 7, 3, 2, t(7, 7, 3, 64), False),        # out: bf16
        lambda: C.stem_wgrad(xp, dy, 7, 7, 3, 2, t(7, 7, 3, 64, dtype=torch.float64), True),
        lambda: C.stem_wgrad(xp, dy, 7, 7, 3, 2, t(7, 7, 3, 32, dtype=torch.float32), False),  # out: size
        lambda: C.stem_wgrad(xp, dy, 7, 7, 3, 2, t(7, 7, 4, 64, dtype=torch.float32), True),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
            pytest.fail(f"refusal {i} did not raise")
    torch.cuda.synchronize()
    # nothing was launched on the operands: the same results as before
    y2, xp2 = C.stem_fwd(x, w, 3, 3, 3, 3, 2, 2)
    assert torch.equal(y, y2) and torch.equal(xp, xp2)


# ------------------------------------------------------------------------------------- autograd wrapper
# asymmetric pads; SH = 1 against the column stride 2 with a last image column no output reaches (with SH = 1
# every row is reached), and SH = 2 with a last image row and a last image column no output reaches
@pytest.mark.parametrize("geo", [(2, 9, 12, 3, 64, 5, 4, 1, (1, 2, 3, 0)), (2, 10, 12, 3, 64, 5, 4, 2, (2, 0, 3, 0))],
                         ids=["s1", "s2"])
def test_autograd_wrapper_exact(C, geo):
    """ops/conv.py _Stem on integers: y bitwise; dx (through conv_f32.dgrad, then rounded to bf16) equals
    bf16_rne of the f64 input gradient and is exactly zero on the row / column no output reaches; the kernel's
    gradient is bf16_rne of the reference; with grad_out a view of an f32 slab receives base + dw exactly, its
    neighbours stay, and no kernel gradient is returned."""
    from tensorflow_distributed_learning_amd.ops import conv as CV

    g = Geo(geo)
    HP, WPv = g.H + g.pads[0] + g.pads[1], g.W + g.pads[2] + g.pads[3]
    assert (WPv - g.KW) % 2 == 1 and g.pads[3] == 0 and ((HP - g.KH) % g.SH == 1 and g.pads[1] == 0 or g.SH == 1)
    a = CR.amp_for(g.KH * g.KW * g.C, 300)
    x, w = CR.coded_ints((g.N, g.H, g.W, g.C), a, 1), CR.coded_ints((g.KH, g.KW, g.C, g.K), a, 2)
    ad = CR.amp_for(g.M, 350)
    dy = CR.coded_ints((g.N, g.OH, g.OW, g.K), min(a, ad), 3)
    xpad, _ = g.padded(_exact_bits(x))
    y_ref, ab = CR.conv_fwd_ref(xpad, w.transpose(3, 0, 1, 2), g.OH, g.OW, g.SH, 2, 0, 0)
    CR.assert_exact(ab)
    dw_ref, ab = CR.conv_wgrad_ref(xpad, dy, g.KH, g.KW, g.SH, 2, 0, 0)
    base = CR.coded_ints(dw_ref.shape, 1000, 7)
    CR.assert_exact(ab + np.abs(base))
    dx_ref, ab = CR.conv_dgrad_ref(dy, w, g.H, g.W, g.SH, 2, g.pads[0], g.pads[2])
    CR.assert_exact(ab)
    # the last padded column (and row, SH = 2) is a pixel of x that no window holds
    unreached = np.zeros(dx_ref.shape, bool)
    unreached[:, :, g.W - 1] = True
    if g.SH == 2:
        unreached[:, g.H - 1] = True
    assert np.all(dx_ref[unreached] == 0) and np.any(dx_ref[:, g.H - 2, g.W - 2] != 0)

    xt = _dev(_exact_bits(x)).requires_grad_(True)
    kt = _dev(_exact_bits(w)).requires_grad_(True)
    yt = CV.stem_conv2d_nhwc(xt, kt, g.pads, (g.SH, 2))
    _same(_bits(yt.detach()), CR.round_bf16(y_ref), f"{g!r} autograd y")
    yt.backward(_dev(_exact_bits(dy)))
    assert xt.grad.dtype == torch.bfloat16 and kt.grad.dtype == torch.bfloat16
    _same(_bits(xt.grad), CR.round_bf16(dx_ref), f"{g!r} autograd dx")
    assert not (_bits(xt.grad)[unreached] & 0x7FFF).any()
    _same(_bits(kt.grad), CR.round_bf16(dw_ref), f"{g!r} autograd dw")

    n = dw_ref.size
    slab = torch.full((n + 64,), 5.0, device="cuda")
    slab[32:32 + n] = _dev32(base).reshape(-1)
    view = slab[32:32 + n].view(dw_ref.shape)
    xt2 = _dev(_exact_bits(x)).requires_grad_(True)
    kt2 = _dev(_exact_bits(w)).requires_grad_(True)
    CV.stem_conv2d_nhwc(xt2, kt2, g.pads, (g.SH, 2), grad_out=view).backward(_dev(_exact_bits(dy)))
    assert kt2.grad is None
    got = _f64(slab)
    _same(got[32:32 + n].reshape(dw_ref.shape), base + dw_ref, f"{g!r} autograd slab view")
    assert np.all(got[:32] == 5.0) and np.all(got[32 + n:] == 5.0)
    _same(_bits(xt2.grad), CR.round_bf16(dx_ref), f"{g!r} autograd dx with grad_out")


# ------------------------------------------------------------------------------------- coverage gate
def test_every_path_ran(C):
    print("\nstem kernels: cases, exact-case ties rounded down / up, largest error / bound")
    for k in PATHS:
        r, n = RATIO.get(k), RAN.get(k, [0, 0, 0])
        print(f"  {k}: {n[0]} cases, ties {n[1]} / {n[2]}, ratio {'-' if r is None else f'{r:.4f}'}")
    assert all(RAN.get(k, [0])[0] > 0 for k in PATHS), RAN
    assert set(RATIO) == set(PATHS) - {"pack f32", "pack bf16"}, RATIO
    for k in ("forward", "wgrad bf16"):
        assert min(RAN[k][1:]) >= 200, (k, RAN[k])
    assert all(v <= 1.0 for v in RATIO.values()), RATIO
