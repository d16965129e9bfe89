"""The bf16 weight-gradient kernels (csrc/kernels/conv_wgrad.hip: k_conv_wgrad, k_conv_wgrad_glds,
k_wgrad_reduce; wgrad3x3.hip: the 3x3 / C = 64 row kernel) against the f64 reference of
tests/conv_refs.py.  The plan (tile, slice count, kind) is always given, so each case knows its kernel.

Exact cases: position-coded small integers, every product sum below 2^24 (asserted by the reference), so
every split-K order and every reduce order is exact: the f32 `out` must equal the f64 value, the bf16 dw
bf16_rne of it bit for bit, and accumulate=True the integer base plus it.  Random-data cases use the derived
bound of conv_refs.error_bound with R = pixels + slices.
"""
import numpy as np
import pytest
import torch

import conv_refs as CR
import kernel_refs as R

pytestmark = pytest.mark.gpu

RAN = {}    # "wmw x wnw kind k [single]" or "row kernel" -> [exact cases, ties down, ties up]
RATIO = {}  # the same keys -> largest error / bound on random data
SUBNORMAL = {}


@pytest.fixture(scope="module")
def C():
    from tensorflow_distributed_learning_amd.ops import hip

    c = hip()
    c.conv_wgrad_force_single(False)
    c.conv_wgrad3x3_set_rows(0)
    yield c
    c.conv_wgrad_force_single(False)
    c.conv_wgrad3x3_set_rows(0)


def _dev(bits):
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).view(torch.bfloat16).cuda()


def _bits(t):
    return t.contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def _to_bits(v):
    b = R.bf16_rne(np.asarray(v, np.float32))
    assert np.array_equal(R.bf16_bits_to_f64(b), np.asarray(v, np.float64)), "test data is not exact in bf16"
    return b


def _same(got, want, what, nan_ok=True):
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


def _affine(n):
    """Per-channel (scale, shift) keeping fmaf(x, scale, shift) exact on small integers, zero at x = t."""
    c = np.arange(n)
    scale = np.array([1.0, 2.0, 4.0, -1.0], np.float32)[c % 4]  # (integers: the products stay integers)
    t = np.array([-3, -2, -1, 1, 2, 3], np.float32)[c % 6]
    return scale, (-scale * t + np.array([0, 0, 1, -2], np.float32)[(c // 4) % 4]).astype(np.float32)


class WProb:
    def __init__(self, N, H, W, Cin, K, KH=1, KW=1, sh=1, sw=1, pt=0, pl=0, OH=None, OW=None, in_bn=False, random=False,
                 salt=0):
        self.N, self.H, self.W, self.C, self.K, self.KH, self.KW = N, H, W, Cin, K, KH, KW
        self.sh, self.sw, self.pt, self.pl = sh, sw, pt, pl
        self.OH = OH if OH is not None else (H + 2 * pt - KH) // sh + 1
        self.OW = OW if OW is not None else (W + 2 * pl - KW) // sw + 1
        self.M = N * self.OH * self.OW
        self.in_bn, self.random = in_bn, random
        if random:
            rng = np.random.RandomState(50 + salt)
            x = R.bf16_bits_to_f64(R.bf16_rne(rng.randn(N, H, W, Cin).astype(np.float32)))
            dy = R.bf16_bits_to_f64(R.bf16_rne((rng.randn(N, self.OH, self.OW, K) * self.M ** -0.5).astype(np.float32)))
        else:
            a = CR.amp_for(self.M, 350)
            x, dy = CR.coded_ints((N, H, W, Cin), a, 1 + 10 * salt), CR.coded_ints((N, self.OH, self.OW, K), a, 2 + 10 * salt)
        self.set(x, dy)

    def set(self, x, dy):
        self.x_bits, self.dy_bits = R.bf16_rne(x.astype(np.float32)), R.bf16_rne(dy.astype(np.float32))
        xin = R.bf16_bits_to_f64(self.x_bits)
        self.ss = None
        if self.in_bn:
            self.ss = _affine(self.C)
            xin = R.bf16_bits_to_f64(CR.in_bn_ref(self.x_bits, *self.ss))
        self.dw, self.ab = CR.conv_wgrad_ref(xin, R.bf16_bits_to_f64(self.dy_bits), self.KH, self.KW, self.sh, self.sw,
                                             self.pt, self.pl)
        if not self.random:
            assert np.all(xin == np.round(xin)) and np.all(dy == np.round(dy)), "exact cases take integers"
            CR.assert_exact(self.ab)
        self.base = CR.coded_ints(self.dw.shape, 1000, 7)
        if not self.random:
            CR.assert_exact(self.ab + np.abs(self.base))
        self._dev = None

    def __repr__(self):
        return (f"wgrad N{self.N} {self.H}x{self.W}x{self.C} -> {self.OH}x{self.OW}x{self.K} f{self.KH}x{self.KW} "
                f"s{self.sh}{self.sw} p{self.pt}{self.pl} M{self.M}{'+in_bn' if self.in_bn else ''}")

    def shapes(self):
        return [self.N, self.H, self.W, self.C], [self.N, self.OH, self.OW, self.K]

    def call(self, c, plan, out=None, accumulate=False):
        if self._dev is None:
            self._dev = (_dev(self.x_bits), _dev(self.dy_bits))
        st = None
        if self.in_bn:
            n = self.C
            st = torch.from_numpy(np.stack([np.zeros(n, np.float32), np.ones(n, np.float32), *self.ss])).cuda()
        return c.conv_wgrad(self._dev[0], self._dev[1], self.KH, self.KW, self.sh, self.sw, self.pt, self.pl, out,
                            accumulate, list(plan), st)


def _key(plan, single=False):
    if not plan:
        return "model's choice"
    if plan[0] == 0:
        return "row kernel"
    kind = plan[3] if len(plan) > 3 else 0
    ring = plan[0] * plan[1] == 8
    return f"{plan[0]}x{plan[1]} kind {kind}" + (" single" if single and not ring and kind == 0 else "")


def check(c, p, plan, single=False, modes=("bf16", "f32", "acc")):
    """p under one plan: the bf16 dw bitwise, the f32 out exactly, accumulate onto an integer base exactly."""
    what = f"{p!r} plan {list(plan)}{' single' if single else ''}"
    c.conv_wgrad_force_single(single)
    try:
        if "bf16" in modes:
            _same(_bits(p.call(c, plan)), CR.round_bf16(p.dw), what + " bf16")
        if "f32" in modes:
            out = torch.full(p.dw.shape, 123.0, device="cuda")
            _same(p.call(c, plan, out, False).cpu().numpy().astype(np.float64), p.dw, what + " f32")
        if "acc" in modes:
            out = torch.from_numpy(p.base.astype(np.float32)).cuda()
            _same(p.call(c, plan, out, True).cpu().numpy().astype(np.float64), p.base + p.dw, what + " accumulate")
    finally:
        c.conv_wgrad_force_single(False)
    dn, up, _, _ = CR.count_ties(p.dw)
    r = RAN.setdefault(_key(plan, single), [0, 0, 0])
    r[0] += 1
    r[1] += dn
    r[2] += up


TILES = [(1, 1, 0), (1, 2, 0), (2, 1, 0), (2, 2, 0), (2, 2, 1), (1, 4, 0), (4, 1, 0), (2, 4, 0), (4, 2, 0)]
_cache = {}


def prob(*a, **k):
    key = (a, tuple(sorted(k.items())))
    if key not in _cache:
        _cache[key] = WProb(*a, **k)
    return _cache[key]


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"{t[0]}x{t[1]}k{t[2]}")
def test_every_tile_and_kind_with_partial_column_tiles(C, tile, single):
    """TC = KH*KW*C with a partial last column tile: C = 192 at 1x1 (direct) against 128- and 256-column
    tiles, and 3x3 with C = 64 (TC = 576 = 4.5 x 128 = 2.25 x 256)."""
    wmw, wnw, kind = tile
    for p, ns in ((prob(2, 9, 9, 192, 256), 2), (prob(2, 5, 13, 64, 256, 3, 3, pt=1, pl=1), 3)):
        check(C, p, [wmw, wnw, ns, kind], single)


@pytest.mark.parametrize("M", [1, 63, 64, 65, 129])
def test_pixel_counts_around_the_64_pixel_stage(C, M):
    for p in (prob(1, 1, M, 64, 128), prob(1, 1, M, 64, 128, 1, 3, pl=1)):
        for plan in ([1, 1, 1], [1, 1, 2], [2, 2, 1], [2, 2, 2, 1], [1, 2, 3], [2, 4, 1], [2, 4, 2]):
            check(C, p, plan, modes=("bf16", "f32"))


@pytest.mark.parametrize("ns", [1, 2, 3, 4, 9])
def test_slice_counts_up_to_and_over_the_stages(C, ns):
    """M = 200 is four 64-pixel stages: 1, 2, 3 slices, one per stage, and more requested than stages (clamped)."""
    p = prob(2, 10, 10, 64, 128, 3, 3, pt=1, pl=1)
    for tile in ((1, 1, 0), (2, 2, 0), (2, 2, 1), (2, 4, 0), (1, 4, 0)):
        check(C, p, [tile[0], tile[1], ns, tile[2]], modes=("bf16", "f32"))
    plans = C.conv_wgrad_plans(*p.shapes(), 3, 3, 1, 1, 1, 1, 64)
    assert max(pl[3] for pl in plans if pl[0]) <= 4  # never more slices than stages


@pytest.mark.parametrize("S", [15, 16, 17, 65])
def test_reduce_kernel_wave_groups_and_unroll_tail(C, S):
    """k_wgrad_reduce sums S slices with min(16, S) waves, four chains each: S = 15, 16, 17 and 65 cover fewer
    waves than 16, exactly 16, a second round for one wave, and the x4 unrolled loop with a tail."""
    p = prob(1, 1, 64 * S - 7, 64, 64, salt=S)
    for tile in ((1, 1, 0), (1, 2, 0)):
        check(C, p, [tile[0], tile[1], S, tile[2]])
    assert -(-p.M // 64) == S


# (N, H, W, KH, KW, sh, sw, pt, pl, OH, OW)
WGEOMS = {
    "direct_1x1": (2, 9, 9, 1, 1, 1, 1, 0, 0, 9, 9),
    "1x1_output_smaller_not_direct": (2, 9, 9, 1, 1, 1, 1, 0, 0, 8, 7),
    "1x1_stride2_odd": (2, 9, 7, 1, 1, 2, 2, 0, 0, 5, 4),
    "3x3_stride2_odd": (2, 9, 7, 3, 3, 2, 2, 1, 1, 5, 4),
    "3x3_stride2_same_even_pt0": (2, 8, 8, 3, 3, 2, 2, 0, 0, 4, 4),
    "3x3_stride2_unused_last": (2, 8, 8, 3, 3, 2, 2, 0, 0, 3, 3),
    "asymmetric_pt0_pl2": (2, 7, 7, 3, 3, 1, 1, 0, 2, 6, 7),
    "pt_kh_minus_1": (2, 6, 6, 3, 3, 1, 1, 2, 2, 6, 6),
    "h_below_kh": (3, 2, 2, 5, 5, 1, 1, 2, 2, 2, 2),
    "f4x8_32taps": (2, 6, 9, 4, 8, 1, 1, 1, 3, 6, 9),
    "f8x4_32taps": (2, 9, 6, 8, 4, 1, 1, 3, 1, 9, 6),
    "f1x7": (2, 5, 9, 1, 7, 1, 1, 0, 3, 5, 9),
}


@pytest.mark.parametrize("geom", list(WGEOMS))
def test_geometries(C, geom):
    N, H, W, KH, KW, sh, sw, pt, pl, OH, OW = WGEOMS[geom]
    for Cin, K in ((64, 128), (192, 64)):
        p = prob(N, H, W, Cin, K, KH, KW, sh, sw, pt, pl, OH, OW)
        for plan in ([1, 1, 2], [1, 2, 1], [2, 2, 2], [2, 2, 2, 1], [2, 4, 2], [1, 4, 1]):
            if K % (64 * plan[0]) == 0:
                check(C, p, plan, modes=("bf16", "acc"))


@pytest.mark.parametrize("shape", [(1, 10, 13, 64, 128), (2, 9, 9, 192, 256), (1, 1, 65, 512, 64)])
def test_input_side_bn_on_every_plan(C, shape):
    """in_bn: x is the BN input, the staging stores relu(x * scale + shift); against the reference of the
    weight gradient over relu(bn(x)), for every plan conv_wgrad_plans(in_bn=True) returns."""
    p = prob(*shape, in_bn=True)
    plans = C.conv_wgrad_plans(*p.shapes(), 1, 1, 1, 1, 0, 0, 64, True)
    assert plans and all(pl[0] * pl[1] <= 4 and pl[4] == 0 for pl in plans)
    tiles = set()
    for pl in plans:
        if (pl[0], pl[1], pl[3]) in tiles:
            continue
        tiles.add((pl[0], pl[1], pl[3]))
        check(C, p, [pl[0], pl[1], pl[3], 0], modes=("bf16", "f32"))
    assert len({t[:2] for t in tiles}) >= 2
    check(C, p, [], modes=("bf16",))  # the model's first choice
    RAN["in_bn"] = [RAN.get("in_bn", [0])[0] + len(tiles), 0, 0]


@pytest.mark.parametrize("W", [1, 2, 31, 32, 33, 63, 64])
@pytest.mark.parametrize("H", [1, 2, 5])
def test_row_kernel_widths_heights_and_slices(C, W, H):
    """Plan [0, 0, 0]: the 3x3 / C = 64 row kernel.  Rows per slice 1, a value that does not divide N * H,
    one larger than H (a slice crosses images) and the heuristic."""
    N = 3
    for K in (64, 192):
        p = prob(N, H, W, 64, K, 3, 3, pt=1, pl=1, salt=W)
        try:
            for rows in (0, 1, 2 if (N * H) % 2 else 4, H + 1, N * H + 5):
                C.conv_wgrad3x3_set_rows(rows)
                check(C, p, [0, 0, 0], modes=("bf16", "acc") if rows in (0, H + 1) else ("f32",))
        finally:
            C.conv_wgrad3x3_set_rows(0)
    assert C.conv_wgrad_plans(*p.shapes(), 3, 3, 1, 1, 1, 1, 4)[0][:2] == [0, 0]


def _nan_case(p, h, w):
    x = R.bf16_bits_to_f64(p.x_bits).copy()
    x[1, h, w, 5] = np.nan
    q = WProb(p.N, p.H, p.W, p.C, p.K, p.KH, p.KW, p.sh, p.sw, p.pt, p.pl, p.OH, p.OW, random=True)
    q.set(x, R.bf16_bits_to_f64(p.dy_bits))
    return q


@pytest.mark.parametrize("pix", [(0, 0), (4, 6), (2, 3)], ids=lambda p: f"h{p[0]}w{p[1]}")
def test_one_nan_pixel_reaches_exactly_the_entries_that_read_it(C, pix):
    """x[1, h, w, 5] = NaN: dw[kh, kw, 5, :] is NaN for the taps under which some output pixel reads (h, w),
    and nothing else is."""
    p = prob(2, 5, 7, 64, 64, 3, 3, pt=1, pl=1)
    q = _nan_case(p, *pix)
    nan = np.isnan(q.dw)
    assert nan[:, :, 5, :].any() and not np.delete(nan, 5, axis=2).any()
    want_taps = np.array([[0 <= pix[0] - kh + 1 < 5 and 0 <= pix[1] - kw + 1 < 7 for kw in range(3)] for kh in range(3)])
    assert np.array_equal(nan[:, :, 5, 0], want_taps) and np.array_equal(nan[:, :, 5, :].all(-1), want_taps)
    for plan in ([1, 1, 2], [1, 2, 1], [1, 4, 2], [0, 0, 0]):
        got = q.call(C, plan, torch.zeros(q.dw.shape, device="cuda"), False).cpu().numpy().astype(np.float64)
        want = q.dw
        if plan[0] == 0 and pix[1] == q.W - 1 and q.W % 32 != 0:
            # the row kernel (wgrad3x3.hip, documented there): its 32-pixel MFMA steps run past the row's end
            # with dy = 0, and under tap kw = 0 the first padded pixel reads x's last column: 0 * NaN
            want = q.dw.copy()
            want[want_taps[:, 1], 0, 5, :] = np.nan
        _same(got, want, f"{q!r} NaN at {pix} plan {plan}")


def test_subnormal_products_and_sums(C):
    """bf16 subnormal inputs with normal products, subnormal products, and normal products cancelling into a
    subnormal sum, in the f32 `out`: the f64 reference as IEEE arithmetic has it."""
    x = np.zeros((1, 1, 4, 64))
    dy = np.zeros((1, 1, 4, 64))
    x[0, 0, 0, 1], dy[0, 0, 0, :] = 2.0 ** -130, 2.0 ** 10       # subnormal input, product 2^-120
    x[0, 0, 1, 2], dy[0, 0, 1, :] = 2.0 ** -100, 2.0 ** -30      # product 2^-130: an f32 subnormal
    x[0, 0, 2, 3], x[0, 0, 3, 3] = 1.5 * 2.0 ** -100, -1.25 * 2.0 ** -100
    dy[0, 0, 2, :], dy[0, 0, 3, :] = 2.0 ** -25, 2.0 ** -25      # 2^-125 (1.5 - 1.25) = 2^-127
    p = WProb(1, 1, 4, 64, 64, random=True)
    p.set(x, dy)
    assert p.dw[0, 0, 1, 0] == 2.0 ** -120 and p.dw[0, 0, 2, 0] == 2.0 ** -130 and p.dw[0, 0, 3, 0] == 2.0 ** -127
    for plan in ([1, 1, 1], [1, 2, 1], [1, 4, 1]):
        got = p.call(C, plan, torch.zeros(p.dw.shape, device="cuda"), False).cpu().numpy().astype(np.float64)
        flushed = {c: got[0, 0, c, 0] == 0 for c in (1, 2, 3)}
        print(f"subnormal wgrad plan {plan}: flushed {flushed}")
        SUBNORMAL[str(plan)] = "flush" if any(flushed.values()) else "ieee"
        _same(got, p.dw, f"subnormal plan {plan}")


@pytest.mark.parametrize("case", ["3x3_c64", "1x1_c192", "1x1_s2"])
def test_random_data_within_the_derived_bound(C, case):
    """|dw - r| <= e for the f32 out and <= 1/2 ulp_bf16(|r| + e) + e for the bf16 dw, e = R 2^-23 sum |x||dy|
    with R = pixels + slices (conv_refs.error_bound): derived, not tuned."""
    p = {"3x3_c64": lambda: WProb(4, 14, 14, 64, 128, 3, 3, pt=1, pl=1, random=True),
         "1x1_c192": lambda: WProb(4, 14, 14, 192, 256, random=True),
         "1x1_s2": lambda: WProb(4, 15, 15, 64, 128, 1, 1, 2, 2, 0, 0, 8, 8, random=True)}[case]()
    plans = [[1, 1, 4], [1, 2, 3], [2, 1, 2], [2, 2, 4], [2, 2, 4, 1], [1, 4, 2], [2, 4, 3]]
    if p.K % 256 == 0:
        plans += [[4, 1, 2], [4, 2, 2]]
    if case == "3x3_c64":
        plans.append([0, 0, 0])
    for plan in plans:
        red = p.M + (p.N * p.H if plan[0] == 0 else plan[2])  # (the row kernel: at most one slice per image row)
        f = p.call(C, plan, torch.zeros(p.dw.shape, device="cuda"), False).cpu().numpy().astype(np.float64)
        b = R.bf16_bits_to_f64(_bits(p.call(C, plan)))
        e = CR.error_bound_f32(p.ab, red)
        r32 = float(np.max(np.abs(f - p.dw) / np.maximum(e + 0.5 * R.ulp32(p.dw), 1e-300)))
        r16 = float(np.max(np.abs(b - p.dw) / CR.error_bound(p.dw, p.ab, red)))
        print(f"bound wgrad {case} plan {plan}: f32 error / bound = {r32:.4f}, bf16 = {r16:.4f}")
        k = _key(plan)
        RATIO[k] = max(RATIO.get(k, 0.0), r32, r16)
        assert r32 <= 1.0 and r16 <= 1.0, (case, plan, r32, r16)


def test_refusals(C):
    def t(*s):
        return torch.ones(*s, device="cuda").bfloat16()

    x, dy = t(2, 8, 8, 64), t(2, 8, 8, 64)
    assert C.conv_wgrad(x, dy, 3, 3, 1, 1, 1, 1).shape == (3, 3, 64, 64)
    st = torch.ones(4, 64, device="cuda")
    bad = [
        lambda: C.conv_wgrad(x, t(2, 10, 8, 64), 3, 3, 1, 1, 1, 1),        # dy larger than the geometry allows
        lambda: C.conv_wgrad(x, t(2, 8, 11, 64), 3, 3, 1, 1, 1, 1),
        lambda: C.conv_wgrad(x, t(3, 8, 8, 64), 3, 3, 1, 1, 1, 1),         # batch mismatch
        lambda: C.conv_wgrad(x, dy.reshape(16, 8, 64), 3, 3, 1, 1, 1, 1),  # dy not 4-D
        lambda: C.conv_wgrad(x, dy, 3, 3, 1, 1, 3, 1),                     # PT >= KH
        lambda: C.conv_wgrad(x, dy, 3, 11, 1, 1, 1, 5),                    # 33 taps
        lambda: C.conv_wgrad(t(2, 8, 8, 96), dy, 1, 1, 1, 1, 0, 0),        # C not a multiple of 64
        lambda: C.conv_wgrad(x, t(2, 8, 8, 128)[..., ::2], 3, 3, 1, 1, 1, 1),   # non-contiguous
        lambda: C.conv_wgrad(x, dy, 3, 3, 1, 1, 1, 1, None, False, [3, 1, 1]),  # bad tile
        lambda: C.conv_wgrad(x, dy, 3, 3, 1, 1, 1, 1, None, False, [2, 1, 1]),  # K = 64 has no 128-row tile
        lambda: C.conv_wgrad(x, dy, 3, 3, 1, 1, 1, 1, None, False, [1, 2, 1, 1]),  # kind 1 is the 2x2 tile's
        lambda: C.conv_wgrad(x, dy, 3, 3, 1, 1, 1, 1, torch.zeros(3, 3, 64, 32, device="cuda"), False),  # out size
        lambda: C.conv_wgrad(x, dy, 3, 3, 1, 1, 1, 1, None, False, [], st),      # in_bn: not 1x1
        lambda: C.conv_wgrad(x, t(2, 4, 4, 64), 1, 1, 2, 2, 0, 0, None, False, [], st),  # in_bn: stride 2
        lambda: C.conv_wgrad(x, t(2, 7, 8, 64), 1, 1, 1, 1, 0, 0, None, False, [], st),  # in_bn: H != OH (not direct)
        lambda: C.conv_wgrad(x, dy, 1, 1, 1, 1, 0, 0, None, False, [2, 4, 1], st),       # in_bn on a ring tile
        lambda: C.conv_wgrad(t(1, 4, 4, 576), t(1, 4, 4, 64), 1, 1, 1, 1, 0, 0, None, False, [], torch.ones(4, 576, device="cuda")),
        lambda: C.conv_wgrad(t(2, 8, 8, 128), dy, 3, 3, 1, 1, 1, 1, None, False, [0, 0, 0]),  # row kernel: C = 128
        lambda: C.conv_wgrad(x, t(2, 6, 6, 64), 3, 3, 1, 1, 0, 0, None, False, [0, 0, 0]),    # row kernel: unpadded
    ]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
            pytest.fail(f"refusal {i} did not raise")
    torch.cuda.synchronize()


def test_every_tile_and_kind_ran(C):
    print("\nwgrad kernel: exact cases, ties rounded down / up, largest error / bound on random data")
    for k in sorted(RAN):
        r = RATIO.get(k)
        print(f"  {k}: {RAN[k][0]} cases, ties {RAN[k][1]} / {RAN[k][2]}, ratio {'-' if r is None else f'{r:.4f}'}")
    print("subnormals:", sorted(set(SUBNORMAL.values())) or "-")
    want = {_key([a, b, 1, k], s) for a, b, k in TILES for s in (False, True)} | {"row kernel", "in_bn"}
    assert want <= set(RAN), want - set(RAN)
    assert all(min(RAN[k][1:]) >= 200 for k in want - {"in_bn"}), RAN
