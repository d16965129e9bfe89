"""The bf16 implicit-GEMM convolution kernels (csrc/kernels/conv.hip: k_conv_igemm, k_conv_glds ring / dma1,
k_conv_halo, with every epilogue and the input-side BN loader) against the f64 references of
tests/conv_refs.py, at the geometries where an indexing slip shows: row-tile tails, one-pixel images,
images smaller than the filter, asymmetric padding, 32-tap filters, halo windows that span many images.

Exact cases: the inputs are position-coded small integers (conv_refs.coded_ints), so every product sum and
every partial sum is an integer below 2^24 -- the references assert it -- and any f32 accumulation order,
MFMA form or tile gives the same value.  The kernel's bf16 output must then equal bf16_rne of the f64
reference bit for bit, and its f32 partial sums the f64 sums exactly; the amplitudes are sized so that many
outputs are exact bf16 ties.  Random-data cases use the derived bound of conv_refs.error_bound.

Every case asks conv_selected which kernel the launch takes under the hooks it sets, runs only the
combinations the selection accepts, records the name, and the last test checks that every kernel
conv_selected can name has run.  Nothing here compares one kernel with another.
"""
import re

import numpy as np
import pytest
import torch

import conv_refs as CR
import kernel_refs as R

pytestmark = pytest.mark.gpu

RAN = {}      # kernel name -> exact cases run
TIES = {}     # kernel name -> [ties rounded down, ties rounded up]
RATIO = {}    # kernel name -> largest error / bound on random data
SUBNORMAL = {}  # what the subnormal cases observed


def _defaults(c):
    c.conv_force_impl(2)
    c.conv_force_tile(0)
    c.conv_force_depth(2)
    c.conv_force_mfma(32)
    c.conv_force_halo(2)


@pytest.fixture(scope="module")
def C():
    from tensorflow_distributed_learning_amd.ops import hip

    c = hip()
    _defaults(c)
    yield c
    _defaults(c)


# (id, hooks, pattern the selected kernel's name must match for the case to count as that loop's; None: any)
LOOPS = [
    ("default", {}, None),
    ("igemm_d0", dict(impl=1, depth=0), r"^igemm_"),
    ("igemm_d1", dict(impl=1, depth=1), r"^igemm_.*_d1_"),
    ("igemm_d2", dict(impl=1, depth=3), r"^igemm_.*_d2_"),
    ("igemm_d3", dict(impl=1, depth=4), r"^igemm_"),
    ("tile1", dict(tile=1), r"^igemm_128x64_"),
    ("tile2", dict(tile=2), r"^igemm_128x"),
    ("tile3", dict(tile=3), r"^igemm_256x128_"),
    ("tile3_d1", dict(tile=3, depth=1), r"^igemm_256x128_d1_"),
    ("tile3_d2", dict(tile=3, depth=3), r"^igemm_256x128_d2_"),
    ("tile3_d3", dict(tile=3, depth=4), r"^igemm_256x128_"),
    ("tile1_d1", dict(tile=1, depth=1), r"^igemm_128x64_d1_"),
    ("tile1_d2", dict(tile=1, depth=3), r"^igemm_128x64_d2_"),
    ("tile1_d3", dict(tile=1, depth=4), r"^igemm_128x64_"),
    ("ring", dict(impl=3), r"^glds_ring_"),
    ("legacy", dict(depth=3), None),
    ("dma1_mf16", dict(impl=4), r"^glds_dma1_.*_w4_mf16_"),
    ("dma1_w3", dict(impl=5), r"^glds_dma1_.*_w3_mf16_"),
    ("dma1_mf32", dict(impl=6), r"^glds_dma1_.*_w4_mf32_"),
    ("mfma16", dict(mfma=16), None),
    ("halo", dict(impl=7), r"^halo_256x"),
    ("halo1", dict(halo=1), r"^halo_256x"),
    ("halo3", dict(halo=3), r"^halo_256x64_"),
    ("halo0", dict(halo=0), r"^(?!halo)"),
]
LOOP_IDS = [l[0] for l in LOOPS]


def _hooks(c, impl=2, tile=0, depth=2, mfma=32, halo=2):
    c.conv_force_impl(impl)
    c.conv_force_tile(tile)
    c.conv_force_depth(depth)
    c.conv_force_mfma(mfma)
    c.conv_force_halo(halo)


def _dev(bits):
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).view(torch.bfloat16).cuda()


def _bits(t):
    return t.contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def _to_bits(v):
    """bf16 bits of values that must be exactly representable."""
    b = R.bf16_rne(np.asarray(v, np.float32))
    assert np.array_equal(R.bf16_bits_to_f64(b), np.asarray(v, np.float64)), "test data is not exact in bf16"
    return b


def _stats4(scale, shift):
    n = len(scale)
    return torch.from_numpy(np.stack([np.zeros(n, np.float32), np.ones(n, np.float32), np.asarray(scale, np.float32),
                                      np.asarray(shift, np.float32)])).cuda()


def _affine(n, ulps):
    """Per-channel (scale, shift) that keep fmaf(x, scale, shift) exact on small integers: scale a power of
    two or -1, shift = -scale * t so that x = t (t in +-1..3) lands exactly on 0; with ulps, two
    channels in three have the shift one f32 ulp above / below that, which puts x = t one ulp either side of
    0 (the mask path only: the sign is all that is read there)."""
    c = np.arange(n)
    scale = np.array([1.0, 2.0, 4.0, -1.0], np.float32)[c % 4]  # (integers: the products stay integers)
    t = np.array([-3, -2, -1, 1, 2, 3], np.float32)[c % 6]
    shift = (-scale * t).astype(np.float32)
    if ulps:
        up, dn = np.nextafter(shift, np.float32(np.inf)), np.nextafter(shift, np.float32(-np.inf))
        shift = np.where(c % 3 == 1, up, np.where(c % 3 == 2, dn, shift)).astype(np.float32)
    else:
        shift = (shift + np.array([0, 0, 1, -2], np.float32)[(c // 4) % 4]).astype(np.float32)
    return scale, shift


class Prob:
    """One convolution problem: direction, geometry, optional operands, its inputs and f64 accumulator."""

    def __init__(self, d, N, H, W, Cin, K, KH=1, KW=1, sh=1, sw=1, pt=0, pl=0, OH=None, OW=None, stats=False, res=False,
                 bn=None, x2=False, in_bn=False, target=350, salt=0, random=False):
        self.d, self.N, self.H, self.W, self.C, self.K = d, N, H, W, Cin, K
        self.KH, self.KW, self.sh, self.sw, self.pt, self.pl = KH, KW, sh, sw, pt, pl
        self.OH = OH if OH is not None else (H + 2 * pt - KH) // sh + 1
        self.OW = OW if OW is not None else (W + 2 * pl - KW) // sw + 1
        self.stats, self.res, self.bn, self.x2, self.in_bn = stats, res, bn, x2, in_bn
        if stats or bn:
            target = min(target, 150)  # sums of squares / products of a whole row tile stay below 2^24
        self.target, self.salt, self.random = target, salt, random
        self.built = False

    def __repr__(self):
        ops = "".join(s for s, on in (("+stats", self.stats), ("+res", self.res), ("+bn_" + str(self.bn), self.bn),
                                      ("+x2", self.x2), ("+in_bn", self.in_bn), ("+random", self.random)) if on)
        return (f"{self.d} N{self.N} {self.H}x{self.W}x{self.C} -> {self.OH}x{self.OW}x{self.K} f{self.KH}x{self.KW} "
                f"s{self.sh}{self.sw} p{self.pt}{self.pl}{ops}")

    @property
    def flags(self):
        return [f for f, on in (("stats", self.stats), ("residual", self.res), ("bn", self.bn is not None),
                                ("bn_ss", self.bn == "ss"), ("in_bn", self.in_bn)) if on]

    @property
    def w_shape(self):
        return [self.K, self.KH, self.KW, self.C] if self.d == "fwd" else [self.KH, self.KW, self.C, self.K]

    def selected(self, c):
        return c.conv_selected(self.d, [self.N, self.H, self.W, self.C], self.w_shape, self.OH, self.OW, self.sh,
                               self.sw, self.pt, self.pl, self.flags)

    def _data(self, shape, amp, salt):
        if self.random:
            rng = np.random.RandomState(1000 + 17 * salt + self.salt)
            return R.bf16_bits_to_f64(R.bf16_rne((rng.randn(*shape) * amp).astype(np.float32)))
        return CR.coded_ints(shape, amp, salt + 10 * self.salt)

    def build(self):
        if self.built:
            return self
        p = self
        red = p.KH * p.KW * (p.C if p.d == "fwd" else p.K)
        self.reduction = red
        a = CR.amp_for(red, p.target)
        ax, aw = (1.0, red ** -0.5) if p.random else (a, a)
        if p.d == "fwd":
            x = self._data((p.N, p.H, p.W, p.C), ax, 1)
            w = self._data((p.K, p.KH, p.KW, p.C), aw, 2)
            self.x_bits, self.w_bits = R.bf16_rne(x.astype(np.float32)), R.bf16_rne(w.astype(np.float32))
            xin = x
            if p.in_bn:
                self.ss = _affine(p.C, ulps=False)
                xin = R.bf16_bits_to_f64(CR.in_bn_ref(self.x_bits, *self.ss))
            self.acc, self.ab = CR.conv_fwd_ref(xin, w, p.OH, p.OW, p.sh, p.sw, p.pt, p.pl)
            self.out_shape = (p.N, p.OH, p.OW, p.K)
        else:
            dy = self._data((p.N, p.OH, p.OW, p.K), ax, 1)
            w = self._data((p.KH, p.KW, p.C, p.K), aw, 2)
            self.x_bits, self.w_bits = R.bf16_rne(dy.astype(np.float32)), R.bf16_rne(w.astype(np.float32))
            if p.d == "dgrad":
                self.acc, self.ab = CR.conv_dgrad_ref(dy, w, p.H, p.W, 1, 1, p.pt, p.pl)
            else:  # the gradient of the even pixels: dy . w^T
                self.acc, self.ab = CR.conv_dgrad_ref(dy, w, p.OH, p.OW, 1, 1, 0, 0)
            self.out_shape = (p.N, p.H, p.W, p.C)
        if not p.random:
            ops = (xin, w) if p.d == "fwd" else (dy, w)
            assert all(np.all(o == np.round(o)) for o in ops), "exact cases take integers"
            CR.assert_exact(self.ab)
        ch = self.out_shape[-1]
        self.res_bits = _to_bits(CR.coded_ints(self.out_shape, 5, 3 + 10 * p.salt)) if p.res else None
        self.by_bits = self.bx_bits = self.bx2_bits = self.bn_ss = None
        if p.bn:
            self.bx_bits = _to_bits(CR.coded_ints(self.out_shape, 3, 5 + 10 * p.salt))
            if p.bn == "y":
                self.by_bits = _to_bits(CR.coded_ints(self.out_shape, 2, 4 + 10 * p.salt))
            else:
                self.bn_ss = _affine(ch, ulps=True)
            if p.x2:
                self.bx2_bits = _to_bits(CR.coded_ints(self.out_shape, 3, 6 + 10 * p.salt))
        self.built, self._exp, self._dev = True, {}, None
        return self

    def dev(self):
        if self._dev is None:
            self._dev = {k: _dev(getattr(self, k)) for k in ("x_bits", "w_bits", "res_bits", "by_bits", "bx_bits", "bx2_bits")
                         if getattr(self, k) is not None}
        return self._dev

    def free(self):
        self._dev = None

    def run(self, c):
        """The kernel's outputs as numpy: (out bits, part or None, part2 or None)."""
        p, d = self, self.dev()
        if p.d == "fwd":
            st = _stats4(*self.ss) if p.in_bn else None
            if p.stats:
                y, part = c.conv_fwd_stats(d["x_bits"], d["w_bits"], p.OH, p.OW, p.sh, p.sw, p.pt, p.pl, st)
                return _bits(y), part.cpu().numpy().astype(np.float64), None
            return _bits(c.conv_fwd(d["x_bits"], d["w_bits"], p.OH, p.OW, p.sh, p.sw, p.pt, p.pl, st)), None, None
        st = _stats4(*self.bn_ss) if p.bn == "ss" else None
        if p.d == "dgrad":
            if p.bn:
                out = c.conv_dgrad_bn(d["x_bits"], d["w_bits"], p.H, p.W, p.pt, p.pl, d.get("res_bits"), d.get("by_bits"),
                                      d["bx_bits"], d.get("bx2_bits"), st)
            else:
                out = [c.conv_dgrad(d["x_bits"], d["w_bits"], p.H, p.W, p.pt, p.pl, d.get("res_bits"))]
        else:
            if p.bn:
                out = c.conv_dgrad_s2_bn(d["x_bits"], d["w_bits"], p.H, p.W, d.get("res_bits"), d.get("by_bits"),
                                         d["bx_bits"], d.get("bx2_bits"), st)
            else:
                out = [c.conv_dgrad_s2(d["x_bits"], d["w_bits"], p.H, p.W, d.get("res_bits"))]
        f = [o.cpu().numpy().astype(np.float64) for o in out[1:]]
        return _bits(out[0]), (f[0] if f else None), (f[1] if len(f) > 1 else None)

    def expect(self, bm):
        """(out bits, part, part2) of the f64 reference for a row tile of bm."""
        if bm in self._exp:
            return self._exp[bm]
        p, exact = self, not self.random
        if p.d == "fwd":
            v = CR.round_bf16(self.acc)
            e = (v, CR.tile_sums(v.reshape(-1, p.K), None, bm, exact) if p.stats else None, None)
        elif p.d == "dgrad":
            e = CR.dgrad_epilogue_ref(self.acc, bm, self.res_bits, self.by_bits, self.bx_bits, self.bn_ss, self.bx2_bits, exact)
        else:
            e = CR.dgrad_s2_epilogue_ref(self.acc, p.H, p.W, bm, self.res_bits, self.by_bits, self.bx_bits, self.bn_ss,
                                         self.bx2_bits, exact)
        self._exp[bm] = e
        return e

    @property
    def rows(self):  # rows of the implicit GEMM (what the row tiles divide)
        p = self
        return p.N * p.H * p.W if p.d == "dgrad" else p.N * p.OH * p.OW


def _same_bits(got, want, what):
    """Bitwise equality, except that any NaN equals any NaN (payload and sign of a NaN are not specified)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got != want) & ~(R.bf16_is_nan(got) & R.bf16_is_nan(want))
    if bad.any():
        i = np.argwhere(bad)
        show = [(tuple(j), hex(got[tuple(j)]), hex(want[tuple(j)])) for j in i[:6]]
        raise AssertionError(f"{what}: {len(i)} of {got.size} bf16 values differ (index, got, want): {show}")


def _same_f32(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got != want) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        i = np.argwhere(bad)
        show = [(tuple(j), got[tuple(j)], want[tuple(j)]) for j in i[:6]]
        raise AssertionError(f"{what}: {len(i)} of {got.size} f32 sums differ (index, got, want): {show}")


def check(c, prob, loop, ran):
    """Run prob under one LOOPS entry if the selection takes the loop the entry is named for; compare every
    output with the reference.  Returns the kernel name, or None when the selection refused the loop."""
    lid, hooks, pat = loop
    _hooks(c, **hooks)
    try:
        name, bm = prob.selected(c)
        if pat is not None and not re.search(pat, name):
            return None
        prob.build()
        got, part, part2 = prob.run(c)
        name2, bm2 = prob.selected(c)
        assert (name2, bm2) == (name, bm)
    finally:
        _defaults(c)
    what = f"{prob!r} [{lid}: {name}]"
    want, wpart, wpart2 = prob.expect(bm)
    _same_bits(got.reshape(want.shape), want, what)
    for g, w_, tag in ((part, wpart, "part"), (part2, wpart2, "part2")):
        assert (g is None) == (w_ is None), (what, tag)
        if g is not None:
            P = (prob.rows + bm - 1) // bm
            assert g.shape[0] == CR.part_rows(P), (what, tag, g.shape, P)  # P data rows + ceil(P/64) scratch rows
            _same_f32(g[:P], w_, f"{what} {tag}")  # every data row on its own, the tail tile included
    RAN[name] = RAN.get(name, 0) + 1
    dn, up, _, _ = CR.count_ties(prob.acc)
    t = TIES.setdefault(name, [0, 0])
    t[0] += dn
    t[1] += up
    ran.append((lid, name))
    return name


def run_loops(c, prob, must=(), loops=LOOPS):
    """prob through every loop the selection accepts for it; `must` names loops that have to accept it."""
    ran = []
    for loop in loops:
        check(c, prob, loop, ran)
    ids = {lid for lid, _ in ran}
    assert set(must) <= ids, f"{prob!r}: the selection refused {sorted(set(must) - ids)}"
    return ran


def assert_ties(prob, least=200):
    dn, up, neg, pos = CR.count_ties(prob.acc)
    assert min(dn, up, neg, pos) >= least, (repr(prob), dn, up, neg, pos)


def test_hooks_select_the_named_kernels(C):
    """conv_selected follows the hooks: each forced main loop is the one named, on a shape every loop takes."""
    p = Prob("fwd", 2, 9, 9, 64, 128, 3, 3, pt=1, pl=1)
    want = {"igemm_d0": "igemm_128x128_d0_ek0", "igemm_d1": "igemm_128x128_d1_ek0", "igemm_d2": "igemm_128x128_d2_ek0",
            "igemm_d3": "igemm_128x128_d3_ek0", "tile1": "igemm_128x64_d0_ek0", "tile2": "igemm_128x128_d0_ek0",
            "tile3": "igemm_256x128_d0_ek0", "dma1_mf16": "glds_dma1_128x128_w4_mf16_ek0",
            "dma1_w3": "glds_dma1_128x128_w3_mf16_ek0", "dma1_mf32": "glds_dma1_128x128_w4_mf32_ek0",
            "halo": "halo_256x128_ek0", "halo1": "halo_256x128_ek0", "halo3": "halo_256x64_ek0",
            "halo0": "glds_dma1_128x128_w4_mf32_ek0", "mfma16": "glds_dma1_128x128_w4_mf16_ek0",
            "default": "glds_dma1_128x128_w4_mf32_ek0", "ring": None}
    for lid, hooks, _ in LOOPS:
        if lid in want:
            _hooks(C, **hooks)
            try:
                name, bm = p.selected(C)
            finally:
                _defaults(C)
            if want[lid] is not None:
                assert name == want[lid], (lid, name)
                assert bm == int(re.search(r"_(\d+)x\d+_", name).group(1))
            else:
                assert not name.startswith("glds_ring")  # 2 x 1 workgroups: far below the ring kernel's 256
    assert len(set(C.conv_kernel_names())) == len(C.conv_kernel_names()) == 79


# ---------------------------------------------------------------------------------- geometries
# 1x1: M = N * OH * OW through the row-tile tails of the 128-row kernels (and, under tile 3, the 256-row one)
TAILS = {"m1": (1, 1, 1), "m127": (1, 1, 127), "m128": (2, 8, 8), "m129": (1, 3, 43), "m255": (1, 15, 17),
         "m256": (1, 16, 16), "m257": (1, 1, 257)}


@pytest.mark.parametrize("tail", list(TAILS))
@pytest.mark.parametrize("K", [64, 128, 192])
def test_row_tile_tails_1x1(C, tail, K):
    N, H, W = TAILS[tail]
    Cin = 192 if K == 64 else 64  # (one k-tile and three)
    run_loops(C, Prob("fwd", N, H, W, Cin, K, stats=True), must=("igemm_d0", "dma1_mf16", "dma1_mf32", "tile1"))
    p = Prob("dgrad", N, H, W, K, Cin, res=True)
    run_loops(C, p, must=("igemm_d0", "dma1_mf32") + (("tile3",) if K % 128 == 0 else ()))
    if N * H * W >= 127:
        assert_ties(p)


# 3x3 pad 1 (the halo kernel takes these): 255, 256, 258 rows around its 256-row tile; the 258-row case and the
# 7x7 / 5x6 images put several images into one tile's padded window
HALO_TAILS = {"m255": (1, 15, 17), "m256": (1, 16, 16), "m258": (2, 3, 43), "img7x7": (8, 7, 7), "img5x6": (10, 5, 6)}


@pytest.mark.parametrize("tail", list(HALO_TAILS))
@pytest.mark.parametrize("K", [64, 128])
def test_row_tile_tails_3x3_and_halo_windows(C, tail, K):
    N, H, W = HALO_TAILS[tail]
    must = ("igemm_d0", "dma1_mf32", "halo", "halo1", "halo3")
    run_loops(C, Prob("fwd", N, H, W, 64, K, 3, 3, pt=1, pl=1, stats=True), must=must)
    p = Prob("dgrad", N, H, W, K, 192, 3, 3, pt=1, pl=1, res=True)
    run_loops(C, p, must=must)
    assert_ties(p)


# (N, H, W, KH, KW, sh, sw, pt, pl, OH, OW)
GEOMS = {
    "ow1_w_below_kw": (2, 9, 1, 3, 3, 1, 1, 1, 1, 9, 1),
    "oh1_h_below_kh": (2, 1, 9, 3, 3, 1, 1, 1, 1, 1, 9),
    "h2_w2_5x5": (3, 2, 2, 5, 5, 1, 1, 2, 2, 2, 2),
    "s2_same_even_pt0_pb1": (2, 8, 8, 3, 3, 2, 2, 0, 0, 4, 4),
    "pt_kh_minus_1": (2, 6, 6, 3, 3, 1, 1, 2, 2, 6, 6),
    "pl_differs_from_pt": (2, 7, 7, 3, 3, 1, 1, 0, 2, 6, 7),
    "pt_differs_both": (2, 7, 6, 3, 3, 1, 1, 2, 0, 7, 5),
    "s2_unused_last_row_col": (2, 8, 8, 3, 3, 2, 2, 0, 0, 3, 3),
    "s2_1x1_odd": (2, 7, 9, 1, 1, 2, 2, 0, 0, 4, 5),
    "s12_rect": (2, 7, 9, 3, 3, 1, 2, 1, 1, 7, 5),
    "f1x7": (2, 5, 9, 1, 7, 1, 1, 0, 3, 5, 9),
    "f7x1": (2, 9, 5, 7, 1, 1, 1, 3, 0, 9, 5),
    "f5x5": (2, 6, 7, 5, 5, 1, 1, 2, 2, 6, 7),
    "f4x8_32taps": (2, 6, 9, 4, 8, 1, 1, 1, 3, 6, 9),
    "f8x4_32taps": (2, 9, 6, 8, 4, 1, 1, 3, 1, 9, 6),
    "f2x2_same": (2, 6, 6, 2, 2, 1, 1, 0, 0, 6, 6),
    "f2x2_valid": (2, 6, 7, 2, 2, 1, 1, 0, 0, 5, 6),
}


@pytest.mark.parametrize("geom", list(GEOMS))
def test_geometry_forward_and_input_gradient(C, geom):
    N, H, W, KH, KW, sh, sw, pt, pl, OH, OW = GEOMS[geom]
    taps = KH * KW
    halo = ("halo",) if sh == 1 and sw == 1 and taps > 1 else ()
    for Cin, K in ((64, 128), (192, 64)):
        p = Prob("fwd", N, H, W, Cin, K, KH, KW, sh, sw, pt, pl, OH, OW, stats=True)
        run_loops(C, p, must=("igemm_d0", "igemm_d2", "dma1_mf16", "dma1_mf32", "tile3" if K == 128 else "tile1") + halo)
        pb, pr = (OH - 1) * sh + KH - H - pt, (OW - 1) * sw + KW - W - pl
        if sh == 1 and sw == 1:
            assert 0 <= pb < KH and 0 <= pr < KW
            run_loops(C, Prob("dgrad", N, H, W, Cin, K, KH, KW, 1, 1, pt, pl, OH, OW, res=True),
                      must=("igemm_d0", "dma1_mf16", "dma1_mf32") + halo)


def _halo_window(N, OH, OW, KH, KW):
    """Longest padded window of a 256-row tile (conv.hip halo_window)."""
    Hp, Wp, M = OH + KH - 1, OW + KW - 1, N * OH * OW

    def pidx(m):
        return ((m // OW // OH) * Hp + (m // OW) % OH) * Wp + m % OW

    return max(pidx(min(m0 + 256, M) - 1) + (KH - 1) * Wp + KW - pidx(m0) for m0 in range(0, M, 256))


def test_halo_window_at_and_over_its_slots(C):
    """A window of exactly 512 slots runs the halo kernel; one of 513 must fall back (same results)."""
    fits = Prob("fwd", 257, 1, 1, 64, 64, 1, 2, pt=0, pl=1, OH=1, OW=1)  # 2 slots per 1x1 image: 255 * 2 + 2
    assert _halo_window(257, 1, 1, 1, 2) == 512
    assert ("halo", "halo_256x64_ek0") in run_loops(C, fits, must=("halo", "igemm_d0"))
    over = Prob("fwd", 3, 19, 4, 64, 64, 1, 6, pt=0, pl=2, OH=19, OW=4)  # 9 slots per row: (2 * 19 + 18) * 9 + 3 + 6
    assert _halo_window(3, 19, 4, 1, 6) == 513
    ran = run_loops(C, over, must=("igemm_d0", "dma1_mf32"))
    assert "halo" not in {lid for lid, _ in ran}
    _hooks(C, impl=7)
    try:
        assert not over.selected(C)[0].startswith("halo")
    finally:
        _defaults(C)


# ---------------------------------------------------------------------------------- epilogues
BN_COMBOS = [(bn, x2, res) for bn in ("y", "ss") for x2 in (False, True) for res in (False, True)]


@pytest.mark.parametrize("combo", BN_COMBOS, ids=lambda c: f"bn_{c[0]}{'_x2' if c[1] else ''}{'_res' if c[2] else ''}")
@pytest.mark.parametrize("cols", [64, 128])
def test_dgrad_bn_epilogues(C, combo, cols):
    """conv_dgrad_bn, every operand combination, on a 3x3 (all main loops) and a 1x1 with a row-tile tail."""
    bn, x2, res = combo
    halo = ("halo", "halo3")
    p = Prob("dgrad", 4, 9, 9, cols, 64, 3, 3, pt=1, pl=1, bn=bn, x2=x2, res=res)
    run_loops(C, p, must=("igemm_d0", "igemm_d1", "igemm_d2", "igemm_d3", "dma1_mf16", "dma1_w3", "dma1_mf32", "tile1",
                          "tile1_d1", "tile1_d2") + halo + (("tile3", "tile3_d1", "tile3_d2") if cols == 128 else ()))
    run_loops(C, Prob("dgrad", 1, 3, 43, cols, 192, bn=bn, x2=x2, res=res), must=("igemm_d0", "dma1_mf32"))


@pytest.mark.parametrize("combo", [(None, False, False), (None, False, True)] + BN_COMBOS,
                         ids=lambda c: f"bn_{c[0]}{'_x2' if c[1] else ''}{'_res' if c[2] else ''}")
@pytest.mark.parametrize("cols", [64, 128])
def test_dgrad_s2_scatter_epilogues(C, combo, cols):
    """conv_dgrad_s2 / conv_dgrad_s2_bn over all four pixels of every 2x2 block: even and odd H and W mixed,
    a row count below one tile and one with a tail."""
    bn, x2, res = combo
    must = ("igemm_d0", "igemm_d1", "igemm_d2", "dma1_mf16", "dma1_w3", "dma1_mf32", "tile1", "tile1_d1", "tile1_d2",
            "tile1_d3") + (("tile3", "tile3_d1", "tile3_d2", "tile3_d3") if cols == 128 else ())
    for i, (N, H, W) in enumerate(((3, 8, 8), (3, 7, 8), (5, 8, 11), (9, 7, 7))):  # M = 48, 48, 120, 144
        p = Prob("dgrad_s2", N, H, W, cols, 64 if i % 2 else 192, 1, 1, 2, 2, 0, 0, (H + 1) // 2, (W + 1) // 2, bn=bn, x2=x2,
                 res=res, salt=i)
        run_loops(C, p, must=must)


@pytest.mark.parametrize("Cin", [64, 512])
@pytest.mark.parametrize("K", [64, 128])
def test_input_side_bn(C, Cin, K):
    """in_bn on conv_fwd and conv_fwd_stats against the reference of conv(relu(bn(x))), M = 130 (a tail)."""
    for stats in (False, True):
        p = Prob("fwd", 1, 10, 13, Cin, K, stats=stats, in_bn=True, target=40 if stats else 350)
        ran = run_loops(C, p, must=("default", "legacy", "mfma16"))  # (the loops that accept any name)
        assert {n for _, n in ran} == {f"igemm_inbn_128x{K}_d0_ek0"}  # no hook moves it
        for lid, hooks, _ in LOOPS:
            _hooks(C, **hooks)
            try:
                assert p.selected(C) == (f"igemm_inbn_128x{K}_d0_ek0", 128), lid
            finally:
                _defaults(C)
        assert (R.bf16_bits_to_f64(CR.in_bn_ref(p.x_bits, *p.ss)) == 0).mean() > 0.2  # the ReLU clips, exact zeros


# ---------------------------------------------------------------------------------- the ring kernel
RING = {
    "fwd_1x1_stats_k512": Prob("fwd", 3, 73, 74, 64, 512, stats=True),
    "fwd_3x3_k512": Prob("fwd", 3, 73, 74, 64, 512, 3, 3, pt=1, pl=1),
    "dgrad_bn_y_res_c512": Prob("dgrad", 3, 73, 74, 512, 64, bn="y", res=True),
    "dgrad_bn_ss_c512": Prob("dgrad", 3, 73, 74, 512, 64, bn="ss"),
    "dgrad_s2_c512": Prob("dgrad_s2", 3, 145, 148, 512, 64, 1, 1, 2, 2, 0, 0, 73, 74),
    "fwd_1x1_stats_k192": Prob("fwd", 2, 105, 104, 64, 192, stats=True),
    "dgrad_bn_y_c192": Prob("dgrad", 2, 105, 104, 192, 64, bn="y"),
    "dgrad_bn_ss_res_c192": Prob("dgrad", 2, 105, 104, 192, 64, bn="ss", res=True),
    "dgrad_s2_bn_y_c192": Prob("dgrad_s2", 2, 209, 208, 192, 64, 1, 1, 2, 2, 0, 0, 105, 104, bn="y"),
}


@pytest.mark.parametrize("case", list(RING))
def test_ring_kernel_at_its_smallest_grid(C, case):
    """impl 3 takes the 3-stage ring kernel from 256 workgroups: 64 row tiles x 4 column tiles (M = 16206,
    just above 63 * 256), or 86 x 3 of the 64-column tile.  The last row tile is a tail."""
    p = RING[case]
    ran = run_loops(C, p, must=("ring",), loops=[l for l in LOOPS if l[0] == "ring"])
    assert ran[0][1].startswith("glds_ring_256x128" if p.out_shape[-1] == 512 else "glds_ring_256x64")
    p.free()


def test_ring_is_refused_one_row_tile_below(C):
    _hooks(C, impl=3)
    try:
        assert C.conv_selected("fwd", [3, 72, 74, 64], [512, 1, 1, 64], 72, 74)[0].startswith("igemm_")  # 63 row tiles
        assert C.conv_selected("fwd", [3, 73, 74, 64], [512, 1, 1, 64], 73, 74) == ("glds_ring_256x128_ek0", 256)
    finally:
        _defaults(C)


# ---------------------------------------------------------------------------------- random data, derived bound
BOUND_LOOPS = [l for l in LOOPS if l[0] in ("igemm_d0", "igemm_d2", "tile1", "tile3", "dma1_mf16", "dma1_w3",
                                            "dma1_mf32", "halo", "halo3")]
BOUNDED = {
    "fwd_3x3_c192": Prob("fwd", 2, 14, 14, 192, 128, 3, 3, pt=1, pl=1, random=True),
    "fwd_3x3_c512": Prob("fwd", 1, 7, 7, 512, 64, 3, 3, pt=1, pl=1, random=True),
    "fwd_1x1_c512": Prob("fwd", 1, 10, 13, 512, 128, random=True),
    "dgrad_3x3_k192": Prob("dgrad", 2, 14, 14, 128, 192, 3, 3, pt=1, pl=1, random=True),
    "dgrad_s2_k192": Prob("dgrad_s2", 3, 9, 10, 128, 192, 1, 1, 2, 2, 0, 0, 5, 5, random=True),
    "ring_fwd_3x3": Prob("fwd", 3, 73, 74, 64, 512, 3, 3, pt=1, pl=1, random=True),
}


@pytest.mark.parametrize("case", list(BOUNDED))
def test_random_data_within_the_derived_bound(C, case):
    """|y - r| <= 1/2 ulp_bf16(|r| + e) + e, e = R 2^-23 sum |a||b| (conv_refs.error_bound): derived from the
    f32 accumulation of an R-term dot product in any order and one rounding to bf16, not tuned.  The
    largest error / bound per kernel goes into RATIO (printed by the last test)."""
    p = BOUNDED[case].build()
    loops = [l for l in LOOPS if l[0] == "ring"] if case.startswith("ring") else BOUND_LOOPS
    n = 0
    for lid, hooks, pat in loops:
        _hooks(C, **hooks)
        try:
            name, bm = p.selected(C)
            if pat is not None and not re.search(pat, name):
                continue
            got, _, _ = p.run(C)
        finally:
            _defaults(C)
        acc = p.acc
        if p.d == "dgrad_s2":
            g = R.bf16_bits_to_f64(got).reshape(p.out_shape)
            assert np.all(g[:, 1::2] == 0) and np.all(g[:, :, 1::2] == 0)
            got = got.reshape(p.out_shape)[:, ::2, ::2]
        err = np.abs(R.bf16_bits_to_f64(got).reshape(acc.shape) - acc)
        ratio = float(np.max(err / CR.error_bound(acc, p.ab, p.reduction)))
        print(f"bound {case} [{lid}: {name}] error / bound = {ratio:.4f}")
        RATIO[name] = max(RATIO.get(name, 0.0), ratio)
        assert ratio <= 1.0, (case, lid, name, ratio)
        n += 1
    assert n >= 1
    p.free()


# ---------------------------------------------------------------------------------- special values
SPECIAL_LOOPS = [l for l in LOOPS if l[0] in ("igemm_d0", "igemm_d2", "dma1_mf16", "dma1_mf32", "halo")]


def _fwd_bits(C, x_bits, w_bits, OH, OW, pt, pl, loops=SPECIAL_LOOPS):
    """conv_fwd (stride 1) of raw bf16 bits under each loop that takes the shape: {kernel name: y bits}."""
    N, H, W, Cin = x_bits.shape
    out = {}
    for lid, hooks, pat in loops:
        _hooks(C, **hooks)
        try:
            name = C.conv_selected("fwd", list(x_bits.shape), list(w_bits.shape), OH, OW, 1, 1, pt, pl)[0]
            if pat is None or re.search(pat, name):
                out[name] = _bits(C.conv_fwd(_dev(x_bits), _dev(w_bits), OH, OW, 1, 1, pt, pl))
        finally:
            _defaults(C)
    assert len(out) >= 3
    return out


def test_nan_and_inf_reach_exactly_their_receptive_fields(C):
    """One NaN pixel next to the padding and one in the last row before the M tail (M = 81): NaN outputs exactly
    where the 3x3 field holds it.  +Inf alone: +-Inf by the weight's sign; +Inf and -Inf in one field: NaN."""
    N, H, W, Cin, K = 1, 9, 9, 64, 64
    x = CR.coded_ints((N, H, W, Cin), 3, 1)
    w = CR.coded_ints((K, 3, 3, Cin), 3, 2)
    w[w == 0] = 1.0  # (a zero weight times Inf would be a NaN of its own)
    wb = _to_bits(w)
    for val, pix in ((np.nan, [(0, 0), (8, 8)]), (np.inf, [(0, 4)]), (np.inf, [(4, 4)])):
        xs = x.copy()
        for (h, ww) in pix:
            xs[0, h, ww, 5] = val
        if val == np.inf and pix == [(4, 4)]:
            xs[0, 4, 6, 9] = -np.inf  # fields holding both: columns 5 (ow 5 sees 4..6)
        ref, _ = CR.conv_fwd_ref(xs, w, 9, 9, 1, 1, 1, 1)
        want = CR.round_bf16(ref)
        field = np.zeros((9, 9), bool)
        for (h, ww) in pix:
            field[max(h - 1, 0):h + 2, max(ww - 1, 0):ww + 2] = True
        if np.isnan(val):
            assert np.array_equal(np.isnan(ref).all(-1)[0], field) and np.array_equal(np.isnan(ref).any(-1)[0], field)
        elif len(pix) == 1 and pix == [(0, 4)]:
            assert np.array_equal(np.isinf(ref).all(-1)[0], field) and not np.isnan(ref).any()
            assert (ref[0, 0, 4] == np.inf).any() and (ref[0, 0, 4] == -np.inf).any()
        else:
            # a field holding both is NaN where the two weights have one sign (Inf - Inf), +-Inf where they differ
            assert np.isnan(ref[0, 4, 5]).any() and np.isinf(ref[0, 4, 5]).any()
            assert np.isinf(ref[0, 4, 3]).all() and np.isinf(ref[0, 4, 7]).all()
        xsb = R.bf16_rne(xs.astype(np.float32))
        for name, got in _fwd_bits(C, xsb, wb, 9, 9, 1, 1).items():
            _same_bits(got, want, f"special {val} {pix} [{name}]")


def test_a_finite_f32_sum_halfway_to_bf16_inf_rounds_to_inf(C):
    """2^127 + 255 * 2^119 is finite in f32 and exactly halfway between the largest bf16 and 2^128: ties to
    even give Inf.  With 254 instead of 255 it is the largest bf16 itself."""
    x = np.zeros((1, 1, 2, 64))
    x[0, 0, :, 3], x[0, 0, :, 40] = 2.0 ** 127, 2.0 ** 119
    w = np.zeros((64, 1, 1, 64))
    w[:, 0, 0, 3] = 1.0
    w[:, 0, 0, 40] = 254.0
    w[0::4, 0, 0, 40] = 255.0
    w[1::4, 0, 0, 3], w[1::4, 0, 0, 40] = -1.0, -255.0
    ref, _ = CR.conv_fwd_ref(x, w, 1, 2)
    want = CR.round_bf16(ref)
    assert set(want[0, 0, 0, :4]) == {0x7F80, 0xFF80, 0x7F7F} and np.isfinite(ref.astype(np.float32)).all()
    loops = [l for l in LOOPS if l[0] in ("igemm_d0", "igemm_d2", "dma1_mf16", "dma1_mf32")]
    for name, got in _fwd_bits(C, _to_bits(x), _to_bits(w), 1, 2, 0, 0, loops).items():
        _same_bits(got, want, f"round to inf [{name}]")


EPI_LOOPS = [l for l in LOOPS if l[0] in ("igemm_d0", "igemm_d2", "igemm_d3", "dma1_mf16", "dma1_mf32", "halo", "tile3")]


@pytest.mark.parametrize("d", ["dgrad", "dgrad_s2"])
@pytest.mark.parametrize("bn", [None, "y", "ss"])
def test_nan_operands_and_mask_lanes_in_the_epilogues(C, d, bn):
    """Residual and bn_x NaNs (0x7fff, 0xffff, 0x7f81) stay NaN through every epilogue, the integer-rounding
    ones (EK 1 / 2) included; bn_y lanes +0, -0, 0x0001, 0x8001, +-Inf and NaN of either sign follow the bit
    rule of relu_mask_bf16x8 (conv_refs.mask_from_bits)."""
    if d == "dgrad":
        p = Prob("dgrad", 2, 9, 9, 128, 64, 3, 3, pt=1, pl=1, bn=bn, x2=bn == "y", res=True).build()
    else:
        p = Prob("dgrad_s2", 3, 7, 8, 128, 64, 1, 1, 2, 2, 0, 0, 4, 4, bn=bn, x2=bn == "y", res=True).build()
    nans = np.array([0x7FFF, 0xFFFF, 0x7F81], np.uint16)
    lanes = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7F81, 0xFFFF], np.uint16)
    res = p.res_bits.reshape(-1)
    res[7:res.size:1013] = nans[np.arange(len(res[7:res.size:1013])) % 3]  # all pixels of the 2x2 blocks over time
    if bn == "y":
        by = p.by_bits.reshape(-1)
        by[3:by.size:37] = lanes[np.arange(len(by[3:by.size:37])) % len(lanes)]
        by[7:by.size:1013] = 0x3F80  # the residual NaNs pass the mask
    if bn:
        bx = p.bx_bits.reshape(-1)
        bx[11:bx.size:1531] = nans[np.arange(len(bx[11:bx.size:1531])) % 3]
    p.random = True  # (NaN sums: the exactness precondition does not apply; equality is still asserted)
    ran = run_loops(C, p, must=("igemm_d0", "dma1_mf32"), loops=EPI_LOOPS)
    want = p.expect(128)[0]
    n_nan = int(R.bf16_is_nan(want).sum())
    n_res = len(res[7:res.size:1013])
    if bn != "ss":
        assert n_nan >= n_res  # every residual NaN is a NaN of the output
    assert len(ran) >= 4


def test_subnormal_inputs_and_sums(C):
    """bf16 subnormal inputs whose products are normal, and products that are f32 subnormals (stored as bf16
    subnormals), against the f64 reference as IEEE arithmetic has it.  (The reference with subnormal inputs
    or sums flushed to zero is computed as well, to say which one a failure matches.)"""
    x = np.zeros((1, 1, 4, 64))
    w = np.zeros((64, 1, 1, 64))
    x[0, 0, 0, 1] = 2.0 ** -130          # bf16 subnormal input, product 2^-120 (normal)
    x[0, 0, 0, 2] = -3 * 2.0 ** -132     # another, negative
    x[0, 0, 1, 1] = 2.0 ** -100          # normal inputs, product 2^-130 (f32 and bf16 subnormal)
    x[0, 0, 2, 1], x[0, 0, 2, 2] = 2.0 ** -100, 2.0 ** -100  # two subnormal products summing to a subnormal
    x[0, 0, 3, 1], x[0, 0, 3, 2] = 2.0 ** -100, -(2.0 ** -100)  # normal products cancelling into a subnormal sum
    w[:, 0, 0, 1] = 2.0 ** 10
    w[:, 0, 0, 2] = 2.0 ** 10
    w2 = w.copy()
    w2[:, 0, 0, 1], w2[:, 0, 0, 2] = 2.0 ** -30, 2.0 ** -31
    w3 = w.copy()
    w3[:, 0, 0, 1], w3[:, 0, 0, 2] = 2.0 ** -25 * 1.5, 2.0 ** -25 * 1.25  # 2^-125 (1.5 - 1.25) = 2^-127
    loops = [l for l in LOOPS if l[0] in ("igemm_d0", "igemm_d2", "dma1_mf16", "dma1_mf32")]
    seen = set()
    for tag, ww in (("inputs", w), ("sums", w2), ("cancel", w3)):
        ref, _ = CR.conv_fwd_ref(x, ww, 1, 4)
        ieee = CR.round_bf16(ref)
        xf = np.where(np.abs(x) < 2.0 ** -126, 0.0, x)
        ftz_ref, _ = CR.conv_fwd_ref(xf, ww, 1, 4)
        ftz = CR.round_bf16(np.where(np.abs(ftz_ref) < 2.0 ** -126, 0.0, ftz_ref))
        assert not np.array_equal(ieee, ftz)  # the case can tell the two apart
        for name, got in _fwd_bits(C, _to_bits(x), _to_bits(ww), 1, 4, 0, 0, loops).items():
            which = "ieee" if np.array_equal(got, ieee) else ("flush" if np.array_equal(got, ftz) else "neither")
            print(f"subnormal {tag} [{name}]: {which}")
            seen.add(which)
            SUBNORMAL[f"{tag} {name}"] = which
            _same_bits(got, ieee, f"subnormal {tag} [{name}]")
    assert seen == {"ieee"}


# ---------------------------------------------------------------------------------- refusals
def _t(*shape):
    return torch.ones(*shape, device="cuda").bfloat16()


def test_inconsistent_and_unsupported_geometries_are_refused(C):
    x, w = _t(2, 8, 8, 64), _t(64, 3, 3, 64)
    ok = C.conv_fwd(x, w, 8, 8, 1, 1, 1, 1)
    assert ok.shape == (2, 8, 8, 64)
    off = torch.ones(2 * 8 * 8 * 64 + 4, device="cuda").bfloat16()[4:].reshape(2, 8, 8, 64)  # 8 bytes past alignment
    bad = [
        lambda: C.conv_fwd(x, w, 10, 8, 1, 1, 1, 1),           # implied bottom padding 3 = KH
        lambda: C.conv_fwd(x, w, 8, 10, 1, 1, 1, 1),           # right padding 3 = KW
        lambda: C.conv_fwd(x, w, 6, 6, 2, 2, 1, 1),            # stride 2: at most 5 rows (pb = 10 + 3 - 8 - 1 = 4)
        lambda: C.conv_fwd_stats(x, w, 10, 8, 1, 1, 1, 1),
        lambda: C.conv_fwd(x, w, 8, 8, 1, 1, 3, 1),            # PT >= KH
        lambda: C.conv_fwd(x, w, 8, 8, 1, 1, 1, 3),            # PL >= KW
        lambda: C.conv_fwd(x, w, 8, 8, 0, 1, 1, 1),            # stride 0
        lambda: C.conv_fwd(_t(2, 8, 8, 96), _t(64, 3, 3, 96), 8, 8, 1, 1, 1, 1),   # C not a multiple of 64
        lambda: C.conv_fwd(x, _t(96, 3, 3, 64), 8, 8, 1, 1, 1, 1),                 # K not a multiple of 64
        lambda: C.conv_fwd(x, _t(64, 3, 11, 64), 8, 8, 1, 1, 1, 5),                # 33 taps
        lambda: C.conv_fwd(off, w, 8, 8, 1, 1, 1, 1),                              # misaligned
        lambda: C.conv_fwd(_t(2, 8, 8, 128)[..., ::2], w, 8, 8, 1, 1, 1, 1),       # non-contiguous
        lambda: C.conv_fwd(x, _t(64, 3, 3, 128)[..., ::2], 8, 8, 1, 1, 1, 1),
        lambda: C.conv_fwd(x.float(), w, 8, 8, 1, 1, 1, 1),                        # not bf16
        lambda: C.conv_fwd(x, _t(64, 3, 3, 128), 8, 8, 1, 1, 1, 1),                # channel mismatch
        # input-side BN: not 1x1 stride 1, and C = 576 > 512
        lambda: C.conv_fwd(x, w, 8, 8, 1, 1, 1, 1, torch.ones(4, 64, device="cuda")),
        lambda: C.conv_fwd(x, _t(64, 1, 1, 64), 4, 4, 2, 2, 0, 0, torch.ones(4, 64, device="cuda")),
        lambda: C.conv_fwd(_t(1, 4, 4, 576), _t(64, 1, 1, 576), 4, 4, 1, 1, 0, 0, torch.ones(4, 576, device="cuda")),
        lambda: C.conv_fwd_stats(_t(1, 4, 4, 576), _t(64, 1, 1, 576), 4, 4, 1, 1, 0, 0, torch.ones(4, 576, device="cuda")),
    ]
    assert C.conv_fwd(x, w, 9, 8, 1, 1, 1, 1).shape == (2, 9, 8, 64)  # bottom padding 2 < KH: legal
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
            pytest.fail(f"refusal {i} did not raise")
    torch.cuda.synchronize()


def test_input_gradient_refusals(C):
    dy, w = _t(2, 8, 8, 64), _t(3, 3, 64, 64)
    assert C.conv_dgrad(dy, w, 8, 8, 1, 1).shape == (2, 8, 8, 64)
    assert C.conv_dgrad(dy, w, 6, 6, 2, 2).shape == (2, 6, 6, 64)      # padding (2, 2) + implied (2, 2)
    assert C.conv_dgrad(dy, w, 10, 10, 0, 0).shape == (2, 10, 10, 64)  # 'valid'
    bad = [
        lambda: C.conv_dgrad(dy, w, 11, 10, 0, 0),   # an 11-row input gives 9 rows of dy (implied padding -1)
        lambda: C.conv_dgrad(dy, w, 10, 11, 0, 0),
        lambda: C.conv_dgrad(dy, w, 5, 6, 0, 0),     # implied bottom padding 3 = KH
        lambda: C.conv_dgrad(dy, w, 8, 7, 1, 0),     # right padding 3 = KW
        lambda: C.conv_dgrad(dy, w, 8, 8, 3, 1),     # PT >= KH
        lambda: C.conv_dgrad(dy.reshape(2 * 8, 8, 64), w, 8, 8, 1, 1),                # dy not 4-D
        lambda: C.conv_dgrad(dy, w, 8, 8, 1, 1, _t(3, 8, 8, 64)),                     # residual of another batch size
        lambda: C.conv_dgrad_bn(dy, w, 8, 8, 1, 1, None, _t(3, 8, 8, 64), _t(2, 8, 8, 64), None, None),
        lambda: C.conv_dgrad_bn(dy, w, 8, 8, 1, 1, None, None, _t(2, 8, 8, 64), None, None),   # bn_x without bn_y / bn_stats
        lambda: C.conv_dgrad(dy, _t(3, 3, 96, 64), 8, 8, 1, 1),                       # C not a multiple of 64
        lambda: C.conv_dgrad(dy, _t(3, 11, 64, 64), 8, 8, 1, 5),                      # 33 taps
        lambda: C.conv_dgrad(_t(2, 8, 8, 128)[..., ::2], w, 8, 8, 1, 1),              # non-contiguous
        lambda: C.conv_dgrad_s2(dy.reshape(2 * 8, 8, 64), _t(1, 1, 64, 64), 16, 16, None),
        lambda: C.conv_dgrad_s2(dy, _t(1, 1, 64, 64), 17, 16, None),                  # 17 rows give 9 rows of dy
        lambda: C.conv_dgrad_s2(dy, _t(1, 1, 64, 64), 14, 16, None),
        lambda: C.conv_dgrad_s2(dy, _t(3, 3, 64, 64), 16, 16, None),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
            pytest.fail(f"refusal {i} did not raise")
    for args in (("fwd", [2, 8, 8, 64], [64, 3, 3, 64], 10, 8, 1, 1, 1, 1), ("dgrad", [2, 11, 10, 64], [3, 3, 64, 64], 8, 8),
                 ("dgrad_s2", [2, 16, 16, 64], [1, 1, 64, 64], 8, 8, 1, 1), ("up", [2, 8, 8, 64], [64, 3, 3, 64], 8, 8, 1, 1, 1, 1),
                 ("fwd", [2, 8, 8, 64], [64, 3, 3, 64], 8, 8, 1, 1, 1, 1, ["in_bn"]),
                 ("fwd", [2, 8, 8, 64], [64, 3, 3, 64], 8, 8, 1, 1, 1, 1, ["bn"])):
        with pytest.raises(RuntimeError):
            C.conv_selected(*args)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------- coverage (keep last)
def test_every_kernel_conv_selected_can_name_has_run(C):
    names = C.conv_kernel_names()
    print("\nkernel: exact cases, ties rounded down / up, largest error / bound on random data")
    for n in names:
        t = TIES.get(n, [0, 0])
        r = RATIO.get(n)
        print(f"  {n}: {RAN.get(n, 0)} cases, ties {t[0]} / {t[1]}, ratio {'-' if r is None else f'{r:.4f}'}")
    print("subnormals:", sorted(set(SUBNORMAL.values())) or "-")
    missing = [n for n in names if RAN.get(n, 0) == 0]
    assert not missing, f"never ran: {missing}"
    assert not set(RAN) - set(names), set(RAN) - set(names)
    assert all(min(TIES[n]) >= 200 for n in names), {n: TIES[n] for n in names if min(TIES[n]) < 200}
