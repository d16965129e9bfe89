"""The generic f32 convolutions (csrc/kernels/gemm_f32.hip: conv_f32_fwd, conv_f32_fwd_pool, conv_f32_dgrad,
conv_f32_wgrad, through the raw bindings) bit-exactly against the f64 references of conv_refs.py at their
edges: one-sided and unequal padding, strides, dilation, filters larger than the image, channel counts around
the 4-element quads, pixel counts and reductions around the 64 / 16 tiles, filters whose mixed-radix counter
wraps many times per step, the appended column of ones, accumulation into guarded outputs, the pooled
epilogue and its split reduces, the pooled-gradient loaders, non-finite values, and one random-data case per
mode checked element by element against the derived bound.  Both operand-loader forms (f32_buf) run.

Integer data (see test_gemm_f32_edges_gpu.py).  Every case asserts the kernel it was built to reach; the last
test asserts that every convolution kernel and every pooled reduce f32_kernel_names() lists has run."""
import itertools

import numpy as np
import pytest
import torch

import conv_refs as CR
import f32_edge_helpers as H
from f32_edge_helpers import Geo

pytestmark = pytest.mark.gpu

BUFS = (True, False)

# Geo(N, H, W, C, K, R, S, stride, pads (top, bottom, left, right), dilation)
GEOMS = {
    "pad_top": Geo(1, 5, 6, 3, 4, 3, 3, pads=(1, 0, 0, 0)),
    "pad_bottom": Geo(1, 5, 6, 3, 4, 3, 3, pads=(0, 1, 0, 0)),
    "pad_left": Geo(1, 5, 6, 3, 4, 3, 3, pads=(0, 0, 1, 0)),
    "pad_right": Geo(1, 5, 6, 3, 4, 3, 3, pads=(0, 0, 0, 1)),
    "pad_unequal": Geo(2, 5, 6, 5, 4, 3, 3, pads=(2, 1, 0, 3)),
    "stride12": Geo(1, 6, 9, 4, 1, 3, 3, stride=(1, 2), pads=(1, 1, 1, 1)),
    "stride21": Geo(1, 9, 6, 8, 4, 3, 3, stride=(2, 1), pads=(1, 1, 1, 1)),
    "stride33": Geo(2, 9, 10, 3, 4, 3, 3, stride=(3, 3), pads=(1, 0, 1, 0)),
    "stride_gt_filter": Geo(1, 9, 11, 4, 4, 2, 2, stride=(3, 4)),            # input pixels no output reads
    "stride2_odd": Geo(1, 7, 9, 4, 5, 3, 3, stride=(2, 2), pads=(0, 1, 1, 0)),
    "dil2": Geo(1, 7, 8, 3, 4, 3, 3, pads=(2, 2, 2, 2), dil=(2, 2)),
    "dil3": Geo(1, 8, 7, 4, 4, 3, 2, pads=(3, 1, 0, 3), dil=(3, 3)),
    "stride_dil": Geo(1, 10, 9, 4, 4, 3, 3, stride=(2, 3), pads=(2, 1, 1, 2), dil=(2, 3)),
    "filter_gt_image": Geo(2, 2, 3, 3, 4, 5, 4, pads=(2, 2, 1, 2)),          # H < R, W < S
    "1x1": Geo(1, 5, 5, 8, 63, 1, 1),
    "c1_k65": Geo(1, 6, 6, 1, 65, 3, 3, pads=(1, 1, 1, 1)),
    "m63": Geo(1, 7, 9, 4, 4, 1, 1),
    "m64": Geo(1, 8, 8, 3, 4, 1, 1),
    "m65": Geo(1, 5, 13, 4, 3, 1, 1),
    "red15": Geo(1, 4, 8, 3, 4, 1, 5), "red16": Geo(1, 5, 5, 4, 4, 2, 2), "red17": Geo(1, 3, 20, 1, 4, 1, 17),
    "red63": Geo(1, 5, 5, 7, 4, 3, 3), "red64": Geo(1, 6, 6, 4, 4, 4, 4), "red65": Geo(1, 3, 16, 5, 4, 1, 13),
    "f9x2_c1": Geo(1, 12, 5, 1, 4, 9, 2, pads=(2, 0, 0, 1)),                 # mid wraps eight times per step
    "f17x2_c1": Geo(1, 20, 4, 1, 3, 17, 2, pads=(1, 1, 0, 0)),               # ... over two steps
    "f3x5_c3": Geo(1, 6, 8, 3, 5, 3, 5, pads=(1, 1, 2, 2)),
}


def test_geometries_are_the_edges_they_claim():
    g = GEOMS
    assert [g[k].N * g[k].OH * g[k].OW for k in ("m63", "m64", "m65")] == [63, 64, 65]
    assert [g[f"red{r}"].R * g[f"red{r}"].S * g[f"red{r}"].C for r in (15, 16, 17, 63, 64, 65)] == [15, 16, 17, 63, 64, 65]
    assert {x.C for x in g.values()} >= {1, 3, 4, 5, 8} and {x.K for x in g.values()} >= {1, 4, 63, 65}
    f = g["f9x2_c1"]
    assert f.S * f.C < 16 and f.R * f.S * f.C > 16 and 16 // (f.S * f.C) == 8
    assert g["f17x2_c1"].R * 2 > 32


@pytest.mark.parametrize("name", list(GEOMS))
def test_forward_geometry(name):
    g = GEOMS[name]
    for i, buf in enumerate(BUFS):
        H.run_fwd(g, bias=True, act=1, buf=buf, salt=i)
        H.run_fwd(g, bias=False, act=0, buf=buf, salt=2 + i)


@pytest.mark.parametrize("mis_x,mis_w", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_forward_loader_flags(mis_x, mis_w):
    """C % 4 and K % 4 with aligned and misaligned operands: all 4 x 2 forward kernels."""
    for C, K in ((4, 8), (5, 8), (4, 7), (3, 5)):
        for buf in BUFS:
            H.run_fwd(Geo(2, 5, 6, C, K, 3, 3, pads=(1, 1, 1, 1)), act=1, mis_x=bool(mis_x), mis_w=bool(mis_w),
                      buf=buf, salt=C + K)


FWD_SPLITS = [  # (geometry, splits, reduce)
    (Geo(1, 5, 5, 29, 5, 3, 3), 5, "reduce8"), (Geo(1, 5, 5, 57, 4, 3, 3), 9, "reduce16"),
    (Geo(1, 5, 5, 128, 6, 3, 3), 18, "wave"), (Geo(4, 66, 66, 32, 4, 3, 3), 4, "reduce4"),
]


@pytest.mark.parametrize("case", FWD_SPLITS, ids=[c[2] for c in FWD_SPLITS])
def test_forward_split_reduces(case):
    g, splits, reduce = case
    for buf in BUFS:
        H.run_fwd(g, act=1, buf=buf, salt=7, reduce=reduce, splits=splits)


# ------------------------------------------------------------------------------------------- input gradient
@pytest.mark.parametrize("name", list(GEOMS))
def test_input_gradient_geometry(name):
    g = GEOMS[name]
    for i, (buf, hwio) in enumerate(itertools.product(BUFS, (True, False))):
        dx, want, _ = H.run_dgrad(g, mask=bool(i & 1), hwio=hwio, buf=buf, salt=i)
        if name == "stride_gt_filter":  # pixels no output reads: written, as exact zeros
            unread = np.ones((g.H, g.W), bool)
            for oy, ox, r, s in itertools.product(range(g.OH), range(g.OW), range(g.R), range(g.S)):
                unread[oy * g.sh + r, ox * g.sw + s] = False
            assert unread.sum() > g.H * g.W // 2
            assert (dx.cpu().numpy()[:, unread] == 0).all() and (want[:, unread] == 0).all()


@pytest.mark.parametrize("mask", [False, True])
def test_input_gradient_loader_flags(mask):
    """K % 4 x mask x alignment (dy, its mask) and C % 4 x storage x alignment (w): all 16 kernels."""
    a_vars = [dict(), dict(K=6), dict(mis_dy=True)] + ([dict(mis_m=True)] if mask else [])
    b_vars = [dict(hwio=False), dict(hwio=False, C=5), dict(hwio=False, mis_w=True), dict(hwio=True),
              dict(hwio=True, mis_w=True)]
    for i, (av, bv) in enumerate(itertools.product(a_vars, b_vars)):
        kw = dict(av, **bv)
        g = Geo(1, 6, 7, kw.pop("C", 4), kw.pop("K", 8), 3, 3, stride=(2, 1), pads=(1, 1, 1, 1))
        for buf in BUFS:
            H.run_dgrad(g, mask=mask, buf=buf, salt=50 + i, **kw)


def test_input_gradient_split_reduce():
    g = Geo(1, 5, 5, 4, 32, 3, 3, pads=(1, 1, 1, 1))  # reduction 3 * 3 * 32 = 288 over 25 pixels: 5 slices
    for buf in BUFS:
        H.run_dgrad(g, mask=True, hwio=False, buf=buf, reduce="reduce8", splits=5)


# ------------------------------------------------------------------------------------------- weight gradient
WGRAD = {
    "ones_is_col63": (Geo(1, 6, 6, 7, 5, 3, 3, pads=(1, 1, 1, 1)), dict(dbias=True)),
    "ones_alone_in_tile2": (Geo(2, 4, 4, 64, 6, 1, 1), dict(dbias=True, mask=True)),  # behind vector quads
    "accumulate": (Geo(2, 6, 5, 4, 9, 3, 2, stride=(2, 1), pads=(1, 0, 0, 1)), dict(acc=True, dbias=True)),
    "accumulate_dil": (Geo(1, 9, 9, 3, 8, 3, 3, pads=(2, 2, 2, 2), dil=(2, 2)), dict(acc=True, dbias=True, mask=True)),
    "out_only": (Geo(1, 5, 5, 5, 4, 2, 2), dict(out=True)),
    "pixels1": (Geo(1, 3, 3, 4, 5, 3, 3), dict(dbias=True)),
    "pixels15": (Geo(1, 5, 7, 3, 5, 3, 3), dict(dbias=True)),
    "pixels16": (Geo(1, 4, 4, 4, 65, 1, 1), dict(mask=True)),
    "pixels17": (Geo(1, 1, 17, 5, 64, 1, 1), dict(dbias=True, mask=True)),
    "k64": (Geo(4, 7, 7, 8, 64, 3, 3, stride=(2, 2), pads=(1, 1, 1, 1)), dict(dbias=True)),
    "filter_gt_image": (Geo(2, 2, 3, 3, 4, 5, 4, pads=(2, 2, 1, 2)), dict(dbias=True)),
}


@pytest.mark.parametrize("name", list(WGRAD))
def test_weight_gradient_edges(name):
    g, opt = WGRAD[name]
    if name == "ones_is_col63":
        assert g.R * g.S * g.C == 63
    if name == "ones_alone_in_tile2":
        assert g.R * g.S * g.C == 64 and g.C == 64
    if name.startswith("pixels"):
        assert g.N * g.OH * g.OW == int(name[6:])
    for i, (buf, mis_x) in enumerate(itertools.product(BUFS, (False, True))):
        H.run_wgrad(g, buf=buf, mis_x=mis_x, salt=i, **opt)
    if not opt.get("mask"):
        H.run_wgrad(g, mask=True, mis_dy=True, mis_m=True, salt=9, **opt)


@pytest.mark.parametrize("K,reduce", [(64, "wave16x16_v4"), (63, "wave16x16_s")])
def test_weight_gradient_sixteen_slices(K, reduce):
    """K output channels against 288 + 1 columns over 1024 pixels: 16 slices of 64."""
    g = Geo(1, 34, 34, 32, K, 3, 3)
    assert g.N * g.OH * g.OW == 1024 and g.R * g.S * g.C + 1 == 289
    for buf in BUFS:
        H.run_wgrad(g, mask=not buf, acc=True, dbias=True, buf=buf, reduce=reduce, splits=16)


# ------------------------------------------------------------------------------------------- pooled forward
def _negative_bias(x, w, bia):
    bia[0::2] = -2.0 ** 20  # every window of these channels is entirely negative before the ReLU


POOLED = {
    "even": Geo(2, 6, 6, 3, 8, 3, 3, pads=(1, 1, 1, 1)),
    "odd_oh": Geo(1, 7, 6, 4, 8, 3, 3, pads=(1, 1, 1, 1)),
    "odd_ow": Geo(1, 6, 9, 4, 5, 3, 3, pads=(1, 1, 1, 1)),
    "odd_both_strided": Geo(2, 11, 11, 3, 8, 3, 3, stride=(2, 2), pads=(0, 0, 0, 0)),
    "rows_cross_tile": Geo(1, 2, 34, 4, 65, 1, 1),                           # 17 windows: rows 64..67 in tile 2
    "dilated": Geo(1, 9, 8, 2, 4, 3, 3, pads=(2, 2, 2, 2), dil=(2, 2)),
}


@pytest.mark.parametrize("name", list(POOLED))
def test_pooled_forward_geometry(name):
    """Integer data ties constantly: the argmax must be the first maximum.  Channels with a large negative
    bias: act = 1 windows entirely <= 0 give maximum 0 and argmax 0; act = 0 windows entirely negative."""
    g = POOLED[name]
    if name == "rows_cross_tile":
        assert g.N * (g.OH // 2) * (g.OW // 2) * 4 == 68
    for i, (buf, act) in enumerate(itertools.product(BUFS, (1, 0))):
        (y, p, arg), _ = H.run_fwd(g, pool=True, act=act, buf=buf, salt=i, poke=_negative_bias)
        if act == 1:
            assert (p[..., 0::2] == 0).all() and (arg[..., 0::2] == 0).all() and (p[..., 1::2] > 0).any()
        else:
            assert (p[..., 0::2] < 0).all() and (arg[..., 0::2] < 4).all()
        H.run_fwd(g, pool=True, act=act, bias=False, buf=buf, salt=4 + i)


def _one_negative_channel(x, w, bia):
    bia[0] = -2.0 ** 20


POOL_SPLITS = [  # (geometry, splits, reduce, unfused splits, hooks); a 3 x 3 output is one window
    (Geo(1, 5, 5, 29, 24, 3, 3), 5, "pool8", 5, {}), (Geo(1, 5, 5, 57, 24, 3, 3), 9, "pool16", 9, {}),
    (Geo(1, 5, 5, 100, 21, 3, 3), 15, "pool16", 15, {}), (Geo(4, 66, 66, 32, 4, 3, 3), 4, "pool4", 4, {}),
    (Geo(1, 5, 5, 29, 24, 3, 3), 5, "pool_rows", 5, dict(hoist=False)),
    (Geo(1, 5, 5, 29, 24, 3, 3), 5, "pool16", 5, dict(narrow=False)),
    (Geo(1, 8, 8, 112, 8, 3, 3), 1, "none", 16, {}),                         # the fallback to one slice
]


@pytest.mark.parametrize("case", POOL_SPLITS, ids=[f"{c[2]}_{c[1]}" + "".join(c[4]) for c in POOL_SPLITS])
def test_pooled_forward_split_reduces(case):
    g, splits, reduce, unfused, hk = case
    for buf in BUFS:
        for act in (1, 0):
            H.run_fwd(g, pool=True, act=act, buf=buf, salt=3, reduce=reduce, splits=splits, unfused=unfused,
                      poke=_one_negative_channel, **hk)


# ------------------------------------------------------------------------------------------- pooled gradients
PIN = {
    "k8": Geo(2, 8, 8, 4, 8, 3, 3, pads=(1, 1, 1, 1)),                       # K % 4 == 0: the 4-byte argmax read
    "k6_odd": Geo(1, 9, 7, 5, 6, 3, 3, pads=(1, 1, 1, 1)),                   # odd conv output: 9 x 7
    "k8_odd_valid": Geo(2, 9, 11, 4, 8, 3, 3),                               # 7 x 9
    "k65": Geo(1, 5, 5, 3, 65, 2, 2, pads=(0, 1, 0, 1)),
}


@pytest.mark.parametrize("name", list(PIN))
def test_pooled_gradient_loaders(name):
    """Input and weight gradient from the POOLED gradient (argmax routing, maximum > 0, some argmax bytes
    255) against the pooled-backward reference followed by the plain references."""
    g = PIN[name]
    for i, (hwio, mis) in enumerate(itertools.product((True, False), (False, True))):
        H.run_dgrad(g, pin=True, hwio=hwio, mis_dy=mis, mis_w=mis and not hwio, salt=i)
        H.run_dgrad(g, pin=True, hwio=hwio, mis_m=mis, buf=False, salt=4 + i)
        H.run_wgrad(g, pin=True, dbias=True, acc=bool(i & 1), mis_x=mis, salt=i)
        H.run_wgrad(g, pin=True, mis_dy=mis, mis_m=not mis, buf=False, salt=4 + i)


# ------------------------------------------------------------------------------------------- non-finite
def _nan_count(t):
    return int(torch.isnan(t).sum())


@pytest.mark.parametrize("buf", BUFS)
def test_single_nan_reaches_exactly_the_outputs_that_read_it(buf):
    g = Geo(1, 6, 7, 4, 5, 3, 3, pads=(1, 1, 1, 1))

    def nan_x(x, w, bia):
        x[0, 5, 6, 3] = np.nan  # the corner pixel: four outputs read it

    y, _ = H.run_fwd(g, act=0, buf=buf, poke=nan_x)  # (same_bits: NaN where and only where the reference has it)
    assert _nan_count(y) == 4 * g.K and torch.isnan(y[0, 4:, 5:]).all()
    y, _ = H.run_fwd(g, act=1, buf=buf, poke=nan_x)  # NaN pre-activations under the ReLU: stored as 0
    assert _nan_count(y) == 0 and (y[0, 4:, 5:] == 0).all()

    def nan_dy(dy, w, m):
        dy[0, 0, 0, 1] = np.nan

    dx, _, _ = H.run_dgrad(g, buf=buf, poke=nan_dy)
    assert _nan_count(dx) == 4 * g.C and torch.isnan(dx[0, :2, :2]).all()

    def nan_xw(x, dy, m):
        x[0, 0, 0, 2] = np.nan

    gw, _, _ = H.run_wgrad(g, buf=buf, dbias=True, poke=nan_xw)
    bad = torch.isnan(gw)
    assert _nan_count(gw) == 4 * g.K and bad[:2, :2, 2].all() and not bad[..., 3, :].any()


@pytest.mark.parametrize("buf", BUFS)
def test_masked_inf_and_nan_contribute_zero(buf):
    g = Geo(1, 5, 5, 4, 8, 3, 3, pads=(1, 1, 1, 1))

    def poke_dy(dy, m):
        for i, mv in enumerate((0.0, -3.0, np.nan, -0.0)):
            dy[0, i, i, i] = np.inf if i & 1 else np.nan
            m[0, i, i, i] = mv

    dx, _, _ = H.run_dgrad(g, mask=True, buf=buf, poke=lambda dy, w, m: poke_dy(dy, m))
    assert torch.isfinite(dx).all()
    gw, _, _ = H.run_wgrad(g, mask=True, dbias=True, buf=buf, poke=lambda x, dy, m: poke_dy(dy, m))
    assert torch.isfinite(gw).all()

    def poke_dp(dp, mx, arg):  # pooled gradient: Inf / NaN under a maximum <= 0, -0 or NaN, at LIVE positions
        for i, mv in enumerate((0.0, -3.0, np.nan, -0.0)):
            at = (0, i // 2, i % 2 + 1, i)
            dp[at], mx[at], arg[at] = (np.inf if i & 1 else np.nan), mv, i  # (argmax i < 4: only the mask drops it)
        assert (arg == 255).any()

    g2 = Geo(1, 6, 6, 4, 8, 3, 3, pads=(1, 1, 1, 1))
    assert torch.isfinite(H.run_dgrad(g2, pin=True, buf=buf, poke=lambda dp, w, mx, arg: poke_dp(dp, mx, arg))[0]).all()
    assert torch.isfinite(H.run_wgrad(g2, pin=True, dbias=True, buf=buf,
                                      poke=lambda x, dp, mx, arg: poke_dp(dp, mx, arg))[0]).all()

    def live(dp, mx, arg):  # such an element under a maximum > 0 does arrive: the pokes above are not vacuous
        dp[0, 0, 1, 0], mx[0, 0, 1, 0], arg[0, 0, 1, 0] = np.inf, 1.0, 0

    assert not torch.isfinite(H.run_dgrad(g2, pin=True, poke=lambda dp, w, mx, arg: live(dp, mx, arg))[0]).all()


@pytest.mark.parametrize("buf", BUFS)
def test_pooled_epilogue_with_non_finite_window_elements(buf):
    """A NaN never wins a window; a window of NaNs (or of -inf) gives -inf and argmax 255: the reference, and
    conv_f32_fwd followed by maxpool_fwd."""
    C = H.hip()
    g = Geo(1, 6, 6, 1, 8, 1, 1)

    def poke(x, w, bia):
        x[0, 0, 1, 0] = np.nan          # one NaN in window (0, 0)
        x[0, 2:4, 2:4, 0] = np.nan      # window (1, 1) all NaN
        bia[3] = -np.inf                # channel 3: every pixel -inf

    (y, p, arg), _ = H.run_fwd(g, pool=True, act=0, buf=buf, poke=poke)
    assert torch.isnan(y[0, 0, 1]).all() and not torch.isnan(p[0, 0, 0]).any() and (arg[0, 0, 0] != 1).all()
    assert (p[0, 1, 1] == -np.inf).all() and (arg[0, 1, 1] == 255).all()
    assert (p[..., 3] == -np.inf).all() and (arg[..., 3] == 255).all()
    x = H.ints((1, 6, 6, 1), H.amp_of(1), 21)
    w, bia = H.ints((1, 1, 1, 8), H.amp_of(1), 22), H.ints((8,), 50, 23)
    poke(x, w, bia)
    with H.hooks(buf=buf):
        y0 = C.conv_f32_fwd(H.dev(x), H.dev(w), H.dev(bia), 6, 6, 1, 1, 0, 0, act=0)
        H.selected(f"fwd_va0_vb1_buf{H.b01(buf)}", "none", 1)
        p0, a0 = C.maxpool_fwd(y0, 2, 2, 2, 2, 0, 0, 3, 3, False)
    assert torch.equal(p, p0) and torch.equal(arg, a0)
    (y, p, arg), _ = H.run_fwd(g, pool=True, act=1, buf=buf, poke=poke)  # under the ReLU every NaN / -inf is 0
    assert (p[0, 1, 1] == 0).all() and (arg[0, 1, 1] == 0).all() and (p[..., 3] == 0).all()


# ------------------------------------------------------------------------------------------- real data
def _randn(shape, seed, scale=1.0):
    return (np.random.RandomState(seed).randn(*shape) * scale).astype(np.float32)


def _within(got, want, ab, count, what):
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - want)
    bound = CR.error_bound_f32(ab, count)
    ok = np.isfinite(err) & (err <= bound)
    print(f"\n{what}: largest error / bound {np.max(err / np.maximum(bound, 1e-300)):.4f}")
    assert ok.all(), (what, np.max(err / np.maximum(bound, 1e-300)))


@pytest.mark.parametrize("g", [Geo(2, 9, 10, 5, 7, 3, 3, stride=(2, 1), pads=(1, 0, 1, 1)),
                               Geo(1, 6, 6, 40, 9, 3, 3, pads=(1, 1, 1, 1), dil=(2, 2))], ids=["one_slice", "split"])
def test_random_data_elementwise_bounds(g):
    """randn data, every output within error_bound_f32(sum |a||b| (+ |bias| + |prior|), Kred + splits + 2)."""
    C = H.hip()
    x, w = _randn((g.N, g.H, g.W, g.C), 1), _randn((g.R, g.S, g.C, g.K), 2, (g.R * g.S * g.C) ** -0.5)
    b, dy = _randn((g.K,), 3), _randn((g.N, g.OH, g.OW, g.K), 4)
    prior = _randn(w.shape, 5)
    x64, w64, dy64 = (v.astype(np.float64) for v in (x, w, dy))
    for buf in BUFS:
        c4, k4, bb = H.b01(g.C % 4 == 0), H.b01(g.K % 4 == 0), H.b01(buf)
        with H.hooks(buf=buf, narrow=True, hoist=True, reduce16=True):
            y = C.conv_f32_fwd(H.dev(x), H.dev(w), H.dev(b), g.OH, g.OW, *g.bind(), act=0)
            sf = H.selected(f"fwd_va{c4}_vb{k4}_buf{bb}")
            dx = C.conv_f32_dgrad(H.dev(dy), H.dev(w), g.H, g.W, *g.bind(), w_hwio=True)
            sd = H.selected(f"dgrad_ma0_va{k4}_vb0_pin0_buf{bb}")
            out = H.Guarded(prior)
            gw = C.conv_f32_wgrad(H.dev(x), H.dev(dy), g.R, g.S, *g.bind(), out=out.view, accumulate=True)
            sw = H.selected(f"wgrad_ma0_vb{c4}_pin0_buf{bb}")
        yr, ab = CR.conv_fwd_ref(x64, w64.transpose(3, 0, 1, 2), g.OH, g.OW, **g.kw)
        _within(y, yr + b, ab + np.abs(b), g.R * g.S * g.C + sf[2] + 2, f"fwd {g}")
        dr, ab = CR.conv_dgrad_ref(dy64, w64, g.H, g.W, **g.kw)
        _within(dx, dr, ab, g.R * g.S * g.K + sd[2] + 2, f"dgrad {g}")
        wr, ab = CR.conv_wgrad_ref(x64, dy64, g.R, g.S, **g.kw)
        _within(gw, wr + prior, ab + np.abs(prior), g.N * g.OH * g.OW + sw[2] + 2, f"wgrad {g}")
        out.check("random wgrad")


@pytest.mark.parametrize("g,unfused", [(Geo(2, 8, 9, 29, 8, 3, 3, pads=(1, 1, 1, 1)), 5),
                                       (Geo(1, 10, 10, 128, 64, 3, 3, pads=(1, 1, 1, 1)), 18)], ids=["u5", "u18"])
def test_pooled_conv_on_random_data(g, unfused):
    """The pooled conv equals the unfused conv bit for bit where the unfused plan has fewer than 16 slices;
    with 16 or more it reduces in one slice and is held to the bound only (gemm_f32.h plan_m)."""
    C = H.hip()
    x, w, b = _randn((g.N, g.H, g.W, g.C), 1), _randn((g.R, g.S, g.C, g.K), 2, (g.R * g.S * g.C) ** -0.5), _randn((g.K,), 3)
    PH, PW = g.OH // 2, g.OW // 2
    Kred = g.R * g.S * g.C
    yr, ab = CR.conv_fwd_ref(x.astype(np.float64), w.astype(np.float64).transpose(3, 0, 1, 2), g.OH, g.OW, **g.kw)
    yr, ab = np.maximum(yr + b, 0.0), ab + np.abs(b)

    def win(v):
        return v[:, :2 * PH, :2 * PW].reshape(g.N, PH, 2, PW, 2, g.K)

    for buf in BUFS:
        xd, wd, bd = H.dev(x), H.dev(w), H.dev(b)
        name = f"fwd_va{H.b01(g.C % 4 == 0)}_vb1_buf{H.b01(buf)}"
        with H.hooks(buf=buf, narrow=True, hoist=True, reduce16=True):
            y, p, arg = C.conv_f32_fwd_pool(xd, wd, bd, g.OH, g.OW, *g.bind(), act=1)
            sp = H.selected(name, "pool8" if unfused < 16 else "none", unfused if unfused < 16 else 1)
            y0 = C.conv_f32_fwd(xd, wd, bd, g.OH, g.OW, *g.bind(), act=1)
            s0 = H.selected(name, "reduce8" if unfused < 16 else "wave16x4_v4", unfused)
        assert unfused == C.f32_plan(g.N * PH * PW * 4, g.K, Kred, True, g.N * g.OH * g.OW)[2]
        # each launch against the bound of ITS OWN slice count
        _within(y[:, :2 * PH, :2 * PW], yr[:, :2 * PH, :2 * PW], ab[:, :2 * PH, :2 * PW], Kred + sp[2] + 2,
                f"pooled y {g} buf{int(buf)}")
        _within(p, win(yr).max((2, 4)), win(ab).max((2, 4)), Kred + sp[2] + 2, f"pooled maximum {g} buf{int(buf)}")
        _within(y0, yr, ab, Kred + s0[2] + 2, f"unfused y {g} buf{int(buf)}")
        p0, a0 = C.maxpool_fwd(y, 2, 2, 2, 2, 0, 0, PH, PW, False)  # the pool of the y it stored, exactly
        assert torch.equal(p, p0) and torch.equal(arg, a0)
        if unfused < 16:
            assert torch.equal(y[:, :2 * PH, :2 * PW], y0[:, :2 * PH, :2 * PW])


# ------------------------------------------------------------------------------------------- Python wrappers
def _wrapper_data():
    g = Geo(2, 6, 7, 3, 8, 3, 3, pads=(1, 1, 1, 1))
    x, w, b = H.ints((g.N, g.H, g.W, g.C), 3, 61), H.ints((g.R, g.S, g.C, g.K), 3, 62), H.ints((g.K,), 9, 63)
    return g, x, w, b


@pytest.mark.parametrize("pool", [False, True])
def test_wrappers_with_only_the_bias_requiring_a_gradient(pool):
    """The `elif want_db` branch of _conv_backward (through unpool() for the pooled op)."""
    from tensorflow_distributed_learning_amd.ops import conv_f32 as cf

    g, x, w, b = _wrapper_data()
    xt, wt = (torch.tensor(v, dtype=torch.float32, device="cuda") for v in (x, w))
    bt = torch.tensor(b, dtype=torch.float32, device="cuda", requires_grad=True)
    pads = (g.pt, g.pb, g.pl, g.pr)
    out = (cf.conv2d_pool if pool else cf.conv2d)(xt, wt, bt, (1, 1), pads, act=1)
    yr, mx, arg, ab = CR.conv_pool_fwd_ref(x, w.transpose(3, 0, 1, 2), b, g.OH, g.OW, **g.kw)
    CR.assert_exact(ab)
    H.same_bits(out, mx if pool else yr, "wrapper forward")
    dout = H.ints(tuple(out.shape), 5, 64)
    out.backward(torch.tensor(dout, dtype=torch.float32, device="cuda"))
    dy = CR.conv_pool_bwd_ref(dout, mx, arg, g.OH, g.OW) if pool else CR.masked_ref(dout, yr)
    H.same_bits(bt.grad, CR.bias_grad_ref(dy)[0], "wrapper bias gradient")


def test_dense_with_only_the_bias_requiring_a_gradient():
    from tensorflow_distributed_learning_amd.ops import conv_f32 as cf

    x, w, b = H.ints((5, 12), 4, 71), H.ints((12, 7), 4, 72), H.ints((7,), 9, 73)
    xt, wt = (torch.tensor(v, dtype=torch.float32, device="cuda") for v in (x, w))
    bt = torch.tensor(b, dtype=torch.float32, device="cuda", requires_grad=True)
    out = cf.dense(xt, wt, bt, act=1)
    yr = CR.bias_act_ref(x @ w, b, 1)
    H.same_bits(out, yr, "dense forward")
    dout = H.ints((5, 7), 5, 74)
    out.backward(torch.tensor(dout, dtype=torch.float32, device="cuda"))
    H.same_bits(bt.grad, CR.bias_grad_ref(dout, yr)[0], "dense bias gradient")


@pytest.mark.parametrize("pool", [False, True])
def test_wrappers_take_bf16_input_of_exact_integers(pool):
    """bf16 activations of small integers: widened exactly, the output back in bf16, values and gradients
    exact (every value here is an integer below 256, exact in bf16)."""
    from tensorflow_distributed_learning_amd.ops import conv_f32 as cf

    g = Geo(1, 4, 4, 2, 8, 2, 2)
    x, w, b = H.ints((g.N, g.H, g.W, g.C), 2, 81), H.ints((g.R, g.S, g.C, g.K), 2, 82), H.ints((g.K,), 3, 83)
    xt = torch.tensor(x, dtype=torch.bfloat16, device="cuda", requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float32, device="cuda", requires_grad=True)
    bt = torch.tensor(b, dtype=torch.float32, device="cuda", requires_grad=True)
    out = (cf.conv2d_pool if pool else cf.conv2d)(xt, wt, bt, (1, 1), (0, 0, 0, 0), act=1)
    assert out.dtype == torch.bfloat16
    yr, mx, arg, ab = CR.conv_pool_fwd_ref(x, w.transpose(3, 0, 1, 2), b, g.OH, g.OW, **g.kw)
    fwd = mx if pool else yr
    assert np.abs(fwd).max() < 256 and ab.max() < 256
    H.same_bits(out.float(), fwd, "bf16 forward")
    dout = H.ints(tuple(out.shape), 1, 84)
    out.backward(torch.tensor(dout, dtype=torch.bfloat16, device="cuda"))
    dy = CR.conv_pool_bwd_ref(dout, mx, arg, g.OH, g.OW) if pool else CR.masked_ref(dout, yr)
    dx, abx = CR.conv_dgrad_ref(dy, w, g.H, g.W, **g.kw)
    gw, _ = CR.conv_wgrad_ref(x, dy, g.R, g.S, **g.kw)
    assert abx.max() < 256 and xt.grad.dtype == torch.bfloat16
    H.same_bits(xt.grad.float(), dx, "bf16 input gradient")
    H.same_bits(wt.grad, gw, "weight gradient")
    H.same_bits(bt.grad, CR.bias_grad_ref(dy)[0], "bias gradient")


def test_every_convolution_and_pooled_reduce_kernel_has_run():
    names = H.hip().f32_kernel_names()
    pooled = {"pool4", "pool8", "pool16", "pool_rows"}
    mine = [n for n in names if n.split("_")[0] in ("fwd", "dgrad", "wgrad") or n in pooled]
    assert len(mine) == 8 + 20 + 10 + 4 and len(names) == len(mine) + 32 + 9  # (the rest: the GEMM file's)
    missing = [n for n in mine if n not in H.RAN]
    assert not missing, f"never ran: {missing}"
    assert not H.RAN - set(names), H.RAN - set(names)
