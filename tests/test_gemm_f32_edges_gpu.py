"""gemm_f32 (csrc/kernels/gemm_f32.hip, kF32Gemm: every f32 Dense of the generic engine) bit-exactly against
f64 at its edges, through the raw binding: tile edges in M, N and the reduction, all four storages, bias /
ReLU / accumulate / masks / bias gradient, every operand-vectorisation flag (by K % 4, N % 4, operand and
mask misalignment), every split-K reduce kernel, both operand-loader forms (f32_buf), non-finite values,
and one random-data case checked element by element against the derived bound.

Integer data: every partial sum in any order is an integer below 2^24 (assert_exact), so the comparison is
np.array_equal and does not depend on the split plan.  Every case asserts the kernels it was built to reach
(f32_last_selected); the last test asserts that every GEMM kernel and every un-pooled reduce kernel
f32_kernel_names() lists has run (the convolution file does the same for the rest)."""
import itertools

import numpy as np
import pytest
import torch

import conv_refs as CR
import f32_edge_helpers as H

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 129]
KS = [1, 3, 4, 15, 16, 17, 63, 64, 65]
FACTORS = ("M", "N", "K", "ta", "tb", "bias", "act", "out", "amask", "bmask", "dbias")


def _table():
    """Every (M, N, K) of the edge sizes, the other factors drawn from a fixed stream: all pairs of factor
    levels occur (test_table_covers_all_pairs).  out: 0 a fresh tensor, 1 a caller tensor, 2 accumulated
    into.  (The binding refuses dbias with an activation.)"""
    rng = np.random.RandomState(5)
    rows = []
    for M, N, K in itertools.product(SIZES, SIZES, KS):
        ta, tb, bias, act, amask, bmask, dbias = (int(v) for v in rng.randint(0, 2, 7))
        out = int(rng.randint(0, 3))
        if dbias and act:
            act = 0 if rng.randint(0, 2) else act
            dbias = 0 if act else dbias
        rows.append(dict(M=M, N=N, K=K, ta=ta, tb=tb, bias=bias, act=act, out=out, amask=amask, bmask=bmask,
                         dbias=dbias))
    return rows


TABLE = _table()


def test_table_covers_all_pairs():
    seen = set()
    for r in TABLE:
        for a, b in itertools.combinations(FACTORS, 2):
            seen.add((a, r[a], b, r[b]))
    levels = {f: sorted({r[f] for r in TABLE}) for f in FACTORS}
    assert levels["out"] == [0, 1, 2] and all(levels[f] == [0, 1] for f in FACTORS[3:] if f != "out")
    missing = [(a, x, b, y) for a, b in itertools.combinations(FACTORS, 2) for x in levels[a] for y in levels[b]
               if (a, x, b, y) not in seen and not ({a, b} == {"act", "dbias"} and x == 1 and y == 1)]
    assert not missing, missing
    assert len(TABLE) == 5 * 5 * 9


@pytest.mark.parametrize("M", SIZES)
def test_gemm_edge_table(M):
    """M = 63 with dbias: the row of ones fills the tile; M = 64: it is alone in a second tile."""
    for i, r in enumerate(TABLE):
        if r["M"] != M:
            continue
        for buf in (True, False):
            H.run_gemm(M, r["N"], r["K"], r["ta"], r["tb"], bool(r["bias"]), r["act"], r["out"] == 2, bool(r["amask"]),
                       bool(r["bmask"]), bool(r["dbias"]), out=True if r["out"] else None, buf=buf, salt=i)


@pytest.mark.parametrize("ma,mb", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_gemm_vector_flags_toggle_separately(ma, mb):
    """VA needs K % 4 == 0, [M][K] storage, an aligned operand and an aligned mask; VB the same of N and
    [K][N] storage.  Each condition is broken on its own, the other operand in each of its states, so all
    16 x 2 GEMM kernels run and every scalar loader is reached with a multiple-of-4 size."""
    a_vars = [dict(), dict(K=18), dict(mis_a=True), dict(ta=1)] + ([dict(mis_am=True)] if ma else [])
    b_vars = [dict(), dict(N=66), dict(mis_b=True), dict(tb=0)] + ([dict(mis_bm=True)] if mb else [])
    for i, (av, bv) in enumerate(itertools.product(a_vars, b_vars)):
        kw = dict(M=65, N=68, K=20, ta=0, tb=1, amask=bool(ma), bmask=bool(mb), bias=bool(i & 1), dbias=bool(i & 2))
        kw.update(av)
        kw.update(bv)
        for buf in (True, False):
            H.run_gemm(buf=buf, salt=100 + i, **kw)


# (M, N, K, splits, reduce kernel, options)
SPLITS = [
    (5, 5, 257, 5, "reduce8", dict(bias=True, act=1)),
    (5, 5, 513, 9, "reduce16", dict(acc=True, dbias=True)),
    (5, 5, 1025, 17, "wave", dict(bias=True, amask=True)),
    (5, 5, 4481, 71, "wave", dict(ta=1, tb=0, dbias=True)),          # lanes 0..6 sum two slices
    (16, 16, 1025, 17, "wave16x4_v4", dict(bias=True, act=1, bmask=True)),
    (17, 17, 1025, 17, "wave16x4_s", dict(acc=True, bias=True)),     # 289 outputs: the last wave holds one
    (128, 64, 1025, 17, "wave16x16_v4", dict(bias=True, acc=True, act=1)),
    (127, 65, 1025, 17, "wave16x16_s", dict(ta=1, amask=True)),
    (128, 64, 4481, 71, "wave16x16_v4", dict(dbias=True, bias=True)),  # 71 slices, the ones row in tile 3
    (1, 1, 70000, 875, "wave", dict(bias=True)),                     # 875 slices of 80
    (16384, 8, 260, 4, "reduce4", dict(bias=True, act=1)),           # 256 tiles
]


@pytest.mark.parametrize("case", SPLITS, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in SPLITS])
def test_gemm_split_reduces(case):
    M, N, K, splits, reduce, opt = case
    for buf in (True, False):
        H.run_gemm(M, N, K, buf=buf, salt=200, reduce=reduce, splits=splits, **opt)
        if reduce.startswith("wave16"):
            _one_wave(M, N, K, splits, reduce, buf)


def _one_wave(M, N, K, splits, reduce, buf):
    """f32_reduce16(False): one wave per output, the same lanes and butterfly as the 4 / 16-output kernels:
    the same bits."""
    C = H.hip()
    amp = H.amp_of(K)
    A, B = H.ints((M, K), amp, 301), H.ints((K, N), amp, 302)
    CR.assert_exact(np.abs(A) @ np.abs(B))
    a_d, b_d = H.dev(A), H.dev(B)
    name = f"gemm_ma0_mb0_va{H.b01(K % 4 == 0)}_vb{H.b01(N % 4 == 0)}_buf{H.b01(buf)}"
    outs = []
    for on in (True, False):
        with H.hooks(buf=buf, narrow=True, hoist=True, reduce16=on):
            outs.append(C.gemm_f32(a_d, 0, b_d, 1))
        H.selected(name, reduce if on else "wave", splits)
    assert torch.equal(outs[0], outs[1])
    H.same_bits(outs[1], A @ B, f"gemm {M}x{N}x{K} one wave per output")


@pytest.mark.parametrize("buf", [True, False])
def test_gemm_reduce16_on_fewer_than_nine_slices(buf):
    """f32_reduce_narrow(False): the 16-load reduce whatever the slice count."""
    C = H.hip()
    A, B = H.ints((5, 257), 3, 1), H.ints((257, 5), 3, 2)
    a_d, b_d = H.dev(A), H.dev(B)
    got = {}
    for narrow in (True, False):
        with H.hooks(buf=buf, narrow=narrow, hoist=True, reduce16=True):
            got[narrow] = C.gemm_f32(a_d, 0, b_d, 1)
        H.selected(f"gemm_ma0_mb0_va0_vb0_buf{H.b01(buf)}", "reduce8" if narrow else "reduce16", 5)
    CR.assert_exact(np.abs(A) @ np.abs(B))
    H.same_bits(got[False], A @ B, "reduce16 over 5 slices")
    assert torch.equal(got[True], got[False])


# ------------------------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize("buf", [True, False])
def test_gemm_single_nan_reaches_exactly_its_row_and_column(buf):
    def nan_a(A, B, AM, BM):
        A[64, 16] = np.nan  # the corner: the only row of tile 2, the last reduction element

    got = H.run_gemm(65, 65, 17, buf=buf, salt=400, poke=nan_a, bias=True)
    bad = torch.isnan(got).cpu().numpy()
    assert bad[64].all() and not bad[:64].any()

    def nan_b(A, B, AM, BM):
        B[0, 64] = np.nan

    got = H.run_gemm(65, 65, 17, ta=1, tb=0, buf=buf, salt=401, poke=nan_b, dbias=True)
    bad = torch.isnan(got).cpu().numpy()
    assert bad[:, 64].all() and not bad[:, :64].any()


@pytest.mark.parametrize("buf", [True, False])
def test_gemm_nan_preactivation_is_zero_under_relu_and_nan_without(buf):
    def nan_a(A, B, AM, BM):
        A[3, 2] = np.nan

    got = H.run_gemm(9, 7, 5, buf=buf, salt=410, poke=nan_a, bias=True, act=1)  # (the reference is fmaxf's)
    assert (got[3] == 0).all() and not torch.isnan(got).any()
    got = H.run_gemm(9, 7, 5, buf=buf, salt=410, poke=nan_a, bias=True, act=0)
    assert torch.isnan(got[3]).all() and not torch.isnan(got[:3]).any()


@pytest.mark.parametrize("buf", [True, False])
def test_gemm_masks_select_rather_than_multiply(buf):
    """Inf / NaN operands under a mask <= 0, a -0 mask or a NaN mask contribute an exact 0."""
    def poke(A, B, AM, BM):
        for i, m in enumerate((0.0, -1.0, np.nan, -0.0)):
            A[i, i] = np.inf if i & 1 else np.nan
            AM[i, i] = m
            B[i + 1, i] = -np.inf
            BM[i + 1, i] = m

    for ta, tb, K in ((0, 1, 8), (1, 0, 7)):
        got = H.run_gemm(6, 8, K, ta=ta, tb=tb, buf=buf, salt=420, poke=poke, amask=True, bmask=True, dbias=True)
        assert torch.isfinite(got).all()


# ------------------------------------------------------------------------------------------- real data
@pytest.mark.parametrize("shape", [(65, 63, 70, 1), (33, 17, 1025, 17), (130, 64, 1030, 17)])
def test_gemm_random_data_within_the_derived_bound_elementwise(shape):
    """randn operands, every output within error_bound_f32(sum |a||b| + |bias| + |prior|, K + splits + 2):
    the roundings any output can see -- the products' additions, the slice sum, the bias and the
    accumulate."""
    M, N, K, splits = shape
    C = H.hip()
    rng = np.random.RandomState(K)
    A, B = rng.randn(M, K).astype(np.float32), rng.randn(K, N).astype(np.float32)
    bias, prior = rng.randn(N).astype(np.float32), rng.randn(M, N).astype(np.float32)
    want = A.astype(np.float64) @ B.astype(np.float64) + bias + prior
    ab = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64) + np.abs(bias) + np.abs(prior)
    for buf in (True, False):
        out = H.Guarded(prior)
        with H.hooks(buf=buf, narrow=True, hoist=True, reduce16=True):
            got = C.gemm_f32(H.dev(A), 0, H.dev(B), 1, bias=H.dev(bias), out=out.view, accumulate=True)
        H.selected(f"gemm_ma0_mb0_va{H.b01(K % 4 == 0)}_vb{H.b01(N % 4 == 0)}_buf{H.b01(buf)}", None, splits)
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        bound = CR.error_bound_f32(ab, K + splits + 2)
        print(f"\ngemm {M}x{N}x{K}: largest error / bound {np.max(err / bound):.4f}")
        assert np.all(err <= bound), np.max(err / bound)
        out.check("random gemm")


def test_every_gemm_and_reduce_kernel_has_run():
    names = H.hip().f32_kernel_names()
    pooled = {"pool4", "pool8", "pool16", "pool_rows"}
    mine = [n for n in names if n.startswith("gemm_") or (n.split("_")[0] not in ("fwd", "dgrad", "wgrad", "gemm")
                                                          and n not in pooled)]
    assert len([n for n in mine if n.startswith("gemm_")]) == 32 and len(mine) == 32 + 9
    # the convolution file answers for every other name: together, all of f32_kernel_names()
    rest = [n for n in names if n not in mine]
    assert all(n.split("_")[0] in ("fwd", "dgrad", "wgrad") or n in pooled for n in rest)
    missing = [n for n in mine if n not in H.RAN]
    assert not missing, f"never ran: {missing}"
    assert not H.RAN - set(names), H.RAN - set(names)
