"""Classifier-head kernels (csrc/kernels/gemm.hip, ops/dense.py) vs f64 references with derived bounds
(and the older float32 PyTorch comparisons): bf16 MFMA GEMM in all four operand storages, contiguous and
strided, NHWC global average pooling, sparse softmax cross-entropy (per-example and the fused loss head), and
the Dense layer's forward/backward incl. direct gradient-slab accumulation."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_refs as R

pytestmark = pytest.mark.gpu


def _r(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).cuda()


def _assert_within(got, ref, bound, what):
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)  # (a NaN is bad)
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, first at {i}: "
                             f"got {got[i].item()!r}, f64 reference {ref[i].item()!r}, bound {bound[i].item():.3e}")


def _gemm_bound(K, mag, ref=None, bf16_out=False):
    """Products of bf16 values are exact in f32, so only the f32 accumulation and the epilogue round:
    |err| <= (K + 4) 2^-23 (|alpha| |A| |B| + |bias| + |out0|) (= mag), plus the output's bf16 rounding."""
    b = (K + 4) * 2.0 ** -23 * mag
    return b + 2.0 ** -8 * ref.abs() if bf16_out else b


@pytest.mark.parametrize("ta", [0, 1])
@pytest.mark.parametrize("tb", [0, 1])
@pytest.mark.parametrize("mnk", [(256, 1000, 2048), (136, 200, 40), (8, 8, 8), (264, 1032, 1000)])
def test_gemm_bf16_all_storages(ta, tb, mnk):
    from tensorflow_distributed_learning_amd.ops import hip

    C = hip()
    M, N, K = mnk
    A = _r(M, K, seed=1).bfloat16()
    B = _r(K, N, seed=2).bfloat16()
    a = A.t().contiguous() if ta else A  # stored [K][M] when ta = 1
    b = B.contiguous() if tb else B.t().contiguous()  # stored [K][N] when tb = 1, [N][K] when 0
    ref, mag = A.double() @ B.double(), A.double().abs() @ B.double().abs()
    bias = _r(N, seed=3)
    y = C.gemm_bf16(a, ta, b, tb, bias=bias)
    assert y.dtype == torch.bfloat16 and y.shape == (M, N)
    _assert_within(y, ref + bias, _gemm_bound(K, mag + bias.abs(), ref + bias, bf16_out=True), "bf16 + bias")
    out = torch.full((M, N), 0.5, device="cuda")
    C.gemm_bf16(a, ta, b, tb, out=out, accumulate=True, alpha=2.0)
    _assert_within(out, 0.5 + 2 * ref, _gemm_bound(K, 2 * mag + 0.5), "f32 accumulate")


def test_gap_fwd_bwd():
    from tensorflow_distributed_learning_amd.ops.dense import gap_nhwc

    x = _r(16, 7, 7, 2048).bfloat16().requires_grad_(True)
    y = gap_nhwc(x)
    xr = x.detach().float().requires_grad_(True)
    yr = xr.mean(dim=(1, 2))
    torch.testing.assert_close(y.float(), yr, atol=1e-2, rtol=1e-2)
    dy = _r(16, 2048, seed=4).bfloat16()
    y.backward(dy)
    yr.backward(dy.float())
    torch.testing.assert_close(x.grad.float(), xr.grad, atol=1e-3, rtol=1e-2)


def test_softmax_xent_matches_cross_entropy():
    from tensorflow_distributed_learning_amd.ops.dense import softmax_xent

    z = (_r(256, 1000) * 3).requires_grad_(True)
    y = torch.randint(0, 1000, (256,), device="cuda")
    l = softmax_xent(z, y)
    zr = z.detach().clone().requires_grad_(True)
    lr = F.cross_entropy(zr, y, reduction="none")
    torch.testing.assert_close(l, lr, atol=1e-5, rtol=1e-5)
    w = _r(256, seed=5)
    (l * w).sum().backward()
    (lr * w).sum().backward()
    torch.testing.assert_close(z.grad, zr.grad, atol=1e-6, rtol=1e-4)


def test_dense_layer_bf16_and_slab_targets():
    from tensorflow_distributed_learning_amd.ops.dense import dense_bf16

    x = _r(64, 512).bfloat16().requires_grad_(True)
    w = (_r(512, 1000, seed=6) * 0.05).bfloat16().requires_grad_(True)
    b = _r(1000, seed=7).requires_grad_(True)
    y = dense_bf16(x, w, b)
    xr, wr, br = (t.detach().float().requires_grad_(True) for t in (x, w, b))
    yr = xr @ wr + br
    torch.testing.assert_close(y.float(), yr, atol=3e-2, rtol=2e-2)
    dy = _r(64, 1000, seed=8).bfloat16()
    y.backward(dy)
    yr.backward(dy.float())
    torch.testing.assert_close(x.grad.float(), xr.grad, atol=5e-2, rtol=2e-2)
    torch.testing.assert_close(w.grad.float(), wr.grad, atol=5e-2, rtol=2e-2)
    torch.testing.assert_close(b.grad, br.grad, atol=1e-3, rtol=1e-3)
    # slab targets: gradients ADDED into f32 views, none returned
    gw, gb = torch.ones(512, 1000, device="cuda"), torch.ones(1000, device="cuda")
    x2 = x.detach().requires_grad_(True)
    y2 = dense_bf16(x2, w.detach(), b.detach(), (gw, gb))
    y2.backward(dy)
    torch.testing.assert_close(gw, 1 + wr.grad, atol=2e-2, rtol=1e-2)
    torch.testing.assert_close(gb, 1 + br.grad, atol=1e-3, rtol=1e-3)
    torch.testing.assert_close(x2.grad, x.grad)


# ------------------------------------------------------------------------------------- gemm_bf16 at the edges
GEMM_SHAPES = [(8, 8, 8), (136, 136, 72), (128, 128, 64), (128, 136, 128), (264, 8, 192), (8, 264, 200)]
BF16_PAD = 2.0 ** 10  # outside the strided operands: a read past a row's logical width shows in the result
F32_PAD_BITS = 0x4B1D5EED


def _stored(logical, transposed, strided):
    """The operand as stored ([K][rows] when transposed), contiguous or as the 16-byte-aligned column view
    wide[:, 8 : 8 + cols] of a wider matrix (leading dimension = cols + 16)."""
    st = logical.t().contiguous() if transposed else logical.contiguous()
    if not strided:
        return st
    wide = torch.full((st.shape[0], st.shape[1] + 16), BF16_PAD, dtype=torch.bfloat16, device="cuda")
    view = wide[:, 8:8 + st.shape[1]]
    view.copy_(st)
    assert view.stride(0) == st.shape[1] + 16 and view.data_ptr() % 16 == 0
    return view


def _f32_out(M, N, strided, fill):
    """(out view [M][N], its whole buffer): strided = columns 4 .. 4 + N of an [M][N + 8] sentinel matrix."""
    if not strided:
        o = torch.full((M, N), fill, device="cuda")
        return o, o
    wide = torch.full((M, N + 8), F32_PAD_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    view = wide[:, 4:4 + N]
    view.fill_(fill)
    return view, wide


def _assert_pad_untouched(wide, N):
    w = wide.view(torch.int32)
    assert (w[:, :4] == F32_PAD_BITS).all() and (w[:, 4 + N:] == F32_PAD_BITS).all(), "gemm wrote outside out"


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("ta", [0, 1])
@pytest.mark.parametrize("tb", [0, 1])
@pytest.mark.parametrize("mnk", GEMM_SHAPES)
def test_gemm_bf16_edges_against_f64(mnk, tb, ta, strided):
    from tensorflow_distributed_learning_amd.ops import hip

    C = hip()
    M, N, K = mnk
    A = _r(M, K, seed=11).bfloat16()
    B = _r(K, N, seed=12).bfloat16()
    a = _stored(A, ta == 1, strided)        # [M][K], or [K][M] when ta = 1
    b = _stored(B, tb == 0, strided)        # [K][N] when tb = 1, [N][K] when 0
    ref, mag = A.double() @ B.double(), A.double().abs() @ B.double().abs()
    bias = _r(N, seed=13)
    # bf16 output, bias, alpha = 0.5
    y = C.gemm_bf16(a, ta, b, tb, bias=bias, alpha=0.5)
    assert y.dtype == torch.bfloat16 and y.shape == (M, N) and y.is_contiguous()
    want = 0.5 * ref + bias
    _assert_within(y, want, _gemm_bound(K, 0.5 * mag + bias.abs(), want, bf16_out=True), "bf16 out, bias, alpha 0.5")
    # f32 out, overwritten: starts as NaN so that an element the kernel does not write shows
    out, whole = _f32_out(M, N, strided, float("nan"))
    r = C.gemm_bf16(a, ta, b, tb, out=out, accumulate=False)
    assert r.data_ptr() == out.data_ptr()
    _assert_within(out, ref, _gemm_bound(K, mag), "f32 out, no accumulate")
    if strided:
        _assert_pad_untouched(whole, N)
    # f32 out, accumulated onto 0.75 with alpha = 2 and a bias
    out, whole = _f32_out(M, N, strided, 0.75)
    C.gemm_bf16(a, ta, b, tb, bias=bias, out=out, accumulate=True, alpha=2.0)
    want = 0.75 + 2 * ref + bias
    _assert_within(out, want, _gemm_bound(K, 2 * mag + bias.abs() + 0.75), "f32 out, accumulate, alpha 2, bias")
    if strided:
        _assert_pad_untouched(whole, N)
        for t in (a, b):
            assert (t._base[:, :8] == BF16_PAD).all() and (t._base[:, 8 + t.shape[1]:] == BF16_PAD).all()


def test_gemm_bf16_output_keeps_nan():
    """A NaN in the f32 epilogue value (here from the bias, with payloads the integer round-to-nearest-even
    sequence carries out of) must be a NaN in the bf16 output, not Inf or zero."""
    from tensorflow_distributed_learning_amd.ops import hip

    A, B = _r(8, 8, seed=14).bfloat16(), _r(8, 16, seed=15).bfloat16()
    bias = torch.zeros(16)
    bias[[1, 6, 11]] = torch.from_numpy(R.NAN_PAYLOADS_F32.copy())
    y = hip().gemm_bf16(A, 0, B.contiguous(), 1, bias=bias.cuda())
    nan = y.isnan().cpu()
    assert nan[:, [1, 6, 11]].all(), f"bf16 bits of row 0: {[hex(v & 0xFFFF) for v in y[0].view(torch.int16).tolist()]}"
    assert int(nan.sum()) == 3 * 8


def test_gemm_bf16_rejects_bad_sizes():
    from tensorflow_distributed_learning_amd.ops import hip

    C = hip()
    ok = torch.zeros(8, 8, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="multiples of 8"):  # M = 12
        C.gemm_bf16(torch.zeros(12, 8, dtype=torch.bfloat16, device="cuda"), 0, ok, 0)
    with pytest.raises(RuntimeError, match="multiples of 8"):  # N = 12
        C.gemm_bf16(ok, 0, torch.zeros(12, 8, dtype=torch.bfloat16, device="cuda"), 0)
    with pytest.raises(RuntimeError):  # K = 12 (the rows are then not 16-byte aligned either)
        C.gemm_bf16(torch.zeros(8, 12, dtype=torch.bfloat16, device="cuda"), 0,
                    torch.zeros(8, 12, dtype=torch.bfloat16, device="cuda"), 0)
    with pytest.raises(RuntimeError, match="multiples of 8"):  # M = 0
        C.gemm_bf16(torch.zeros(0, 8, dtype=torch.bfloat16, device="cuda"), 0, ok, 0)
    torch.cuda.synchronize()
    assert (torch.ones(4, device="cuda") + 1).sum().item() == 8.0


# ------------------------------------------------------------------------------------- global average pooling
GAP_SHAPES = [(1, 1, 1, 8), (5, 3, 5, 24), (33, 2, 2, 64), (3, 7, 7, 2048), (2, 5, 10, 16)]


def _gap_fwd_bound(x64, ref):
    hw = x64.shape[1] * x64.shape[2]
    return 2.0 ** -8 * ref.abs() + hw * 2.0 ** -23 * x64.abs().mean(dim=(1, 2))


@pytest.mark.parametrize("shape", GAP_SHAPES, ids=str)
def test_gap_fwd_against_f64(shape):
    from tensorflow_distributed_learning_amd.ops import hip

    x = (_r(*shape, seed=21) + 0.5).bfloat16()
    y = hip().gap_fwd(x)
    assert y.shape == (shape[0], shape[3]) and y.dtype == torch.bfloat16
    ref = x.double().mean(dim=(1, 2))
    _assert_within(y, ref, _gap_fwd_bound(x.double(), ref), "gap_fwd")


# (32, 14, 14, 1536): the smallest shape whose N HW C / 8 exceeds the 256 * 16 * 256 threads of the grid
@pytest.mark.parametrize("shape", GAP_SHAPES + [(32, 14, 14, 1536)], ids=str)
def test_gap_bwd_against_f64(shape):
    from tensorflow_distributed_learning_amd.ops import hip

    n, h, w, c = shape
    dy = _r(n, c, seed=22).bfloat16()
    dx = hip().gap_bwd(dy, h, w)
    assert dx.shape == shape and dx.dtype == torch.bfloat16
    ref = (dy.double() / (h * w))[:, None, None, :].expand(shape)
    _assert_within(dx, ref, 2.0 ** -8 * ref.abs(), "gap_bwd")


def test_gap_nhwc_autograd_against_f64():
    from tensorflow_distributed_learning_amd.ops.dense import gap_nhwc

    shape = (5, 3, 5, 24)
    x = (_r(*shape, seed=23) + 0.5).bfloat16().requires_grad_(True)
    y = gap_nhwc(x)
    ref = x.detach().double().mean(dim=(1, 2))
    _assert_within(y.detach(), ref, _gap_fwd_bound(x.detach().double(), ref), "gap_nhwc")
    dy = _r(5, 24, seed=24).bfloat16()
    y.backward(dy)
    rg = (dy.double() / 15)[:, None, None, :].expand(shape)
    _assert_within(x.grad, rg, 2.0 ** -8 * rg.abs(), "gap_nhwc backward")


def test_gap_keeps_nan():
    from tensorflow_distributed_learning_amd.ops import hip

    x = _r(2, 3, 3, 16, seed=25).bfloat16()
    x[0, 1, 1, 3] = float("nan")
    x[1, 0, 0, 5], x[1, 2, 2, 5] = float("inf"), float("-inf")  # Inf - Inf
    xb = x.view(torch.int16)
    xb[0, 0, 0, 9], xb[1, 1, 1, 0] = 0x7FFF, -1  # all-ones payloads, both signs
    y = hip().gap_fwd(x).cpu()
    want = torch.zeros(2, 16, dtype=torch.bool)
    want[0, 3] = want[1, 5] = want[0, 9] = want[1, 0] = True
    assert torch.equal(y.isnan(), want)
    dy = _r(2, 16, seed=26).bfloat16()
    dy.view(torch.int16)[0, 2], dy.view(torch.int16)[1, 7] = 0x7FFF, -1
    dx = hip().gap_bwd(dy, 3, 3).cpu()
    assert torch.equal(dx.isnan(), dy.isnan().cpu()[:, None, None, :].expand(2, 3, 3, 16))


def test_gap_empty_batch():
    from tensorflow_distributed_learning_amd.ops import hip

    y = hip().gap_fwd(torch.zeros(0, 7, 7, 16, dtype=torch.bfloat16, device="cuda"))
    dx = hip().gap_bwd(torch.zeros(0, 16, dtype=torch.bfloat16, device="cuda"), 7, 7)
    torch.cuda.synchronize()
    assert y.shape == (0, 16) and y.dtype == torch.bfloat16 and dx.shape == (0, 7, 7, 16) and dx.dtype == torch.bfloat16
    assert (torch.ones(4, device="cuda") + 1).sum().item() == 8.0


# ------------------------------------------------------------------------------------- softmax cross-entropy
# (1024, 64), (1025, 64), (1100, 64): 65536, 65600 and 70400 logits, on both sides of xent_head's switch from
# one workgroup to k_xent_rows + k_xent_finish (the last two with more rows than k_xent_finish has threads)
XENT_SHAPES = [(1, 1), (1, 2), (5, 64), (4, 65), (7, 1000), (9, 129), (1024, 64), (1025, 64), (1100, 64)]
XENT_FAMILIES = ["randn3", "randn30", "offset1e4", "dupmax"]


@functools.lru_cache(maxsize=None)
def _xent_case(N, K, family):
    """Logits, labels, the f64 reference and the tolerances of one case, from the CPU alone.  At least 64
    rows are drawn and the kernels get the first N: the tolerance is 4 E + one f32 ulp with E = the largest
    error of the f32 emulation (kernel_refs.xent_emul_f32) over the drawn rows, and over 1 or 5 rows a
    maximum would understate what f32 arithmetic in this order costs."""
    rng = np.random.default_rng(1000 * N + K)
    Mr = max(N, 64)
    z = rng.standard_normal((Mr, K))
    z = {"randn3": z * 3, "randn30": z * 30, "offset1e4": z + 1e4, "dupmax": z * 3}[family].astype(np.float32)
    y = rng.integers(0, K, Mr)
    if family == "dupmax" and K >= 2:
        for r in range(Mr):  # the row's maximum at two indices i < j; the label on either
            i, j = sorted(rng.choice(K, 2, replace=False))
            z[r, i] = z[r, j] = z[r].max() + np.float32(1.0)
            y[r] = i if r % 2 == 0 else j
    if N >= 4:
        y[1], y[2] = -1, K  # out of range
    loss, lse, p, dz = R.xent_ref(z, y)
    el, elg, edz = R.xent_emul_f32(z, y)
    e_loss, e_lse, e_dz = np.abs(el - loss).max(), np.abs(elg - lse).max(), np.abs(edz - dz).max()
    valid = (y >= 0) & (y < K)
    zy = np.where(valid, z[np.arange(Mr), np.where(valid, y, 0)], 0.0).astype(np.float64)
    tol = {
        # the loss is the difference of two f32 numbers: one ulp of the larger of them (and of itself)
        "loss": 4 * e_loss + R.ulp32(np.maximum(np.maximum(np.abs(lse), np.abs(zy)), np.abs(loss))),
        "lse": 4 * e_lse + R.ulp32(lse),
        "dz": 4 * e_dz + R.ulp32(np.maximum(p, np.abs(dz))),
    }
    correct = valid & (z.argmax(axis=1) == y)  # numpy's argmax: the first index of a duplicated maximum
    ref = {"loss": loss, "lse": lse, "dz": dz, "correct": correct}
    emax = {"loss": e_loss, "lse": e_lse, "dz": e_dz}
    return z[:N], y[:N], {k: v[:N] for k, v in ref.items()}, {k: v[:N] for k, v in tol.items()}, emax


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


@pytest.mark.parametrize("family", XENT_FAMILIES)
@pytest.mark.parametrize("nk", XENT_SHAPES, ids=str)
def test_xent_fwd_bwd_against_f64(nk, family):
    from tensorflow_distributed_learning_amd.ops import hip

    N, K = nk
    z, y, ref, tol, emax = _xent_case(N, K, family)
    zt, yt = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    loss, lse = hip().xent_fwd(zt, yt)
    print(f"xent {nk} {family}: emulation max err loss {emax['loss']:.3e} lse {emax['lse']:.3e} dz {emax['dz']:.3e}")
    _assert_within(loss, _t64(ref["loss"]), _t64(tol["loss"]), "loss")
    _assert_within(lse, _t64(ref["lse"]), _t64(tol["lse"]), "lse")
    invalid = torch.from_numpy((y < 0) | (y >= K)).cuda()
    assert (loss[invalid] == 0).all(), "a label outside [0, K) contributes no loss"
    g = torch.from_numpy(np.random.default_rng(N + K).standard_normal(N).astype(np.float32)).cuda()
    dz = hip().xent_bwd(zt, yt, g)
    want = _t64(ref["dz"]) * g.double()[:, None]
    # (dz * g: the tolerance scales with |g|, plus the rounding of that product)
    bound = _t64(tol["dz"]) * g.double().abs()[:, None] + _t64(R.ulp32(want.cpu().numpy()))
    _assert_within(dz, want, bound, "dz")


@pytest.mark.parametrize("family", XENT_FAMILIES)
@pytest.mark.parametrize("nk", XENT_SHAPES, ids=str)
def test_xent_head_against_f64(nk, family):
    from tensorflow_distributed_learning_amd.ops import hip

    N, K = nk
    z, y, ref, tol, _ = _xent_case(N, K, family)
    zt, yt = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    gn = 2 * N + 3
    accs = [torch.tensor([v], dtype=torch.float64, device="cuda") for v in (10.0, 3.0, 1.0, 2.0)]
    loss, dz = hip().xent_head(zt, yt, float(gn), *accs)
    total, total_tol = ref["loss"].sum(), tol["loss"].sum()
    # rows are summed in f64; the result is rounded to f32 once
    assert abs(loss.item() - total / gn) <= total_tol / gn + R.ulp32(total / gn), (loss.item(), total / gn)
    assert abs(accs[0].item() - (10.0 + total)) <= total_tol
    ncorrect = int(ref["correct"].sum())
    assert accs[1].item() == 3.0 + N and accs[2].item() == 1.0 + ncorrect and accs[3].item() == 2.0 + N
    want = _t64(ref["dz"]) / gn
    # (dz * f32(1 / gn): one more ulp for the rounded reciprocal and the product)
    _assert_within(dz, want, _t64(tol["dz"]) / gn + _t64(R.ulp32(want.cpu().numpy())), "dz")


def test_xent_head_counts_first_index_of_a_tie_and_skips_bad_labels():
    from tensorflow_distributed_learning_amd.ops import hip

    K = 70
    z = np.zeros((6, K), dtype=np.float32)
    z[:, 3] = z[:, 66] = 5.0  # the maximum twice, in different 64-lane trips
    y = np.array([3, 66, -1, K, 3, 0])
    accs = [torch.zeros(1, dtype=torch.float64, device="cuda") for _ in range(4)]
    loss, dz = hip().xent_head(torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda(), 6.0, *accs)
    assert accs[2].item() == 2.0 and accs[3].item() == 6.0 and accs[1].item() == 6.0  # rows 0 and 4 only
    _, _, p, rdz = R.xent_ref(z, y)
    np.testing.assert_allclose(dz.cpu().numpy()[2:4] * 6.0, p[2:4], rtol=1e-5, atol=1e-7)  # softmax, no one-hot
    np.testing.assert_allclose(dz.cpu().numpy() * 6.0, rdz, rtol=1e-5, atol=1e-7)


def test_xent_bwd_rejects_cpu_labels():
    from tensorflow_distributed_learning_amd.ops import hip

    z = torch.zeros(4, 10, device="cuda")
    with pytest.raises(RuntimeError, match="GPU labels"):
        hip().xent_bwd(z, torch.zeros(4, dtype=torch.int64), torch.ones(4, device="cuda"))


def test_xent_empty_batch():
    from tensorflow_distributed_learning_amd.ops import hip

    z = torch.zeros(0, 10, device="cuda")
    y = torch.zeros(0, dtype=torch.int64, device="cuda")
    loss, lse = hip().xent_fwd(z, y)
    dz = hip().xent_bwd(z, y, torch.zeros(0, device="cuda"))
    torch.cuda.synchronize()
    assert loss.shape == (0,) and lse.shape == (0,) and dz.shape == (0, 10) and dz.dtype == torch.float32
    assert (torch.ones(4, device="cuda") + 1).sum().item() == 8.0
