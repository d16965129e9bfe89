"""Synchronized batch-norm kernels (csrc/kernels/bn.hip: k_bn_sync_pack, k_bn_sync_fwd_finalize,
k_bn_sync_bwd_finalize) in one process: a batch is cut into R unequal row chunks, each chunk is packed
as replica r would, the all-reduce is the sum of the R exchange buffers, and every chunk is finalized
from that sum.  The concatenated results must be the batch norm of the WHOLE batch (float64 reference)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MOM, EPS = 0.9, 1e-3
RS, MS, CS = [2, 3, 8], [9, 300], [8, 72, 136]
DTYPES = [torch.float32, torch.bfloat16]
U = 2.0 ** -24  # f32 unit roundoff


def _hip():
    from tensorflow_distributed_learning_amd.ops import hip

    return hip()


def _sizes(M, R):
    """R unequal chunk sizes summing to M, the first one a single row."""
    rest, k = M - 1, R - 1
    w = list(range(1, k + 1))
    s = [1 + (rest - k) * wi // sum(w) for wi in w]
    s[-1] += rest - sum(s)
    out = [1] + s
    assert sum(out) == M and min(out) >= 1 and len(out) == R
    return out


def _chunks(t, M, R):
    return list(torch.split(t, _sizes(M, R), dim=0))


@functools.lru_cache(maxsize=None)
def _case(M, C, dtype, mode):
    """Inputs and the float64 reference of one shape (computed once, shared, never modified):
    mode 0 y = bn(x), 1 relu(bn(x)), 2 relu(bn(x) + res)."""
    gen = torch.Generator(device="cpu").manual_seed(1000 * M + 10 * C + mode)
    x = (torch.randn(M, C, generator=gen) * 2 + 0.5).to(dtype).to(DEV)
    res = torch.randn(M, C, generator=gen).to(dtype).to(DEV)
    g = (torch.rand(C, generator=gen) + 0.5).to(DEV)
    b = torch.randn(C, generator=gen).to(DEV)
    mm, mv = torch.randn(C, generator=gen).to(DEV), (torch.rand(C, generator=gen) + 0.5).to(DEV)
    dy = torch.randn(M, C, generator=gen).to(dtype).to(DEV)
    x64 = x.double().requires_grad_(True)
    g64, b64 = g.double().requires_grad_(True), b.double().requires_grad_(True)
    mm64, mv64 = mm.double().clone(), mv.double().clone()
    z = F.batch_norm(x64, mm64, mv64, g64, b64, training=True, momentum=1 - MOM, eps=EPS)
    if mode == 2:
        z = z + res.double()
    y64 = F.relu(z) if mode else z
    if mode:
        # where the pre-activation is within 1e-3 of zero the f32 kernels may take the other side of the
        # ReLU than float64 does: no gradient arrives there, so either side gives the same result
        dy = torch.where(z.detach().abs() < 1e-3, torch.zeros_like(dy), dy)
    y64.backward(dy.double())
    xd = x.double()
    mu = xd.mean(0)
    var = xd.var(0, unbiased=False)
    inv = torch.rsqrt(var + EPS)
    st64 = torch.stack([mu, inv, g.double() * inv, b.double() - mu * g.double() * inv])
    # worst-case error of the f32 accumulation of M terms (the partial pass), propagated: the bound on
    # each statistic, from the data alone
    e_mu = 2 * M * U * xd.abs().mean(0) + U * mu.abs()
    e_var = 2 * M * U * (xd * xd).mean(0) + 2 * mu.abs() * e_mu
    e_inv = inv * (0.5 * e_var / (var + EPS) + 2 * U)
    e_sc = g.double() * e_inv + 2 * U * st64[2].abs()
    e_sh = U * b.double().abs() + st64[2].abs() * e_mu + (mu * g.double()).abs() * e_inv + 4 * U * (mu * st64[2]).abs()
    st_tol = torch.stack([e_mu, e_inv, e_sc, e_sh])
    return dict(x=x, res=res, g=g, b=b, mm=mm, mv=mv, dy=dy, y64=y64.detach(), mm64=mm64, mv64=mv64, st64=st64,
                st_tol=st_tol, dx64=x64.grad, dg64=g64.grad, db64=b64.grad)


def _forward(c, M, R, mode, numel=0):
    """pack per chunk -> sum of the buffers -> finalize + apply per chunk: (ys, stats, moving, bufs)"""
    C_ = _hip()
    xs, rs = _chunks(c["x"], M, R), _chunks(c["res"], M, R)
    bufs = [C_.bn_sync_forward_pack(xc, r, R, None, numel) for r, xc in enumerate(xs)]
    tot = bufs[0].clone()
    for t in bufs[1:]:
        tot += t
    ys, sts, mvs = [], [], []
    for r, xc in enumerate(xs):
        mm, mv = c["mm"].clone(), c["mv"].clone()
        y, st = C_.bn_sync_forward_finalize(xc, tot, R, c["g"], c["b"], mm, mv, MOM, EPS, mode > 0,
                                            rs[r] if mode == 2 else None, None, True)
        ys.append(y)
        sts.append(st)
        mvs.append((mm, mv))
    return ys, sts, mvs, bufs


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("R", RS)
def test_forward_chunks_match_whole_batch_fp64(R, M, C, dtype):
    c = _case(M, C, dtype, 0)
    ys, sts, mvs, _ = _forward(c, M, R, 0)
    y = torch.cat(ys)
    assert y.dtype == dtype and y.shape == c["x"].shape
    tol = dict(atol=2e-4, rtol=2e-4) if dtype == torch.float32 else dict(atol=4e-2, rtol=2e-2)
    torch.testing.assert_close(y.double(), c["y64"], **tol)
    for st, (mm, mv) in zip(sts, mvs):
        assert torch.equal(st, sts[0]), "statistics differ between replicas"
        assert torch.equal(mm, mvs[0][0]) and torch.equal(mv, mvs[0][1])
    torch.testing.assert_close(mvs[0][0].double(), c["mm64"], atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(mvs[0][1].double(), c["mv64"], atol=1e-4, rtol=1e-4)
    err = (sts[0].double() - c["st64"]).abs()
    assert bool((err <= c["st_tol"]).all()), (err / c["st_tol"]).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("R", RS)
def test_backward_chunks_match_whole_batch_fp64(R, M, C, mode, dtype):
    C_ = _hip()
    c = _case(M, C, dtype, mode)
    ys, sts, _, _ = _forward(c, M, R, mode)
    st = sts[0]
    xs, dys = _chunks(c["x"], M, R), _chunks(c["dy"], M, R)
    packed = [C_.bn_sync_backward_pack(dys[r], xs[r], ys[r] if mode == 2 else None, st, mode, r, R)
              for r in range(R)]
    tot = packed[0][0].clone()
    for p in packed[1:]:
        tot += p[0]
    dxs = [C_.bn_sync_backward_finalize(packed[r][3], xs[r], tot, R, c["g"], st, mode == 1) for r in range(R)]
    gtol = dict(atol=5e-4, rtol=1e-3) if dtype == torch.float32 else dict(atol=6e-2, rtol=3e-2)
    torch.testing.assert_close(torch.cat(dxs).double(), c["dx64"], **gtol)
    if mode == 2:  # the residual's gradient is the masked dz
        want = torch.where(c["y64"] > 0, c["dy"].double(), torch.zeros_like(c["y64"]))
        torch.testing.assert_close(torch.cat([p[3] for p in packed]).double(), want, atol=0, rtol=0)
    # dgamma / dbeta are LOCAL: their sum over the replicas is the whole batch's
    ptol = dict(atol=gtol["atol"] * max(1.0, M ** 0.5 / 8) * 4, rtol=gtol["rtol"])
    dg = torch.stack([p[1].double() for p in packed])
    db = torch.stack([p[2].double() for p in packed])
    torch.testing.assert_close(dg.sum(0), c["dg64"], **ptol)
    torch.testing.assert_close(db.sum(0), c["db64"], **ptol)
    with pytest.raises(AssertionError):  # ... and one replica's alone is not
        torch.testing.assert_close(dg[R - 1], c["dg64"], **ptol)


def _int_data(M, C, dtype, seed):
    """Small integers: every f32 partial sum of x, x*x, dz and dz*x is exact, whatever the grouping."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randint(-6, 7, (M, C), generator=gen).to(dtype).to(DEV)
    dz = torch.randint(-4, 5, (M, C), generator=gen).to(dtype).to(DEV)
    return x, dz


def _rows(a, b, P):
    """[P + ceil(P/64)][2][C] partial rows of sum(a), sum(a*b) over P row groups (a conv epilogue's layout)."""
    M, C = a.shape
    part = torch.zeros(P + (P + 63) // 64, 2, C, device=DEV)
    for p, (ga, gb) in enumerate(zip(torch.tensor_split(a.float(), P), torch.tensor_split(b.float(), P))):
        part[p, 0] = ga.sum(0)
        part[p, 1] = (ga * gb).sum(0)
    return part


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [8, 136])
def test_given_parts_equal_internal_partial_pass_bitwise(C, dtype):
    C_ = _hip()
    M, R, P = 77, 2, 5
    x, dz = _int_data(M, C, dtype, 5 + C)
    g = torch.rand(C, device=DEV) + 0.5
    own = C_.bn_sync_forward_pack(x, 1, R)
    given = C_.bn_sync_forward_pack(x, 1, R, _rows(x, x, P))
    assert torch.equal(own, given)
    outs = []
    for buf in (own, given):
        mm, mv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        y, st = C_.bn_sync_forward_finalize(x, buf, R, g, None, mm, mv, MOM, EPS)
        outs.append((y, st, mm, mv))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    st = outs[0][1]
    for mode in (0, 2):  # given rows: dy IS the group's masked gradient in every mode
        a = C_.bn_sync_backward_pack(dz, x, None, st, 0, 1, R)
        b = C_.bn_sync_backward_pack(dz, x, None, st, mode, 1, R, None, None, _rows(dz, x, P))
        assert all(torch.equal(s, t) for s, t in zip(a, b))
        assert b[3].data_ptr() == dz.data_ptr()
        assert torch.equal(C_.bn_sync_backward_finalize(a[3], x, a[0], R, g, st, False),
                           C_.bn_sync_backward_finalize(b[3], x, b[0], R, g, st, False))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(4, 7, 7, 64), (300, 136), (1, 1, 3, 8)])
def test_one_replica_through_sync_kernels_matches_plain_kernels(shape, dtype):
    """R = 1: the hi/lo pair carries each sum to about 2^-48, so the f32 statistics can differ from the
    plain finalize's by a last-place rounding (plus the cancellation in shift)."""
    C_ = _hip()
    torch.manual_seed(0)
    C = shape[-1]
    x = (torch.randn(shape, device=DEV) * 2 + 0.5).to(dtype)
    g, b = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV)
    mm0, mv0 = torch.randn(C, device=DEV), torch.rand(C, device=DEV) + 0.5
    mm1, mv1 = mm0.clone(), mv0.clone()
    plain = C_.bn_stats_train(x, g, b, mm0, mv0, MOM, EPS, None, None)
    buf = C_.bn_sync_forward_pack(x, 0, 1)
    (st,) = C_.bn_sync_forward_finalize(x, buf, 1, g, b, mm1, mv1, MOM, EPS, False, None, None, False)
    torch.testing.assert_close(st, plain, rtol=2.5e-7, atol=1e-7)
    torch.testing.assert_close(mm1, mm0, rtol=2.5e-7, atol=1e-7)
    torch.testing.assert_close(mv1, mv0, rtol=2.5e-7, atol=1e-7)


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("R,rank", [(2, 0), (3, 1), (8, 7)])
def test_exchange_buffer_is_an_exact_gather(R, rank, C):
    C_ = _hip()
    P, M = 7, 300
    gen = torch.Generator(device="cpu").manual_seed(C + R)
    x = (torch.randn(M, C, generator=gen) + 3.0).to(DEV)
    part = _rows(x, x, P)
    n = int(C_.bn_sync_xbuf_numel(C, R))
    slot = n // R
    assert n % R == 0 and slot >= 4 * C + 2 and slot % 4 == 0
    for numel in (0, n + 8):  # (a padded buffer: the tail is zeroed as well)
        buf = C_.bn_sync_forward_pack(x, rank, R, part, numel)
        assert buf.dtype == torch.float32 and buf.numel() == max(n, numel) and buf.data_ptr() % 16 == 0
        own = buf[rank * slot:(rank + 1) * slot]
        foreign = torch.cat([buf[:rank * slot], buf[(rank + 1) * slot:]])
        assert int(torch.count_nonzero(foreign)) == 0
        cp = (slot - 4) // 4
        rows = own[:4 * cp].view(4, cp).double()
        assert int(torch.count_nonzero(rows[:, C:])) == 0
        ref = part[:P].double().sum(0)  # [2][C]
        for k in range(2):
            got = rows[2 * k, :C] + rows[2 * k + 1, :C]
            rel = ((got - ref[k]).abs() / ref[k].abs()).max()
            assert float(rel) <= 2.0 ** -45, float(rel)
        hdr = own[4 * cp:].double()
        assert float(hdr[0] + hdr[1] * 2 ** 24) == M and int(torch.count_nonzero(hdr[2:])) == 0


class _PeerStub:
    """Rank 1 of 2 in one process: ``all_reduce`` adds what rank 0 would have packed (computed by the
    closures the test queues, in call order)."""

    world_size, rank = 2, 1

    def __init__(self):
        self.peer = []

    def all_reduce(self, t, op="sum"):
        assert op == "sum"
        t += self.peer.pop(0)(t.numel())
        return t


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("form", ["plain", "relu", "add_relu_bias", "relu_deferred_given_parts"])
def test_batch_norm_train_sync_every_form(form, dtype):
    """ops/batchnorm.py ``batch_norm_train(sync=comm)`` end to end on the larger of two chunks (the peer
    holds a single row): plain, BN -> ReLU, BN -> Add -> ReLU with a folded conv bias and slab-style
    gradient targets, and the statistics-only (deferred apply) form fed conv-epilogue partial rows."""
    from tensorflow_distributed_learning_amd.ops.batchnorm import batch_norm_train

    C_ = _hip()
    M, C = 300, 72
    mode = {"plain": 0, "relu": 1, "add_relu_bias": 2, "relu_deferred_given_parts": 1}[form]
    c = _case(M, C, dtype, mode)
    (x0, x1), (r0, r1), (dy0, dy1) = (_chunks(c[k], M, 2) for k in ("x", "res", "dy"))
    comm = _PeerStub()
    tot = C_.bn_sync_forward_pack(x0, 0, 2) + C_.bn_sync_forward_pack(x1, 1, 2)
    y0, st = C_.bn_sync_forward_finalize(x0, tot, 2, c["g"], c["b"], None, None, MOM, EPS, mode > 0,
                                         r0 if mode == 2 else None, None, True)
    comm.peer.append(lambda n: C_.bn_sync_forward_pack(x0, 0, 2, None, n))
    comm.peer.append(lambda n: C_.bn_sync_backward_pack(dy0, x0, y0 if mode == 2 else None, st, mode, 0, 2, None, None,
                                                        None, n)[0])
    xin = x1.clone().requires_grad_(True)
    rin = r1.clone().requires_grad_(True) if mode == 2 else None
    g, b = c["g"].clone().requires_grad_(True), c["b"].clone().requires_grad_(True)
    mm, mv = c["mm"].clone(), c["mv"].clone()
    kw = {}
    gt = None
    if form == "add_relu_bias":
        cb = torch.randn(C, device=DEV).requires_grad_(True)
        gt = (torch.ones(C, device=DEV), torch.ones(C, device=DEV))  # targets the gradients are ADDED into
        kw = dict(conv_bias=cb, grad_out=gt)
    if form == "relu_deferred_given_parts":
        kw = dict(stats_out=[], defer_apply=True, part=_rows(x1, x1, 3))
    y = batch_norm_train(xin, g, b, mm, mv, MOM, EPS, relu=mode > 0, residual=rin, sync=comm, **kw)
    n0 = x0.shape[0]
    tol = dict(atol=2e-4, rtol=2e-4) if dtype == torch.float32 else dict(atol=4e-2, rtol=2e-2)
    if form == "relu_deferred_given_parts":
        assert y.data_ptr() == xin.data_ptr() or torch.equal(y, xin)  # a stand-in for relu(bn(x))
        err = (kw["stats_out"][0].double() - c["st64"]).abs()
        assert bool((err <= c["st_tol"]).all()), (err / c["st_tol"]).max()
    else:
        torch.testing.assert_close(y.double(), c["y64"][n0:], **tol)
    off = 0.1 * kw["conv_bias"].detach().double() if "conv_bias" in kw else 0.0
    torch.testing.assert_close(mm.double(), c["mm64"] + off, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(mv.double(), c["mv64"], atol=1e-4, rtol=1e-4)
    y.backward(dy1)
    assert not comm.peer  # one exchange per direction
    gtol = dict(atol=5e-4, rtol=1e-3) if dtype == torch.float32 else dict(atol=6e-2, rtol=3e-2)
    torch.testing.assert_close(xin.grad.double(), c["dx64"][n0:], **gtol)
    if mode == 2:
        want = torch.where(c["y64"][n0:] > 0, dy1.double(), torch.zeros_like(c["y64"][n0:]))
        torch.testing.assert_close(rin.grad.double(), want, atol=0, rtol=0)
    # this replica's dgamma / dbeta plus the peer's are the whole batch's
    p0 = C_.bn_sync_backward_pack(dy0, x0, y0 if mode == 2 else None, st, mode, 0, 2)
    ptol = dict(atol=gtol["atol"] * max(1.0, M ** 0.5 / 8) * 4, rtol=gtol["rtol"])
    mine = (gt[0] - 1.0, gt[1] - 1.0) if gt is not None else (g.grad, b.grad)
    torch.testing.assert_close(mine[0].double() + p0[1].double(), c["dg64"], **ptol)
    torch.testing.assert_close(mine[1].double() + p0[2].double(), c["db64"], **ptol)
    if gt is not None:
        assert g.grad is None and float(kw["conv_bias"].grad.abs().max()) == 0.0


def test_exchange_size_steps_past_the_gradient_buckets():
    """xGMI channels are keyed by element count: an exchange never gets the size of a gradient bucket
    that can be in flight on the side stream (engine/trainer.py fills ``_bn_sync_avoid``)."""
    from tensorflow_distributed_learning_amd.ops.batchnorm import sync_exchange_numel

    class Comm:
        world_size, rank = 2, 0

    n = int(_hip().bn_sync_xbuf_numel(64, 2))
    assert sync_exchange_numel(Comm(), 64) == n
    c = Comm()
    c._bn_sync_avoid = {n, n + 4, 7}
    assert sync_exchange_numel(c, 64) == n + 8
    assert sync_exchange_numel(c, 128) == int(_hip().bn_sync_xbuf_numel(128, 2))


def test_nonfinite_input_propagates_as_in_the_plain_kernels():
    C_ = _hip()
    C = 16
    x = torch.randn(40, C, device=DEV)
    x[3, 2] = float("inf")
    x[5, 9] = float("nan")
    plain = C_.bn_stats_train(x, None, None, None, None, MOM, EPS, None, None)
    bufs = [C_.bn_sync_forward_pack(xc, r, 2) for r, xc in enumerate(torch.split(x, [7, 33]))]
    (st,) = C_.bn_sync_forward_finalize(x[:7], bufs[0] + bufs[1], 2, None, None, None, None, MOM, EPS, False, None,
                                        None, False)
    assert torch.equal(torch.isnan(st), torch.isnan(plain)) and torch.equal(torch.isinf(st), torch.isinf(plain))
    assert not bool(torch.isfinite(st[:, 2]).all()) and not bool(torch.isfinite(st[:, 9]).all())
    assert bool(torch.isfinite(st[:, [0, 1, 3, 15]]).all())
