"""k_grad_accum (csrc/kernels/accum.hip) against the numpy f32 fold of tests/accum_refs.py, bit for bit.

A pure streaming kernel can go wrong at its edges: the slab's end inside a tile (vector part and scalar tail),
the grid-stride wrap when the slab has more tiles than the grid has workgroups, a tail that lands in a second
pass, an index beyond a tile of the last pass.  The sizes sit on those boundaries, at the production grid cap
and at caps of 1, 2 and 3 workgroups; the values hold signed zeros, infinities, NaNs, denormals and pairs that
cancel exactly.  Every launch is checked for what it must leave alone as well: A in mode 2, G in modes 0 / 1
without zero_grad, and guard words in front of and behind both slabs.
"""
import numpy as np
import pytest
import torch

import accum_refs as AR
from tensorflow_distributed_learning_amd import ops

pytestmark = pytest.mark.gpu

PAD = 64  # guard floats on either side of a slab (256 bytes: the slab stays 16-byte aligned)
SENTINEL = 12345.678
RESNET50 = 25_583_616  # the whole ResNet-50 slab (a multiple of 4)


def C():
    return ops.hip()


def BE() -> int:
    return int(C().ACCUM_BLOCK_ELEMS)


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 1.4e-45, 3.0e-39, -3.0e-39, 1.5, -1.5,
                     3.4e38, -3.4e38, 1.17549435e-38], dtype=np.float32)


def make_grads(n: int, k: int, seed: int):
    """k micro-step gradients of n floats: normals, with the special values planted so that every pair of them
    meets at some position over the cycle (micro-step j plants the list rotated by j), -0 + -0, x + (-x) and
    Inf + (-Inf) among them."""
    rng = np.random.default_rng(seed)
    gs = [rng.standard_normal(n).astype(np.float32) for _ in range(k)]
    if n == 0:
        return gs
    m = len(SPECIALS)
    pos = (np.arange(m * m, dtype=np.int64) * 7919 + 3) % n
    for j, g in enumerate(gs):
        for r in range(m):  # block r of positions: this micro-step's list rotated by r * j
            g[pos[r * m:(r + 1) * m]] = np.roll(SPECIALS, r * j)
    if n >= 64:  # exact cancellation of ordinary values, and of everything the cycle has summed so far
        gs[1][n // 2:n // 2 + 8] = -gs[0][n // 2:n // 2 + 8]
        gs[-1][n - 9:n - 1] = -np.sum(np.stack(gs[:-1])[:, n - 9:n - 1], axis=0, dtype=np.float32)
    return gs


def guarded(n: int, fill=None):
    """(whole buffer, the n-float slab inside it at a 16-byte aligned offset)."""
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    slab = buf[PAD:PAD + n]
    assert slab.data_ptr() % 16 == 0
    if fill is not None:
        slab.copy_(torch.from_numpy(fill))
    return buf, slab


def bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy().view(np.int32)


def guards_ok(buf: torch.Tensor, n: int) -> bool:
    g = torch.cat([buf[:PAD], buf[PAD + n:]])
    return bool((g == SENTINEL).all())


def run_cycle(n: int, k: int, zero: bool, max_blocks=None, seed=0):
    """A full cycle of k launches over guarded slabs, every launch checked; returns the bits of the final G."""
    gs = make_grads(n, k, seed)
    c = AR.recip(k)
    # A starts as garbage (NaNs included): mode 0 must overwrite it, not add to it
    a_ref = np.full(n, np.nan, dtype=np.float32)
    Abuf, A = guarded(n, a_ref)
    Gbuf, G = guarded(n)
    kw = {} if max_blocks is None else {"max_blocks": max_blocks}
    for p, g in enumerate(gs):
        mode = AR.mode_of(p, k)
        G.copy_(torch.from_numpy(g))
        a_before = bits(A).copy()
        z = zero and mode != 2
        C().grad_accum(G, A, mode, float(c), zero_grad=z, **kw)
        a_ref, g_ref = AR.step(a_ref, g, mode, c)
        a_dev, g_dev = A.cpu().numpy(), G.cpu().numpy()
        where = f"n={n} k={k} p={p} mode={mode} zero={z} max_blocks={max_blocks}"
        assert AR.same_bits(a_dev, a_ref), where
        if mode == 2:
            assert np.array_equal(a_dev.view(np.int32), a_before), "mode 2 must leave A bit-unchanged: " + where
            assert AR.same_bits(g_dev, g_ref), where
        elif z:
            assert not g_dev.view(np.int32).any(), "zero_grad must leave +0.0 everywhere: " + where
        else:
            assert np.array_equal(g_dev.view(np.int32), g.view(np.int32)), "G must stay bit-unchanged: " + where
        assert guards_ok(Abuf, n) and guards_ok(Gbuf, n), "guard words overwritten: " + where
    return bits(G)


def test_exported_constants():
    assert int(C().ACCUM_MAX_BLOCKS) >= 256 and BE() % 1024 == 0 and BE() >= 1024


@pytest.mark.parametrize("zero", [False, True], ids=["keep-g", "zero-g"])
@pytest.mark.parametrize("k", [2, 3, 7])
def test_cycle_matches_numpy_at_tile_boundaries(k, zero):
    """Production grid cap: the empty slab, sizes around one vector, around one wave's row of vectors and
    around one workgroup's tile."""
    for n in (0, 1, 3, 4, 5, 1023, 1024, 1025, BE() - 1, BE(), BE() + 1):
        run_cycle(n, k, zero, seed=n + k)


@pytest.mark.parametrize("zero", [False, True], ids=["keep-g", "zero-g"])
@pytest.mark.parametrize("n", [RESNET50, RESNET50 + 3], ids=["resnet50", "resnet50+3"])
def test_cycle_matches_numpy_at_the_resnet50_slab(n, zero):
    """More tiles (6246) than the production grid cap: every workgroup strides, the last tile is partial; + 3
    adds a scalar tail.  k = 3 runs every mode."""
    assert -(-n // BE()) > int(C().ACCUM_MAX_BLOCKS)
    run_cycle(n, 3, zero, seed=1)


@pytest.mark.parametrize("zero", [False, True], ids=["keep-g", "zero-g"])
@pytest.mark.parametrize("k", [2, 3, 7])
@pytest.mark.parametrize("mb", [1, 2, 3])
def test_cycle_matches_numpy_at_the_grid_stride_wrap(mb, k, zero):
    """With the grid capped at mb workgroups: the slab ends just before, at and just after the end of the
    first pass (+5: one whole vector and a scalar into the second pass), and one element into a third."""
    full = mb * BE()
    for n in (full - 1, full, full + 1, full + 5, 2 * full + 1):
        run_cycle(n, k, zero, max_blocks=mb, seed=n + k)


def test_grid_cap_does_not_change_the_bits():
    n = 3 * BE() + 5
    want = run_cycle(n, 3, False)
    for mb in (1, 2, 3, int(C().ACCUM_MAX_BLOCKS)):
        assert np.array_equal(run_cycle(n, 3, False, max_blocks=mb), want)


def test_same_bits_at_two_allocations():
    """Determinism: the result depends on the operands alone, not on where they live."""
    n, k = 2 * BE() + 7, 3
    first = run_cycle(n, k, False, seed=5)
    hold = [torch.empty(1 << 18, device="cuda"), torch.empty(12345, device="cuda")]  # shift the next allocations
    second = run_cycle(n, k, False, seed=5)
    del hold
    assert np.array_equal(first, second)


def test_argument_errors_raise_and_launch_nothing():
    n = 1000
    rng = np.random.default_rng(0)
    g0, a0 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    Gbuf, G = guarded(n, g0)
    Abuf, A = guarded(n, a0)
    f = C().grad_accum
    bad = [
        ("dtype", lambda: f(G.double(), A, 1, 0.5)),
        ("dtype of a", lambda: f(G, A.double(), 1, 0.5)),
        ("misaligned view", lambda: f(G[1:], A[1:], 1, 0.5)),
        ("g is a", lambda: f(G, G, 1, 0.5)),
        ("overlap", lambda: f(G[:n - 4], G[4:], 1, 0.5)),
        ("mode 3", lambda: f(G, A, 3, 0.5)),
        ("mode -1", lambda: f(G, A, -1, 0.5)),
        ("zero_grad with mode 2", lambda: f(G, A, 2, 0.5, zero_grad=True)),
        ("numel mismatch", lambda: f(G, A[:n - 4], 1, 0.5)),
        ("non-contiguous", lambda: f(G[::2], A[::2], 1, 0.5)),
        ("cpu tensor", lambda: f(G.cpu(), A.cpu(), 1, 0.5)),
        ("max_blocks 0", lambda: f(G, A, 1, 0.5, max_blocks=0)),
        ("max_blocks too large", lambda: f(G, A, 1, 0.5, max_blocks=int(C().ACCUM_MAX_BLOCKS) + 1)),
    ]
    for name, call in bad:
        with pytest.raises((RuntimeError, TypeError, ValueError)):
            call()
        torch.cuda.synchronize()
        assert np.array_equal(bits(G), g0.view(np.int32)) and np.array_equal(bits(A), a0.view(np.int32)), name
        assert guards_ok(Gbuf, n) and guards_ok(Abuf, n), name
