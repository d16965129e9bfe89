"""Reference for gradient accumulation (csrc/kernels/accum.hip, ``Optimizer.accumulate``): the left fold of a
cycle's micro-step gradients in numpy f32, operation by operation as the issue states it.

    p == 0: A = g        0 < p < k-1: A = fl(A + g)        p == k-1: G = fl(fl(A + g) * c),  c = float32(1 / k)

numpy's f32 ``+`` and ``*`` are single IEEE roundings (no FMA), so a correct implementation agrees bit for bit
on every value that is not a NaN.  Where the result is a NaN its position must agree; its payload and sign are
not defined by IEEE 754 for a generated NaN (Inf - Inf gives 0xffc00000 on x86 and 0x7fc00000 on gfx950), so
``same_bits`` compares NaNs by position.
"""
import numpy as np


def recip(k: int) -> np.float32:
    """c: the f64 quotient 1 / k rounded once to f32."""
    return np.float32(1.0 / k)


def step(a: np.ndarray, g: np.ndarray, mode: int, c=np.float32(1.0)):
    """One micro-step: (new A, new G) for f32 arrays ``a`` and ``g`` (mode as the kernel's; no zero_grad)."""
    assert a.dtype == np.float32 and g.dtype == np.float32
    with np.errstate(all="ignore"):
        if mode == 0:
            return g.copy(), g.copy()
        if mode == 1:
            return a + g, g.copy()
        s = a + g
        return a.copy(), s * np.float32(c)


def mode_of(p: int, k: int) -> int:
    return 0 if p == 0 else (2 if p == k - 1 else 1)


def fold(gs, k: int) -> np.ndarray:
    """The gradient a cycle's apply micro-step hands on: the fold of its k local gradients ``gs``."""
    assert len(gs) == k and k >= 2
    a = np.zeros_like(gs[0])
    out = None
    for p, g in enumerate(gs):
        a, out = step(a, np.asarray(g, dtype=np.float32), mode_of(p, k), recip(k))
    return out


def same_bits(x: np.ndarray, y: np.ndarray) -> bool:
    """Bit equality of two f32 arrays (signs of zeros, denormals, infinities included) with NaNs compared by
    position."""
    x, y = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)
    if x.shape != y.shape:
        return False
    nx, ny = np.isnan(x), np.isnan(y)
    if not np.array_equal(nx, ny):
        return False
    return np.array_equal(np.where(nx, 0, x.view(np.int32)), np.where(ny, 0, y.view(np.int32)))
