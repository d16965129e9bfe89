"""Reference for the weight EMA (``use_ema``; csrc/kernels/ema.hip, the EMA instantiations of the update kernels,
``Optimizer.ema_after``): one step of the moving average in numpy f32, operation by operation as the issue states it.

    E_new = fl(fl(m32 * E) + fl(c32 * W)),   m32 = float32(m),   c32 = float32(1.0 - m)  (the subtraction in f64)
    mode 1: W is left alone        mode 2 (an overwrite step): W = E_new

numpy's f32 ``*`` and ``+`` are single IEEE roundings (no FMA), so a correct implementation agrees bit for bit on
every value that is not a NaN.  Where the result is a NaN its position must agree; its payload and sign are not
defined by IEEE 754 for a generated NaN (Inf - Inf gives 0xffc00000 on x86 and 0x7fc00000 on gfx950), so
``same_bits`` treats any NaN as equal to any NaN.
"""
import numpy as np

SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 1.4e-45, 3.0e-39, -3.0e-39, 1.5, -1.5,
                     3.4e38, -3.4e38, 1.17549435e-38], dtype=np.float32)


def coeffs(m: float):
    """(m32, c32): the two f32 coefficients of momentum ``m``."""
    return np.float32(m), np.float32(1.0 - float(m))


def step(e: np.ndarray, w: np.ndarray, m: float, mode: int = 1):
    """One update of the average: (new E, new W) for f32 arrays ``e`` and ``w`` (mode as the kernels')."""
    assert e.dtype == np.float32 and w.dtype == np.float32 and mode in (1, 2)
    m32, c32 = coeffs(m)
    with np.errstate(all="ignore"):
        e_new = m32 * e + c32 * w
    assert e_new.dtype == np.float32
    return e_new, (e_new.copy() if mode == 2 else w.copy())


def mode_of(step_count: int, f) -> int:
    """The mode of the update whose 1-based step count is ``step_count`` under ``ema_overwrite_frequency=f``."""
    return 2 if f is not None and step_count % f == 0 else 1


def fold(w0: np.ndarray, ws, m: float) -> np.ndarray:
    """E after the updates that produced the weights ``ws`` (no overwrite steps), from E = ``w0``."""
    e = np.asarray(w0, dtype=np.float32).copy()
    for w in ws:
        e, _ = step(e, np.asarray(w, dtype=np.float32), m, 1)
    return e


def same_bits(x: np.ndarray, y: np.ndarray) -> bool:
    """Bit equality of two f32 arrays (signs of zeros, denormals, infinities included); any NaN equals any NaN."""
    x, y = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)
    if x.shape != y.shape:
        return False
    nx, ny = np.isnan(x), np.isnan(y)
    if not np.array_equal(nx, ny):
        return False
    return np.array_equal(np.where(nx, 0, x.view(np.int32)), np.where(ny, 0, y.view(np.int32)))


def plant_specials(arrs, m: float, seed: int = 0):
    """Plant the special values into the f32 arrays ``arrs`` (in place) so that every pair of them meets at some
    position (array j holds the list rotated by r * j in block r), and, in ``arrs[0]`` (E) and ``arrs[1]`` (W),
    pairs with ``m32 * E = -c32 * W``: the two products cancel exactly where both are representable."""
    n = arrs[0].size
    if n == 0:
        return
    k = len(SPECIALS)
    pos = (np.arange(k * k, dtype=np.int64) * 7919 + 3) % n
    for j, a in enumerate(arrs):
        for r in range(k):
            a[pos[r * k:(r + 1) * k]] = np.roll(SPECIALS, r * j)
    if n >= 64 and len(arrs) >= 2:
        m32, c32 = coeffs(m)
        e, w = arrs[0], arrs[1]
        lo = n // 2
        # E = c32 * x, W = -m32 * x: m32 * E and c32 * W are then x * m32 * c32 with opposite signs whenever the
        # first products are exact (x a small power of two times an integer keeps them so)
        x = (np.arange(1, 9, dtype=np.float32) * np.float32(0.25)).astype(np.float32)
        e[lo:lo + 8] = c32 * x
        w[lo:lo + 8] = -(m32 * x)
