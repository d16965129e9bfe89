"""f64 references of gradient clipping over a flat slab (csrc/kernels/clip.hip and the clip operands of the
optimizer kernels), shared by test_clip_kernels_gpu.py, test_clip_fit_gpu.py and test_clip_cpu.py.  numpy
only; nothing here touches a GPU.  The formulas are those of keras/optimizers.py ``Optimizer._clip``:
clamp by ``clipvalue``, then the norm of the clamped gradient, then the scale
``min(1, clipnorm / (norm + 1e-12))``.  Constants enter as the f32 values the kernels receive.
"""
import numpy as np

from kernel_refs import f32


def clamp_ref(g, clipvalue):
    """clamp(g, +-clipvalue) in f64; a NaN stays a NaN (Tensor.clamp_), +-Inf becomes +-clipvalue."""
    g = np.asarray(g, dtype=np.float64)
    if clipvalue is None:
        return g
    cv = f32(clipvalue)
    with np.errstate(invalid="ignore"):
        return np.where(g > cv, cv, np.where(g < -cv, -cv, g))


def norm_ref(g, clipvalue=None) -> float:
    """sqrt(sum clamp(g)^2) in f64 (a product of two f32 values is exact in f64; numpy's pairwise f64 sum of
    <= 2^25 terms has a relative error far below an f32 ulp)."""
    c = clamp_ref(g, clipvalue)
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.sqrt(np.sum(c * c)))


def scale_ref(norm: float, clipnorm) -> float:
    """min(1, clipnorm / (norm + 1e-12)) in f64; a NaN norm gives NaN, an infinite norm 0."""
    r = f32(clipnorm) / (norm + f32(1e-12))
    if np.isnan(r):
        return r
    return min(1.0, r)


def clip_ref(g, clipnorm=None, clipvalue=None):
    """(clipped gradient, norm or None, scale or None), all f64."""
    c = clamp_ref(g, clipvalue)
    if clipnorm is None:
        return c, None, None
    n = norm_ref(g, clipvalue)
    s = scale_ref(n, clipnorm)
    with np.errstate(invalid="ignore"):
        return c * s, n, s
