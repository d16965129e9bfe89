"""References of the layer / RMS normalisation kernels (csrc/kernels/layernorm.hip); numpy only.

* ``ln_fwd_ref`` / ``ln_bwd_ref``: the textbook formulas in f64, x as [R, C].
* ``ln_fwd_emul`` / ``ln_bwd_emul``: the kernels' formulas (csrc/kernels/layernorm.h) -- f64 centred statistics,
  a = f32(r), b = f32(-mean r), one f32 operation per step, one rounding to the output dtype -- so that
  ``|emulation - reference|`` measures what the f32 elementwise arithmetic costs on the case's own inputs.  The
  order of the f64 sums is not mirrored (at most 16 k f32 terms: far below that).  ``var="f32-uncentred"`` takes
  the variance as E[x^2] - mean^2 from f32 sums, the form the kernels must NOT have.
"""
import numpy as np

from kernel_refs import _fma32, _store

F32 = np.float32


def _f64(v, C, fill):
    return np.full(C, fill) if v is None else np.asarray(v, dtype=np.float64)


def ln_fwd_ref(x, gamma, beta, eps, rms=False):
    x = np.asarray(x, dtype=np.float64)
    C = x.shape[1]
    mean = np.zeros(x.shape[0]) if rms else x.mean(axis=1)
    r = 1.0 / np.sqrt(((x - mean[:, None]) ** 2).mean(axis=1) + eps)
    xhat = (x - mean[:, None]) * r[:, None]
    return dict(mean=mean, r=r, xhat=xhat, y=xhat * _f64(gamma, C, 1.0) + _f64(None if rms else beta, C, 0.0))


def ln_bwd_ref(dy, x, gamma, eps, rms=False, dgamma0=None, dbeta0=None):
    dy = np.asarray(dy, dtype=np.float64)
    C = dy.shape[1]
    f = ln_fwd_ref(x, None, None, eps, rms)
    gy = dy * _f64(gamma, C, 1.0)
    m1 = 0.0 if rms else gy.mean(axis=1, keepdims=True)
    m2 = (gy * f["xhat"]).mean(axis=1, keepdims=True)
    return dict(dx=f["r"][:, None] * (gy - m1 - f["xhat"] * m2),
                dgamma=(dy * f["xhat"]).sum(axis=0) + _f64(dgamma0, C, 0.0), dbeta=dy.sum(axis=0) + _f64(dbeta0, C, 0.0))


def _xhat32(x, mean, r, rms):
    a = r.astype(F32)[:, None]
    return (x * a if rms else _fma32(x, a, (-mean * r).astype(F32)[:, None])), a


def ln_fwd_emul(x, gamma, beta, eps, rms=False, bf16=False, var="f64-centred"):
    """x: f32 values (bf16-representable when ``bf16``).  mean, r (f64, as saved) and y as stored, as f64 arrays."""
    x = np.asarray(x, dtype=F32)
    R, C = x.shape
    if var == "f64-centred":
        x64 = x.astype(np.float64)
        mean = np.zeros(R) if rms else x64.sum(axis=1) / C
        v = ((x64 - mean[:, None]) ** 2).sum(axis=1) / C
    else:  # sequential f32 sums of x and x^2
        s, q = np.zeros(R, dtype=F32), np.zeros(R, dtype=F32)
        for c in range(C):
            s, q = s + x[:, c], _fma32(x[:, c], x[:, c], q)
        m32 = np.zeros(R, dtype=F32) if rms else s / F32(C)
        v, mean = np.maximum(q / F32(C) - m32 * m32, F32(0)).astype(np.float64), m32.astype(np.float64)
    r = 1.0 / np.sqrt(v + eps)
    y, _ = _xhat32(x, mean, r, rms)
    g, b = (None if p is None else np.asarray(p, F32)[None, :] for p in (gamma, None if rms else beta))
    if g is not None:
        y = _fma32(y, g, b) if b is not None else y * g
    elif b is not None:
        y = y + b
    return dict(mean=mean, r=r, y=_store(y, bf16))


def ln_bwd_emul(dy, x, gamma, mean, r, rms=False, dgamma0=None, dbeta0=None, bf16=False):
    """mean, r: the saved [R] f64 statistics (the emulation's own forward's)."""
    dy, x = np.asarray(dy, dtype=F32), np.asarray(x, dtype=F32)
    C = x.shape[1]
    xh, a = _xhat32(x, mean, r, rms)
    g = dy if gamma is None else dy * np.asarray(gamma, F32)[None, :]
    g64, xh64, dy64 = g.astype(np.float64), xh.astype(np.float64), dy.astype(np.float64)
    m1 = (g64.sum(axis=1) / C).astype(F32)[:, None]
    m2 = ((g64 * xh64).sum(axis=1) / C).astype(F32)[:, None]
    dx = a * _fma32(-xh, m2, g if rms else g - m1)
    dgamma, dbeta = (dy64 * xh64).sum(axis=0).astype(F32), dy64.sum(axis=0).astype(F32)
    if dgamma0 is not None:
        dgamma = np.asarray(dgamma0, dtype=F32) + dgamma
    if dbeta0 is not None:
        dbeta = np.asarray(dbeta0, dtype=F32) + dbeta
    return dict(dx=_store(dx, bf16), dgamma=dgamma.astype(np.float64), dbeta=dbeta.astype(np.float64))
