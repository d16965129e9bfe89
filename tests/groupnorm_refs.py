"""References of the group-normalisation kernels (csrc/kernels/groupnorm.hip), shared by
test_groupnorm_cpu.py and test_groupnorm_kernels_gpu.py.  numpy only; nothing here touches a GPU.

* ``gn_fwd_ref`` / ``gn_bwd_ref``: the textbook formulas in f64 (two-pass variance), x as [N, P, C].
* ``gn_fwd_emul`` / ``gn_bwd_emul``: the kernels' own formulas -- per-(sample, channel) sums over the pixels
  taken sequentially, folded into groups, coefficients formed in f64 and rounded to f32 once, one f32 fma
  per element, one rounding to the output dtype -- so that ``|emulation - reference|`` measures what the
  f32 coefficient tables and the f32 elementwise arithmetic cost on the case's own inputs.  ``sums="f64"``
  is what the kernels do; ``sums="f32"`` accumulates the same sums in f32 (one rounding per add / fma), the
  form the kernels are NOT allowed to have: the tests use it to show that their bound tells the two apart
  on data with a large mean.
"""
import numpy as np

from kernel_refs import _fma32, _store


def groups_of(C, G):
    return C if G == -1 else G


def _grouped(a, G):
    """[N, P, C] -> [N, P, G, C/G]"""
    N, P, C = a.shape
    return a.reshape(N, P, G, C // G)


def _per_channel(v, G, C):
    """[N, G] -> [N, 1, C]: a group's value for each of its channels."""
    return np.repeat(v, C // G, axis=1)[:, None, :]


# --------------------------------------------------------------------------------------- f64 references
def gn_fwd_ref(x, G, gamma, beta, eps):
    x = np.asarray(x, dtype=np.float64)
    N, P, C = x.shape
    h = _grouped(x, G)
    mean = h.mean(axis=(1, 3))
    var = ((h - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
    r = 1.0 / np.sqrt(var + eps)
    g = np.ones(C) if gamma is None else np.asarray(gamma, dtype=np.float64)
    b = np.zeros(C) if beta is None else np.asarray(beta, dtype=np.float64)
    xhat = (x - _per_channel(mean, G, C)) * _per_channel(r, G, C)
    return dict(mean=mean, r=r, y=xhat * g + b)


def gn_bwd_ref(dy, x, G, gamma, eps, dgamma0=None, dbeta0=None):
    dy = np.asarray(dy, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    N, P, C = x.shape
    f = gn_fwd_ref(x, G, None, None, eps)
    xhat = f["y"]
    g = np.ones(C) if gamma is None else np.asarray(gamma, dtype=np.float64)
    dgamma = (dy * xhat).sum(axis=(0, 1))
    dbeta = dy.sum(axis=(0, 1))
    gy = dy * g
    m1 = _grouped(gy, G).mean(axis=(1, 3))
    m2 = _grouped(gy * xhat, G).mean(axis=(1, 3))
    dx = _per_channel(f["r"], G, C) * (gy - _per_channel(m1, G, C) - xhat * _per_channel(m2, G, C))
    if dgamma0 is not None:
        dgamma = dgamma + np.asarray(dgamma0, dtype=np.float64)
    if dbeta0 is not None:
        dbeta = dbeta + np.asarray(dbeta0, dtype=np.float64)
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta)


# --------------------------------------------------------------------------------------- kernel formulas
def _seq_sums(u, x, sums):
    """Per (n, c): (sum_p u, sum_p u x), added sequentially over p; f64, or f32 with one rounding per step."""
    N, P, C = x.shape
    if sums == "f64":
        u64, x64 = u.astype(np.float64), x.astype(np.float64)
        return np.cumsum(u64, axis=1)[:, -1, :], np.cumsum(u64 * x64, axis=1)[:, -1, :]
    s = np.zeros((N, C), dtype=np.float32)
    q = np.zeros((N, C), dtype=np.float32)
    for p in range(P):
        s = s + u[:, p, :]
        q = _fma32(u[:, p, :], x[:, p, :], q)
    return s.astype(np.float64), q.astype(np.float64)


def gn_fwd_emul(x, G, gamma, beta, eps, bf16=False, sums="f64"):
    """x: f32 values (bf16-representable when ``bf16``).  Returns mean, r [N, G] (f64, as saved), the f32
    scale / shift tables [N, C] and y as stored, all as f64 arrays."""
    x = np.asarray(x, dtype=np.float32)
    N, P, C = x.shape
    m = float(P * (C // G))
    s1, s2 = _seq_sums(x, x, sums)
    t1 = s1.reshape(N, G, C // G).sum(axis=2)
    t2 = s2.reshape(N, G, C // G).sum(axis=2)
    mean = t1 / m
    v = t2 / m - mean * mean
    var = np.where(v < 0.0, 0.0, v)
    r = 1.0 / np.sqrt(var + eps)
    g = np.ones(C) if gamma is None else np.asarray(gamma, dtype=np.float32).astype(np.float64)
    b = np.zeros(C) if beta is None else np.asarray(beta, dtype=np.float32).astype(np.float64)
    sc = g[None, :] * np.repeat(r, C // G, axis=1)
    scale = sc.astype(np.float32)
    shift = (b[None, :] - np.repeat(mean, C // G, axis=1) * sc).astype(np.float32)
    y = _fma32(x, scale[:, None, :], shift[:, None, :])
    return dict(mean=mean, r=r, scale=scale.astype(np.float64), shift=shift.astype(np.float64), y=_store(y, bf16))


def gn_bwd_emul(dy, x, G, gamma, mean, r, dgamma0=None, dbeta0=None, bf16=False, sums="f64"):
    """mean, r: the saved [N, G] f64 statistics (the emulation's own forward's)."""
    dy = np.asarray(dy, dtype=np.float32)
    x = np.asarray(x, dtype=np.float32)
    N, P, C = x.shape
    cpg = C // G
    m = float(P * cpg)
    a, b = _seq_sums(dy, x, sums)
    g = np.ones(C) if gamma is None else np.asarray(gamma, dtype=np.float32).astype(np.float64)
    mean_c, r_c = np.repeat(mean, cpg, axis=1), np.repeat(r, cpg, axis=1)
    dbeta = np.cumsum(a, axis=0)[-1]
    dgamma = np.cumsum(r_c * (b - mean_c * a), axis=0)[-1]
    S1 = (g[None, :] * a).reshape(N, G, cpg).sum(axis=2)
    S2 = r * (g[None, :] * (b - mean_c * a)).reshape(N, G, cpg).sum(axis=2)
    A = (g[None, :] * r_c).astype(np.float32)
    B = np.repeat(-(r * r) * S2 / m, cpg, axis=1).astype(np.float32)
    D = np.repeat((r * r) * mean * S2 / m - r * S1 / m, cpg, axis=1).astype(np.float32)
    dx = _fma32(A[:, None, :], dy, _fma32(B[:, None, :], x, D[:, None, :]))
    dgamma, dbeta = dgamma.astype(np.float32), dbeta.astype(np.float32)
    if dgamma0 is not None:
        dgamma = np.asarray(dgamma0, dtype=np.float32) + dgamma
    if dbeta0 is not None:
        dbeta = np.asarray(dbeta0, dtype=np.float32) + dbeta
    return dict(dx=_store(dx, bf16), dgamma=dgamma.astype(np.float64), dbeta=dbeta.astype(np.float64))
