"""References of the weighted / smoothed loss head (csrc/kernels/loss_head.hip), numpy only; nothing here touches
a GPU.  ``head_ref`` is the f64 oracle, ``head_emul_f32`` the kernel's order of operations in f32 with sequential
sums (as kernel_refs.xent_emul_f32), used only to size tolerances.

Per row of the logits z [N, K], with m = max z, u_k = z_k - m, se = sum exp(u_k), p_k = exp(u_k) / se:

* sparse target, label y in [0, K):  q_k = (1 - eps) [k == y] + eps / K,  S = 1,
  loss = log(se) - (1 - eps) u_y - (eps / K) sum_k u_k
* sparse target, y outside [0, K):  q = 0, loss = 0, class weight 1
* dense target t [N, K]:  q_k = (1 - eps) t_k + eps / K,  S = sum q_k,  loss = S log(se) - sum q_k u_k,
  class = argmax t (first index on ties)
* w = sw[r] * cw[class] (an absent factor is 1),  dz_k = (p_k S - q_k) * w / gn

``eps`` is the f32 value the kernel receives, widened (kernel_refs.f32: a constant's representation error is not
counted against a kernel).
"""
import numpy as np

import kernel_refs as R


def _is_dense(target) -> bool:
    return np.asarray(target).ndim == 2


def head_ref(z, target, sw=None, cw=None, eps=0.0, gn=1.0):
    """The f64 oracle.  Returns a dict of per-row arrays: ``loss`` (unweighted), ``w``, ``S``, ``cls`` (-1 for an
    invalid sparse label), ``correct`` (bool), ``mag`` (the largest term the f32 loss is put together from) and
    the [N, K] arrays ``p``, ``q``, ``dzu`` (= p S - q, unscaled) and ``dz`` (= dzu * w / gn)."""
    z = np.asarray(z, dtype=np.float64)
    N, K = z.shape
    eps = R.f32(eps)
    m = z.max(axis=1, keepdims=True) if N else np.zeros((0, 1))
    u = z - m
    se = np.exp(u).sum(axis=1)
    p = np.exp(u) / se[:, None]
    lg = np.log(se)
    am = z.argmax(axis=1) if N else np.zeros(0, dtype=np.int64)  # numpy: the first index of a duplicated maximum
    if _is_dense(target):
        t = np.asarray(target, dtype=np.float64)
        q = (1.0 - eps) * t + eps / K
        S = q.sum(axis=1)
        qu = (q * u).sum(axis=1)
        loss = S * lg - qu
        cls = t.argmax(axis=1) if N else np.zeros(0, dtype=np.int64)
        valid = np.ones(N, dtype=bool)
        mag = np.maximum(np.abs(S * lg), np.abs(qu))
    else:
        y = np.asarray(target, dtype=np.int64)
        valid = (y >= 0) & (y < K)
        ys = np.where(valid, y, 0)
        onehot = np.zeros((N, K))
        onehot[np.arange(N), ys] = 1.0
        q = ((1.0 - eps) * onehot + eps / K) * valid[:, None]
        S = np.ones(N)
        uy = u[np.arange(N), ys]
        loss = np.where(valid, lg - (1.0 - eps) * uy - (eps / K) * u.sum(axis=1), 0.0)
        cls = np.where(valid, y, -1)
        # the kernel's unsmoothed sparse form is xent_head's lse - z[y] on the unshifted logits
        zy = z[np.arange(N), ys]
        mag = np.where(valid, np.maximum(np.abs(m[:, 0] + lg), np.abs(zy)) if eps == 0.0 else
                       np.maximum(np.abs(lg), np.maximum(np.abs(uy), np.abs(eps / K * u.sum(axis=1)))), 0.0)
    w = np.ones(N)
    if sw is not None:
        w = w * np.asarray(sw, dtype=np.float64)
    if cw is not None:
        cwa = np.asarray(cw, dtype=np.float64)
        w = w * np.where(cls >= 0, cwa[np.maximum(cls, 0)], 1.0)
    dzu = p * S[:, None] - q
    return {"loss": loss, "w": w, "S": S, "cls": cls, "correct": valid & (am == cls), "p": p, "q": q, "dzu": dzu,
            "dz": dzu * (w / gn)[:, None], "mag": np.maximum(mag, np.abs(loss))}


def _seq_sum_f32(a):
    """Row sums of a [N, K] f32 array, added one column after the other in f32."""
    s = np.zeros(a.shape[0], dtype=np.float32)
    for k in range(a.shape[1]):
        s += a[:, k]
    return s


def head_emul_f32(z, target, sw=None, cw=None, eps=0.0, gn=1.0):
    """The kernel's operations in f32: (w * loss [N], dz [N, K], w [N]) as f64 arrays.  Sums over the classes are
    sequential; exp and log are numpy's f32 ones."""
    f = np.float32
    z = np.asarray(z, dtype=f)
    N, K = z.shape
    eps = f(eps)
    ome, epk = f(1.0) - eps, eps / f(K)
    inv_gn = f(1.0 / gn)
    mx = z.max(axis=1)
    u = (z - mx[:, None]).astype(f)
    se = _seq_sum_f32(np.exp(u, dtype=f))
    lg = np.log(se, dtype=f)
    lse = (mx + lg).astype(f)
    pe = np.exp((z - lse[:, None]).astype(f), dtype=f)
    w = np.ones(N, dtype=f) if sw is None else np.asarray(sw, dtype=f).copy()
    if _is_dense(target):
        t = np.asarray(target, dtype=f)
        q = (ome * t + epk).astype(f) if eps != 0 else t
        sq = _seq_sum_f32(q)
        squ = _seq_sum_f32((q * u).astype(f))
        loss = ((sq * lg).astype(f) - squ).astype(f)
        if cw is not None:
            w = (w * np.asarray(cw, dtype=f)[t.argmax(axis=1)]).astype(f)
        dzu = ((pe * sq[:, None]).astype(f) - q).astype(f)
    else:
        y = np.asarray(target, dtype=np.int64)
        valid = (y >= 0) & (y < K)
        ys = np.where(valid, y, 0)
        q = np.zeros((N, K), dtype=f)
        if eps != 0:
            q[:] = epk
            q[np.arange(N), ys] = ome + epk
            q[~valid] = 0
            su = _seq_sum_f32(u)
            uy = u[np.arange(N), ys]
            loss = ((lg - (ome * uy).astype(f)).astype(f) - (epk * su).astype(f)).astype(f)
        else:
            q[np.arange(N), ys] = valid.astype(f)
            loss = (lse - z[np.arange(N), ys]).astype(f)
        loss = np.where(valid, loss, f(0))
        if cw is not None:
            w = np.where(valid, (w * np.asarray(cw, dtype=f)[ys]).astype(f), w)
        dzu = (pe - q).astype(f)
    scale = (w * inv_gn).astype(f) if (sw is not None or cw is not None) else np.full(N, inv_gn, dtype=f)
    dz = (dzu * scale[:, None]).astype(f)
    return w.astype(np.float64) * loss.astype(np.float64), dz.astype(np.float64), w.astype(np.float64)
