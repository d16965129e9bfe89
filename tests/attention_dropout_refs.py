"""Float64 attention with dropout on the probabilities (z [B,H,T,S] the kernels' keep mask from the numpy Philox stream,
c = keep_scale(rate)) and the bounds of the DROP kernels: those of attention_refs.py re-derived with P~ = c z P.  o and dV
sum P~-weighted terms: p -> c z p there.  dS = P (c z dP - delta): the error of dP (eps |dP| and its dot product's
(Dv + 2) 2^-23 sum |do||v|) is multiplied by c z before it meets delta, so |dP| -> c z |dP| in eta and dP's dot-product
term carries c z; delta's terms do not.  The multiply by c is one more f32 rounding: n + 2 -> n + 3 in every relative
count.  A flushed value is scaled by c afterwards: every FTZ term times c.  lse is the undropped row's: unchanged."""
import numpy as np

import attention_refs as AR
from tensorflow_distributed_learning_amd.ops import dropout as DO

KEY, U23 = DO.stream_key(7, 1, 0), 2.0 ** -23


def keep_mask(key, ticket, rate, B, H, T, S):
    """z of mask index m = 4 (((b H + h) ceil(T / 4) + (i >> 2)) S + j) + (i & 3): kept iff its word >= threshold."""
    bh, i, j = np.arange(B * H, dtype=np.uint64)[:, None, None], np.arange(T, dtype=np.uint64)[:, None], np.arange(S, dtype=np.uint64)
    m = 4 * ((bh * np.uint64(-(-T // 4)) + (i >> np.uint64(2))) * np.uint64(S) + j) + (i & np.uint64(3))
    return (DO.philox_words(key, ticket, m) >= np.uint64(DO.threshold(rate))).reshape(B, H, T, S)


def forward(q, k, v, scale, adm, z, c, bf16):
    """(o, lse, p undropped, tol_o, tol_lse)."""
    _, lse, p = AR.forward(q, k, v, scale, adm)
    pt, av, S, (eps, u, r) = c * z * p, np.abs(v, dtype=np.float64), k.shape[1], AR._rounding(q, k, scale, adm, bf16)
    o = np.einsum("bhts,bshe->bthe", pt, v.astype(np.float64))
    rel = (eps + (S + 3) * U23 + r).transpose(0, 2, 1)[..., None]
    tol_o = rel * np.einsum("bhts,bshe->bthe", pt, av) + u * np.abs(o) + c * AR.FTZ * (av.sum(axis=1)[:, None] + S + 1)
    with np.errstate(invalid="ignore"):
        return o, lse, p, tol_o, eps + U23 * (1 + np.abs(lse))


def backward(q, k, v, o, lse, do, scale, adm, z, c, bf16):
    """((dq, dk, dv), their bounds) from the given o and lse (the kernels' saved values, rounded)."""
    q, k, v, o, do, lse = (np.asarray(a, dtype=np.float64) for a in (q, k, v, o, do, lse))
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.where(adm & np.isfinite(lse)[..., None],
                     np.exp(scale * np.einsum("bthd,bshd->bhts", q, k) - np.where(np.isfinite(lse), lse, 0.0)[..., None]), 0.0)
    cz, delta, ado = c * z, np.einsum("bthe,bthe->bht", do, o)[..., None], np.abs(do)
    dP = cz * np.einsum("bthe,bshe->bhts", do, v)
    dS = p * (dP - delta)
    grads = (scale * np.einsum("bhts,bshd->bthd", dS, k), scale * np.einsum("bhts,bthd->bshd", dS, q), np.einsum("bhts,bthe->bshe", cz * p, do))
    (eps, u, r), T, S, Dv, f = AR._rounding(q, k, scale, adm, bf16), q.shape[1], k.shape[1], v.shape[3], c * AR.FTZ
    eps = eps[..., None]
    inner = cz * np.einsum("bthe,bshe->bhts", ado, np.abs(v)) + np.einsum("bthe,bthe->bht", ado, np.abs(o))[..., None]
    eta = p * (eps * (np.abs(dP) + np.abs(delta)) + (Dv + 3) * U23 * inner) + r * np.abs(dS) + f * (np.abs(dP) + np.abs(delta) + 1)
    tols = (scale * np.einsum("bhts,bshd->bthd", eta + (S + 3) * U23 * np.abs(dS), np.abs(k)) + u * np.abs(grads[0]) + (S + 1) * f,
            scale * np.einsum("bhts,bthd->bshd", eta + (T + 3) * U23 * np.abs(dS), np.abs(q)) + u * np.abs(grads[1]) + (T + 1) * f,
            np.einsum("bhts,bthe->bshe", (eps + (T + 3) * U23 + r) * cz * p + f, ado) + u * np.abs(grads[2]) + (T + 1) * f)
    return grads, tols
