"""Float64 scaled-dot-product attention, its gradients and the issue's rounding bounds of the fused kernels
(csrc/kernels/attention.h) with q [B,T,H,D], k [B,S,H,D], v [B,S,H,Dv] and scores, p and `adm` (admitted) [B,H,T,S].

Underflow (beside the issue's relative terms).  The kernels' f32 arithmetic flushes what falls below the smallest
normal f = 2^-126 to zero (v_exp_f32 and the MFMA produce no denormals) where float64 keeps it: the rescaling case
has probabilities near 1e-44.  So every p carries an absolute error f beside its relative one (an unnormalised
p <= 1 is flushed, then scaled by 1 / l <= 1), every dS f (|dP| + |delta| + 1), a sum of n products n f, the stored
value f: p_ij is followed by "+ f" in the o and dV bounds, eta_ij gains f (|dP_ij| + |delta_i| + 1), and every bound
ends in + (n + 1) f (n = S, or T for dK, dV).
"""
import numpy as np

import kernel_refs as R

FTZ = 2.0 ** -126  # the smallest normal f32: what the kernels flush to zero below

# id: (B, H, T, S, D, Dv), causal, mask kind, layout -- each the smallest shape that reaches one thing
_CASES = {
    "one_tile": ((1, 1, 16, 16, 16, 16), False, None, ""),
    "tile_plus_one": ((1, 2, 65, 65, 8, 8), False, None, ""),            # a row and a key past a tile; smallest head
    "cross_odd_heads": ((2, 1, 33, 130, 40, 24), False, None, ""),       # D != Dv, three key tiles
    "causal": ((2, 3, 100, 100, 16, 16), True, None, ""),                # a skipped key tile
    "causal_T_ne_S": ((1, 1, 20, 70, 16, 16), True, None, ""),
    "mask_bts": ((2, 2, 70, 70, 16, 16), True, "bts", ""),               # an empty row and key tile, causal on top
    "mask_bhts": ((2, 2, 70, 70, 16, 16), True, "bhts", ""),             # the same with per-head masks
    "head128": ((1, 1, 70, 70, 128, 128), False, None, ""),
    "packed_qkv": ((1, 2, 40, 40, 16, 16), False, None, "packed"),       # three views of one [B,T,3,H,D] buffer
    "rescaling": ((1, 1, 48, 192, 16, 16), False, None, "steep"),        # scores to +-100, the max rises every tile
}
IDS, CASES = list(_CASES), list(_CASES.values())


def round_bf16(x):
    return R.bf16_bits_to_f64(R.bf16_rne(np.asarray(x, dtype=np.float32))).astype(np.float32)


def inputs(case, bf16, seed=5):
    """(q, k, v, do) f32 (bf16: pre-rounded), mask (uint8 or None), scale."""
    (B, H, T, S, D, Dv), _, kind, layout = case
    rng = np.random.default_rng(seed)
    q, k = rng.standard_normal((B, T, H, D)), rng.standard_normal((B, S, H, D))
    v, do = rng.standard_normal((B, S, H, Dv)), rng.standard_normal((B, T, H, Dv))
    scale = 1.0 / np.sqrt(D)
    if layout == "steep":  # scale q.k = 4 g_i r_j (+ noise), g in [12.5, 25], r rising from -1 to 1 along the keys
        sign = np.where(np.arange(D) % 2 == 0, 1.0, -1.0)
        q = 0.1 * q + (12.5 * (1 + np.arange(T) / (T - 1)))[None, :, None, None] * sign
        k = 0.1 * k + np.linspace(-1.0, 1.0, S)[None, :, None, None] * sign
    mask = None
    if kind is not None:
        mask = (rng.random((B, H, T, S) if kind == "bhts" else (B, T, S)) < 0.7).astype(np.uint8)
        mask[..., 64:] = 0      # the second key tile
        mask[0, ..., 5, :] = 0  # an empty row (in every head of batch 0)
        if kind == "bhts":
            mask[1, 1, 9, :] = 0
    arrs = [np.asarray(a, dtype=np.float32) for a in (q, k, v, do)]
    return [round_bf16(a) for a in arrs] if bf16 else arrs, mask, float(scale)


def admitted(B, H, T, S, causal, mask):
    adm = np.ones((B, H, T, S), dtype=bool)
    if causal:
        adm &= np.arange(S)[None, :] <= np.arange(T)[:, None]
    if mask is not None:
        adm &= (mask if mask.ndim == 4 else mask[:, None]) != 0
    return adm


def _rounding(q, k, scale, adm, bf16):
    """(eps_i [B,H,T] -- score rounding, exp2, the rescales --, u: the output rounding, r: that of P and dS in bf16)."""
    mag = scale * np.einsum("bthd,bshd->bhts", np.abs(q, dtype=np.float64), np.abs(k, dtype=np.float64))
    eps = 2 * (q.shape[3] + 4) * 2.0 ** -23 * np.where(adm, mag, 0.0).max(axis=3) + (8 - (-k.shape[1] // 64)) * 2.0 ** -23
    return (eps, 2.0 ** -8, 2.0 ** -8) if bf16 else (eps, 2.0 ** -24, 0.0)


def forward(q, k, v, scale, adm):
    """(o [B,T,H,Dv], lse [B,H,T], p [B,H,T,S]) in float64."""
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    s = np.where(adm, scale * np.einsum("bthd,bshd->bhts", q, k), -np.inf)
    m = np.maximum(s.max(axis=3, keepdims=True), -1e300)  # (finite for a row without an admitted key)
    e = np.exp(s - m)
    l = e.sum(axis=3, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(l > 0, e / l, 0.0)
        lse = np.where(l > 0, m + np.log(l), -np.inf)[..., 0]
    return np.einsum("bhts,bshe->bthe", p, v), lse, p


def layer(w, q_in, v_in, k_in, attend, einsum=np.einsum):
    """MultiHeadAttention's function from its weights (query, key, value, output: kernel, bias); attend(q, k, v) -> o."""
    q, k, v = (einsum("btc,chd->bthd", x, w[i]) + w[i + 1] for x, i in ((q_in, 0), (k_in, 2), (v_in, 4)))
    return einsum("bthe,heo->bto", attend(q, k, v), w[6]) + w[7]


def forward_bounds(q, k, v, scale, adm, p, o, lse, bf16):
    (eps, u, r), S, av = _rounding(q, k, scale, adm, bf16), k.shape[1], np.abs(v, dtype=np.float64)
    rel = (eps + (S + 2) * 2.0 ** -23 + r).transpose(0, 2, 1)[..., None]
    tol_o = rel * np.einsum("bhts,bshe->bthe", p, av) + u * np.abs(o) + FTZ * (av.sum(axis=1)[:, None] + S + 1)
    with np.errstate(invalid="ignore"):
        return tol_o, eps + 2.0 ** -23 * (1 + np.abs(lse))


def backward(q, k, v, o, lse, do, scale, adm, bf16):
    """(dq, dk, dv) and their bounds from the given o and lse (the kernels' saved values, rounded)."""
    q, k, v, o, do, lse = (np.asarray(a, dtype=np.float64) for a in (q, k, v, o, do, lse))
    s = scale * np.einsum("bthd,bshd->bhts", q, k)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.where(adm & np.isfinite(lse)[..., None], np.exp(s - np.where(np.isfinite(lse), lse, 0.0)[..., None]), 0.0)
    delta = np.einsum("bthe,bthe->bht", do, o)[..., None]
    dP = np.einsum("bthe,bshe->bhts", do, v)
    dS = p * (dP - delta)
    dv = np.einsum("bhts,bthe->bshe", p, do)
    dq = scale * np.einsum("bhts,bshd->bthd", dS, k)
    dk = scale * np.einsum("bhts,bthd->bshd", dS, q)

    (eps, u, r), T, S, Dv = _rounding(q, k, scale, adm, bf16), q.shape[1], k.shape[1], v.shape[3]
    eps, ado = eps[..., None], np.abs(do)
    tol_dv = np.einsum("bhts,bthe->bshe", (eps + (T + 2) * 2.0 ** -23 + r) * p + FTZ, ado) + u * np.abs(dv) + (T + 1) * FTZ
    inner = np.einsum("bthe,bshe->bhts", ado, np.abs(v)) + np.einsum("bthe,bthe->bht", ado, np.abs(o))[..., None]
    eta = (p * (eps * (np.abs(dP) + np.abs(delta)) + (Dv + 2) * 2.0 ** -23 * inner) + r * np.abs(dS)
           + FTZ * (np.abs(dP) + np.abs(delta) + 1))
    tol_dq = (scale * np.einsum("bhts,bshd->bthd", eta + (S + 2) * 2.0 ** -23 * np.abs(dS), np.abs(k)) + u * np.abs(dq)
              + (S + 1) * FTZ)
    tol_dk = (scale * np.einsum("bhts,bthd->bshd", eta + (T + 2) * 2.0 ** -23 * np.abs(dS), np.abs(q)) + u * np.abs(dk)
              + (T + 1) * FTZ)
    return (dq, dk, dv), (tol_dq, tol_dk, tol_dv)
