"""References of the GRU scan kernels (csrc/kernels/gru.h): float64, and an emulation of the kernels' contract (f32
products summed in f32, sigma(z) = 1 / (1 + exp(-z)) and tanh(z) = 2 sigma(2 z) - 1 with numpy's f32 exp, one rounding
per operation; bf16: R, every stored h, the saved planes, dzx and dzh rounded where the kernels round)."""
import numpy as np

import kernel_refs as KR


def _bf16(v):
    return KR.bf16_bits_to_f64(KR.bf16_rne(np.asarray(v, dtype=np.float32))).astype(np.float32)


def gru_scan_ref(zx, R, b_rec=None, h0=None, dhs=None, dh_last=None, rev=False, mode="f64"):
    """Forward and backward of the scan.  zx [B,T,3U], dzx and dzh by time, hs / dhs by processing step.  mode: "f64"
    (the reference), "f32" or "bf16" (the emulations).  Returns hs, h_last, dzx, dzh, dh0 as float64."""
    ft = np.float64 if mode == "f64" else np.float32
    st = _bf16 if mode == "bf16" else (lambda v: v)  # what a store in the data's dtype keeps
    one, two = ft(1), ft(2)
    if mode == "f64":
        sig, tanh = (lambda z: one / (one + np.exp(-z))), np.tanh
    else:
        sig = lambda z: one / (one + np.exp(-z, dtype=ft))  # noqa: E731
        tanh = lambda z: two * sig(two * z) - one  # noqa: E731
    B, T, U = zx.shape[0], zx.shape[1], zx.shape[2] // 3
    zx, R = zx.astype(ft), st(R.astype(ft))
    b = b_rec.astype(ft) if b_rec is not None else np.zeros(3 * U, ft)
    h = st(h0.astype(ft)) if h0 is not None else np.zeros((B, U), ft)
    hprev, saved = [], []
    with np.errstate(over="ignore"):
        for s in range(T):
            m = zx[:, T - 1 - s if rev else s]
            mh = h @ R
            z, r = sig((m[:, :U] + b[:U]) + mh[:, :U]), sig((m[:, U:2 * U] + b[U:2 * U]) + mh[:, U:2 * U])
            q = b[2 * U:] + mh[:, 2 * U:]
            hh = tanh(m[:, 2 * U:] + r * q)
            hprev.append(h)
            h = st(z * h + (one - z) * hh)
            saved.append([st(v) for v in (z, r, hh, q)])
        hs = hprev[1:] + [h]
        dh = st(dh_last.astype(ft)) if dh_last is not None else np.zeros((B, U), ft)
        dzx, dzh = np.zeros((B, T, 3 * U), ft), np.zeros((B, T, 3 * U), ft)
        for s in range(T - 1, -1, -1):
            z, r, hh, q = saved[s]
            d = dh + dhs[:, s].astype(ft) if dhs is not None else dh
            omz = one - z
            ah = (d * omz) * (one - hh * hh)
            az = (d * (hprev[s] - hh)) * (z * omz)
            ar = (ah * q) * (r * (one - r))
            t = T - 1 - s if rev else s
            dzx[:, t] = st(np.concatenate([az, ar, ah], 1))
            dzh[:, t] = st(np.concatenate([az, ar, ah * r], 1))
            dh = d * z + dzh[:, t] @ R.T
    f8 = lambda v: np.asarray(v, dtype=np.float64)  # noqa: E731
    return dict(hs=f8(np.stack(hs, 1)), h_last=f8(hs[-1]), dzx=f8(dzx), dzh=f8(dzh), dh0=f8(st(dh)))
