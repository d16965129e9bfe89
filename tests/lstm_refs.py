"""References of the LSTM scan kernels (csrc/kernels/lstm.h): float64, and an emulation of the kernels' contract
(f32 products summed in f32, sigma(z) = 1 / (1 + exp(-z)) and tanh(z) = 2 sigma(2 z) - 1 with numpy's f32 exp, one
rounding per operation; bf16: R, every stored h, the saved gates and dZ rounded where the kernels round)."""
import numpy as np

import kernel_refs as KR


def _bf16(v):
    return KR.bf16_bits_to_f64(KR.bf16_rne(np.asarray(v, dtype=np.float32))).astype(np.float32)


def lstm_scan_ref(zx, R, h0=None, c0=None, dhs=None, dh_last=None, dc_last=None, rev=False, mode="f64"):
    """Forward and backward of the scan.  zx [B,T,4U] and dz by time, hs / dhs by processing step.  mode: "f64" (the
    reference), "f32" or "bf16" (the emulations).  Returns hs, h_last, c_last, dz, dh0, dc0 as float64."""
    ft = np.float64 if mode == "f64" else np.float32
    st = _bf16 if mode == "bf16" else (lambda v: v)  # what a store in the data's dtype keeps
    one, two = ft(1), ft(2)
    if mode == "f64":
        sig, tanh = (lambda z: one / (one + np.exp(-z))), np.tanh
    else:
        sig = lambda z: one / (one + np.exp(-z, dtype=ft))  # noqa: E731
        tanh = lambda z: two * sig(two * z) - one  # noqa: E731
    B, T, U = zx.shape[0], zx.shape[1], zx.shape[2] // 4
    zx, R = zx.astype(ft), st(R.astype(ft))
    h = st(h0.astype(ft)) if h0 is not None else np.zeros((B, U), ft)
    c = c0.astype(ft) if c0 is not None else np.zeros((B, U), ft)
    cprev0, hs, gates, cs = c, [], [], []
    with np.errstate(over="ignore"):
        for s in range(T):
            z = zx[:, T - 1 - s if rev else s] + h @ R
            i, f, g, o = sig(z[:, :U]), sig(z[:, U:2 * U]), tanh(z[:, 2 * U:3 * U]), sig(z[:, 3 * U:])
            c = f * c + i * g
            h = st(o * tanh(c))
            hs.append(h), cs.append(c), gates.append([st(v) for v in (i, f, g, o)])
        dh = st(dh_last.astype(ft)) if dh_last is not None else np.zeros((B, U), ft)
        dc = dc_last.astype(ft) if dc_last is not None else np.zeros((B, U), ft)
        dz = np.zeros((B, T, 4 * U), ft)
        for s in range(T - 1, -1, -1):
            i, f, g, o = gates[s]
            cp = cs[s - 1] if s > 0 else cprev0
            d = dh + dhs[:, s].astype(ft) if dhs is not None else dh
            tc = tanh(cs[s])
            zo = d * tc * (o * (one - o))
            dcv = dc + d * o * (one - tc * tc)
            zi, zf, zg = dcv * g * (i * (one - i)), dcv * cp * (f * (one - f)), dcv * i * (one - g * g)
            dc = dcv * f
            zt = st(np.concatenate([zi, zf, zg, zo], 1))
            dz[:, T - 1 - s if rev else s] = zt
            dh = zt @ R.T
    f8 = lambda v: np.asarray(v, dtype=np.float64)  # noqa: E731
    return dict(hs=f8(np.stack(hs, 1)), h_last=f8(hs[-1]), c_last=f8(cs[-1]), dz=f8(dz), dh0=f8(st(dh)), dc0=f8(dc))
