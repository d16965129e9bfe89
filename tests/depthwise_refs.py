"""float64 numpy references of the depthwise convolution (x [N,H,W,C], w [kh,kw,C,dm], y [N,OH,OW,C*dm], output
channel c*dm + m reads input channel c): a plain loop over the taps of the definition.  Every function also
returns the sum of the absolute values of its terms, which the error bounds of the tests need."""
import numpy as np


def same_pads(size, k, s, d):
    total = max((-(-size // s) - 1) * s + (k - 1) * d + 1 - size, 0)
    return total // 2, total - total // 2


def geometry(shape, k, s, d, padding):
    """(pads (top, bottom, left, right), OH, OW) of TF 'same' / 'valid' padding."""
    ph = same_pads(shape[1], k[0], s[0], d[0]) if padding == "same" else (0, 0)
    pw = same_pads(shape[2], k[1], s[1], d[1]) if padding == "same" else (0, 0)
    oh = (shape[1] + sum(ph) - (k[0] - 1) * d[0] - 1) // s[0] + 1
    ow = (shape[2] + sum(pw) - (k[1] - 1) * d[1] - 1) // s[1] + 1
    return (ph[0], ph[1], pw[0], pw[1]), oh, ow


def _taps(x_shape, w, s, d, pads, oh, ow):
    """(padded zero array shape, [(i, j, index of the [N,OH,OW,C] window of tap (i, j) in the padded array)])."""
    kh, kw = w.shape[:2]
    hp = max((oh - 1) * s[0] + (kh - 1) * d[0] + 1, pads[0] + x_shape[1])
    wp = max((ow - 1) * s[1] + (kw - 1) * d[1] + 1, pads[2] + x_shape[2])
    idx = [(i, j, (slice(None), slice(i * d[0], i * d[0] + (oh - 1) * s[0] + 1, s[0]),
                   slice(j * d[1], j * d[1] + (ow - 1) * s[1] + 1, s[1])))
           for i in range(kh) for j in range(kw)]
    return (x_shape[0], hp, wp, x_shape[3]), idx


def _padded(x, shape, pads):
    xp = np.zeros(shape, dtype=np.float64)
    xp[:, pads[0]:pads[0] + x.shape[1], pads[2]:pads[2] + x.shape[2]] = x
    return xp


def forward(x, w, b, s, d, pads, oh, ow):
    """(y before any activation, sum |x w| + |b|)"""
    shape, taps = _taps(x.shape, w, s, d, pads, oh, ow)
    xp, w = _padded(x, shape, pads), w.astype(np.float64)
    y = np.zeros((x.shape[0], oh, ow) + w.shape[2:])
    mag = np.zeros_like(y)
    for i, j, ix in taps:
        t = xp[ix][..., None] * w[i, j]
        y += t
        mag += np.abs(t)
    if b is not None:
        y += b.astype(np.float64).reshape(w.shape[2:])
        mag += np.abs(b.astype(np.float64)).reshape(w.shape[2:])
    return y.reshape(y.shape[:3] + (-1,)), mag.reshape(y.shape[:3] + (-1,))


def dgrad(dy, w, x_shape, s, d, pads):
    """(dx, sum |dy w|)"""
    oh, ow = dy.shape[1:3]
    shape, taps = _taps(x_shape, w, s, d, pads, oh, ow)
    w = w.astype(np.float64)
    dy5 = dy.astype(np.float64).reshape(dy.shape[:3] + w.shape[2:])
    dxp, mag = np.zeros(shape), np.zeros(shape)
    for i, j, ix in taps:
        dxp[ix] += (dy5 * w[i, j]).sum(-1)
        mag[ix] += np.abs(dy5 * w[i, j]).sum(-1)
    crop = (slice(None), slice(pads[0], pads[0] + x_shape[1]), slice(pads[2], pads[2] + x_shape[2]))
    return dxp[crop], mag[crop]


def wgrad(x, dy, k, dm, s, d, pads):
    """(dW, sum |dy x| per dW element, db, sum |dy| per db element)"""
    oh, ow = dy.shape[1:3]
    w = np.zeros(tuple(k) + (x.shape[3], dm))
    shape, taps = _taps(x.shape, w, s, d, pads, oh, ow)
    xp = _padded(x, shape, pads)
    dy5 = dy.astype(np.float64).reshape(dy.shape[:3] + w.shape[2:])
    mag = np.zeros_like(w)
    for i, j, ix in taps:
        t = dy5 * xp[ix][..., None]
        w[i, j] = t.sum((0, 1, 2))
        mag[i, j] = np.abs(t).sum((0, 1, 2))
    return w, mag, dy5.sum((0, 1, 2)).reshape(-1), np.abs(dy5).sum((0, 1, 2)).reshape(-1)
