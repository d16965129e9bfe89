"""float64 numpy references of the grouped convolution (x [N,H,W,C], w [kh,kw,C/g,F], filter f in group f // (F/g)):
plain loops over groups and taps.  Every function also returns the sum of the absolute values of its terms."""
import numpy as np

from depthwise_refs import _padded, _taps, geometry  # noqa: F401  (the same 'same' / 'valid' geometry)


def _groups(C, F, g):
    return [(slice(j * (C // g), (j + 1) * (C // g)), slice(j * (F // g), (j + 1) * (F // g))) for j in range(g)]


def forward(x, w, b, g, s, d, pads, oh, ow):
    """(y before any activation, sum |x w| + |b|)"""
    shape, taps = _taps(x.shape, w, s, d, pads, oh, ow)
    xp, w = _padded(x, shape, pads), w.astype(np.float64)
    y = np.zeros((x.shape[0], oh, ow, w.shape[3]))
    mag = np.zeros_like(y)
    for cs, fs in _groups(x.shape[3], w.shape[3], g):
        for i, j, ix in taps:
            y[..., fs] += xp[ix][..., cs] @ w[i, j, :, fs]
            mag[..., fs] += np.abs(xp[ix][..., cs]) @ np.abs(w[i, j, :, fs])
    if b is not None:
        y += b.astype(np.float64)
        mag += np.abs(b.astype(np.float64))
    return y, mag


def dgrad(dy, w, g, x_shape, s, d, pads):
    """(dx, sum |dy w|)"""
    shape, taps = _taps(x_shape, w, s, d, pads, dy.shape[1], dy.shape[2])
    w, dy = w.astype(np.float64), dy.astype(np.float64)
    dxp, mag = np.zeros(shape), np.zeros(shape)
    for cs, fs in _groups(x_shape[3], w.shape[3], g):
        for i, j, ix in taps:
            dxp[ix + (cs,)] += dy[..., fs] @ w[i, j, :, fs].T
            mag[ix + (cs,)] += np.abs(dy[..., fs]) @ np.abs(w[i, j, :, fs]).T
    crop = (slice(None), slice(pads[0], pads[0] + x_shape[1]), slice(pads[2], pads[2] + x_shape[2]))
    return dxp[crop], mag[crop]


def wgrad(x, dy, k, g, s, d, pads):
    """(dW, sum |dy x| per dW element, db, sum |dy| per db element)"""
    w = np.zeros(tuple(k) + (x.shape[3] // g, dy.shape[3]))
    shape, taps = _taps(x.shape, w, s, d, pads, dy.shape[1], dy.shape[2])
    xp, dy = _padded(x, shape, pads), dy.astype(np.float64)
    mag = np.zeros_like(w)
    for cs, fs in _groups(x.shape[3], dy.shape[3], g):
        for i, j, ix in taps:
            w[i, j, :, fs] = np.einsum("nhwc,nhwk->ck", xp[ix][..., cs], dy[..., fs])
            mag[i, j, :, fs] = np.einsum("nhwc,nhwk->ck", np.abs(xp[ix][..., cs]), np.abs(dy[..., fs]))
    return w, mag, dy.sum((0, 1, 2)), np.abs(dy).sum((0, 1, 2))
