"""float64 numpy references of the transposed convolution (x [N,H,W,C], w [kh,kw,F,C], y [N,OH,OW,F]) in its
scatter form: tap (i, j) sends input pixel (iy, ix) to output pixel (iy sh - pt + i dh, ix sw - pl + j dw).  Every
function also returns the sum of the absolute values of its terms."""
import numpy as np

# x [N,H,W,C], F, kernel, strides, dilation, padding, output_padding, fused ReLU
CASES = [
    ((1, 1, 1, 4), 4, (1, 1), (1, 1), (1, 1), "valid", None, 0),     # one pixel
    ((1, 1, 2, 4), 8, (3, 3), (1, 1), (1, 1), "same", None, 0),      # kernel larger than the image
    ((2, 3, 4, 8), 16, (4, 4), (2, 2), (1, 1), "same", None, 0),     # four phases of 2 x 2 taps
    ((2, 3, 4, 8), 16, (4, 4), (2, 2), (1, 1), "same", None, 1),
    ((2, 3, 4, 8), 8, (3, 3), (2, 2), (1, 1), "same", None, 1),      # phases with 2 and 1 taps, asymmetric pads
    ((1, 4, 3, 4), 4, (2, 2), (3, 3), (1, 1), "valid", None, 0),     # ke < s: phases with no tap, bias-only pixels
    ((2, 3, 3, 6), 5, (3, 3), (2, 2), (1, 1), "valid", (1, 1), 0),   # per-element loads, odd F, untouched last row
    ((2, 3, 3, 6), 5, (3, 3), (2, 2), (1, 1), "same", (1, 0), 0),    # per-element loads, 'same', mixed output_padding
    ((1, 4, 4, 4), 4, (3, 3), (2, 2), (2, 2), "valid", None, 0),     # dilation and stride share a factor
    ((1, 5, 4, 4), 4, (3, 2), (1, 2), (2, 1), "same", None, 0),      # non-square kernel, mixed stride and dilation
    ((1, 6, 6, 40), 72, (3, 3), (2, 2), (1, 1), "same", None, 0),    # k-chunks, two filter blocks, a short tile
    ((1, 20, 37, 8), 8, (4, 4), (2, 2), (1, 1), "same", None, 0),    # several pixel tiles per phase, a short last one
    ((4, 16, 16, 16), 16, (3, 3), (2, 2), (1, 1), "same", None, 0),  # 1024-pixel wgrad reduction, split
]
IDS = [f"{'x'.join(map(str, c[0]))}-F{c[1]}-k{c[2][0]}x{c[2][1]}-s{c[3][0]}{c[3][1]}-d{c[4][0]}{c[4][1]}-{c[5]}-"
       f"op{c[6]}-act{c[7]}".replace(" ", "") for c in CASES]


def geometry(shape, k, s, d, padding, op=None):
    """(OH, OW, pt, pl): the sizes and leading crops of the layer's rules."""
    out = []
    for a in (0, 1):
        ke = (k[a] - 1) * d[a] + 1
        if op is None:
            o = shape[1 + a] * s[a] + (max(ke - s[a], 0) if padding == "valid" else 0)
        else:
            o = (shape[1 + a] - 1) * s[a] + ke + op[a] - (2 * (ke // 2) if padding == "same" else 0)
        lead = 0 if padding == "valid" else max((-(-o // s[a]) - 1) * s[a] + ke - o, 0) // 2
        out.append((o, lead))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def _taps(H, W, oh, ow, k, s, d, pt, pl):
    """[(i, j, input window, output window)]: the input pixels tap (i, j) sends into the image, and where."""
    def axis(n, o, i, s_, d_, p):
        q = [q for q in range(n) if 0 <= q * s_ - p + i * d_ < o]
        return (slice(q[0], q[-1] + 1), slice(q[0] * s_ - p + i * d_, q[-1] * s_ - p + i * d_ + 1, s_)) if q else None
    taps = []
    for i in range(k[0]):
        for j in range(k[1]):
            ay, ax = axis(H, oh, i, s[0], d[0], pt), axis(W, ow, j, s[1], d[1], pl)
            if ay and ax:
                taps.append((i, j, (slice(None), ay[0], ax[0]), (slice(None), ay[1], ax[1])))
    return taps


def forward(x, w, b, s, d, geo):
    """(y before any activation, sum |x w| + |b|)"""
    oh, ow, pt, pl = geo
    x, w = x.astype(np.float64), w.astype(np.float64)
    y = np.zeros((x.shape[0], oh, ow, w.shape[2]))
    mag = np.zeros_like(y)
    for i, j, src, dst in _taps(x.shape[1], x.shape[2], oh, ow, w.shape[:2], s, d, pt, pl):
        y[dst] += x[src] @ w[i, j].T
        mag[dst] += np.abs(x[src]) @ np.abs(w[i, j]).T
    if b is not None:
        y += b.astype(np.float64)
        mag += np.abs(b.astype(np.float64))
    return y, mag


def dgrad(dy, w, x_shape, s, d, geo):
    """(dx, sum |dy w|)"""
    oh, ow, pt, pl = geo
    dy, w = dy.astype(np.float64), w.astype(np.float64)
    dx, mag = np.zeros(x_shape), np.zeros(x_shape)
    for i, j, src, dst in _taps(x_shape[1], x_shape[2], oh, ow, w.shape[:2], s, d, pt, pl):
        dx[src] += dy[dst] @ w[i, j]
        mag[src] += np.abs(dy[dst]) @ np.abs(w[i, j])
    return dx, mag


def wgrad(x, dy, k, s, d, geo):
    """(dW, sum |dy x| per dW element, db, sum |dy| per db element)"""
    oh, ow, pt, pl = geo
    x, dy = x.astype(np.float64), dy.astype(np.float64)
    w = np.zeros(tuple(k) + (dy.shape[3], x.shape[3]))
    mag = np.zeros_like(w)
    for i, j, src, dst in _taps(x.shape[1], x.shape[2], oh, ow, k, s, d, pt, pl):
        w[i, j] = np.einsum("nhwf,nhwc->fc", dy[dst], x[src])
        mag[i, j] = np.einsum("nhwf,nhwc->fc", np.abs(dy[dst]), np.abs(x[src]))
    return w, mag, dy.sum((0, 1, 2)), np.abs(dy).sum((0, 1, 2))
