"""f64 reference of every stage of the fused MNIST-CNN train step (csrc/kernels/mnist_cnn.hip), shared by
test_mnist_refs_cpu.py and test_mnist_exact_gpu.py.  numpy only, no autograd; nothing here touches a GPU.

Every stage is its own function of that stage's inputs, so a test can feed it either the previous
reference stage (the whole step, `step_ref`) or what the kernel itself stored (the stage-wise bounds).  Each
returns, next to its outputs, the sum of the absolute values of the terms of the output's last reduction
("abs sum"): the input of conv_refs.error_bound_f32 on real data and of the exactness condition on
integer data (conv_refs.assert_exact).

Conventions, as mnist_cnn.h / mnist_cnn.hip state them:

* NHWC, TF weight layouts: w1 [3,3,1,32], w2 [3,3,32,64] (HWIO), w3 [1600,128], w4 [128,10] ([in,out]).
* P1 / A1 are [b,13,13,32], P2 / A2 [b,5,5,64] == [b,1600]: flattened feature f = (ph*5 + pw)*64 + c.
* A pool's argmax code is dy*2 + dx of the window's 2 x 2 cells.  The scan is `if (v > m)` in the order
  0, 1, 2, 3 on the convolution sums (bias and ReLU come after the maximum, they commute with it): the
  FIRST maximum wins, as in test_reference_pool_routes_ties_to_first.
* Where a pooled value is 0 (the maximum + bias is <= 0) the gradient is masked and the argmax carries
  no information the step uses; the tests require only A < 4 there (`argmax_checked`).
* The second pool takes floor(11 / 2) = 5 windows, so only conv2 outputs 0..9 and P1 rows / columns
  0..11 are live.  The kernel stores zeros in P1 / A1 row 12 and column 12; they are not compared
  (`LIVE`).  conv2 is evaluated here on its 10 x 10 used positions only.
* dense1 runs as four partials (part3 [4][b][128]): quarter cq holds conv2 channels 16cq..16cq+15, i.e. the
  features with (f % 64) // 16 == cq (`quarter_of_feature`); H = relu(b3 + the four partials).
* dL = (softmax - onehot) * scale with scale = 1 / global batch; dH and dP2 are stored ReLU-masked
  (H > 0, P2 > 0); dC2 is dP2 at the window's argmax cell and 0 elsewhere.
* Per-image partial slabs: part2 [b][289][64], row = tap*32 + ci (tap = kh*3 + kw), row 288 = db2; the fused
  backward stores it as [b][73][64][4] (row quad, column, row in quad; quad 72 = bias + 3 zero rows), see
  `part2_rows`.  part1 has 2 (k_conv_bwd: pixel halves) or 4 (fused: channel quarters) rows of 320 per image,
  column = tap*32 + c, columns 288.. = db1; an image's rows add up to its conv1 gradient (`part1_image`).
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

LIVE = 12  # P1 / A1 rows and columns 0..11 are compared


def f64(t):
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.asarray(t, np.float64)


def quarter_of_feature(f):
    return (np.asarray(f) % 64) // 16


def argmax_checked(got, want, pooled, what):
    """Argmax bytes equal where the pooled value is positive; below 4 everywhere."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (got < 4).all(), f"{what}: argmax byte {got.max()} > 3"
    sel = np.asarray(pooled) > 0
    bad = np.argwhere(sel & (got != want))
    assert len(bad) == 0, f"{what}: {len(bad)} of {int(sel.sum())} differ, first at {bad[0].tolist()}: " \
                          f"got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


# ------------------------------------------------------------------------------------------- forward
def _patches(x, oh, ow):
    """[b, oh, ow, 9*C] 3 x 3 patches of x [b,H,W,C] in (kh, kw, c) order, for output pixels (0..oh-1, 0..ow-1)."""
    b, H, W, C = x.shape
    v = sliding_window_view(x, (3, 3), axis=(1, 2))[:, :oh, :ow]  # [b, oh, ow, C, 3, 3]
    return np.ascontiguousarray(v.transpose(0, 1, 2, 4, 5, 3)).reshape(b, oh, ow, 9 * C)


def pool_first_max(pre):
    """2 x 2 / stride-2 'valid' max pool of pre [b,H,W,C]: (maximum, argmax code dy*2 + dx, the first
    maximum in code order; number of windows whose maximum is attained more than once)."""
    b, H, W, C = pre.shape
    ph, pw = H // 2, W // 2
    win = np.stack([pre[:, dy:2 * ph:2, dx:2 * pw:2] for dy in (0, 1) for dx in (0, 1)], axis=0)
    arg = win.argmax(0)  # numpy: the first occurrence
    mx = win.max(0)
    return mx, arg.astype(np.uint8), (win == mx).sum(0) > 1


def conv_pool(x, w, bias, oh, ow):
    """relu(maxpool(conv3x3(x, w) + bias)) over conv outputs (0..oh-1, 0..ow-1).  Returns (pre-activations
    conv + bias [b,oh,ow,K], pooled P, argmax A, abs sum of the pre-activations, tie flags of the windows)."""
    x, w, bias = f64(x), f64(w), f64(bias)
    K = w.shape[-1]
    pt = _patches(x, oh, ow)
    pre = pt @ w.reshape(-1, K) + bias
    ab = np.abs(pt) @ np.abs(w.reshape(-1, K)) + np.abs(bias)
    mx, arg, tie = pool_first_max(pre)
    return pre, np.maximum(mx, 0.0), arg, ab, tie


def conv1_pool(x, w1, b1):
    """x [b,28,28,1] -> (C1 [b,26,26,32], P1 [b,13,13,32], A1, abs sum, ties)."""
    return conv_pool(x, w1, b1, 26, 26)


def conv2_pool(P1, w2, b2):
    """P1 [b,13,13,32] -> (C2 [b,10,10,64], P2 [b,1600], A2 [b,1600], abs sum, ties [b,1600])."""
    pre, P, A, ab, tie = conv_pool(P1, w2, b2, 10, 10)
    b = pre.shape[0]
    return pre, P.reshape(b, 1600), A.reshape(b, 1600), ab, tie.reshape(b, 1600)


def dense1_parts(P2, w3):
    """The four quarter partials part3 [4,b,128] of P2 [b,1600] @ w3, and their abs sums."""
    P2, w3 = f64(P2), f64(w3)
    q = quarter_of_feature(np.arange(1600))
    parts = np.stack([P2[:, q == c] @ w3[q == c] for c in range(4)])
    ab = np.stack([np.abs(P2[:, q == c]) @ np.abs(w3[q == c]) for c in range(4)])
    return parts, ab


def dense1(P2, w3, b3):
    """H = relu(b3 + P2 @ w3) [b,128] (1601 terms each) and the abs sum."""
    parts, ab = dense1_parts(P2, w3)
    b3 = f64(b3)
    return np.maximum(parts.sum(0) + b3, 0.0), ab.sum(0) + np.abs(b3)


def dense2(H, w4, b4):
    """logits [b,10] = H @ w4 + b4 (129 terms each) and the abs sum."""
    H, w4, b4 = f64(H), f64(w4), f64(b4)
    return H @ w4 + b4, np.abs(H) @ np.abs(w4) + np.abs(b4)


def softmax_xent(logits, y, scale):
    """(per-row loss [b], correct flags [b] -- the first maximum is the prediction --, dL [b,10] =
    (softmax - onehot) * scale)."""
    lg = f64(logits)
    y = np.asarray(y).astype(np.int64)
    m = lg.max(1, keepdims=True)
    e = np.exp(lg - m)
    se = e.sum(1, keepdims=True)
    rows = np.arange(lg.shape[0])
    loss = (m + np.log(se))[:, 0] - lg[rows, y]
    onehot = np.zeros_like(lg)
    onehot[rows, y] = 1.0
    return loss, lg.argmax(1) == y, (e / se - onehot) * scale


def softmax_xent_saturated(logits, y, scale):
    """The same where every row's top logit leads by >= 128: in f32 exp(lg - max) is exactly 1 for the top
    class and exactly 0 for the others (e^-128 < 2^-184 rounds to 0 even with denormals), so se = 1,
    log(se) = 0, loss = max - lg[y] and dL = (onehot(top) - onehot(y)) * scale.  (In f64 e^-128 is not 0:
    this is the f32 head's value, not an approximation of it.)"""
    lg = f64(logits)
    y = np.asarray(y).astype(np.int64)
    top2 = np.sort(lg, 1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0] >= 128).all(), "softmax_xent_saturated: a logit gap below 128"
    rows = np.arange(lg.shape[0])
    pred = lg.argmax(1)
    d = np.zeros_like(lg)
    d[rows, pred] += 1.0
    d[rows, y] -= 1.0
    return lg[rows, pred] - lg[rows, y], pred == y, d * scale


# ------------------------------------------------------------------------------------------- backward
def dense2_bwd(dL, H, w4):
    """dH [b,128] = (dL @ w4^T) * 1[H > 0] (10 terms each) and the abs sum."""
    dL, H, w4 = f64(dL), f64(H), f64(w4)
    mask = H > 0
    return np.where(mask, dL @ w4.T, 0.0), np.where(mask, np.abs(dL) @ np.abs(w4.T), 0.0)


def dense1_bwd(dH, P2, w3):
    """dP2 [b,1600] = (dH @ w3^T) * 1[P2 > 0] (128 terms each) and the abs sum."""
    dH, P2, w3 = f64(dH), f64(P2), f64(w3)
    mask = P2 > 0
    return np.where(mask, dH @ w3.T, 0.0), np.where(mask, np.abs(dH) @ np.abs(w3.T), 0.0)


def pool2_bwd(dP2, A2):
    """dC2 [b,10,10,64]: the (masked) dP2 of each window at its argmax cell, 0 elsewhere."""
    b = dP2.shape[0]
    d, A = f64(dP2).reshape(b, 5, 5, 64), np.asarray(A2).reshape(b, 5, 5, 64)
    dC = np.zeros((b, 10, 10, 64))
    for q in range(4):
        dC[:, q // 2::2, q % 2::2] = np.where(A == q, d, 0.0)
    return dC


def conv2_wgrad(P1, dC2):
    """Per-image part2 [b,289,64] (rows 0..287 dW2 in (tap, ci) order, row 288 db2) over the 100 used
    positions, and the abs sums."""
    P1, dC2 = f64(P1), f64(dC2)
    b = P1.shape[0]
    pt = _patches(P1, 10, 10).reshape(b, 100, 288)
    d = dC2.reshape(b, 100, 64)
    dw = np.matmul(pt.transpose(0, 2, 1), d)
    ab = np.matmul(np.abs(pt).transpose(0, 2, 1), np.abs(d))
    return (np.concatenate([dw, d.sum(1, keepdims=True)], axis=1),
            np.concatenate([ab, np.abs(d).sum(1, keepdims=True)], axis=1))


def conv2_dgrad(dC2, w2):
    """dP1 [b,13,13,32] = dC2 (*) w2^T (up to 9 taps x 64 channels each) and the abs sum."""
    dC2, w2 = f64(dC2), f64(w2)
    b = dC2.shape[0]
    dP1, ab = np.zeros((b, 13, 13, 32)), np.zeros((b, 13, 13, 32))
    for kh in range(3):
        for kw in range(3):
            dP1[:, kh:kh + 10, kw:kw + 10] += dC2 @ w2[kh, kw].T
            ab[:, kh:kh + 10, kw:kw + 10] += np.abs(dC2) @ np.abs(w2[kh, kw].T)
    return dP1, ab


def pool1_bwd(dP1, P1, A1):
    """dC1 [b,26,26,32]: dP1 * 1[P1 > 0] of each window at its argmax cell."""
    d = np.where(f64(P1) > 0, f64(dP1), 0.0)
    A = np.asarray(A1)
    dC = np.zeros((d.shape[0], 26, 26, 32))
    for q in range(4):
        dC[:, q // 2::2, q % 2::2] = np.where(A == q, d, 0.0)
    return dC


def conv1_wgrad(x, dC1, dC1_err=None):
    """Per-image conv1 gradient [b,320] (columns tap*32 + c, then db1) and the abs sums.  With dC1_err (a
    bound of each dC1 element's own error) also the error that passes through the sum: sum |x| err."""
    x, dC1 = f64(x), f64(dC1)
    b = x.shape[0]
    pt = _patches(x.reshape(b, 28, 28, 1), 26, 26).reshape(b, 676, 9)
    d = dC1.reshape(b, 676, 32)

    def both(v):
        return np.concatenate([np.matmul(np.abs(pt).transpose(0, 2, 1), v).reshape(b, 288), v.sum(1)], axis=1)

    out = np.concatenate([np.matmul(pt.transpose(0, 2, 1), d).reshape(b, 288), d.sum(1)], axis=1)
    if dC1_err is None:
        return out, both(np.abs(d))
    return out, both(np.abs(d)), both(f64(dC1_err).reshape(b, 676, 32))


def dense_wgrads(P2, H, dH, dL):
    """(dW3 [1600,128], db3, dW4 [128,10], db4) summed over the batch (b terms each), and their abs sums."""
    P2, H, dH, dL = f64(P2), f64(H), f64(dH), f64(dL)
    g = (P2.T @ dH, dH.sum(0), H.T @ dL, dL.sum(0))
    ab = (np.abs(P2).T @ np.abs(dH), np.abs(dH).sum(0), np.abs(H).T @ np.abs(dL), np.abs(dL).sum(0))
    return g, ab


# ------------------------------------------------------------------------------------------- the whole step
class Step(dict):
    """A dict whose items are also attributes."""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def step_ref(params, x, y, scale, saturated=False):
    """Every stage of one train step in f64 from (params, x [b,28,28,1], y [b], scale).  Returns (S, AB):
    S the stage outputs by name, AB the abs sum of each output that is a reduction.  S.grads: the eight
    summed gradients in variable order; S.part2 / S.part1: the per-image conv partials.  saturated: the
    loss head of softmax_xent_saturated (integer-coded data)."""
    w1, b1, w2, b2, w3, b3, w4, b4 = [f64(p) for p in params]
    x = f64(x).reshape(-1, 28, 28, 1)
    S, AB = Step(), Step()
    S.C1, S.P1, S.A1, AB.C1, S.tie1 = conv1_pool(x, w1, b1)
    S.C2, S.P2, S.A2, AB.C2, S.tie2 = conv2_pool(S.P1, w2, b2)
    S.part3, AB.part3 = dense1_parts(S.P2, w3)
    S.H, AB.H = dense1(S.P2, w3, b3)
    S.logits, AB.logits = dense2(S.H, w4, b4)
    S.loss, S.correct, S.dL = (softmax_xent_saturated if saturated else softmax_xent)(S.logits, y, scale)
    S.dH, AB.dH = dense2_bwd(S.dL, S.H, w4)
    S.dP2, AB.dP2 = dense1_bwd(S.dH, S.P2, w3)
    S.dC2 = pool2_bwd(S.dP2, S.A2)
    S.part2, AB.part2 = conv2_wgrad(S.P1, S.dC2)
    S.dP1, AB.dP1 = conv2_dgrad(S.dC2, w2)
    S.dC1 = pool1_bwd(S.dP1, S.P1, S.A1)
    S.part1, AB.part1 = conv1_wgrad(x, S.dC1)
    (S.dW3, S.db3, S.dW4, S.db4), (AB.dW3, AB.db3, AB.dW4, AB.db4) = dense_wgrads(S.P2, S.H, S.dH, S.dL)
    p1, p2 = S.part1.sum(0), S.part2.sum(0)
    a1, a2 = AB.part1.sum(0), AB.part2.sum(0)
    S.grads = [p1[:288].reshape(3, 3, 1, 32), p1[288:], p2[:288].reshape(3, 3, 32, 64), p2[288], S.dW3, S.db3,
               S.dW4, S.db4]
    AB.grads = [a1[:288].reshape(3, 3, 1, 32), a1[288:], a2[:288].reshape(3, 3, 32, 64), a2[288], AB.dW3, AB.db3,
                AB.dW4, AB.db4]
    return S, AB


# ------------------------------------------------------------------------------------------- kernel layouts
def part2_rows(buf, b, fused):
    """The kernel's part2 buffer as per-image [b,289,64]: plain [b][289][64], or the fused backward's
    [b][73][64][4] (quad, column, row in quad), whose rows 289..291 (padding of the bias quad) must be 0."""
    a = f64(buf).reshape(-1)
    if not fused:
        return a[:b * 289 * 64].reshape(b, 289, 64)
    q = a[:b * 73 * 256].reshape(b, 73, 64, 4).transpose(0, 1, 3, 2).reshape(b, 292, 64)
    assert not q[:, 289:].any(), "fused part2: the bias quad's padding rows are not zero"
    return q[:, :289]


def part1_image(buf, b, fused):
    """The kernel's part1 rows summed per image [b,320] (f64 sums of 2 or 4 rows)."""
    r = 4 if fused else 2
    return f64(buf).reshape(-1)[:b * r * 320].reshape(b, r, 320).sum(1)


# ------------------------------------------------------------------------------------------- integer-coded inputs
class Coded:
    """Integer-coded ("saturated") inputs of one step, on which every stage of the step is exact in f32:

    pixels in {0..3} (about 40 % zeros), w1 in [-2, 2], w2 in {-1, 0, 1} (half zero; every `tie_every`-th output
    channel keeps only one or two of its 288 weights, so that its sums are small and pool-2 windows tie),
    w3 in {-1, 0, 1} (`w3_zero` zero), w4 = +-2^w4_exp, small integer biases of both signs, lr = 2^-6,
    scale = 1 / global_batch with global_batch a power of two >= b.

    The data set holds a pool of images; `idx` lists, in three chunks of b, images whose top logit leads by
    at least 128 (so the softmax is exactly one-hot in f32), and every fourth of them is labelled with its
    prediction, the others with a class that is not.  `check()` asserts the conditions (a) - (d) of
    test_mnist_exact_gpu.py on the f64 reference of a chunk."""

    def __init__(self, b, R=1, seed=0, w4_exp=None, w3_zero=None, tie_every=2):
        rng = np.random.RandomState(1000 * seed + b)
        self.b, self.R = b, R
        gb = 1
        while gb < b * R:
            gb *= 2
        self.global_batch, self.scale, self.lr = gb, 1.0 / gb, 2.0 ** -6
        if w4_exp is None:
            w4_exp = 3 if b <= 17 else (1 if b <= 65 else 0)
        if w3_zero is None:
            w3_zero = 0.75 if b <= 65 else 0.875
        w1 = rng.randint(-2, 3, (3, 3, 1, 32))
        b1 = rng.randint(-3, 3, (32,))
        w2 = rng.randint(-1, 2, (3, 3, 32, 64)) * (rng.rand(3, 3, 32, 64) < 0.75)  # (a third of randint is 0)
        w2r = w2.reshape(288, 64)  # (a view)
        for c in range(0, 64, tie_every):  # the tie channels: one +1 and, in every other one, a second weight of either sign
            taps = 1 + (c // tie_every) % 2
            r = rng.choice(288, taps, replace=False)
            w2r[:, c] = 0
            w2r[r, c] = rng.choice([-1, 1], taps)
            w2r[r[0], c] = 1
        b2 = rng.randint(-2, 2, (64,))
        b2[0::tie_every] = rng.randint(-1, 1, (len(b2[0::tie_every]),))
        w3 = rng.choice([-1, 1], (1600, 128)) * (rng.rand(1600, 128) >= w3_zero)
        b3 = rng.randint(-8, 9, (128,))
        w4 = rng.choice([-1, 1], (128, 10)) * 2 ** w4_exp
        b4 = rng.randint(-4, 5, (10,))
        self.params = [np.asarray(p, np.float64) for p in (w1, b1, w2, b2, w3, b3, w4, b4)]
        n = 3 * b + 3 * max(4, b // 4)
        X = rng.randint(0, 4, (n, 28, 28, 1)) * (rng.rand(n, 28, 28, 1) < 0.8)
        self.X = X.astype(np.float64)
        _, P1, _, _, _ = conv1_pool(self.X, w1, b1)
        _, P2, _, _, _ = conv2_pool(P1, w2, b2)
        H, _ = dense1(P2, w3, b3)
        lg, _ = dense2(H, w4, b4)
        top2 = np.sort(lg, 1)[:, -2:]
        ok = np.flatnonzero(top2[:, 1] - top2[:, 0] >= 128)
        assert ok.size >= 3 * b, f"b={b}: only {ok.size} of {n} images have a logit gap >= 128"
        self.idx = ok[rng.permutation(ok.size)[:3 * b]].astype(np.int32)
        pred = lg.argmax(1)
        Y = (pred + rng.randint(1, 10, n)) % 10  # a class that is not the prediction
        hit = self.idx[np.arange(3 * b) % 4 == 3]
        Y[hit] = pred[hit]
        self.Y = Y.astype(np.int32)

    def chunk(self, k):
        ids = self.idx[k * self.b:(k + 1) * self.b]
        return self.X[ids], self.Y[ids]

    def ref(self, k):
        x, y = self.chunk(k)
        return step_ref(self.params, x, y, self.scale, saturated=True)

    def check(self, S, AB):
        """Conditions (a) - (d) on a chunk's reference; returns the measured figures."""
        b, s = self.b, self.scale
        lim = 2.0 ** 24
        fwd = max(float(np.max(AB[k])) for k in ("C1", "C2", "H", "logits"))
        fwd = max(fwd, float(AB.part3.sum(0).max()))
        bwd = max(float(np.max(AB[k])) for k in ("dH", "dP2", "dP1", "dW3", "db3", "dW4", "db4"))
        bwd = max(bwd, max(float(np.max(a)) for a in AB.grads)) / s
        assert fwd < lim, f"(a) b={b}: forward abs sum {fwd} >= 2^24"
        assert bwd < lim, f"(a) b={b}: backward abs sum / scale {bwd} >= 2^24"
        top2 = np.sort(S.logits, 1)[:, -2:]
        gap = float((top2[:, 1] - top2[:, 0]).min())
        assert gap >= 128, f"(b) b={b}: logit gap {gap} < 128"
        assert set(np.unique(S.dL / s)) <= {-1.0, 0.0, 1.0} and (S.loss == np.round(S.loss)).all(), "(b) softmax"
        wrong = int((~S.correct).sum())
        assert wrong >= 1 and (b < 8 or 4 * wrong >= b), f"(c) b={b}: {wrong} mispredicted"
        assert b < 4 or wrong < b, f"(c) b={b}: no image is predicted correctly (no all-zero dL row)"
        ties = []
        for P, tie in ((S.P1[:, :LIVE, :LIVE], S.tie1[:, :LIVE, :LIVE]), (S.P2, S.tie2)):
            pos = P > 0
            ties.append(float((tie & pos).sum()) / max(1, int(pos.sum())))
        assert min(ties) >= 0.05, f"(d) b={b}: {ties[0]:.3f} / {ties[1]:.3f} of the positive windows of pool 1 / 2 tie"
        # the SGD update itself is exact
        for p, g in zip(self.params, S.grads):
            w = p - self.lr * g
            assert np.array_equal(w.astype(np.float32).astype(np.float64), w), "W - lr G is not exact in f32"
        return dict(fwd=fwd, bwd=bwd, gap=gap, wrong=wrong, tie1=ties[0], tie2=ties[1])


# every (per-replica batch, replicas) the exact GPU test runs; the generator and the f64 reference of a chunk
# are computed once per process and shared (the tests do not modify them)
CODED_CASES = [(1, 1), (8, 1), (8, 2), (16, 1), (17, 1), (17, 2), (64, 1), (64, 2), (65, 1), (128, 1), (129, 1),
               (256, 1)]
_coded, _coded_ref = {}, {}


def coded(b, R=1):
    if (b, R) not in _coded:
        _coded[(b, R)] = Coded(b, R)
    return _coded[(b, R)]


def coded_ref(b, R=1, k=1):
    """(S, AB) of chunk k of coded(b, R), with the conditions (a) - (d) asserted."""
    if (b, R, k) not in _coded_ref:
        c = coded(b, R)
        S, AB = c.ref(k)
        c.check(S, AB)
        _coded_ref[(b, R, k)] = (S, AB)
    return _coded_ref[(b, R, k)]
