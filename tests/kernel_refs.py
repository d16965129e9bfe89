"""High-precision references of the small per-step kernels (optimizer updates, the f32 -> bf16 slab
cast, softmax cross-entropy, batch norm, max pool), shared by test_kernel_refs_cpu.py,
test_slab_kernels_gpu.py, test_head_gpu.py, test_bn_edges_gpu.py and test_pool_edges_gpu.py.  numpy only;
nothing here touches a GPU.

The optimizer references take the hyper-parameters as the kernels receive them: rounded to f32 and
widened to f64 (``f32(0.999)``), so the representation error of a constant is not counted against
a kernel.  The formulas are those of keras/optimizers.py.
"""
import numpy as np


def f32(x) -> float:
    """The f32 value a kernel receives for the Python number ``x``, as an f64."""
    return float(np.float32(x))


def ulp32(x):
    """Spacing of f32 at |x| (elementwise, f64 in and out; at least the smallest normal's)."""
    a = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


# ------------------------------------------------------------------------------------- bf16
def bf16_rne(x) -> np.ndarray:
    """bf16 bits (uint16) of f32 ``x``: round to nearest, ties to even; Inf stays Inf, a NaN stays a
    NaN (quieted, sign kept) whatever its payload."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (u >> 16) | 0x0040, r)
    return r.astype(np.uint16)


def bf16_bits_to_f64(b) -> np.ndarray:
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_is_nan(b) -> np.ndarray:
    return (np.asarray(b, dtype=np.uint16) & 0x7FFF) > 0x7F80


SPECIALS_F32 = np.array(
    [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF,  # +-0, +-Inf, +-largest finite
     0x00000001, 0x80000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x00800000,  # denormals, smallest normal
     0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # exact halfway: down to even, up to even (both signs)
     0x3F808001, 0x3F807FFF, 0x7F7F8000, 0x7F7F7FFF],  # next to halfway; halfway that rounds to Inf; just below
    dtype=np.uint32).view(np.float32)
# payloads the integer `u + 0x7fff + lsb` rounding carries out of: it gives +Inf, -0 and +0 for them
NAN_PAYLOADS_F32 = np.array([0x7F800001, 0x7FFFFFFF, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)


# ------------------------------------------------------------------------------------- optimizers
# Every update takes and returns f64 arrays (new arrays; the inputs are left alone).
def sgd_ref(w, g, lr, v=None, momentum=0.0, nesterov=False):
    lr = f32(lr)
    if v is None:
        return w - lr * g, None
    m = f32(momentum)
    v = m * v - lr * g
    w = w + (m * v - lr * g if nesterov else v)
    return w, v


def adam_ref(w, g, m, v, vhat, lr, t, b1, b2, eps, wd=0.0):
    """Adam / AdamW (wd != 0: decoupled decay w *= 1 - lr wd first) / AMSGrad (vhat given) at step t >= 1."""
    lr, b1, b2, eps, wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    lr_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    if wd != 0.0:
        w = w * (1.0 - lr * wd)
    m = m * b1 + g * (1.0 - b1)
    v = v * b2 + g * g * (1.0 - b2)
    vv = v
    if vhat is not None:
        vhat = np.maximum(vhat, v)
        vv = vhat
    w = w - lr_t * m / (np.sqrt(vv) + eps)
    return w, m, v, vhat


def rmsprop_ref(w, g, rms, mom, mg, lr, rho, momentum, eps):
    """RMSprop; mom given: with momentum; mg given: centered.  Returns (w, rms, mom, mg, denom)."""
    lr, rho, momentum, eps = f32(lr), f32(rho), f32(momentum), f32(eps)
    rms = rms * rho + g * g * (1.0 - rho)
    denom = rms
    if mg is not None:
        mg = mg * rho + g * (1.0 - rho)
        denom = rms - mg * mg
    step = g / (np.sqrt(denom) + eps)
    if mom is not None:
        mom = mom * momentum + lr * step
        w = w - mom
    else:
        w = w - lr * step
    return w, rms, mom, mg, denom


def adagrad_ref(w, g, acc, lr, eps):
    lr, eps = f32(lr), f32(eps)
    acc = acc + g * g
    return w - lr * g / (np.sqrt(acc) + eps), acc


# ------------------------------------------------------------------------------------- cross-entropy
def xent_ref(z, labels):
    """f64 sparse softmax cross-entropy of logits z [N, K]: (loss [N], lse [N], softmax [N, K], dz [N, K]).
    A label outside [0, K) contributes no loss and no one-hot term (what the kernels do)."""
    z = np.asarray(z, dtype=np.float64)
    N, K = z.shape
    mx = z.max(axis=1, keepdims=True)
    e = np.exp(z - mx)
    se = e.sum(axis=1, keepdims=True)
    lse = (mx + np.log(se))[:, 0]
    p = e / se
    labels = np.asarray(labels, dtype=np.int64)
    valid = (labels >= 0) & (labels < K)
    rows = np.nonzero(valid)[0]
    loss = np.zeros(N)
    loss[rows] = lse[rows] - z[rows, labels[rows]]
    dz = p.copy()
    dz[rows, labels[rows]] -= 1.0
    return loss, lse, p, dz


def xent_emul_f32(z, labels):
    """The kernels' order of operations in f32: max, then sum exp(z - max), then max + log, loss =
    lse - z[label], dz = exp(z - lse) - onehot.  Used only to size tolerances."""
    z = np.asarray(z, dtype=np.float32)
    N, K = z.shape
    mx = z.max(axis=1, keepdims=True)
    e = np.exp(z - mx, dtype=np.float32)
    se = np.zeros((N, 1), dtype=np.float32)
    for k in range(K):  # (sequential f32 sum: no pairwise tree that would be more accurate than a kernel)
        se[:, 0] += e[:, k]
    lse = (mx + np.log(se, dtype=np.float32)).astype(np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    valid = (labels >= 0) & (labels < K)
    rows = np.nonzero(valid)[0]
    loss = np.zeros(N, dtype=np.float32)
    loss[rows] = lse[rows, 0] - z[rows, labels[rows]]
    dz = np.exp(z - lse, dtype=np.float32)
    dz[rows, labels[rows]] -= np.float32(1.0)
    return loss.astype(np.float64), lse[:, 0].astype(np.float64), dz.astype(np.float64)


# ------------------------------------------------------------------------------------- batch norm
def ulp_bf16(x):
    """Spacing of bf16 at |x| (elementwise, f64 in and out; at least the smallest normal's)."""
    a = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


def _relu(v):
    """max(v, 0) of the f64 reference: a NaN stays a NaN."""
    return np.maximum(v, 0.0)


def _relu_fmaxf(v):
    """max(v, 0) as the kernels' fmaxf takes it (the emulations): a NaN pre-activation gives 0."""
    return np.where(v > 0, v, 0.0)


def bn_fwd_ref(x, gamma, beta, moving_mean, moving_var, momentum, eps, residual=None, mean_off=None, relu=False):
    """f64 training batch norm of x [M, C] (csrc/kernels/bn.h): dict of mean, var (biased), invstd, scale,
    shift, pre (x*scale + shift [+ residual], before the ReLU), y, and moving_mean / moving_var (None
    without moving statistics).  Keras momentum convention (moving = moving*m + batch*(1-m)); the moving
    variance is unbiased (left as computed when M == 1); mean_off shifts the moving mean only.  Parameters
    and hyper-parameters are f32 values widened to f64; the variance is two-pass."""
    x = np.asarray(x, dtype=np.float64)
    M, C = x.shape
    g = np.ones(C) if gamma is None else np.asarray(gamma, dtype=np.float64)
    b = np.zeros(C) if beta is None else np.asarray(beta, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mu = x.sum(axis=0) / M
        var = ((x - mu) ** 2).sum(axis=0) / M
        inv = 1.0 / np.sqrt(var + f32(eps))
        scale = g * inv
        shift = b - mu * scale
        pre = x * scale + shift
        if residual is not None:
            pre = pre + np.asarray(residual, dtype=np.float64)
        out = dict(mean=mu, var=var, invstd=inv, scale=scale, shift=shift, pre=pre, y=_relu(pre) if relu else pre,
                   moving_mean=None, moving_var=None)
        if moving_mean is not None:
            m = f32(momentum)
            unb = var * M / (M - 1) if M > 1 else var
            mu_o = mu if mean_off is None else mu + np.asarray(mean_off, dtype=np.float64)
            out["moving_mean"] = np.asarray(moving_mean, dtype=np.float64) * m + mu_o * (1.0 - m)
            out["moving_var"] = np.asarray(moving_var, dtype=np.float64) * m + unb * (1.0 - m)
    return out


def bn_bwd_ref(dy, x, gamma, mean, invstd, mode, scale=None, shift=None, y=None, dgamma0=None, dbeta0=None):
    """f64 batch-norm backward: dict of dz, dgamma, dbeta, dx.  mode 0: dz = dy; mode 1: dy masked by the
    sign of this reference's own x*scale + shift; mode 2: dy masked by y > 0.  dgamma0 / dbeta0: existing
    values the sums are added into (the kernels' `acc` bits).  mean / invstd: the reference forward's."""
    dy, x = np.asarray(dy, dtype=np.float64), np.asarray(x, dtype=np.float64)
    M, C = x.shape
    g = np.ones(C) if gamma is None else np.asarray(gamma, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == 1:
            dz = np.where(x * scale + shift > 0, dy, 0.0)
        elif mode == 2:
            dz = np.where(np.asarray(y, dtype=np.float64) > 0, dy, 0.0)
        else:
            dz = dy
        xhat = (x - mean) * invstd
        db = dz.sum(axis=0)
        dg = (dz * xhat).sum(axis=0)
        dx = g * invstd * (dz - db / M - xhat * dg / M)
    return dict(dz=dz, dgamma=dg if dgamma0 is None else np.asarray(dgamma0, dtype=np.float64) + dg,
                dbeta=db if dbeta0 is None else np.asarray(dbeta0, dtype=np.float64) + db, dx=dx)


def _seq_sums_f32(a, b):
    """Per channel (sum a, sum a*b) over rows, sequentially in f32 with one rounding per fma (the product
    of two f32 is exact in f64) -- no pairwise tree, which would be more accurate than a kernel."""
    s = np.zeros(a.shape[1], dtype=np.float32)
    q = np.zeros(a.shape[1], dtype=np.float32)
    for r in range(a.shape[0]):
        s = s + a[r]
        q = (a[r].astype(np.float64) * b[r].astype(np.float64) + q.astype(np.float64)).astype(np.float32)
    return s, q


def _fma32(a, b, c):
    """f32 fma(a, b, c): the exact product added in f64, rounded to f32."""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def _store(v, bf16):
    """f32 values as the kernels store them (bf16: rounded to nearest even), as f64."""
    return bf16_bits_to_f64(bf16_rne(v)) if bf16 else np.asarray(v, np.float32).astype(np.float64)


def bn_fwd_emul_f32(x, gamma, beta, moving_mean, moving_var, momentum, eps, residual=None, mean_off=None,
                    relu=False, bf16=False):
    """bn_fwd_ref's outputs by the kernels' formulas in their precision: f32 sequential sums of x and x*x,
    mean / variance (Q/M - mean^2) from them in f64, f32 parameters, y = f32 fma(x, scale, shift).  Used
    only to size tolerances."""
    x = np.asarray(x, dtype=np.float32)
    M, C = x.shape
    g = np.ones(C, np.float32) if gamma is None else np.asarray(gamma, np.float32)
    b = np.zeros(C, np.float32) if beta is None else np.asarray(beta, np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        S, Q = _seq_sums_f32(x, x)
        mu = S.astype(np.float64) / M
        var = Q.astype(np.float64) / M - mu * mu
        var = np.where(var < 0, 0.0, var)
        inv = (1.0 / np.sqrt(var + f32(eps))).astype(np.float32)
        scale = g * inv
        shift = b - mu.astype(np.float32) * g * inv
        pre = _fma32(x, scale, shift)
        if residual is not None:
            pre = pre + np.asarray(residual, np.float32)
        y = _relu_fmaxf(pre).astype(np.float32) if relu else pre
        out = dict(mean=mu.astype(np.float32).astype(np.float64), var=var, invstd=inv.astype(np.float64),
                   scale=scale.astype(np.float64), shift=shift.astype(np.float64), pre=pre.astype(np.float64),
                   y=_store(y, bf16), moving_mean=None, moving_var=None)
        if moving_mean is not None:
            m = np.float32(momentum)
            unb = var * M / (M - 1) if M > 1 else var
            mu_o = mu.astype(np.float32) + (np.float32(0) if mean_off is None else np.asarray(mean_off, np.float32))
            one_m = np.float32(1) - m
            out["moving_mean"] = (np.asarray(moving_mean, np.float32) * m + mu_o * one_m).astype(np.float64)
            out["moving_var"] = (np.asarray(moving_var, np.float32) * m + unb.astype(np.float32) * one_m).astype(np.float64)
    return out


def bn_bwd_emul_f32(dy, x, gamma, mean, invstd, mode, scale=None, shift=None, y=None, dgamma0=None, dbeta0=None,
                    bf16=False):
    """bn_bwd_ref's outputs by the kernels' formulas in their precision: f32 sequential sums of dz and
    dz*x, the coefficients from them in f64 rounded to f32, dx = f32 fma(A, dz, fma(B, x, D)).  mean /
    invstd / scale / shift: the f32 emulation's forward statistics.  Used only to size tolerances."""
    dy, x = np.asarray(dy, dtype=np.float32), np.asarray(x, dtype=np.float32)
    M, C = x.shape
    g = np.ones(C) if gamma is None else np.asarray(gamma, np.float32).astype(np.float64)
    mu, inv = np.asarray(mean, np.float32).astype(np.float64), np.asarray(invstd, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == 1:
            dz = np.where(_fma32(x, scale, shift) > 0, dy, np.float32(0))
        elif mode == 2:
            dz = np.where(np.asarray(y, np.float32) > 0, dy, np.float32(0))
        else:
            dz = dy
        S, Q = _seq_sums_f32(dz, x)
        S, Q = S.astype(np.float64), Q.astype(np.float64)
        dg = ((Q - mu * S) * inv).astype(np.float32)
        db = S.astype(np.float32)
        A = g * inv
        B = -g * inv * inv * ((Q - mu * S) * inv) / M
        D = -A * S / M - B * mu
        dx = _fma32(A, dz, _fma32(B, x, D))
    return dict(dz=dz.astype(np.float64),
                dgamma=(dg if dgamma0 is None else np.asarray(dgamma0, np.float32) + dg).astype(np.float64),
                dbeta=(db if dbeta0 is None else np.asarray(dbeta0, np.float32) + db).astype(np.float64),
                dx=_store(dx, bf16))


# ------------------------------------------------------------------------------------- max pool
def pool_out(i, k, s, p0, p1):
    return (i + p0 + p1 - k) // s + 1


def maxpool_fwd_ref(x, kh, kw, sh, sw, pt, pb, pl, pr, pad_zero):
    """NHWC max pool with explicit loops: (y, arg).  arg is the window position i*kw + k of the first
    maximum, 255 where an implicit zero-padding element won.  The running maximum starts at -inf and only
    a strictly greater element replaces it (csrc/kernels/pool.hip): a NaN never wins, and a window of
    nothing but -inf / NaN gives -inf with arg 255.  -inf padding takes no part."""
    x = np.asarray(x)
    N, H, W, C = x.shape
    OH, OW = pool_out(H, kh, sh, pt, pb), pool_out(W, kw, sw, pl, pr)
    y = np.full((N, OH, OW, C), -np.inf, dtype=x.dtype)
    arg = np.full((N, OH, OW, C), 255, dtype=np.uint8)
    zero = np.zeros((N, C), dtype=x.dtype)
    for oh in range(OH):
        for ow in range(OW):
            for i in range(kh):
                for k in range(kw):
                    h, w = oh * sh - pt + i, ow * sw - pl + k
                    inside = 0 <= h < H and 0 <= w < W
                    if not inside and not pad_zero:
                        continue
                    v = x[:, h, w, :] if inside else zero
                    better = v > y[:, oh, ow, :]
                    y[:, oh, ow, :] = np.where(better, v, y[:, oh, ow, :])
                    arg[:, oh, ow, :] = np.where(better, i * kw + k if inside else 255, arg[:, oh, ow, :])
    return y, arg


def maxpool_bwd_ref(dy, arg, in_shape, kh, kw, sh, sw, pt, pl, dtype=np.float64):
    """Input gradient of the NHWC max pool from dy and the argmax bytes: every window's dy added to the
    input element its arg points at (255: to none), windows in row-major order, accumulated in `dtype`."""
    dy, arg = np.asarray(dy), np.asarray(arg)
    N, H, W, C = in_shape
    dx = np.zeros((N, H, W, C), dtype=dtype)
    for oh in range(dy.shape[1]):
        for ow in range(dy.shape[2]):
            for i in range(kh):
                for k in range(kw):
                    h, w = oh * sh - pt + i, ow * sw - pl + k
                    if 0 <= h < H and 0 <= w < W:
                        hit = arg[:, oh, ow, :] == i * kw + k
                        dx[:, h, w, :] += np.where(hit, dy[:, oh, ow, :], 0).astype(dtype)
    return dx
