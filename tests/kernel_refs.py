"""High-precision references of the small per-step kernels (optimizer updates, the f32 -> bf16 slab
cast, softmax cross-entropy), shared by test_kernel_refs_cpu.py, test_slab_kernels_gpu.py and
test_head_gpu.py.  numpy only; nothing here touches a GPU.

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
