"""f64 references of the layer-wise optimizers (LARS, LAMB: keras/optimizers.py, csrc/kernels/layerwise.hip)
over a slab layout, the test layout and inputs shared by test_layerwise_cpu.py and
test_layerwise_kernels_gpu.py, and the CPU f32 path's error E against the references.  numpy (and, for the
CPU path, torch on CPU tensors) only; nothing here touches a GPU.

Inputs and constants enter as the f32 values the kernels receive.  The gradient an update sees is
g' = f32(f32 clamp(g, +-clipvalue) * scale word): the scale word is an INPUT here (on the GPU it is read back
from ``clip_norm``, which has its own tests; without a GPU it is the rounded f64 scale of clip_refs).
"""
import functools

import numpy as np

import clip_refs as CR
from kernel_refs import f32

ALIGN = 64
LR = (0.05, 0.05, 0.0125)  # the last one is changed on the device
WD = 0.01
MOM, EETA, LARS_EPS = 0.9, 0.001, 0.0
B1, B2, LAMB_EPS = 0.9, 0.999, 1e-6
CLIPVALUE = 0.6  # |g| ~ 0.5 N(0, 1): a good part of the elements is clamped
NORM_FRACTION = 0.5  # clipnorm = this fraction of the smallest of the 3 steps' (clamped) norms: always active
MODES = ["none", "clipvalue", "norm", "both"]
NO_ADAPT, NO_DECAY, ZERO_W, ZERO_G = 2, 3, 8, 9
NAMES = ["v0/kernel", "v1/bias", "v2/noadapt", "v3/nodecay", "v4/kernel", "v5/kernel", "v6/kernel", "v7/kernel",
         "v8/zero_w", "v9/zero_g"]


def sizes_of(CH):
    return [1, 3, 64, 65, CH - 1, CH, CH + 1, 2 * CH + 3, 10, 128]


def offsets_of(sizes, align=ALIGN):
    offs, off = [], 0
    for s in sizes:
        offs.append(off)
        off = (off + s + align - 1) // align * align
    return offs, off


class Case:
    """The test layout at chunk size CH with its inputs (f32) and per-variable operands."""

    def __init__(self, CH, seed=17):
        self.CH = CH
        self.sizes = sizes_of(CH)
        self.offsets, self.total = offsets_of(self.sizes)
        self.V = len(self.sizes)
        self.wd = [0.0 if i == NO_DECAY else WD for i in range(self.V)]
        self.adapt = [i != NO_ADAPT for i in range(self.V)]
        rng = np.random.default_rng(seed)
        self.mask = np.zeros(self.total, dtype=bool)
        for o, s in zip(self.offsets, self.sizes):
            self.mask[o:o + s] = True
        self.w0 = self.scatter(rng.standard_normal(self.mask.sum()).astype(np.float32))
        self.grads = [self.scatter((rng.standard_normal(self.mask.sum()) * 0.5).astype(np.float32)) for _ in range(3)]
        self.span(self.w0, ZERO_W)[:] = 0.0
        for g in self.grads:
            self.span(g, ZERO_G)[:] = 0.0

    def scatter(self, packed):
        """A zero-padded slab from the variables' elements."""
        out = np.zeros(self.total, dtype=packed.dtype)
        out[self.mask] = packed
        return out

    def span(self, flat, i):
        return flat[self.offsets[i]:self.offsets[i] + self.sizes[i]]

    def clip_consts(self, mode):
        """(clipnorm or None, clipvalue or None) of a mode, from the inputs alone."""
        cv = CLIPVALUE if mode in ("clipvalue", "both") else None
        cn = None
        if mode in ("norm", "both"):
            cn = float(np.float32(NORM_FRACTION * min(CR.norm_ref(g[self.mask], cv) for g in self.grads)))
        return cn, cv

    def ref_scales(self, mode):
        """The scale words of the 3 steps without a GPU: the f64 scale rounded to f32."""
        cn, cv = self.clip_consts(mode)
        if cn is None:
            return [None] * 3
        return [np.float32(CR.scale_ref(CR.norm_ref(g[self.mask], cv), cn)) for g in self.grads]


@functools.lru_cache(maxsize=None)
def case(CH):
    return Case(int(CH))


def gprime(g32, clipvalue, scale_word):
    """g' as the kernels form it (GradClip): f32 clamp, one f32 product with the scale word; as f64."""
    g = np.asarray(g32, dtype=np.float32)
    if clipvalue is not None:
        cv = np.float32(clipvalue)
        with np.errstate(invalid="ignore"):
            g = np.where(g > cv, cv, np.where(g < -cv, -cv, g)).astype(np.float32)
    if scale_word is not None:
        with np.errstate(invalid="ignore"):
            g = (g * np.float32(scale_word)).astype(np.float32)
    return g.astype(np.float64)


def _norm(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.sqrt(np.sum(x * x)))


def lars_step_ref(c, w, gp, v, lr, nesterov, wd=None, adapt=None):
    """One LARS step in f64 over the layout of ``c``; returns new (w, v), ratios [V], norms [V, 2]."""
    wd = c.wd if wd is None else wd
    adapt = c.adapt if adapt is None else adapt
    lr, mu, eeta, eps = f32(lr), f32(MOM), f32(EETA), f32(LARS_EPS)
    w, v = w.copy(), v.copy()
    ratios, norms = np.ones(c.V), np.zeros((c.V, 2))
    for i in range(c.V):
        wi, gi, vi, lam = c.span(w, i), c.span(gp, i), c.span(v, i), f32(wd[i])
        nw, ng = _norm(wi), _norm(gi)
        norms[i] = nw, ng
        if adapt[i] and nw > 0 and ng > 0:
            ratios[i] = eeta * nw / (ng + lam * nw + eps)
        with np.errstate(invalid="ignore"):
            d = gi + lam * wi if lam != 0 else gi
            s = lr * ratios[i]
            vi[:] = mu * vi - s * d
            wi[:] = wi + (mu * vi - s * d if nesterov else vi)
    return w, v, ratios, norms


def lamb_step_ref(c, w, gp, m, v, lr, t):
    """One LAMB step (t >= 1) in f64; returns new (w, m, v), ratios [V], norms [V, 2] (|w_i|, |u_i|)."""
    lr, b1, b2, eps = f32(lr), f32(B1), f32(B2), f32(LAMB_EPS)
    w, m, v = w.copy(), m.copy(), v.copy()
    ratios, norms = np.ones(c.V), np.zeros((c.V, 2))
    for i in range(c.V):
        wi, gi, mi, vi, lam = c.span(w, i), c.span(gp, i), c.span(m, i), c.span(v, i), f32(c.wd[i])
        with np.errstate(invalid="ignore"):
            mi[:] = b1 * mi + (1.0 - b1) * gi
            vi[:] = b2 * vi + (1.0 - b2) * gi * gi
            u = (mi / (1.0 - b1 ** t)) / (np.sqrt(vi / (1.0 - b2 ** t)) + eps) + lam * wi
        nw, nu = _norm(wi), _norm(u)
        norms[i] = nw, nu
        if c.adapt[i] and nw > 0 and nu > 0:
            ratios[i] = nw / nu
        with np.errstate(invalid="ignore"):
            wi[:] = wi - lr * ratios[i] * u
    return w, m, v, ratios, norms


def run_ref(c, kind, nesterov, mode, scales, grads=None, steps=3):
    """``steps`` steps of the f64 reference; scales: the steps' scale words (None: no norm clip).
    Returns ({name: final f64 slab}, [ratios per step], [norms per step])."""
    grads = c.grads if grads is None else grads
    _, cv = c.clip_consts(mode)
    w = c.w0.astype(np.float64)
    st = {"momentum": np.zeros(c.total)} if kind == "lars" else {"m": np.zeros(c.total), "v": np.zeros(c.total)}
    ratios, norms = [], []
    for k in range(steps):
        gp = gprime(grads[k], cv, scales[k])
        if kind == "lars":
            w, st["momentum"], r, nm = lars_step_ref(c, w, gp, st["momentum"], LR[k], nesterov)
        else:
            w, st["m"], st["v"], r, nm = lamb_step_ref(c, w, gp, st["m"], st["v"], LR[k], k + 1)
        ratios.append(r)
        norms.append(nm)
    return dict(st, w=w), ratios, norms


def make_optimizer(c, kind, nesterov, mode):
    from tensorflow_distributed_learning_amd.engine.slab import SlabLayout
    from tensorflow_distributed_learning_amd.keras import optimizers as O

    cn, cv = c.clip_consts(mode)
    kw = dict(weight_decay_rate=WD, exclude_from_weight_decay=["nodecay"], exclude_from_layer_adaptation=["noadapt"],
              clipvalue=cv, global_clipnorm=cn)
    if kind == "lars":
        opt = O.LARS(LR[0], momentum=MOM, eeta=EETA, epsilon=LARS_EPS, nesterov=nesterov, **kw)
    else:
        opt = O.LAMB(LR[0], beta_1=B1, beta_2=B2, epsilon=LAMB_EPS, **kw)
    opt.set_layout(SlabLayout.from_shapes([(n, (s,)) for n, s in zip(NAMES, c.sizes)], align=ALIGN))
    return opt


def run_cpu(c, kind, nesterov, mode):
    """The 3 steps through the optimizer's CPU f32 path (``apply_flat`` on CPU tensors, clipping included).
    Returns ({name: final f32 slab as f64}, [ratios per step])."""
    import torch

    opt = make_optimizer(c, kind, nesterov, mode)
    assert opt._layout.offsets == c.offsets and opt._layout.total == c.total
    W = torch.from_numpy(c.w0.copy())
    ratios = []
    for k in range(3):
        opt.learning_rate = LR[k]
        opt.apply_flat(W, torch.from_numpy(c.grads[k].copy()))
        ratios.append(np.array(opt._cpu_ratios, dtype=np.float64))
    assert opt.layer_operands(opt._layout) == (c.wd, c.adapt)
    out = {k: v.numpy().astype(np.float64) for k, v in opt.slots().items()}
    out["w"] = W.numpy().astype(np.float64)
    return out, ratios


@functools.lru_cache(maxsize=None)
def cpu_error(CH, kind, nesterov, mode):
    """({name: E}, relative ratio error) of the CPU f32 path against the f64 reference over the 3 steps, the
    reference taking the rounded f64 scale words."""
    c = case(CH)
    ref, rr, _ = run_ref(c, kind, nesterov, mode, c.ref_scales(mode))
    got, gr = run_cpu(c, kind, nesterov, mode)
    E = {k: float(np.abs(got[k] - ref[k])[c.mask].max()) for k in ref}
    rel = max(float((np.abs(a - b) / np.abs(b)).max()) for a, b in zip(gr, rr))
    return E, rel
