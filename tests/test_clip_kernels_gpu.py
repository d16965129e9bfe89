"""Gradient clipping on the device, kernel by kernel: the two launches of ``_C.clip_norm``
(csrc/kernels/clip.hip: k_clip_partials, k_clip_scale) and the clip operands (``gscale``, ``clipvalue``) of the
five flat-slab optimizer kernels, against the f64 references of tests/clip_refs.py / tests/kernel_refs.py.

Every operand is a 16-byte-aligned view inside a sentinel-filled buffer and every test checks that nothing
outside the views was written.  Sizes come from the extension's own constants (CLIP_CHUNK: elements per
partial sum, CLIP_SCALE_THREADS: k_clip_scale's workgroup), so they follow the kernels.

Tolerances.  The sum of squares is accumulated in f64 from exact products: over <= 2^25 terms its relative
error is <= 2^-28, which leaves the rounding of the square root and of the cast to f32: the norm word is
allowed 1 f32 ulp of the f64 value.  The scale word takes three f32 roundings (norm, norm + 1e-12, the
quotient): 2 ulp.  The clipped optimizer updates are allowed 4 E + 1 ulp, E = the largest error of the
optimizer's own f32 torch formulas on the CPU (``apply_flat`` on CPU tensors, clipping included) against the
f64 reference over the variant's runs (all tested sizes: a maximum over 5 elements alone would understate the
f32 error).

Range.  The kernels take the sum in f64, so a slab of 3e30 everywhere has a finite norm here, while the CPU
fallback's f32 sum of squares overflows to inf (and its scale to 0): the two paths differ above a norm of
~1.8e19, by design; every comparison against the CPU emulation below uses |g| < 1e15.
"""
import functools

import numpy as np
import pytest
import torch

import clip_refs as CR
import kernel_refs as R

pytestmark = pytest.mark.gpu

PAD = 4  # floats of sentinel in front of a view (16 bytes: the view stays vector-aligned) and at least behind it
SENT_BITS = 0x4B1D5EED  # a finite f32 pattern (as int32)
SENT64 = 0x4B1D5EED4B1D5EED  # and as int64, for the f64 partial sums
LR = (0.05, 0.0125)  # learning rate of steps 1-2 and, after a device-side change, of step 3
MOM, B1, B2, EPS, RHO, RMOM = 0.9, 0.9, 0.999, 1e-7, 0.9, 0.8


def _C():
    from tensorflow_distributed_learning_amd.ops import hip

    return hip()


@functools.lru_cache(maxsize=None)
def _consts():
    C = _C()
    return int(C.CLIP_CHUNK), int(C.CLIP_SCALE_THREADS)


def _norm_sizes():
    CH, T = _consts()
    return [1, 3, 4, 5, 63, 64, CH - 1, CH, CH + 1, 2 * CH + 3, T * CH + 5]


def _update_sizes():
    CH, _ = _consts()
    return [5, 1025, 2 * CH + 3]


class _Operand:
    """An n-element f32 operand as the 16-byte-aligned view buf[pad : pad + n] of a sentinel-filled buffer."""

    def __init__(self, values, pad=PAD):
        values = np.ascontiguousarray(values, dtype=np.float32)
        n = len(values)
        self.n, self.pad = n, pad
        self.buf = torch.full((n + 2 * pad + 3,), SENT_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
        self.view = self.buf[pad:pad + n]
        if n:
            self.view.copy_(torch.from_numpy(values))
        assert self.view.data_ptr() % 16 == 0

    def get(self) -> np.ndarray:
        return self.view.cpu().numpy()

    def assert_outside_untouched(self, what):
        b = self.buf.view(torch.int32).cpu().numpy()
        out = np.concatenate([b[:self.pad], b[self.pad + self.n:]])
        assert (out == SENT_BITS).all(), f"{what}: wrote outside its {self.n} elements"


class _ClipBufs:
    """partials (f64, exactly the P elements clip_norm needs) and out ([scale, norm]) as aligned views inside
    sentinel-filled buffers."""

    def __init__(self, n):
        self.P = int(_C().clip_partials(n))
        self.pbuf = torch.full((self.P + 4,), SENT64, dtype=torch.int64, device="cuda")
        self.partials = self.pbuf[2:2 + self.P].view(torch.float64)
        self.obuf = torch.full((PAD + 2 + PAD,), SENT_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
        self.out = self.obuf[PAD:PAD + 2]
        assert self.partials.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0

    def words(self):
        """(scale, norm) as f32 numpy scalars."""
        o = self.out.cpu().numpy()
        return o[0], o[1]

    def bits(self):
        return (self.partials.cpu().numpy().view(np.uint64).copy(), self.out.cpu().numpy().view(np.uint32).copy())

    def assert_outside_untouched(self, what):
        p = self.pbuf.cpu().numpy()
        assert (np.concatenate([p[:2], p[2 + self.P:]]) == SENT64).all(), f"{what}: wrote outside partials"
        o = self.obuf.view(torch.int32).cpu().numpy()
        assert (np.concatenate([o[:PAD], o[PAD + 2:]]) == SENT_BITS).all(), f"{what}: wrote outside out"


def _clip_norm(g_np, clipnorm, clipvalue=None, pad=PAD):
    g = _Operand(g_np, pad)
    bufs = _ClipBufs(len(g_np))
    _C().clip_norm(g.view, bufs.partials, bufs.out, clipnorm, clipvalue)
    torch.cuda.synchronize()
    g.assert_outside_untouched("clip_norm g")
    bufs.assert_outside_untouched("clip_norm")
    assert (g.get().view(np.uint32) == np.ascontiguousarray(g_np, np.float32).view(np.uint32)).all(), \
        "clip_norm must not write g"
    return bufs


@functools.lru_cache(maxsize=None)
def _normal(n, seed=11):
    return (np.random.default_rng(seed).standard_normal(n) * 0.5).astype(np.float32)


# ------------------------------------------------------------------------------------- norm and scale
@pytest.mark.parametrize("clamp", [False, True], ids=["norm", "clamp+norm"])
@pytest.mark.parametrize("k", range(11))
def test_norm_and_scale_match_f64(k, clamp):
    n = _norm_sizes()[k]
    g = _normal(_norm_sizes()[-1])[:n]
    cv = 0.6 if clamp else None
    ref_norm = CR.norm_ref(g, cv)
    c = 0.37 * ref_norm  # active: the scale is about 0.37
    ref_scale = CR.scale_ref(ref_norm, c)
    assert abs(ref_norm - R.f32(c)) > 4 * R.ulp32(ref_norm), "the < 1 decision must not hang on a rounding"
    scale, norm = _clip_norm(g, c, cv).words()
    print(f"n={n}: norm {norm!r} vs f64 {ref_norm!r} ({abs(float(norm) - ref_norm) / R.ulp32(ref_norm):.3f} ulp), "
          f"scale {scale!r} vs {ref_scale!r} ({abs(float(scale) - ref_scale) / R.ulp32(ref_scale):.3f} ulp)")
    assert abs(float(norm) - ref_norm) <= R.ulp32(ref_norm)
    assert abs(float(scale) - ref_scale) <= 2 * R.ulp32(ref_scale)
    assert float(scale) < 1.0


def test_partials_are_the_chunk_sums():
    """partials[p] is the f64 sum of squares of elements [p CH, (p + 1) CH): the layout the order rests on."""
    CH, _ = _consts()
    n = 2 * CH + 3
    g = _normal(n)
    bufs = _clip_norm(g, 1.0)
    got = bufs.partials.cpu().numpy()
    g64 = g.astype(np.float64)
    want = np.array([np.sum(g64[p * CH:(p + 1) * CH] ** 2) for p in range(3)])
    assert got.shape == (3,)
    assert (np.abs(got - want) <= 2.0 ** -40 * want).all()


# ------------------------------------------------------------------------------------- update kernels
def _variants():
    v = [("sgd", ())]
    v += [("sgd_momentum", (nest,)) for nest in (False, True)]
    v += [("adam", (wd, ams)) for wd in (0.0, 0.01) for ams in (False, True)]
    v += [("rmsprop", (mom, cen)) for mom in (False, True) for cen in (False, True)]
    v += [("adagrad", ())]
    return v


VARIANTS = _variants()
MODES = ["clipvalue", "norm", "both"]
CLIPVALUE = 0.6  # |g| ~ 0.5 N(0, 1) (rmsprop: [0.5, 1.5)): a good part of the elements is clamped
NORM_FRACTION = 0.5  # clipnorm = this fraction of the smallest of the 3 steps' (clamped) norms: always active
_id = lambda v: v[0] + "".join(f"-{f}" for f in v[1])  # noqa: E731


@functools.lru_cache(maxsize=None)
def _inputs(kind):
    nmax = _update_sizes()[-1]
    rng = np.random.default_rng({"sgd": 1, "sgd_momentum": 2, "adam": 3, "rmsprop": 4, "adagrad": 5}[kind])
    w0 = rng.standard_normal(nmax).astype(np.float32)
    if kind == "rmsprop":
        # |g| in [0.5, 1.5): keeps the centered variance rms - mg^2 well above zero (checked in _reference)
        grads = [((0.5 + rng.random(nmax)) * rng.choice([-1.0, 1.0], nmax)).astype(np.float32) for _ in range(3)]
    else:
        grads = [(rng.standard_normal(nmax) * 0.5).astype(np.float32) for _ in range(3)]
    return w0, grads


def _state0(kind, flags, n):
    z = np.zeros(n, dtype=np.float32)
    if kind == "sgd_momentum":
        return {"v": z.copy()}
    if kind == "adam":
        return {"m": z.copy(), "v": z.copy(), "vhat": z.copy() if flags[1] else None}
    if kind == "rmsprop":
        return {"rms": z.copy(), "mom": z.copy() if flags[0] else None, "mg": z.copy() if flags[1] else None}
    if kind == "adagrad":
        return {"acc": np.full(n, 0.1, dtype=np.float32)}
    return {}


def _clip_consts(kind, mode, n):
    """(clipnorm or None, clipvalue or None) of a case, from the inputs alone."""
    _, grads = _inputs(kind)
    cv = CLIPVALUE if mode in ("clipvalue", "both") else None
    cn = None
    if mode in ("norm", "both"):
        cn = float(np.float32(NORM_FRACTION * min(CR.norm_ref(g[:n], cv) for g in grads)))
    return cn, cv


def _reference_n(kind, flags, mode, n):
    """{name: f64 reference} and {name: |CPU f32 path - reference|} after the 3 steps at size n."""
    from tensorflow_distributed_learning_amd.keras import optimizers as O

    w0, grads = _inputs(kind)
    cn, cv = _clip_consts(kind, mode, n)
    st = {k: (None if v is None else v.astype(np.float64)) for k, v in _state0(kind, flags, n).items()}
    w = w0[:n].astype(np.float64)
    for k, g32 in enumerate(grads):
        g, norm, scale = CR.clip_ref(g32[:n], cn, cv)
        if cn is not None:
            assert scale < 1.0 and abs(norm - cn) > 4 * R.ulp32(norm), "the clip must be active, and clearly so"
        lr = LR[0] if k < 2 else LR[1]
        if kind == "sgd":
            w, _ = R.sgd_ref(w, g, lr)
        elif kind == "sgd_momentum":
            w, st["v"] = R.sgd_ref(w, g, lr, st["v"], MOM, flags[0])
        elif kind == "adam":
            w, st["m"], st["v"], st["vhat"] = R.adam_ref(w, g, st["m"], st["v"], st["vhat"], lr, k + 1, B1, B2, EPS,
                                                        flags[0])
        elif kind == "rmsprop":
            w, st["rms"], st["mom"], st["mg"], denom = R.rmsprop_ref(w, g, st["rms"], st["mom"], st["mg"], lr, RHO,
                                                                     RMOM if flags[0] else 0.0, EPS)
            assert denom.min() >= 1e-4, "the test is about the kernel, not about sqrt of a rounding-negative"
        else:
            w, st["acc"] = R.adagrad_ref(w, g, st["acc"], lr, EPS)
    kw = dict(clipvalue=cv, global_clipnorm=cn)
    if kind in ("sgd", "sgd_momentum"):
        opt = O.SGD(LR[0], momentum=MOM if kind == "sgd_momentum" else 0.0, nesterov=bool(flags and flags[0]), **kw)
    elif kind == "adam":
        wd, ams = flags
        opt = O.AdamW(LR[0], weight_decay=wd, beta_1=B1, beta_2=B2, epsilon=EPS, amsgrad=ams, **kw) if wd else \
            O.Adam(LR[0], beta_1=B1, beta_2=B2, epsilon=EPS, amsgrad=ams, **kw)
    elif kind == "rmsprop":
        opt = O.RMSprop(LR[0], rho=RHO, momentum=RMOM if flags[0] else 0.0, epsilon=EPS, centered=flags[1], **kw)
    else:
        opt = O.Adagrad(LR[0], initial_accumulator_value=0.1, epsilon=EPS, **kw)
    W = torch.from_numpy(w0[:n].copy())
    for k, g32 in enumerate(grads):
        opt.learning_rate = LR[0] if k < 2 else LR[1]
        opt.apply_flat(W, torch.from_numpy(g32[:n].copy()))
    slot = {"v": "momentum"} if kind == "sgd_momentum" else {}
    ref, err = {"w": w}, {}
    emul = {"w": W.numpy().astype(np.float64)}
    for name, val in st.items():
        if val is not None:
            ref[name] = val
            emul[name] = opt.slots()[slot.get(name, name)].numpy().astype(np.float64)
    for name in ref:
        err[name] = float(np.abs(emul[name] - ref[name]).max())
    return ref, err


@functools.lru_cache(maxsize=None)
def _reference(kind, flags, mode):
    """{n: reference}, and per tensor name E = the CPU f32 path's largest error over the variant's sizes."""
    refs, emax = {}, {}
    for n in _update_sizes():
        refs[n], err = _reference_n(kind, flags, mode, n)
        for name, e in err.items():
            emax[name] = max(emax.get(name, 0.0), e)
    return refs, emax


def _launch(kind, flags, ops, lr_dev, t0_dev, zero_grad, gscale, clipvalue):
    C = _C()
    w, g = ops["w"].view, ops["g"].view
    s = {k: (o.view if o is not None else None) for k, o in ops.items()}
    kw = dict(gscale=gscale, clipvalue=clipvalue)
    if kind == "sgd":
        C.sgd(w, g, lr_dev, zero_grad=zero_grad, **kw)
    elif kind == "sgd_momentum":
        C.sgd_momentum(w, g, s["v"], lr_dev, MOM, flags[0], zero_grad=zero_grad, **kw)
    elif kind == "adam":
        C.adam(w, g, s["m"], s["v"], s["vhat"], lr_dev, t0_dev, 0, B1, B2, EPS, flags[0], **kw)
    elif kind == "rmsprop":
        C.rmsprop(w, g, s["rms"], s["mom"], s["mg"], lr_dev, RHO, RMOM if flags[0] else 0.0, EPS, **kw)
    else:
        C.adagrad(w, g, s["acc"], lr_dev, EPS, **kw)


def _run_kernel(kind, flags, n, clipnorm=None, clipvalue=None, zero_grad=False, steps=3, grads=None, w0=None):
    """`steps` steps of the kernel on n-element views (clip_norm first where a norm clip is set); returns
    {name: f32 result}, the gradient operand's content after the last step and the last [scale, norm] words,
    and checks every operand's surroundings."""
    iw0, igrads = _inputs(kind)
    w0 = iw0 if w0 is None else w0
    grads = igrads if grads is None else grads
    ops = {"w": _Operand(w0[:n]), "g": _Operand(grads[0][:n])}
    for name, val in _state0(kind, flags, n).items():
        ops[name] = _Operand(val) if val is not None else None
    bufs = _ClipBufs(n)
    lr_dev = torch.tensor([LR[0]], dtype=torch.float32, device="cuda")
    t0_dev = torch.zeros(1, dtype=torch.float32, device="cuda")
    for k in range(steps):
        if k:
            ops["g"].view.copy_(torch.from_numpy(grads[k][:n].copy()))
        if k == 2:
            lr_dev.fill_(LR[1])  # changed on the device: the kernels read it there
        t0_dev.fill_(float(k))
        if clipnorm is not None:
            _C().clip_norm(ops["g"].view, bufs.partials, bufs.out, clipnorm, clipvalue)
        _launch(kind, flags, ops, lr_dev, t0_dev, zero_grad, bufs.out if clipnorm is not None else None, clipvalue)
    torch.cuda.synchronize()
    for name, o in ops.items():
        if o is not None:
            o.assert_outside_untouched(f"{kind}{flags} n={n} operand {name}")
    bufs.assert_outside_untouched(f"{kind}{flags} n={n}")
    out = {name: o.get() for name, o in ops.items() if o is not None and name != "g"}
    return out, ops["g"].get(), bufs


@pytest.mark.parametrize("ni", range(3))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", VARIANTS, ids=_id)
def test_clipped_update_matches_f64_reference(variant, mode, ni):
    kind, flags = variant
    n = _update_sizes()[ni]
    refs, emax = _reference(kind, flags, mode)
    ref = refs[n]
    cn, cv = _clip_consts(kind, mode, n)
    got, g_after, _ = _run_kernel(kind, flags, n, cn, cv)
    _, grads = _inputs(kind)
    assert (g_after.view(np.uint32) == grads[2][:n].view(np.uint32)).all(), "the gradient is read-only here"
    for name, r in ref.items():
        tol = 4.0 * emax[name] + R.ulp32(r)
        err = np.abs(got[name].astype(np.float64) - r)
        worst = int(np.argmax(err / tol))
        print(f"{kind}{flags} {mode} n={n} {name}: max err {err.max():.3e}, emulation max {emax[name]:.3e}")
        assert (err <= tol).all(), (
            f"{name}[{worst}]: kernel {got[name][worst]!r} vs f64 {r[worst]!r}, err {err[worst]:.3e} > "
            f"{tol[worst]:.3e}")


@pytest.mark.parametrize("ni", range(3))
@pytest.mark.parametrize("variant", [("sgd", ()), ("sgd_momentum", (False,)), ("sgd_momentum", (True,))], ids=_id)
def test_zero_grad_with_clip_operands(variant, ni):
    kind, flags = variant
    n = _update_sizes()[ni]
    cn, cv = _clip_consts(kind, "both", n)
    keep, _, kb = _run_kernel(kind, flags, n, cn, cv, zero_grad=False)
    zero, g_after, zb = _run_kernel(kind, flags, n, cn, cv, zero_grad=True)
    assert (g_after.view(np.uint32) == 0).all(), "g must be all +0.0 after zero_grad=True"
    for name in keep:
        assert (keep[name].view(np.uint32) == zero[name].view(np.uint32)).all(), name
    assert (kb.bits()[1] == zb.bits()[1]).all()


@pytest.mark.parametrize("variant", VARIANTS, ids=_id)
def test_inactive_clip_is_the_unclipped_update_bit_for_bit(variant):
    """norm << clipnorm: the scale word is exactly 1.0f and the update has the unclipped kernel's bits."""
    kind, flags = variant
    n = 1025
    plain, _, _ = _run_kernel(kind, flags, n)
    clipped, _, bufs = _run_kernel(kind, flags, n, clipnorm=1e6, clipvalue=1e6)
    scale, norm = bufs.words()
    assert scale.view(np.uint32) == np.float32(1.0).view(np.uint32)
    assert 0 < float(norm) < 1e3
    for name in plain:
        assert (plain[name].view(np.uint32) == clipped[name].view(np.uint32)).all(), name


# ------------------------------------------------------------------------------------- order, determinism, range
def test_norm_bits_do_not_depend_on_run_or_address():
    CH, T = _consts()
    for n in (5, CH + 1, 2 * CH + 3, T * CH + 5):
        rng = np.random.default_rng(n)
        g = (10.0 ** rng.uniform(-12, 12, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        rng.shuffle(g)
        ref = CR.norm_ref(g)
        a = _clip_norm(g, 1.0)
        b = _clip_norm(g, 1.0)
        c = _clip_norm(g, 1.0, pad=8)  # the same data at another buffer offset
        for other in (b, c):
            assert (a.bits()[0] == other.bits()[0]).all(), f"n={n}: partials differ"
            assert (a.bits()[1] == other.bits()[1]).all(), f"n={n}: norm / scale differ"
        assert abs(float(a.words()[1]) - ref) <= R.ulp32(ref)


@pytest.mark.parametrize("which", ["small", "chunks"])
def test_norm_of_huge_gradients_is_finite_where_the_f32_sum_overflows(which):
    CH, _ = _consts()
    n = 5 if which == "small" else CH + 1
    g = np.full(n, 3e30, dtype=np.float32)
    ref = CR.norm_ref(g)
    scale, norm = _clip_norm(g, 1.0).words()
    assert np.isfinite(norm) and abs(float(norm) - ref) <= R.ulp32(ref)
    ref_scale = CR.scale_ref(ref, 1.0)
    assert abs(float(scale) - ref_scale) <= 2 * R.ulp32(ref_scale)
    # the difference from the CPU fallback (Optimizer._clip): its f32 sum of squares overflows
    assert torch.isinf(torch.linalg.vector_norm(torch.from_numpy(g)))


# ------------------------------------------------------------------------------------- non-finite values
def _positions(n):
    CH, _ = _consts()
    return {"first": 0, "last": n - 1, "tail": 2 * CH + 1, "middle": CH + 7}


@pytest.mark.parametrize("where", ["first", "last", "tail", "middle"])
def test_nan_gradient_poisons_scale_and_every_weight(where):
    CH, _ = _consts()
    n = 2 * CH + 3
    g = _normal(n).copy()
    g[_positions(n)[where]] = np.nan
    got, _, bufs = _run_kernel("sgd", (), n, clipnorm=1.0, steps=1, grads=[g])
    scale, norm = bufs.words()
    assert np.isnan(norm) and np.isnan(scale)
    assert np.isnan(got["w"]).all()


@pytest.mark.parametrize("where", ["first", "last", "tail", "middle"])
def test_inf_gradient_gives_scale_zero(where):
    CH, _ = _consts()
    n = 2 * CH + 3
    g = _normal(n).copy()
    p = _positions(n)[where]
    g[p] = np.inf
    w0, _ = _inputs("sgd")
    got, _, bufs = _run_kernel("sgd", (), n, clipnorm=1.0, steps=1, grads=[g])
    scale, norm = bufs.words()
    assert np.isinf(norm) and scale.view(np.uint32) == 0
    w = got["w"]
    assert np.isnan(w[p])  # inf * 0
    rest = np.arange(n) != p
    assert (w[rest].view(np.uint32) == w0[:n][rest].view(np.uint32)).all(), "finite gradients become 0: w unchanged"


@pytest.mark.parametrize("variant", VARIANTS, ids=_id)
def test_clipvalue_keeps_nan_and_clamps_inf(variant):
    """clipvalue, no norm clip: a NaN gradient stays NaN, +-Inf clamps to +-clipvalue (Tensor.clamp_)."""
    kind, flags = variant
    CH, _ = _consts()
    n = 2 * CH + 3
    _, grads = _inputs(kind)
    g = grads[0][:n].copy()
    pos = _positions(n)
    g[pos["first"]], g[pos["middle"]], g[pos["tail"]], g[pos["last"]] = np.nan, np.inf, -np.inf, np.nan
    want = g.copy()
    want[pos["middle"]], want[pos["tail"]] = CLIPVALUE, -CLIPVALUE
    got, _, _ = _run_kernel(kind, flags, n, clipvalue=CLIPVALUE, steps=1, grads=[g])
    same, _, _ = _run_kernel(kind, flags, n, clipvalue=CLIPVALUE, steps=1, grads=[want])
    for name in got:
        if name != "vhat":  # (AMSGrad's running maximum is an fmaxf, which keeps the finite operand)
            assert np.isnan(got[name][[pos["first"], pos["last"]]]).all(), f"{name}: the NaN gradient was dropped"
        assert (got[name].view(np.uint32) == same[name].view(np.uint32)).all(), name


# ------------------------------------------------------------------------------------- capture
def test_captured_clip_norm_and_adam_replay_like_eager():
    CH, _ = _consts()
    n = 2 * CH + 3
    w0, grads = _inputs("adam")
    cn, cv = _clip_consts("adam", "both", n)
    C = _C()
    lrs, t0s = (0.05, 0.0125, 0.03), (0.0, 1.0, 7.0)

    def fresh():
        ops = {"w": _Operand(w0[:n]), "g": _Operand(grads[0][:n])}
        for name in ("m", "v"):
            ops[name] = _Operand(np.zeros(n, np.float32))
        return ops, _ClipBufs(n), torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")

    def step(ops, bufs, lr_dev, t_dev):
        C.clip_norm(ops["g"].view, bufs.partials, bufs.out, cn, cv)
        C.adam(ops["w"].view, ops["g"].view, ops["m"].view, ops["v"].view, None, lr_dev, t_dev, 0, B1, B2, EPS, 0.0,
               gscale=bufs.out, clipvalue=cv)

    def run(replay):
        ops, bufs, lr_dev, t_dev = fresh()
        graph = None
        if replay:
            graph = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=s):
                step(ops, bufs, lr_dev, t_dev)
            torch.cuda.synchronize()
        words = []
        for k in range(3):
            ops["g"].view.copy_(torch.from_numpy(grads[k][:n].copy()))
            lr_dev.fill_(lrs[k])
            t_dev.fill_(t0s[k])
            if replay:
                graph.replay()
            else:
                step(ops, bufs, lr_dev, t_dev)
            torch.cuda.synchronize()
            words.append(bufs.bits()[1])
        for name, o in ops.items():
            o.assert_outside_untouched(name)
        bufs.assert_outside_untouched("capture")
        return {k: o.get().view(np.uint32) for k, o in ops.items()}, words

    eager, ew = run(False)
    replayed, rw = run(True)
    for k in range(3):
        assert (ew[k] == rw[k]).all(), f"step {k}: [scale, norm] differ"
    assert len({tuple(w) for w in ew}) == 3, "the three steps must see three different norms"
    for name in eager:
        assert (eager[name] == replayed[name]).all(), name


# ------------------------------------------------------------------------------------- bindings
def test_clip_norm_rejects_misaligned_and_short_operands():
    C = _C()
    CH, _ = _consts()
    n = CH + 1  # needs 2 partial sums

    def f32buf(k):
        return torch.zeros(k + 8, dtype=torch.float32, device="cuda")

    g, out = f32buf(n)[4:4 + n], f32buf(2)[4:6]
    part = torch.zeros(4, dtype=torch.float64, device="cuda")
    C.clip_norm(g, part[:2], out, 1.0)  # (the well-formed call)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        C.clip_norm(f32buf(n)[1:1 + n], part[:2], out, 1.0)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        C.clip_norm(g, part[1:3], out, 1.0)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        C.clip_norm(g, part[:2], f32buf(2)[1:3], 1.0)
    with pytest.raises(RuntimeError, match="partials too small"):
        C.clip_norm(g, part[:1], out, 1.0)
    with pytest.raises(RuntimeError, match="float64"):
        C.clip_norm(g, f32buf(8)[4:8], out, 1.0)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        C.sgd(g, g.clone(), torch.ones(1, device="cuda"), gscale=f32buf(2)[1:3])
    torch.cuda.synchronize()


def test_clip_norm_of_an_empty_slab_writes_norm_zero_scale_one():
    C = _C()
    assert C.clip_partials(0) == 0
    gbuf = torch.full((16,), SENT_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    bufs = _ClipBufs(0)
    C.clip_norm(gbuf[4:4], bufs.partials, bufs.out, 0.5)
    torch.cuda.synchronize()  # (an empty grid would leave a launch error behind for the next call to find)
    assert (torch.ones(4, device="cuda") + 1).sum().item() == 8.0
    scale, norm = bufs.words()
    assert scale.view(np.uint32) == np.float32(1.0).view(np.uint32) and norm.view(np.uint32) == 0
    bufs.assert_outside_untouched("empty")
    assert (gbuf.view(torch.int32) == SENT_BITS).all()
    # and the update kernels with clip operands over an empty slab launch nothing
    w = torch.full((16,), SENT_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    C.sgd(w[4:4], gbuf[4:4], torch.ones(1, device="cuda"), gscale=bufs.out, clipvalue=0.5)
    torch.cuda.synchronize()
    assert (w.view(torch.int32) == SENT_BITS).all()
