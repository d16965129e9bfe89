"""The kernels that run on every step of every model, called directly and compared with the f64
references of tests/kernel_refs.py: the five flat-slab optimizer updates (csrc/kernels/optim.hip, k_sgd /
k_sgd_momentum of mnist_cnn.hip), the f32 -> bf16 weight-slab cast and transpose, and the device batch
gather (csrc/kernels/ops.hip).

Exact where the operation is exact (gather, sentinels around every operand, cast / transpose of finite
values, zero_grad, Adam's t0 + t_add).  The optimizer tolerances are computed from the references alone:
E = max |f32 torch formulas on the CPU - f64 reference| over the variant's 3073-element input (of which
every tested size takes a prefix; a maximum over 1 or 2 elements would understate the f32 error), and
the kernel is allowed 4 E + one f32 ulp of the reference value.
"""
import functools

import numpy as np
import pytest
import torch

import kernel_refs as R

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 4 * 256 * 3 + 1]
NMAX = max(SIZES)
PAD = 4  # floats of sentinel in front of a view (16 bytes: the view stays vector-aligned) and at least behind it
SENT_BITS = 0x4B1D5EED  # a finite f32 pattern (as int32)
LR = (0.05, 0.0125)  # learning rate of steps 1-2 and, after a device-side change, of step 3


def _C():
    from tensorflow_distributed_learning_amd.ops import hip

    return hip()


def _sent_f32(n):
    return torch.full((n,), SENT_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


class _Operand:
    """An n-element f32 operand as the 16-byte-aligned view buf[4 : 4 + n] of a sentinel-filled buffer."""

    def __init__(self, values: np.ndarray):
        n = len(values)
        self.n = n
        self.buf = _sent_f32(n + 2 * PAD + 3)
        self.view = self.buf[PAD:PAD + n]
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)))
        assert self.view.data_ptr() % 16 == 0

    def get(self) -> np.ndarray:
        return self.view.cpu().numpy()

    def assert_outside_untouched(self, what):
        b = self.buf.view(torch.int32).cpu().numpy()
        out = np.concatenate([b[:PAD], b[PAD + self.n:]])
        assert (out == SENT_BITS).all(), f"{what}: wrote outside its {self.n} elements"


# ------------------------------------------------------------------------------------- optimizer variants
# (kind, flags): flags depend on the kind
def _variants():
    v = [("sgd", ())]
    v += [("sgd_momentum", (nest,)) for nest in (False, True)]
    v += [("adam", (wd, ams, 0, 0)) for wd in (0.0, 0.01) for ams in (False, True)]
    v += [("adam", (0.0, False, t0, ta)) for t0, ta in ((0, 3), (5, 0), (5, 3))]
    v += [("rmsprop", (mom, cen)) for mom in (False, True) for cen in (False, True)]
    v += [("adagrad", ())]
    return v


VARIANTS = _variants()
MOM, B1, B2, EPS, RHO, RMOM = 0.9, 0.9, 0.999, 1e-7, 0.9, 0.8
STATE_NAMES = {"sgd": [], "sgd_momentum": ["v"], "adam": ["m", "v", "vhat"], "rmsprop": ["rms", "mom", "mg"],
               "adagrad": ["acc"]}


def _inputs(kind):
    rng = np.random.default_rng({"sgd": 1, "sgd_momentum": 2, "adam": 3, "rmsprop": 4, "adagrad": 5}[kind])
    w0 = rng.standard_normal(NMAX).astype(np.float32)
    if kind == "rmsprop":
        # |g| in [0.5, 1.5): keeps the centered variance rms - mg^2 well above zero (checked in _reference)
        grads = [((0.5 + rng.random(NMAX)) * rng.choice([-1.0, 1.0], NMAX)).astype(np.float32) for _ in range(3)]
    else:
        grads = [(rng.standard_normal(NMAX) * 0.5).astype(np.float32) for _ in range(3)]
    return w0, grads


def _state0(kind, flags):
    z = np.zeros(NMAX, dtype=np.float32)
    if kind == "sgd_momentum":
        return {"v": z.copy()}
    if kind == "adam":
        return {"m": z.copy(), "v": z.copy(), "vhat": z.copy() if flags[1] else None}
    if kind == "rmsprop":
        return {"rms": z.copy(), "mom": z.copy() if flags[0] else None, "mg": z.copy() if flags[1] else None}
    if kind == "adagrad":
        return {"acc": np.full(NMAX, 0.1, dtype=np.float32)}
    return {}


@functools.lru_cache(maxsize=None)
def _reference(kind, flags):
    """(f64 reference, tolerance) per tensor name after the 3 steps, from the CPU alone."""
    from tensorflow_distributed_learning_amd.keras import optimizers as O

    w0, grads = _inputs(kind)
    st = {k: (None if v is None else v.astype(np.float64)) for k, v in _state0(kind, flags).items()}
    w = w0.astype(np.float64)
    for k, g32 in enumerate(grads):
        g, lr = g32.astype(np.float64), LR[0] if k < 2 else LR[1]
        if kind == "sgd":
            w, _ = R.sgd_ref(w, g, lr)
        elif kind == "sgd_momentum":
            w, st["v"] = R.sgd_ref(w, g, lr, st["v"], MOM, flags[0])
        elif kind == "adam":
            wd, _, t0, ta = flags
            w, st["m"], st["v"], st["vhat"] = R.adam_ref(w, g, st["m"], st["v"], st["vhat"], lr, t0 + ta + k + 1,
                                                        B1, B2, EPS, wd)
        elif kind == "rmsprop":
            w, st["rms"], st["mom"], st["mg"], denom = R.rmsprop_ref(w, g, st["rms"], st["mom"], st["mg"], lr, RHO,
                                                                     RMOM if flags[0] else 0.0, EPS)
            assert denom.min() >= 1e-3, "the test is about the kernel, not about sqrt of a rounding-negative"
        else:
            w, st["acc"] = R.adagrad_ref(w, g, st["acc"], lr, EPS)
    # the f32 emulation: the optimizer's own torch formulas on CPU tensors
    if kind in ("sgd", "sgd_momentum"):
        opt = O.SGD(LR[0], momentum=MOM if kind == "sgd_momentum" else 0.0, nesterov=bool(flags and flags[0]))
    elif kind == "adam":
        wd, ams, t0, ta = flags
        opt = O.AdamW(LR[0], weight_decay=wd, beta_1=B1, beta_2=B2, epsilon=EPS, amsgrad=ams) if wd else \
            O.Adam(LR[0], beta_1=B1, beta_2=B2, epsilon=EPS, amsgrad=ams)
        opt.iterations = t0 + ta
    elif kind == "rmsprop":
        opt = O.RMSprop(LR[0], rho=RHO, momentum=RMOM if flags[0] else 0.0, epsilon=EPS, centered=flags[1])
    else:
        opt = O.Adagrad(LR[0], initial_accumulator_value=0.1, epsilon=EPS)
    W = torch.from_numpy(w0.copy())
    for k, g32 in enumerate(grads):
        opt.learning_rate = LR[0] if k < 2 else LR[1]
        opt.apply_flat(W, torch.from_numpy(g32.copy()))
    slot = {"v": "momentum"} if kind == "sgd_momentum" else {}
    ref, tol, emax = {"w": w}, {}, {}
    emul = {"w": W.numpy().astype(np.float64)}
    for name, val in st.items():
        if val is not None:
            ref[name] = val
            emul[name] = opt.slots()[slot.get(name, name)].numpy().astype(np.float64)
    for name in ref:
        emax[name] = float(np.abs(emul[name] - ref[name]).max())
        tol[name] = 4.0 * emax[name] + R.ulp32(ref[name])
    return ref, tol, emax


def _launch(kind, flags, ops, lr_dev, t0_dev, zero_grad):
    C = _C()
    w, g = ops["w"].view, ops["g"].view
    s = {k: (o.view if o is not None else None) for k, o in ops.items()}
    if kind == "sgd":
        C.sgd(w, g, lr_dev, zero_grad=zero_grad)
    elif kind == "sgd_momentum":
        C.sgd_momentum(w, g, s["v"], lr_dev, MOM, flags[0], zero_grad=zero_grad)
    elif kind == "adam":
        C.adam(w, g, s["m"], s["v"], s["vhat"], lr_dev, t0_dev, flags[3], B1, B2, EPS, flags[0])
    elif kind == "rmsprop":
        C.rmsprop(w, g, s["rms"], s["mom"], s["mg"], lr_dev, RHO, RMOM if flags[0] else 0.0, EPS)
    else:
        C.adagrad(w, g, s["acc"], lr_dev, EPS)


def _run_kernel(kind, flags, n, zero_grad=False):
    """3 steps of the kernel on n-element views; returns {name: f32 result}, the gradient operand's content
    after the last step, and checks every operand's surroundings."""
    w0, grads = _inputs(kind)
    ops = {"w": _Operand(w0[:n]), "g": _Operand(grads[0][:n])}
    for name, val in _state0(kind, flags).items():
        ops[name] = _Operand(val[:n]) if val is not None else None
    lr_dev = torch.tensor([LR[0]], dtype=torch.float32, device="cuda")
    t0_dev = torch.zeros(1, dtype=torch.float32, device="cuda")
    for k in range(3):
        if k:
            ops["g"].view.copy_(torch.from_numpy(grads[k][:n].copy()))
        if k == 2:
            lr_dev.fill_(LR[1])  # changed on the device: the kernels read it there
        if kind == "adam":
            t0_dev.fill_(float(flags[2] + k))  # the host refreshes t0 per execution; t_add stays baked in
        _launch(kind, flags, ops, lr_dev, t0_dev, zero_grad)
    torch.cuda.synchronize()
    for name, o in ops.items():
        if o is not None:
            o.assert_outside_untouched(f"{kind}{flags} n={n} operand {name}")
    out = {name: o.get() for name, o in ops.items() if o is not None and name != "g"}
    return out, ops["g"].get()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: v[0] + "".join(f"-{f}" for f in v[1]))
def test_optimizer_kernel_matches_f64_reference(variant, n):
    kind, flags = variant
    ref, tol, emax = _reference(kind, flags)
    got, g_after = _run_kernel(kind, flags, n)
    _, grads = _inputs(kind)
    assert (g_after.view(np.uint32) == grads[2][:n].view(np.uint32)).all(), "the gradient is read-only here"
    for name, r in ref.items():
        err = np.abs(got[name].astype(np.float64) - r[:n])
        worst = int(np.argmax(err / tol[name][:n]))
        print(f"{kind}{flags} n={n} {name}: max err {err.max():.3e}, emulation max {emax[name]:.3e}")
        assert (err <= tol[name][:n]).all(), (
            f"{name}[{worst}]: kernel {got[name][worst]!r} vs f64 {r[worst]!r}, err {err[worst]:.3e} > "
            f"{tol[name][worst]:.3e}")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("variant", [("sgd", ()), ("sgd_momentum", (False,)), ("sgd_momentum", (True,))],
                         ids=lambda v: v[0] + "".join(f"-{f}" for f in v[1]))
def test_sgd_zero_grad_zeroes_g_and_changes_nothing_else(variant, n):
    kind, flags = variant
    keep, _ = _run_kernel(kind, flags, n, zero_grad=False)
    zero, g_after = _run_kernel(kind, flags, n, zero_grad=True)
    assert (g_after.view(np.uint32) == 0).all(), "g must be all +0.0 after zero_grad=True"
    for name in keep:
        assert (keep[name].view(np.uint32) == zero[name].view(np.uint32)).all(), name


@pytest.mark.parametrize("n", [1, 5, 1025])
def test_adam_t0_plus_t_add_is_one_step_count(n):
    a, _ = _run_kernel("adam", (0.0, False, 5, 3), n)
    b, _ = _run_kernel("adam", (0.0, False, 8, 0), n)
    for name in a:
        assert (a[name].view(np.uint32) == b[name].view(np.uint32)).all(), name


def _call_with(kind, make):
    """kind's kernel with every slab operand made by make(name)."""
    flags = {"sgd": (), "sgd_momentum": (False,), "adam": (0.0, True, 0, 0), "rmsprop": (True, True), "adagrad": ()}[kind]
    ops = {name: make(name) for name in ["w", "g"] + STATE_NAMES[kind]}

    class _V:  # (what _launch expects of an operand)
        def __init__(self, t):
            self.view = t

    lr_dev = torch.tensor([LR[0]], dtype=torch.float32, device="cuda")
    t0_dev = torch.zeros(1, dtype=torch.float32, device="cuda")
    _launch(kind, flags, {k: _V(t) for k, t in ops.items()}, lr_dev, t0_dev, False)
    return ops


@pytest.mark.parametrize("kind", list(STATE_NAMES))
def test_optimizer_bindings_reject_misaligned_views(kind):
    """A contiguous slab view such as W[1:] is 4-byte aligned only; the kernels use 16-byte accesses."""
    for bad in ["w", "g"] + STATE_NAMES[kind]:
        def make(name):
            buf = torch.zeros(64 + 8, dtype=torch.float32, device="cuda")
            return buf[1:65] if name == bad else buf[4:68]

        with pytest.raises(RuntimeError, match="16-byte aligned"):
            _call_with(kind, make)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", list(STATE_NAMES))
def test_optimizer_kernels_accept_empty_slabs(kind):
    bufs = {}

    def make(name):
        bufs[name] = _sent_f32(16)
        return bufs[name][4:4]

    _call_with(kind, make)
    torch.cuda.synchronize()  # (an empty grid used to leave a launch error behind for the next call to find)
    assert (torch.ones(4, device="cuda") + 1).sum().item() == 8.0
    for name, b in bufs.items():
        assert (b.view(torch.int32) == SENT_BITS).all(), name


# ------------------------------------------------------------------------------------- slab_cast_bf16
BF16_SENT = 0x5A5B


def _cast_pool():
    rng = np.random.default_rng(7)
    rnd = (rng.standard_normal(25) * 2.0 ** rng.integers(-20, 20, 25)).astype(np.float32)  # 40 binades
    return np.concatenate([R.SPECIALS_F32, R.NAN_PAYLOADS_F32, rnd])  # 48 values


def _bf16_sentinel(n):
    return torch.full((n,), BF16_SENT, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def _check_bf16(got_bits, src, what):
    nan = np.isnan(src)
    want = R.bf16_rne(src)
    assert R.bf16_is_nan(got_bits[nan]).all(), (
        f"{what}: NaN in must give NaN out, got {[hex(v) for v in got_bits[nan][:8]]}")
    bad = np.nonzero(got_bits[~nan] != want[~nan])[0]
    assert bad.size == 0, (f"{what}: {bad.size} finite values differ from round-to-nearest-even, first "
                           f"{src[~nan][bad[0]]!r}: {got_bits[~nan][bad[0]]:#06x} vs {want[~nan][bad[0]]:#06x}")


def _cast(src_np):
    n = len(src_np)
    src = torch.from_numpy(src_np.copy()).cuda()
    buf = _bf16_sentinel(n + 24)
    _C().slab_cast_bf16(src, buf[8:8 + n])
    bits = buf.view(torch.int16).cpu().numpy().view(np.uint16)
    assert (bits[:8] == BF16_SENT).all() and (bits[8 + n:] == BF16_SENT).all(), "cast wrote outside dst"
    return bits[8:8 + n]


@pytest.mark.parametrize("n", [8, 16])
def test_slab_cast_bf16_small(n):
    pool = _cast_pool()
    finite = pool[~np.isnan(pool)]
    for c in range(0, len(finite) - n + 1, n):
        _check_bf16(_cast(finite[c:c + n]), finite[c:c + n], f"cast n={n} finite chunk {c}")
    _check_bf16(_cast(finite[-n:]), finite[-n:], f"cast n={n} last chunk")


@pytest.mark.parametrize("n", [8, 16])
def test_slab_cast_bf16_keeps_nan(n):
    src = np.resize(np.concatenate([R.NAN_PAYLOADS_F32, np.float32([1.5, -2.0])]), n).astype(np.float32)
    _check_bf16(_cast(src), src, f"cast n={n}")


def _big_cast_input():
    n = 2048 * 256 * 8 + 8  # the smallest size at which the grid-stride loop takes a second trip
    rng = np.random.default_rng(8)
    x = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    finite = _cast_pool()
    finite = finite[~np.isnan(finite)]
    x[:len(finite)] = finite
    x[-len(finite):] = finite  # (the second trip's elements too)
    return x


def test_slab_cast_bf16_grid_stride_second_trip():
    x = _big_cast_input()
    _check_bf16(_cast(x), x, "cast 16 MiB")


def test_slab_cast_bf16_grid_stride_keeps_nan():
    x = _big_cast_input()
    x[5:8] = R.NAN_PAYLOADS_F32
    x[-3:] = R.NAN_PAYLOADS_F32
    _check_bf16(_cast(x), x, "cast 16 MiB with NaN")


def test_slab_cast_bf16_rejects_sizes_off_the_vector_width():
    src = torch.zeros(12, device="cuda")
    dst = torch.zeros(12, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 8"):
        _C().slab_cast_bf16(src, dst)


# ------------------------------------------------------------------------------------- slab_transpose_bf16
def _transpose_case(with_nan):
    from tensorflow_distributed_learning_amd.engine.slab import SlabLayout, VarSpec, transpose_tables

    shapes = [(7,), (3, 3, 1, 32), (33,), (3, 3, 32, 64), (5, 3), (7, 7, 3, 64), (1, 1, 64, 256), (),
              (1, 1, 8, 8), (3, 3, 5, 7), (3,)]
    layout = SlabLayout([VarSpec(f"p{i}", s) for i, s in enumerate(shapes)], align=1)
    assert any(o % 2 for o in layout.offsets)
    rng = np.random.default_rng(9)
    W = (rng.standard_normal(layout.total) * 2.0 ** rng.integers(-8, 8, layout.total)).astype(np.float32)
    finite = R.SPECIALS_F32
    for i in (1, 9):  # the special values inside the first and the ragged kernel
        W[layout.offsets[i] + 3: layout.offsets[i] + 3 + len(finite)] = finite
    if with_nan:
        for i in (1, 5, 9):
            W[layout.offsets[i] + 40: layout.offsets[i] + 43] = R.NAN_PAYLOADS_F32
    entries, tiles = transpose_tables(layout.specs, layout.offsets)
    assert len(entries) == 6
    return layout, W, entries, tiles


@pytest.mark.parametrize("with_nan", [False, True], ids=["finite", "nan"])
def test_slab_transpose_bf16(with_nan):
    layout, W, entries, tiles = _transpose_case(with_nan)
    src = torch.from_numpy(W.copy()).cuda()
    dst = _bf16_sentinel(layout.total)
    _C().slab_transpose_bf16(src, dst, torch.tensor(entries, dtype=torch.int32, device="cuda"),
                             torch.tensor(tiles, dtype=torch.int32, device="cuda"))
    bits = dst.view(torch.int16).cpu().numpy().view(np.uint16)
    covered = np.zeros(layout.total, dtype=bool)
    for soff, doff, r, k in entries:
        block = W[soff:soff + r * k].reshape(r, k).T.reshape(-1)
        _check_bf16(bits[doff:doff + r * k], np.ascontiguousarray(block), f"transpose R={r} K={k}")
        covered[doff:doff + r * k] = True
    assert (bits[~covered] == BF16_SENT).all(), "transpose wrote outside the conv kernels' blocks"


# ------------------------------------------------------------------------------------- gather_xy
@pytest.mark.parametrize("rows", [1, 5, 64])
@pytest.mark.parametrize("ldtype", [torch.int64, torch.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("row_elems", [1, 3, 4, 7, 784, 1028, 2052])
def test_gather_xy_bitwise(row_elems, ldtype, rows):
    N = 70
    g = torch.Generator().manual_seed(row_elems * 131 + rows)
    shape = (N, 28, 28, 1) if row_elems == 784 else (N, row_elems)
    X = torch.randn(shape, generator=g).cuda()
    Y = torch.randint(-5, 1 << 30, (N,), generator=g).to(ldtype).cuda()
    assert X.data_ptr() % 16 == 0
    if rows == 1:
        idxs = [[0], [N - 1]]
    else:
        r = torch.randint(0, N, (rows,), generator=g).tolist()
        r[0], r[1], r[2], r[3] = N - 1, 0, r[4], r[4]  # the last and first row, and a repeat
        idxs = [r]
    for idx in idxs:
        buf = torch.full((rows + 7,), N + 1000, dtype=torch.int32, device="cuda")  # (the trainer passes such slices)
        ii = buf[3:3 + rows]
        ii.copy_(torch.tensor(idx, dtype=torch.int32))
        x, y = _C().gather_xy(X, Y, ii)
        il = ii.long()
        assert x.shape == (rows,) + tuple(shape[1:]) and x.dtype == torch.float32
        assert y.shape == (rows,) and y.dtype == ldtype
        assert torch.equal(x.view(torch.int32), X.index_select(0, il).view(torch.int32))
        assert torch.equal(y, Y.index_select(0, il))


@pytest.mark.parametrize("ldtype", [torch.int64, torch.int32], ids=["i64", "i32"])
def test_gather_xy_empty_batch(ldtype):
    X = torch.randn(10, 28, 28, 1).cuda()
    Y = torch.arange(10).to(ldtype).cuda()
    x, y = _C().gather_xy(X, Y, torch.zeros(8, dtype=torch.int32, device="cuda")[3:3])
    torch.cuda.synchronize()
    assert x.shape == (0, 28, 28, 1) and x.dtype == torch.float32 and x.is_cuda
    assert y.shape == (0,) and y.dtype == ldtype and y.is_cuda


def test_gather_xy_rejects_misaligned_rows():
    buf = torch.zeros(10 * 4 + 4, device="cuda")
    X = buf[1:41].view(10, 4)
    Y = torch.arange(10, device="cuda")
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _C().gather_xy(X, Y, torch.zeros(2, dtype=torch.int32, device="cuda"))
