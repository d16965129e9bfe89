"""The weight EMA on the device against the numpy f32 step of tests/ema_refs.py, bit for bit: the stand-alone
k_weight_ema (csrc/kernels/ema.hip) and the EMA instantiation of every update kernel (k_sgd, k_sgd_momentum,
k_adam, k_rmsprop, k_adagrad, the LARS and LAMB apply kernels).

The stand-alone kernel is a streaming kernel and can go wrong at its edges: the slab's end inside a tile (vector
part and scalar tail), the grid-stride wrap when the slab has more tiles than the grid has workgroups, a tail in
a second pass.  The sizes sit on those boundaries, at the production grid cap and at caps of 1, 2 and 3
workgroups.  An update kernel with the average inside must not perturb its update: in mode 1 its W and every
slot carry the bits of the same launch without EMA on copies of the inputs, and E the oracle's bits from that W;
in mode 2 W carries E's.  The values hold signed zeros, infinities, NaNs, denormals, +-3.4e38 and pairs whose two
products cancel; guard words in front of and behind every slab must stay intact.
"""
import numpy as np
import pytest
import torch

import ema_refs as ER
from tensorflow_distributed_learning_amd import ops

pytestmark = pytest.mark.gpu

PAD = 64  # guard floats on either side of a slab (256 bytes: the slab stays 16-byte aligned)
SENTINEL = 12345.678
MOMENTA = (0.0, 0.5, 0.99, 0.999, 1.0)


def C():
    return ops.hip()


def BE() -> int:
    return int(C().EMA_BLOCK_ELEMS)


def guarded(fill: np.ndarray):
    """(whole buffer, the slab inside it at a 16-byte aligned offset) holding ``fill``."""
    n = fill.size
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    slab = buf[PAD:PAD + n]
    assert slab.data_ptr() % 16 == 0
    if n:
        slab.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype=np.float32)))
    return buf, slab


def guards_ok(buf: torch.Tensor) -> bool:
    n = buf.numel() - 2 * PAD
    return bool((torch.cat([buf[:PAD], buf[PAD + n:]]) == SENTINEL).all())


def host(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy()


def make_we(n: int, m: float, seed: int):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(n).astype(np.float32)
    w = rng.standard_normal(n).astype(np.float32)
    ER.plant_specials([e, w], m, seed)
    return e, w


# ------------------------------------------------------------------------------------------ stand-alone kernel
def check_standalone(n: int, m: float, mode: int, max_blocks=None, seed: int = 0):
    e0, w0 = make_we(n, m, seed)
    Wb, W = guarded(w0)
    Eb, E = guarded(e0)
    C().weight_ema(W, E, m, mode, max_blocks=max_blocks)
    torch.cuda.synchronize()
    e_ref, w_ref = ER.step(e0, w0, m, mode)
    tag = f"n={n} m={m} mode={mode} max_blocks={max_blocks}"
    assert ER.same_bits(host(E), e_ref), f"E differs from the oracle ({tag})"
    assert ER.same_bits(host(W), w_ref), f"W differs ({tag})"
    if mode == 1:
        assert np.array_equal(host(W).view(np.int32), w0.view(np.int32)), f"mode 1 wrote W ({tag})"
    else:
        assert ER.same_bits(host(W), host(E)), f"mode 2: W has not E's bits ({tag})"
    assert guards_ok(Wb) and guards_ok(Eb), f"a guard word was written ({tag})"
    return e0, w0, host(E)


def edge_sizes():
    be = BE()
    return [0, 1, 3, 4, 5, 1023, 1024, 1025, be - 1, be, be + 1]


@pytest.mark.parametrize("mode", [1, 2])
def test_standalone_edges_every_momentum(mode):
    for n in edge_sizes():
        for i, m in enumerate(MOMENTA):
            check_standalone(n, m, mode, seed=i)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("cap", [1, 2, 3])
def test_standalone_grid_stride_at_small_caps(mode, cap):
    """More tiles than workgroups: every workgroup strides, the guarded last tile lands in a later pass."""
    be = BE()
    for n in (be + 1, 2 * be, 3 * be + 5, 4 * be - 1, 7 * be + 1027):
        check_standalone(n, 0.99, mode, max_blocks=cap, seed=cap)


@pytest.mark.parametrize("mode", [1, 2])
def test_standalone_above_the_production_grid_cap(mode):
    """One size with more tiles than the production grid has workgroups, at the production cap."""
    n = int(C().EMA_MAX_BLOCKS) * BE() + BE() + 7
    check_standalone(n, 0.999, mode)


def test_standalone_momentum_0_and_1_with_finite_operands():
    """m = 0 gives E == W and m = 1 leaves E unchanged (finite operands: 0 * Inf would be a NaN)."""
    rng = np.random.default_rng(5)
    n = BE() + 13
    w0 = rng.standard_normal(n).astype(np.float32)
    e0 = rng.standard_normal(n).astype(np.float32)
    for m, want in ((0.0, w0), (1.0, e0)):
        _, W = guarded(w0)
        _, E = guarded(e0)
        C().weight_ema(W, E, m, 1)
        torch.cuda.synchronize()
        # (a + 0 * b keeps a's value; the sign of a zero sum is the oracle's business)
        assert np.array_equal(host(E), want)
        assert ER.same_bits(host(E), ER.step(e0, w0, m, 1)[0])


def test_standalone_rejects_bad_operands():
    w = torch.zeros(8, device="cuda")
    with pytest.raises(RuntimeError):
        C().weight_ema(w, torch.zeros(4, device="cuda"), 0.9, 1)
    with pytest.raises(RuntimeError):
        C().weight_ema(w, torch.zeros(8, device="cuda"), 0.9, 0)
    with pytest.raises(RuntimeError):
        C().weight_ema(w, torch.zeros(8, device="cuda"), 1.5, 1)
    with pytest.raises(RuntimeError):
        C().weight_ema(w, w, 0.9, 1)
    with pytest.raises(RuntimeError):
        C().weight_ema(w, torch.zeros(8, device="cuda"), 0.9, 1, max_blocks=0)


# ------------------------------------------------------------------------------------------ update kernels
SIZES = (1, 3, 4, 5, 1023, 1025, 4099)


def clip_ops(on: bool) -> dict:
    if not on:
        return {}
    return {"gscale": torch.tensor([0.5, 0.0, 0.0, 0.0], dtype=torch.float32, device="cuda"), "clipvalue": 0.75}


def dev_word(v: float) -> torch.Tensor:
    return torch.tensor([v], dtype=torch.float32, device="cuda")


def layer_spans(n: int):
    """Two variables with a three-element gap between them once the slab is long enough, else one."""
    if n < 64:
        return [0], [n]
    o1 = (n // 2) // 4 * 4
    return [0, o1], [o1 - 3, n - o1]


class Variant:
    """One update kernel in one configuration: its slots, and how to launch it."""

    def __init__(self, name, slots, launch, positive=(), zero_grad=False, layered=False):
        self.name, self.slots, self.launch, self.positive = name, slots, launch, positive
        self.zero_grad, self.layered = zero_grad, layered


def _sgd(W, G, S, x):
    C().sgd(W, G, dev_word(0.05), zero_grad=True, **x)


def _mom(nesterov):
    def f(W, G, S, x):
        C().sgd_momentum(W, G, S["momentum"], dev_word(0.05), 0.9, nesterov, zero_grad=True, **x)
    return f


def _adam(ams, wd):
    def f(W, G, S, x):
        C().adam(W, G, S["m"], S["v"], S.get("vhat"), dev_word(0.01), dev_word(3.0), 1, 0.9, 0.999, 1e-7, wd, **x)
    return f


def _rms(mom, centered):
    def f(W, G, S, x):
        C().rmsprop(W, G, S["rms"], S.get("mom"), S.get("mg"), dev_word(0.01), 0.9, 0.8 if mom else 0.0, 1e-7, **x)
    return f


def _adagrad(W, G, S, x):
    C().adagrad(W, G, S["acc"], dev_word(0.01), 1e-7, **x)


def _tables(n):
    offs, sizes = layer_spans(n)
    return C().layer_tables(offs, sizes, n, [1e-4] * len(offs), [True] * len(offs))


def _lars(W, G, S, x):
    n = W.numel()
    T = _tables(n)
    clip = {k: v for k, v in x.items() if k in ("gscale", "clipvalue")}
    ema = {k: v for k, v in x.items() if k.startswith("ema")}
    part = torch.zeros(max(2, 2 * T.C), dtype=torch.float64, device="cuda")
    ratio = torch.ones(max(1, T.V), dtype=torch.float32, device="cuda")
    norms = torch.zeros(max(1, T.V), 2, dtype=torch.float32, device="cuda")
    C().lars_sums(T, W, G, part, **clip)
    C().lars_ratio(T, part, ratio, norms, 0.001, 0.0)
    C().lars_update(T, W, G, S["momentum"], ratio, dev_word(0.05), 0.9, True, **clip, **ema)


def _lamb(W, G, S, x):
    n = W.numel()
    T = _tables(n)
    clip = {k: v for k, v in x.items() if k in ("gscale", "clipvalue")}
    ema = {k: v for k, v in x.items() if k.startswith("ema")}
    part = torch.zeros(max(2, 2 * T.C), dtype=torch.float64, device="cuda")
    ratio = torch.ones(max(1, T.V), dtype=torch.float32, device="cuda")
    norms = torch.zeros(max(1, T.V), 2, dtype=torch.float32, device="cuda")
    hp = (dev_word(3.0), 1, 0.9, 0.999, 1e-6)
    C().lamb_sums(T, W, G, S["m"], S["v"], part, *hp, **clip)
    C().lamb_ratio(T, part, ratio, norms)
    C().lamb_update(T, W, S["m"], S["v"], ratio, dev_word(0.01), *hp, **ema)


VARIANTS = [
    Variant("sgd", (), _sgd, zero_grad=True),
    Variant("momentum", ("momentum",), _mom(False), zero_grad=True),
    Variant("momentum-nesterov", ("momentum",), _mom(True), zero_grad=True),
    Variant("adam", ("m", "v"), _adam(False, 0.0), positive=("v",)),
    Variant("adam-amsgrad", ("m", "v", "vhat"), _adam(True, 0.0), positive=("v", "vhat")),
    Variant("adamw", ("m", "v"), _adam(False, 0.004), positive=("v",)),
    Variant("adamw-amsgrad", ("m", "v", "vhat"), _adam(True, 0.004), positive=("v", "vhat")),
    Variant("rmsprop", ("rms",), _rms(False, False), positive=("rms",)),
    Variant("rmsprop-momentum", ("rms", "mom"), _rms(True, False), positive=("rms",)),
    Variant("rmsprop-centered", ("rms", "mg"), _rms(False, True), positive=("rms",)),
    Variant("rmsprop-momentum-centered", ("rms", "mom", "mg"), _rms(True, True), positive=("rms",)),
    Variant("adagrad", ("acc",), _adagrad, positive=("acc",)),
    Variant("lars", ("momentum",), _lars, layered=True),
    Variant("lamb", ("m", "v"), _lamb, positive=("v",), layered=True),
]


def run_update(v: Variant, inputs: dict, clip: bool, ema_mode: int, m: float):
    """One launch over guarded copies of ``inputs``; returns {name: host array} and whether every guard held."""
    bufs = {k: guarded(a) for k, a in inputs.items()}
    S = {k: bufs[k][1] for k in v.slots}
    x = clip_ops(clip)
    if ema_mode:
        x.update(ema=bufs["E"][1], ema_momentum=m, ema_mode=ema_mode)
    v.launch(bufs["W"][1], bufs["G"][1], S, x)
    torch.cuda.synchronize()
    return {k: host(b[1]) for k, b in bufs.items()}, all(guards_ok(b[0]) for b in bufs.values())


@pytest.mark.parametrize("v", VARIANTS, ids=[v.name for v in VARIANTS])
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
def test_update_kernel_with_the_average_inside(v, clip):
    m = 0.99
    for n in SIZES:
        rng = np.random.default_rng(n)
        inputs = {"E": rng.standard_normal(n).astype(np.float32), "W": rng.standard_normal(n).astype(np.float32),
                  "G": rng.standard_normal(n).astype(np.float32)}
        ER.plant_specials([inputs["E"], inputs["W"], inputs["G"]], m, n)
        for s in v.slots:
            a = rng.standard_normal(n).astype(np.float32)
            inputs[s] = np.abs(a) if s in v.positive else a
        tag = f"{v.name} clip={clip} n={n}"
        base, ok0 = run_update(v, inputs, clip, 0, m)
        got1, ok1 = run_update(v, inputs, clip, 1, m)
        got2, ok2 = run_update(v, inputs, clip, 2, m)
        assert ok0 and ok1 and ok2, f"a guard word was written ({tag})"
        assert np.array_equal(base["E"].view(np.int32), inputs["E"].view(np.int32)), f"E written without EMA ({tag})"
        # what the kernel touches: everything, or, for the layer-wise kernels, the variables' spans only
        touched = np.ones(n, dtype=bool)
        if v.layered:
            touched[:] = False
            for o, s in zip(*layer_spans(n)):
                touched[o:o + s] = True
        e_ref, _ = ER.step(inputs["E"], base["W"], m, 1)
        e_ref = np.where(touched, e_ref, inputs["E"])
        # mode 1: the update is the one without EMA, E the oracle's from that W
        assert ER.same_bits(got1["W"], base["W"]), f"mode 1: the average perturbed W ({tag})"
        for s in v.slots:
            assert ER.same_bits(got1[s], base[s]), f"mode 1: the average perturbed slot {s} ({tag})"
            assert ER.same_bits(got2[s], base[s]), f"mode 2: slot {s} differs from mode 1's ({tag})"
        assert ER.same_bits(got1["E"], e_ref), f"mode 1: E differs from the oracle ({tag})"
        # mode 2: the same average, stored as W too
        assert ER.same_bits(got2["E"], e_ref), f"mode 2: E differs from the oracle ({tag})"
        assert ER.same_bits(got2["W"], np.where(touched, e_ref, base["W"])), f"mode 2: W has not E's bits ({tag})"
        # G: zeroed where the kernel zeroes it, untouched elsewhere
        for got in (base, got1, got2):
            if v.zero_grad:
                assert not got["G"].view(np.int32).any(), f"zero_grad left G nonzero ({tag})"
            else:
                assert np.array_equal(got["G"].view(np.int32), inputs["G"].view(np.int32)), f"G written ({tag})"


def test_update_kernels_reject_bad_ema_operands():
    w, g = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    lr = dev_word(0.1)
    with pytest.raises(RuntimeError):
        C().sgd(w, g, lr, ema=torch.zeros(4, device="cuda"), ema_momentum=0.9, ema_mode=1)
    with pytest.raises(RuntimeError):
        C().sgd(w, g, lr, ema_momentum=0.9, ema_mode=1)
    with pytest.raises(RuntimeError):
        C().sgd(w, g, lr, ema=torch.zeros(8, device="cuda"), ema_momentum=0.9, ema_mode=3)
    with pytest.raises(RuntimeError):
        C().sgd(w, g, lr, ema=w, ema_momentum=0.9, ema_mode=1)
