"""The seeded augmentation kernels (csrc/kernels/augment.hip) bit for bit against the numpy reference of
ops/augment.py (itself checked against a per-pixel loop in tests/test_augment_cpu.py): the 16-byte vector path
and the per-element path in every fill mode, the edges of a workgroup's span and of the grid-stride loop, the
ticket past 2^32, and the device-side ticket, eagerly and in a replayed graph.

Inputs are views inside sentinel-filled buffers (16-byte aligned, or deliberately 4 bytes off; the kernels
only read them, the call counter is the one operand they write), and every test checks that nothing but the
counter changed in those buffers.  Outputs are allocated by the bindings.  Sizes come from the extension's
constants: AUGMENT_WG_ELEMS work items (16-byte vectors on the vector path, elements on the element path) per
workgroup and trip, AUGMENT_MAX_GRID the grid cap, lowered by ``augment_force_max_grid`` to reach the second
trip with a small tensor."""
import functools

import pytest
import torch

from tensorflow_distributed_learning_amd.ops import augment as A

pytestmark = pytest.mark.gpu

KEY = (0x1234ABCD, 0x9E3779B9)
SENT = {torch.float32: (torch.int32, 0x4B1D5EED), torch.bfloat16: (torch.int16, 0x4B1D)}  # finite patterns
SENT64 = 0x4B1D5EED4B1D5EED
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


def _C():
    from tensorflow_distributed_learning_amd.ops import hip

    return hip()


@functools.lru_cache(maxsize=None)
def _consts():
    C = _C()
    return int(C.AUGMENT_WG_ELEMS), int(C.AUGMENT_MAX_GRID)


def _ibits(t):
    return t.contiguous().view(SENT[t.dtype][0])


class _Operand:
    """``values`` (a CPU tensor) as a view inside a sentinel-filled device buffer, 16-byte aligned or
    ``shift`` elements past that."""

    def __init__(self, values, shift=0):
        values = values.contiguous()
        self.itype, self.sent = SENT[values.dtype]
        n = values.numel()
        pad = 16 // values.element_size()
        self.buf = torch.full((n + 2 * pad + 3,), self.sent, dtype=self.itype, device="cuda")
        self.view = self.buf[pad + shift:pad + shift + n].view(values.dtype).view(values.shape)
        self.view.copy_(values)
        assert self.view.data_ptr() % 16 == shift * values.element_size()
        self.before = self.buf.clone()

    def assert_unchanged(self, what):
        assert torch.equal(self.buf, self.before), f"{what}: a read-only operand's buffer was written"


class _State:
    """[calls, arrivals] as an aligned view inside a sentinel-filled int64 buffer."""

    def __init__(self, calls=0):
        self.buf = torch.full((6,), SENT64, dtype=torch.int64, device="cuda")
        self.view = self.buf[2:4]
        self.view.copy_(torch.tensor([calls, 0], dtype=torch.int64))
        assert self.view.data_ptr() % 16 == 0

    def get(self):
        b = self.buf.cpu().tolist()
        assert b[:2] == [SENT64] * 2 and b[4:] == [SENT64] * 2, "the call counter's neighbours were written"
        return b[2:4]


def _values(shape, dtype, seed=0):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    flat = x.view(-1)
    flat[::7] = float("inf")  # a copy keeps every bit pattern
    flat[3::11] = -0.0
    flat[5::13] = 1e-39  # subnormal in both dtypes
    return x.to(dtype)


def _grads(shape, dtype, seed=1):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    x.view(-1)[3::11] = -0.0  # +0 + -0 = +0: the sum starts from +0
    return x.to(dtype)


def _want_fwd(x, ticket, spec):
    """x (CPU) through augment_reference, on the bits (numpy has no bf16); the fill rounded once by torch."""
    itype = SENT[x.dtype][0]
    fill = torch.tensor(spec.fill_value, dtype=torch.float64).to(x.dtype).view(itype).numpy()
    return torch.from_numpy(A.augment_reference(x.contiguous().view(itype).numpy(), KEY, ticket, spec, fill=fill))


def _want_bwd(dy, ticket, spec, H, W):
    dx = A.augment_backward_reference(dy.float().numpy(), KEY, ticket, spec, H, W)
    return _ibits(torch.from_numpy(dx).to(dy.dtype))  # bf16: the f32 sum rounded once


def _check_pair(x, spec, ticket0=3, shift=0, what=""):
    """Forward and backward of one call against the reference; returns the forward output."""
    C = _C()
    N, H, W, Ch = x.shape
    st = _State(ticket0)
    xo = _Operand(x, shift)
    dy = _grads((N, spec.out_h, spec.out_w, Ch), x.dtype)
    dyo = _Operand(dy, shift)
    y, t = C.augment_fwd(xo.view, st.view, KEY[0], KEY[1], *spec.args())
    assert t.dtype == torch.int64 and t.numel() == 1 and int(t.cpu()[0]) == ticket0, f"{what}: ticket"
    assert st.get() == [ticket0 + 1, 0], f"{what}: state after the call"
    assert tuple(y.shape) == (N, spec.out_h, spec.out_w, Ch) and y.dtype == x.dtype and y.is_contiguous()
    assert torch.equal(_ibits(y.cpu()), _want_fwd(x, ticket0, spec)), f"{what}: forward"
    dx = C.augment_bwd(dyo.view, t, KEY[0], KEY[1], *spec.args(), H, W)
    assert tuple(dx.shape) == tuple(x.shape) and dx.dtype == x.dtype
    assert torch.equal(_ibits(dx.cpu()), _want_bwd(dy, ticket0, spec, H, W)), f"{what}: backward"
    assert st.get() == [ticket0 + 1, 0], f"{what}: the backward touched the state"
    xo.assert_unchanged(what + " x")
    dyo.assert_unchanged(what + " dy")
    return y


def _full_spec(H, W, mode="constant", fill=0.0, Ho=None, Wo=None):
    """Both flips drawn, every offset the kernels accept."""
    return A.Spec(flip_h=True, flip_w=True, off_h_lo=-H, off_h_count=2 * H + 1, off_w_lo=-W, off_w_count=2 * W + 1,
                  out_h=Ho or H, out_w=Wo or W, fill_mode=mode, fill_value=fill)


# ------------------------------------------------------------------------------------------------ 1: paths, modes
# (dtype, C, shift): C * element size a multiple of 16 at an aligned pointer = the vector path
PATHS = [(torch.float32, 4, 0), (torch.float32, 12, 0), (torch.bfloat16, 8, 0), (torch.bfloat16, 24, 0),
         (torch.float32, 1, 0), (torch.float32, 3, 0), (torch.float32, 5, 0), (torch.bfloat16, 1, 0),
         (torch.bfloat16, 3, 0), (torch.bfloat16, 5, 0), (torch.bfloat16, 4, 0), (torch.float32, 4, 1)]


@pytest.mark.parametrize("dtype,C,shift", PATHS, ids=[
    f"{'f32' if d == torch.float32 else 'bf16'}-C{c}" + ("-4B-off" if s else "") for d, c, s in PATHS])
def test_paths_and_fill_modes(dtype, C, shift):
    for H in (1, 5, 7):
        for W in (1, 5, 7):
            for N in (1, 3):
                x = _values((N, H, W, C), dtype, seed=H * 8 + W)
                for mode in A.FILL_MODES:
                    for fill in (-0.0, 1.5):
                        _check_pair(x, _full_spec(H, W, mode, fill), shift=shift, what=f"{N}x{H}x{W}x{C} {mode} {fill}")


@DTYPES
def test_fill_bits_and_crops(dtype):
    C = 8
    # everything is fill: the value arrives rounded once to the dtype, -0.0 keeps its sign
    for fill in (-0.0, 1.5, 1.00390625 + 2.0 ** -20):
        spec = A.Spec(off_h_lo=5, out_h=5, out_w=7, fill_value=fill)
        y = _check_pair(_values((2, 5, 7, C), dtype), spec, what=f"fill {fill}")
        want = torch.tensor(fill, dtype=torch.float64).to(dtype)
        assert (_ibits(y.cpu()) == _ibits(want.reshape(1))[0]).all()
    # an output smaller than the input (RandomCrop): every window position, down to 1 x 1
    for Ho, Wo in ((1, 1), (3, 4), (5, 7), (5, 1), (1, 7)):
        spec = A.Spec(off_h_count=5 - Ho + 1, off_w_count=7 - Wo + 1, out_h=Ho, out_w=Wo)
        _check_pair(_values((3, 5, 7, C), dtype), spec, what=f"crop {Ho}x{Wo}")
        _check_pair(_values((3, 5, 7, 3), dtype), _full_spec(5, 7, "reflect", 0.0, Ho, Wo), what=f"window {Ho}x{Wo}")


# ------------------------------------------------------------------------------------------------ 2: grid edges
def _shape_of(items, per_item):
    """An NHWC shape of ``items`` work items of ``per_item`` channels each: [1, h, w, C] with h * w = items and
    h the largest divisor up to 40 (1 for a prime), so both axes matter where they can."""
    h = max(d for d in range(1, 41) if items % d == 0)
    return (1, h, items // h, per_item)


@pytest.mark.parametrize("dtype,per_item",
                         [(torch.float32, 1), (torch.bfloat16, 1), (torch.float32, 4), (torch.bfloat16, 8)],
                         ids=["f32-elem", "bf16-elem", "f32-vec", "bf16-vec"])
def test_workgroup_span_edges(dtype, per_item):
    """The tensor ends one work item before, at and after the span of the first and of the second workgroup."""
    WG, _ = _consts()
    for items in (WG - 1, WG, WG + 1, 2 * WG - 1, 2 * WG, 2 * WG + 1):
        shape = _shape_of(items, per_item)
        H, W = shape[1], shape[2]
        for mode in ("reflect", "constant"):
            spec = A.Spec(flip_h=True, flip_w=True, off_h_lo=-min(H, 3), off_h_count=2 * min(H, 3) + 1, off_w_lo=-3,
                          off_w_count=7, out_h=H, out_w=W, fill_mode=mode, fill_value=1.5)
            _check_pair(_values(shape, dtype), spec, what=f"{items} items {shape} {mode}")


@pytest.mark.parametrize("dtype,per_item", [(torch.float32, 1), (torch.bfloat16, 8)], ids=["f32-elem", "bf16-vec"])
def test_second_grid_stride_trip(dtype, per_item):
    C = _C()
    WG, MAXG = _consts()
    assert MAXG >= 3
    C.augment_force_max_grid(3)
    try:
        # 3 workgroups: the second trip holds 5 items; the third holds two whole spans and 5 items
        for items in (3 * WG + 5, 8 * WG + 5):
            shape = _shape_of(items, per_item)
            H, W = shape[1], shape[2]
            spec = A.Spec(flip_h=True, flip_w=True, off_h_lo=-1, off_h_count=3, off_w_lo=-3, off_w_count=7, out_h=H,
                          out_w=W, fill_mode="nearest")
            _check_pair(_values(shape, dtype), spec, what=f"cap 3, {items} items {shape}")
        # several samples per workgroup and trip: the draw is refreshed where the sample changes
        _check_pair(_values((40, 9, 11, per_item), dtype), _full_spec(9, 11, "wrap"), what="cap 3, 40 samples")
    finally:
        C.augment_force_max_grid(0)


def test_ticket_carries_into_the_high_word():
    C = _C()
    x = _values((3, 5, 7, 3), torch.float32)
    xo, st = _Operand(x), _State((1 << 32) - 1)
    spec = _full_spec(5, 7, "reflect")
    outs = []
    for want_t in ((1 << 32) - 1, 1 << 32):
        y, t = C.augment_fwd(xo.view, st.view, KEY[0], KEY[1], *spec.args())
        assert int(t.cpu()[0]) == want_t
        assert torch.equal(_ibits(y.cpu()), _want_fwd(x, want_t, spec))
        outs.append(y)
    assert st.get() == [(1 << 32) + 1, 0]
    assert not torch.equal(outs[0], outs[1])
    assert not torch.equal(_ibits(outs[1].cpu()), _want_fwd(x, 0, spec)), "ticket 2^32 drew as ticket 0"
    xo.assert_unchanged("x")


# ------------------------------------------------------------------------------------------------ 3: the ticket
@pytest.mark.parametrize("which", ["one workgroup", "many workgroups", "capped grid"])
def test_three_eager_calls_take_tickets_in_order(which):
    C = _C()
    shape = {"one workgroup": (3, 5, 7, 3), "many workgroups": (8, 33, 31, 3), "capped grid": (8, 33, 31, 3)}[which]
    x = _values(shape, torch.bfloat16)
    xo, st = _Operand(x), _State(0)
    spec = _full_spec(shape[1], shape[2], "wrap")
    if which == "capped grid":
        C.augment_force_max_grid(4)
    try:
        outs = []
        for k in range(3):
            y, t = C.augment_fwd(xo.view, st.view, KEY[0], KEY[1], *spec.args())
            assert int(t.cpu()[0]) == k and st.get() == [k + 1, 0]
            assert torch.equal(_ibits(y.cpu()), _want_fwd(x, k, spec)), f"call {k}"
            outs.append(y)
    finally:
        C.augment_force_max_grid(0)
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    xo.assert_unchanged("x")


def test_graph_replays_draw_fresh_transforms():
    C = _C()
    x = _values((8, 33, 31, 4), torch.float32)
    xo, st = _Operand(x), _State(0)
    spec = _full_spec(33, 31, "reflect")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=s):
        y, t = C.augment_fwd(xo.view, st.view, KEY[0], KEY[1], *spec.args())
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert st.get() == [0, 0], "the capture consumed a ticket"
    outs = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert int(t.cpu()[0]) == k and st.get() == [k + 1, 0]
        outs.append(y.cpu().clone())
        assert torch.equal(_ibits(outs[-1]), _want_fwd(x, k, spec)), f"replay {k}"
    assert st.get() == [3, 0]
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2]) and \
        not torch.equal(outs[0], outs[2])
    xo.assert_unchanged("x")


@DTYPES
def test_backward_redraws_from_the_saved_ticket(dtype):
    """The backward runs after the counter has moved on: it must use the forward's ticket, not ``calls``."""
    C = _C()
    x = _values((3, 5, 7, 8), dtype)
    xo, st = _Operand(x), _State(2)
    spec = _full_spec(5, 7, "nearest")
    _, t2 = C.augment_fwd(xo.view, st.view, KEY[0], KEY[1], *spec.args())
    _, t3 = C.augment_fwd(xo.view, st.view, KEY[0], KEY[1], *spec.args())
    assert st.get() == [4, 0]
    dy = _grads((3, 5, 7, 8), dtype)
    dyo = _Operand(dy)
    for t, k in ((t2, 2), (t3, 3), (t2, 2)):
        dx = C.augment_bwd(dyo.view, t, KEY[0], KEY[1], *spec.args(), 5, 7)
        assert torch.equal(_ibits(dx.cpu()), _want_bwd(dy, k, spec, 5, 7)), f"ticket {k}"
    assert not torch.equal(_want_bwd(dy, 2, spec, 5, 7), _want_bwd(dy, 3, spec, 5, 7))
    assert st.get() == [4, 0]
    dyo.assert_unchanged("dy")


# ------------------------------------------------------------------------------------------------ 4: backward extremes
@pytest.mark.parametrize("dtype,C", [(torch.float32, 3), (torch.float32, 4), (torch.bfloat16, 5), (torch.bfloat16, 8)],
                         ids=["f32-elem", "f32-vec", "bf16-elem", "bf16-vec"])
@pytest.mark.parametrize("mode", A.FILL_MODES)
def test_backward_at_forced_extreme_offsets(dtype, C, mode):
    """``count = 1`` pins the offset: at +-H the whole image is out of range (``nearest`` piles all H rows of
    ``dy`` on one edge row: a run of |off| + 1 = H + 1 candidates of which H exist), at +-(H - 1) one row is
    left; both flips drawn and off."""
    H, W = 5, 7
    x = _values((3, H, W, C), dtype)
    for oh, ow in ((H, W), (-H, -W), (H - 1, -(W - 1)), (-(H - 1), W - 1), (H, 0), (0, -W), (2, -3)):
        for flips in (False, True):
            spec = A.Spec(flip_h=flips, flip_w=flips, off_h_lo=oh, off_w_lo=ow, out_h=H, out_w=W, fill_mode=mode,
                          fill_value=1.5)
            _check_pair(x, spec, what=f"off ({oh}, {ow}) flips {flips}")
    if mode == "nearest":  # the run itself: every dy row lands on input row H - 1, summed in ascending order
        spec = A.Spec(off_h_lo=H, out_h=H, out_w=W, fill_mode=mode)
        dy = _grads((3, H, W, C), dtype)
        dx = _C().augment_bwd(dy.cuda(), torch.tensor([0], device="cuda"), KEY[0], KEY[1], *spec.args(), H, W).cpu()
        acc = torch.zeros(3, W, C)
        for r in range(H):
            acc = acc + dy[:, r].float()
        assert torch.equal(dx[:, H - 1].float(), acc.to(dtype).float()) and not dx[:, :H - 1].any()


# ------------------------------------------------------------------------------------------------ the bindings, the op
def test_bindings_refuse_what_the_kernels_do_not_take():
    C = _C()
    st = _State(0)
    x = torch.zeros(2, 4, 4, 3, device="cuda")
    ok = A.Spec(out_h=4, out_w=4)
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    for bad in (ok._replace(out_h=5), ok._replace(out_w=0), ok._replace(off_h_lo=-5), ok._replace(off_w_lo=3, off_w_count=3),
                ok._replace(off_h_count=0)):
        with pytest.raises(RuntimeError):
            C.augment_fwd(x, st.view, 1, 2, *bad.args())
        with pytest.raises(RuntimeError):
            C.augment_bwd(x[:, :bad.out_h, :max(bad.out_w, 1)].contiguous(), t, 1, 2, *bad.args(), 4, 4)
    args = list(ok.args())
    args[8] = 4  # no such fill mode
    with pytest.raises(RuntimeError):
        C.augment_fwd(x, st.view, 1, 2, *args)
    with pytest.raises(RuntimeError):
        C.augment_fwd(x.double(), st.view, 1, 2, *ok.args())
    with pytest.raises(RuntimeError):
        C.augment_fwd(x.permute(0, 2, 1, 3), st.view, 1, 2, *ok.args())  # not contiguous
    with pytest.raises(RuntimeError):
        C.augment_fwd(x[0], st.view, 1, 2, *ok.args())  # not 4-D
    with pytest.raises(RuntimeError):
        C.augment_fwd(x, st.view, 1 << 32, 2, *ok.args())
    with pytest.raises(RuntimeError):
        C.augment_fwd(x, st.view.to(torch.int32), 1, 2, *ok.args())
    with pytest.raises(RuntimeError):
        C.augment_bwd(x, t, 1, 2, *ok.args(), 3, 4)  # dy larger than the input it claims
    with pytest.raises(RuntimeError):
        C.augment_bwd(x, t.cpu(), 1, 2, *ok.args(), 4, 4)
    assert st.get() == [0, 0]


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64, torch.float32, torch.bfloat16],
                         ids=["f16", "f64", "f32", "bf16"])
def test_op_matches_the_cpu_path(dtype):
    """ops.augment on the GPU (f16 / f64 through the f32 kernel, a non-contiguous input made contiguous)
    against the same call on the CPU: outputs and input gradients, bit for bit; it works under no_grad."""
    base = torch.randn(3, 7, 6, 4, generator=torch.Generator().manual_seed(2)).to(dtype)
    for spec in (_full_spec(6, 7, "reflect"), _full_spec(6, 7, "constant", 1.00390625 + 2.0 ** -20),
                 A.Spec(off_h_count=4, off_w_count=3, out_h=3, out_w=5)):
        st = torch.tensor([4, 0], dtype=torch.int64, device="cuda")
        xg = base.cuda().permute(0, 2, 1, 3).requires_grad_(True)  # [3, 6, 7, 4], non-contiguous
        xh = base.permute(0, 2, 1, 3).clone().requires_grad_(True)
        yg = A.augment(xg, spec, KEY, state=st)
        yh = A.augment(xh, spec, KEY, ticket=4)
        assert yg.dtype == dtype and yg.shape == yh.shape
        assert torch.equal(yg.detach().cpu().contiguous().view(torch.uint8), yh.detach().contiguous().view(torch.uint8))
        dy = torch.randn(yh.shape, generator=torch.Generator().manual_seed(3)).to(dtype)
        yg.backward(dy.cuda())
        yh.backward(dy)
        assert torch.equal(xg.grad.cpu().contiguous().view(torch.uint8), xh.grad.contiguous().view(torch.uint8))
        assert st.cpu().tolist() == [5, 0]
        with torch.no_grad():
            A.augment(xg, spec, KEY, state=st)
        assert st.cpu().tolist() == [6, 0]
