"""The seeded-dropout kernels (csrc/kernels/dropout.hip) bit for bit against the numpy Philox reference of
ops/dropout.py: the full-shape kernel at the edges of its vectors, workgroups and grid-stride trips, the
broadcast (noise_shape) kernel in both of its forms, the counter words (group index and ticket past 2^32),
and the device-side ticket, eagerly and in a replayed graph.

Inputs are 16-byte-aligned views inside sentinel-filled buffers (the kernels read them; the call counter is
the one operand they write), and every test checks that nothing but the counter changed in those buffers.
Outputs are allocated by the bindings.  Sizes come from the extension's constants: DROPOUT_WG_ELEMS elements
per workgroup and trip, DROPOUT_SMALL_WG_ELEMS for tensors of up to DROPOUT_SMALL_N elements (the same kernel
at another workgroup size: both sides of that threshold are tested), DROPOUT_MAX_GRID the grid cap.  The
second grid-stride trip is reached with the cap lowered by ``dropout_force_max_grid``, since MAX_GRID *
WG_ELEMS elements are too many for a quick test."""
import functools

import numpy as np
import pytest
import torch

from tensorflow_distributed_learning_amd.ops import dropout as D

pytestmark = pytest.mark.gpu

KEY = (0x1234ABCD, 0x9E3779B9)
SENT = {torch.float32: (torch.int32, 0x4B1D5EED), torch.bfloat16: (torch.int16, 0x4B1D)}  # finite patterns
SENT64 = 0x4B1D5EED4B1D5EED


def _C():
    from tensorflow_distributed_learning_amd.ops import hip

    return hip()


@functools.lru_cache(maxsize=None)
def _consts():
    C = _C()
    return int(C.DROPOUT_WG_ELEMS), int(C.DROPOUT_MAX_GRID)


@functools.lru_cache(maxsize=None)
def _small():
    C = _C()
    return int(C.DROPOUT_SMALL_WG_ELEMS), int(C.DROPOUT_SMALL_N)


def _sizes():
    WG, _ = _consts()
    SWG, SN = _small()
    assert SN % WG == 0 and WG % SWG == 0
    small = [1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 1023, 1024, 1025, SWG - 1, SWG, SWG + 1, WG - 1, WG, WG + 1, SN - 1, SN]
    # past the threshold: kDropoutWgElems per workgroup; a last workgroup of 1, WG - 1, WG (a whole trip), WG + 1
    # elements, and one that ends in whole vectors and a tail
    return small + [SN + 1, SN + WG - 1, SN + WG, SN + WG + 1, SN + 1029]


def _ibits(t):
    return t.contiguous().view(SENT[t.dtype][0] if t.dtype in SENT else torch.int64)


class _Operand:
    """``values`` (a CPU tensor of any shape) as an aligned view inside a sentinel-filled device buffer."""

    def __init__(self, values):
        values = values.contiguous()
        self.itype, self.sent = SENT[values.dtype]
        n = values.numel()
        pad = 16 // values.element_size()
        self.buf = torch.full((n + 2 * pad + 3,), self.sent, dtype=self.itype, device="cuda")
        self.view = self.buf[pad:pad + n].view(values.dtype).view(values.shape)
        self.view.copy_(values)
        assert self.view.data_ptr() % 16 == 0
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
    flat[::7] = float("inf")  # a dropped inf must become 0, not NaN
    flat[3::11] = float("-inf")
    flat[5::13] = 1e-39  # subnormal in both dtypes
    return x.to(dtype)


def _want(x, ticket, rate, off=0, noise_shape=None):
    """x (CPU) through the reference mask: x * f32 scale in f32, rounded to x's dtype; dropped = +0."""
    shape = tuple(noise_shape) if noise_shape is not None else tuple(x.shape)
    keep = torch.from_numpy(D.philox_reference(KEY, ticket, None, D.threshold(rate), off, shape))
    y = (x.float() * torch.tensor(D.keep_scale(rate), dtype=torch.float32)).to(x.dtype)
    return torch.where(keep, y, torch.zeros((), dtype=x.dtype))


def _check_pair(x, rate, ticket0=3, off=0, noise_shape=None, what=""):
    """Forward and backward of one call against the reference; returns the forward output."""
    C = _C()
    st = _State(ticket0)
    xo = _Operand(x)
    dy = _values(tuple(x.shape), x.dtype, seed=1)
    dyo = _Operand(dy)
    ns = D._noise_strides(noise_shape) if noise_shape is not None else None
    T, scale = D.threshold(rate), D.keep_scale(rate)
    y, t = C.dropout_fwd(xo.view, st.view, KEY[0], KEY[1], T, scale, ns, off)
    assert t.dtype == torch.int64 and t.numel() == 1 and int(t.cpu()[0]) == ticket0, f"{what}: ticket"
    assert st.get() == [ticket0 + 1, 0], f"{what}: state after the call"
    assert y.shape == x.shape and y.dtype == x.dtype
    assert torch.equal(_ibits(y.cpu()), _ibits(_want(x, ticket0, rate, off, noise_shape))), f"{what}: forward"
    dx = C.dropout_bwd(dyo.view, t, KEY[0], KEY[1], T, scale, ns, off)
    assert torch.equal(_ibits(dx.cpu()), _ibits(_want(dy, ticket0, rate, off, noise_shape))), f"{what}: backward"
    assert st.get() == [ticket0 + 1, 0], f"{what}: the backward touched the state"
    xo.assert_unchanged(what + " x")
    dyo.assert_unchanged(what + " dy")
    return y


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_full_shape_sizes(dtype):
    for n in _sizes():
        _check_pair(_values((n,), dtype), 0.5, what=f"n={n}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_second_grid_stride_trip(dtype):
    C = _C()
    WG, MAXG = _consts()
    SWG, SN = _small()
    assert MAXG >= 3
    C.dropout_force_max_grid(3)
    try:
        _check_pair(_values((3 * SWG + 5,), dtype), 0.5, what="cap 3, 3 SWG + 5")  # trip 2: a tail of 5
        _check_pair(_values((7 * SWG + 1029,), dtype), 0.5, what="cap 3, 7 SWG + 1029")  # trip 3: vectors + a tail
        # the large-tensor form: 3 workgroups stride over 64 whole trips and a last one of 5 / of 1029 elements
        _check_pair(_values((SN + 5,), dtype), 0.5, what="cap 3, SMALL_N + 5")
        _check_pair(_values((SN + 2 * WG + 1029,), dtype), 0.5, what="cap 3, SMALL_N + 2 WG + 1029")
    finally:
        C.dropout_force_max_grid(0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rate", [0.1, 0.5, 1 - 2.0 ** -20, 1.0], ids=["0.1", "0.5", "1-2^-20", "1"])
def test_rates(dtype, rate):
    WG, _ = _consts()
    y = _check_pair(_values((WG + 5,), dtype), rate, what=f"rate={rate}")
    if rate == 1.0:
        assert (_ibits(y) == 0).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_group_index_crosses_2_32(dtype):
    off = (1 << 34) - 8
    y = _check_pair(_values((16,), dtype), 0.5, off=off, what="elem_offset 2^34 - 8")
    # the high group word is used: the same call without it gives another mask
    low = _check_pair(_values((16,), dtype), 0.5, off=off & 0xFFFFFFFF, what="low offset")
    assert not torch.equal(_ibits(y), _ibits(low))


def test_ticket_carries_into_the_high_word():
    C = _C()
    x = _values((1029,), torch.float32)
    xo, st = _Operand(x), _State((1 << 32) - 1)
    T, scale = D.threshold(0.5), D.keep_scale(0.5)
    outs = []
    for want_t in ((1 << 32) - 1, 1 << 32):
        y, t = C.dropout_fwd(xo.view, st.view, KEY[0], KEY[1], T, scale)
        assert int(t.cpu()[0]) == want_t
        assert torch.equal(_ibits(y.cpu()), _ibits(_want(x, want_t, 0.5)))
        outs.append(y)
    assert st.get() == [(1 << 32) + 1, 0]
    assert not torch.equal(outs[0], outs[1])
    # ticket 2^32 is not ticket 0
    assert not torch.equal(_ibits(outs[1].cpu()), _ibits(_want(x, 0, 0.5)))
    xo.assert_unchanged("x")


@pytest.mark.parametrize("which", ["one workgroup", "many workgroups", "capped grid", "large form"])
def test_twenty_calls_take_tickets_in_order(which):
    C = _C()
    WG, _ = _consts()
    n = {"one workgroup": 1000, "many workgroups": 37 * WG + 3, "capped grid": 9 * WG + 3,
         "large form": _small()[1] + 3 * WG + 3}[which]
    x = _values((n,), torch.bfloat16)
    xo, st = _Operand(x), _State(0)
    T, scale = D.threshold(0.25), D.keep_scale(0.25)
    if which == "capped grid":
        C.dropout_force_max_grid(4)
    try:
        for k in range(20):
            y, t = C.dropout_fwd(xo.view, st.view, KEY[0], KEY[1], T, scale)
            assert int(t.cpu()[0]) == k and st.get() == [k + 1, 0]
            if k in (0, 19):
                assert torch.equal(_ibits(y.cpu()), _ibits(_want(x, k, 0.25)))
    finally:
        C.dropout_force_max_grid(0)
    xo.assert_unchanged("x")


def test_graph_replays_draw_fresh_masks():
    C = _C()
    WG, _ = _consts()
    x = _values((2 * WG + 77,), torch.float32)
    xo, st = _Operand(x), _State(5)
    T, scale = D.threshold(0.5), D.keep_scale(0.5)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=s):
        y, t = C.dropout_fwd(xo.view, st.view, KEY[0], KEY[1], T, scale)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert st.get() == [5, 0], "the capture consumed a ticket"
    outs = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert int(t.cpu()[0]) == 5 + k and st.get() == [6 + k, 0]
        outs.append(y.cpu().clone())
        assert torch.equal(_ibits(outs[-1]), _ibits(_want(x, 5 + k, 0.5))), f"replay {k}"
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2]) and \
        not torch.equal(outs[0], outs[2])
    xo.assert_unchanged("x")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_broadcast(dtype):
    for c in (1, 5, 8, 16, 24):
        _check_pair(_values((3, 2, 3, c), dtype), 0.5, noise_shape=(3, 1, 1, c), what=f"C={c}")
    _check_pair(_values((4, 6), dtype), 0.5, noise_shape=(4, 1), what="(4, 6) / (4, 1)")
    _check_pair(_values((4, 8), dtype), 0.5, noise_shape=(4, 1), what="(4, 8) / (4, 1)")  # vector form, stride 0
    _check_pair(_values((5, 3, 8), dtype), 0.5, noise_shape=(1, 3, 8), what="leading broadcast")
    _check_pair(_values((2, 3, 4, 12), dtype), 0.5, noise_shape=(2, 1, 4, 1), what="alternating")
    # more than one workgroup, and a capped grid that strides
    C = _C()
    C.dropout_force_max_grid(2)
    try:
        _check_pair(_values((5, 9, 7, 24), dtype), 0.25, noise_shape=(5, 1, 1, 24), what="strided vector form")
        _check_pair(_values((5, 9, 7, 12), dtype), 0.25, noise_shape=(5, 1, 1, 12), what="strided 4-wide form")
        _check_pair(_values((5, 9, 24), dtype), 0.25, noise_shape=(5, 9, 1), what="strided vector form, stride 0")
        _check_pair(_values((5, 9, 7, 23), dtype), 0.25, noise_shape=(5, 1, 1, 23), what="strided scalar form")
    finally:
        C.dropout_force_max_grid(0)


def test_bindings_refuse_what_the_kernels_do_not_take():
    C = _C()
    st = _State(0)
    x = torch.zeros(16, device="cuda")
    T, scale = D.threshold(0.5), D.keep_scale(0.5)
    with pytest.raises(RuntimeError):
        C.dropout_fwd(x.double(), st.view, 1, 2, T, scale)
    with pytest.raises(RuntimeError):
        C.dropout_fwd(x, st.view, 1, 2, T, scale, None, 2)  # elem_offset not a multiple of 4
    with pytest.raises(RuntimeError):
        C.dropout_fwd(x, st.view, 1, 2, (1 << 32) + 1, scale)
    with pytest.raises(RuntimeError):
        C.dropout_fwd(x[1:], st.view, 1, 2, T, scale)  # misaligned
    with pytest.raises(RuntimeError):
        C.dropout_fwd(x, st.view.to(torch.int32), 1, 2, T, scale)
    assert st.get() == [0, 0]


# ------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize("dtype", [torch.float16, torch.float64, torch.float32, torch.bfloat16],
                         ids=["f16", "f64", "f32", "bf16"])
def test_op_matches_the_cpu_path(dtype):
    """ops.dropout on the GPU (f16 / f64 through the f32 kernel, a misaligned non-contiguous input made
    contiguous) against the same call on the CPU: outputs and input gradients, bit for bit."""
    base = torch.randn(33, 70, generator=torch.Generator().manual_seed(2)).to(dtype)
    xc = base[:, 1:66].t()  # non-contiguous, first element off the 16-byte grid
    for ns in (None, (65, 1)):
        st = torch.tensor([4, 0], dtype=torch.int64, device="cuda")
        xg = base.cuda()[:, 1:66].t().requires_grad_(True)
        xh = xc.clone().requires_grad_(True)
        yg = D.dropout(xg, 0.3, KEY, state=st, noise_shape=ns)
        yh = D.dropout(xh, 0.3, KEY, ticket=4, noise_shape=ns)
        assert yg.dtype == dtype and yg.shape == xh.shape
        assert torch.equal(yg.detach().cpu().view(torch.uint8), yh.detach().contiguous().view(torch.uint8))
        dy = torch.randn(65, 33, generator=torch.Generator().manual_seed(3)).to(dtype)
        yg.backward(dy.cuda())
        yh.backward(dy)
        assert torch.equal(xg.grad.cpu().contiguous().view(torch.uint8), xh.grad.contiguous().view(torch.uint8))
        assert st.cpu().tolist() == [5, 0]
        with torch.no_grad():
            D.dropout(xg, 0.3, KEY, state=st, noise_shape=ns)
        assert st.cpu().tolist() == [6, 0]
