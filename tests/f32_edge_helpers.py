"""Shared plumbing of test_gemm_f32_edges_gpu.py and test_conv_f32_edges_gpu.py (csrc/kernels/gemm_f32.hip
through its raw bindings): operands as views inside NaN-filled buffers (aligned, or offset by one float to
take the scalar loaders), caller-supplied outputs between sentinel blocks, bitwise comparison against the
f64 references of conv_refs.py on exactly representable integers, and the record of which kernels ran.

Every runner takes a dict of options, launches once, asserts the selection the case was designed for
(f32_last_selected), and compares.  Each sets every A/B hook for its launch (so the kernel a case expects does
not depend on the TDL_F32_* variables the process started with) and puts the earlier values back.  Nothing here chooses a tolerance: integer data is compared with
np.array_equal after assert_exact; the random-data checks use conv_refs.error_bound_f32."""
import contextlib

import numpy as np
import torch

import conv_refs as CR

RAN = set()      # every main / reduce kernel name a case of either file has launched
PAD = 64         # floats of NaN around every operand (256 B: keeps the view 16-byte aligned)
GUARD = 256      # sentinel floats on either side of a caller-supplied output
SENTINEL = -7.0e33


def hip():
    from tensorflow_distributed_learning_amd.ops import hip as _hip

    return _hip()


@contextlib.contextmanager
def hooks(buf=None, narrow=None, hoist=None, reduce16=None):
    """The run-time A/B hooks given (None: left alone) set for the block; each setter returns the value it
    replaced, and that value -- whatever the process started with -- is put back afterwards."""
    C = hip()
    setters = ((C.f32_buf, buf), (C.f32_reduce_narrow, narrow), (C.f32_pool_hoist, hoist), (C.f32_reduce16, reduce16))
    undo = []
    try:
        for f, v in setters:
            if v is not None:
                undo.append((f, f(bool(v))))
        yield
    finally:
        for f, was in reversed(undo):
            f(was)


def dev(arr, mis=False, dtype=torch.float32):
    """A contiguous CUDA view holding arr, inside a buffer of NaNs (0xFF bytes for uint8): 16-byte aligned,
    or one float past alignment when mis (the host then has to pick the element-wise loader)."""
    a = np.ascontiguousarray(arr)
    n = a.size
    if dtype == torch.uint8:
        buf = torch.full((n + 2 * PAD * 4,), 0xFF, dtype=torch.uint8, device="cuda")
        off = PAD * 4
        src = torch.from_numpy(a.astype(np.uint8))
    else:
        buf = torch.full((n + 2 * PAD + 4,), float("nan"), dtype=torch.float32, device="cuda")
        off = PAD + (1 if mis else 0)
        with np.errstate(invalid="ignore", over="ignore"):
            src = torch.from_numpy(a.astype(np.float32))
    v = buf[off:off + n].view(a.shape)
    v.copy_(src.view(a.shape))
    if dtype != torch.uint8:
        assert v.data_ptr() % 16 == (4 if mis else 0)
    assert v.is_contiguous()
    return v


class Guarded:
    """A caller-supplied output (prior contents given) between two blocks of sentinels."""

    def __init__(self, prior):
        p = np.ascontiguousarray(prior, dtype=np.float32)
        self.buf = torch.full((p.size + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.view = self.buf[GUARD:GUARD + p.size].view(p.shape)
        self.view.copy_(torch.from_numpy(p))
        self.n = p.size
        self.before = self.buf.view(torch.int32).clone()

    def check(self, what):
        now = self.buf.view(torch.int32)
        assert torch.equal(now[:GUARD], self.before[:GUARD]), f"{what}: wrote before the output"
        assert torch.equal(now[GUARD + self.n:], self.before[GUARD + self.n:]), f"{what}: wrote past the output"


def selected(expect_main=None, expect_reduce=None, expect_splits=None):
    """The selection of the launch just made, recorded and compared with what the case was built for."""
    main, red, splits, kchunk = hip().f32_last_selected()
    RAN.add(main)
    RAN.add(red)
    if expect_main is not None:
        assert main == expect_main, (main, expect_main)
    if expect_reduce is not None:
        assert red == expect_reduce, (red, splits, expect_reduce)
    if expect_splits is not None:
        assert splits == expect_splits, (splits, kchunk, expect_splits)
    return main, red, splits, kchunk


def same_bits(got, want, what):
    """got (CUDA f32) == want (f64 reference, exactly representable) element for element; NaNs where and
    only where the reference has them (-0 == +0)."""
    g = got.detach().cpu().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.asarray(want, np.float64).astype(np.float32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w, equal_nan=True):
        bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} differ, first at {i}: got {g[i]}, want {w[i]}")


def ints(shape, amp, salt, zero_frac=0.0):
    return CR.coded_ints(shape, amp, salt, zero_frac)


def amp_of(reduction):
    """Amplitude for a reduction of this length: output std about 300, every sum far below 2^24."""
    return CR.amp_for(reduction, 300.0)


def b01(v):
    return "1" if v else "0"


# ------------------------------------------------------------------------------------------- GEMM
def run_gemm(M, N, K, ta=0, tb=1, bias=False, act=0, acc=False, amask=False, bmask=False, dbias=False, out=None,
             mis_a=False, mis_b=False, mis_am=False, mis_bm=False, buf=True, salt=0, reduce=None, splits=None,
             poke=None):
    """One gemm_f32 launch on integer data against the f64 product.  A is [M][K] (ta = 1: stored [K][M]),
    B is [K][N] (tb = 0: stored [N][K]); masks share the stored layout.  out: None (a fresh tensor) or True
    (a guarded caller tensor; acc adds into its integer contents).  poke(A, B, AM, BM) may edit the logical
    f64 operands (non-finite cases).  Returns the output tensor."""
    C = hip()
    amp = amp_of(K)
    A, B = ints((M, K), amp, 11 + salt), ints((K, N), amp, 12 + salt)
    AM = ints((M, K), 2, 13 + salt) if amask else None  # values in [-2, 2]: about 40 % pass
    BM = ints((K, N), 2, 14 + salt) if bmask else None
    if poke is not None:
        poke(A, B, AM, BM)
    bia = ints((N,), 50, 15 + salt) if bias else None
    use_out = out is not None or acc
    prior = ints((M, N), 40, 16 + salt) if use_out else None
    dprior = ints((N,), 40, 17 + salt) if dbias else None
    Am, Bm = CR.masked_ref(A, AM), CR.masked_ref(B, BM)
    with np.errstate(invalid="ignore", over="ignore"):
        want = Am @ Bm
        ab = np.abs(np.nan_to_num(Am, nan=0.0, posinf=0.0, neginf=0.0)) @ np.abs(
            np.nan_to_num(Bm, nan=0.0, posinf=0.0, neginf=0.0))
    want = CR.bias_act_ref(want, bia, act, prior if acc else None)
    CR.assert_exact(ab + (np.abs(bia) if bias else 0) + (np.abs(prior) if acc else 0))

    def store(x, t, mis):
        return None if x is None else dev(x.T if t else x, mis)

    a_d, am_d = store(A, ta, mis_a), store(AM, ta, mis_am)
    b_d, bm_d = store(B, not tb, mis_b), store(BM, not tb, mis_bm)
    go = Guarded(prior) if use_out else None
    gd = Guarded(dprior) if dbias else None
    with hooks(buf=buf, narrow=True, hoist=True, reduce16=True):
        got = C.gemm_f32(a_d, ta, b_d, tb, bias=dev(bia) if bias else None, out=go.view if go else None,
                         accumulate=acc, act=act, amask=am_d, bmask=bm_d, dbias=gd.view if gd else None)
    va = ta == 0 and K % 4 == 0 and not mis_a and not (amask and mis_am)
    vb = tb == 1 and N % 4 == 0 and not mis_b and not (bmask and mis_bm)
    name = f"gemm_ma{b01(amask)}_mb{b01(bmask)}_va{b01(va)}_vb{b01(vb)}_buf{b01(buf)}"
    what = f"gemm {M}x{N}x{K} ta{ta} tb{tb} {name}"
    _, red, sp, _ = selected(name, reduce, splits)
    if K <= 256:
        assert (red, sp) == ("none", 1), (what, red, sp)
    same_bits(got, want, what)
    if go:
        assert got.data_ptr() == go.view.data_ptr()
        go.check(what)
    if gd:
        with np.errstate(invalid="ignore", over="ignore"):
            dwant = Bm.sum(0) + (dprior if acc else 0)
        CR.assert_exact(np.abs(np.nan_to_num(Bm, nan=0.0, posinf=0.0, neginf=0.0)).sum(0) + np.abs(dprior))
        same_bits(gd.view, dwant, what + " dbias")
        gd.check(what + " dbias")
    return got


# ------------------------------------------------------------------------------------------- convolutions
def out_size(i, k, s, d, p0, p1):
    return (i + p0 + p1 - (k - 1) * d - 1) // s + 1


class Geo:
    """(N, H, W, C, K, R, S) with strides, pads (top, bottom, left, right) and dilations."""

    def __init__(self, N, H, W, C, K, R, S, stride=(1, 1), pads=(0, 0, 0, 0), dil=(1, 1)):
        self.N, self.H, self.W, self.C, self.K, self.R, self.S = N, H, W, C, K, R, S
        self.sh, self.sw = stride
        self.pt, self.pb, self.pl, self.pr = pads
        self.dh, self.dw = dil
        self.OH = out_size(H, R, self.sh, self.dh, self.pt, self.pb)
        self.OW = out_size(W, S, self.sw, self.dw, self.pl, self.pr)
        assert self.OH >= 1 and self.OW >= 1, "empty output"

    @property
    def kw(self):  # the references' geometry arguments after (oh, ow) / (h, w) / (r, s)
        return dict(sh=self.sh, sw=self.sw, pt=self.pt, pl=self.pl, dh=self.dh, dw=self.dw)

    def bind(self):  # the bindings' (sh, sw, pt, pl, dh, dw)
        return (self.sh, self.sw, self.pt, self.pl, self.dh, self.dw)

    def __repr__(self):
        return (f"N{self.N} {self.H}x{self.W}x{self.C}->{self.OH}x{self.OW}x{self.K} f{self.R}x{self.S} "
                f"s{self.sh}{self.sw} p{self.pt}{self.pb}{self.pl}{self.pr} d{self.dh}{self.dw}")


def _finite_abs(v):
    return np.abs(np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0))


def run_fwd(g, bias=True, act=0, mis_x=False, mis_w=False, buf=True, salt=0, reduce=None, splits=None, poke=None,
            pool=False, hoist=True, narrow=True, unfused=None):
    """conv_f32_fwd (or, pool, conv_f32_fwd_pool) on integer data against the f64 convolution."""
    C = hip()
    red_len = g.R * g.S * g.C
    amp = amp_of(red_len)
    x, w = ints((g.N, g.H, g.W, g.C), amp, 21 + salt), ints((g.R, g.S, g.C, g.K), amp, 22 + salt)
    bia = ints((g.K,), 50, 23 + salt) if bias else None
    if poke is not None:
        poke(x, w, bia)
    w_ohwi = w.transpose(3, 0, 1, 2)
    _, ab = CR.conv_fwd_ref(_finite_abs(x), _finite_abs(w_ohwi), g.OH, g.OW, **g.kw)
    CR.assert_exact(ab + (_finite_abs(bia) if bias else 0))
    xd, wd, bd = dev(x, mis_x), dev(w, mis_w), (dev(bia) if bias else None)
    name = f"fwd_va{b01(g.C % 4 == 0 and not mis_x)}_vb{b01(g.K % 4 == 0 and not mis_w)}_buf{b01(buf)}"
    what = f"{'pooled ' if pool else ''}fwd {g} act{act} {name}"
    with hooks(buf=buf, hoist=hoist, narrow=narrow, reduce16=True):
        if not pool:
            y = C.conv_f32_fwd(xd, wd, bd, g.OH, g.OW, *g.bind(), act=act)
            sel = selected(name, reduce, splits)
            acc, _ = CR.conv_fwd_ref(x, w_ohwi, g.OH, g.OW, **g.kw)
            same_bits(y, CR.bias_act_ref(acc, bia, act), what)
            return y, sel
        y, p, arg = C.conv_f32_fwd_pool(xd, wd, bd, g.OH, g.OW, *g.bind(), act=act)
        sel = selected(name, reduce, splits)
    PH, PW = g.OH // 2, g.OW // 2
    M_unf = g.N * g.OH * g.OW
    s, c, u = C.f32_plan(g.N * PH * PW * 4, g.K, red_len, True, M_unf)
    assert (sel[2], sel[3]) == (s, c), (what, sel, s, c)
    if unfused is not None:
        assert u == unfused, (what, u, unfused)
    yr, mr, ar, _ = CR.conv_pool_fwd_ref(x, w_ohwi, bia, g.OH, g.OW, **g.kw, act=act)
    with np.errstate(invalid="ignore"):  # (the data tells a window's positions apart: a swapped decode shows)
        assert (yr[:, 0:2 * PH:2, 1:2 * PW:2] != yr[:, 1:2 * PH:2, 0:2 * PW:2]).any(), what
        assert len(np.unique(ar[ar < 4])) >= 3 or ar.size < 8, what
    same_bits(y[:, :2 * PH, :2 * PW], yr[:, :2 * PH, :2 * PW], what + " y (inside the windows)")
    same_bits(p, mr, what + " maximum")
    assert torch.equal(arg.cpu(), torch.from_numpy(ar)), what + " argmax"
    return (y, p, arg), sel


def _pin_data(g, salt, k255=True):
    """Synthetic pooled backward inputs for a conv output of g.OH x g.OW: the pool's output gradient, the
    pooled maximum (about 40 % <= 0) and argmax bytes in {0..3} with some 255 set by hand."""
    PH, PW = g.OH // 2, g.OW // 2
    shape = (g.N, PH, PW, g.K)
    dp = ints(shape, amp_of(g.R * g.S * g.K), 31 + salt)
    mx = ints(shape, 2, 32 + salt)
    arg = (ints(shape, 8, 33 + salt) + 8).astype(np.int64) % 4
    if k255:
        arg = np.where(ints(shape, 5, 34 + salt) == 5, 255, arg)
        arg.reshape(-1)[-1] = 255
    return dp, mx, arg.astype(np.uint8)


def run_dgrad(g, mask=False, hwio=True, mis_dy=False, mis_w=False, mis_m=False, buf=True, salt=0, reduce=None,
              splits=None, poke=None, pin=False):
    """conv_f32_dgrad on integer data against the f64 input gradient (pin: from the POOLED gradient,
    against conv_pool_bwd_ref followed by the same reference).  poke(dy, w, mask), or with pin
    poke(dp, w, maximum, argmax), may edit the f64 operands."""
    C = hip()
    amp = amp_of(g.R * g.S * g.K)
    w = ints((g.R, g.S, g.C, g.K), amp, 42 + salt)
    if pin:
        dp, mx, arg = _pin_data(g, salt)
        if poke is not None:
            poke(dp, w, mx, arg)
        dy = CR.conv_pool_bwd_ref(dp, mx, arg, g.OH, g.OW)
        a_np, m_np = dp, mx
    else:
        dy0 = ints((g.N, g.OH, g.OW, g.K), amp, 41 + salt)
        m_np = ints(dy0.shape, 2, 43 + salt) if mask else None
        if poke is not None:
            poke(dy0, w, m_np)
        dy = CR.masked_ref(dy0, m_np)
        a_np = dy0
    want, _ = CR.conv_dgrad_ref(dy, w, g.H, g.W, **g.kw)
    _, ab = CR.conv_dgrad_ref(_finite_abs(dy), _finite_abs(w), g.H, g.W, **g.kw)
    CR.assert_exact(ab)
    a_d = dev(a_np, mis_dy)
    m_d = dev(m_np, mis_m) if m_np is not None else None
    w_d = dev(w if hwio else w.transpose(0, 1, 3, 2), mis_w)
    va = g.K % 4 == 0 and not mis_dy and not (m_np is not None and mis_m)
    vb = (not hwio) and g.C % 4 == 0 and not mis_w
    use_buf = buf and not pin
    name = f"dgrad_ma{b01(m_np is not None)}_va{b01(va)}_vb{b01(vb)}_pin{b01(pin)}_buf{b01(use_buf)}"
    what = f"dgrad {g} hwio{int(hwio)} {name}"
    kw = dict(pin_arg=dev(arg, dtype=torch.uint8), out_h=g.OH, out_w=g.OW) if pin else {}
    with hooks(buf=buf, narrow=True, hoist=True, reduce16=True):
        dx = C.conv_f32_dgrad(a_d, w_d, g.H, g.W, *g.bind(), dy_mask=m_d, w_hwio=hwio, **kw)
    sel = selected(name, reduce, splits)
    same_bits(dx, want, what)
    return dx, want, sel


def run_wgrad(g, mask=False, acc=False, out=False, dbias=False, mis_x=False, mis_dy=False, mis_m=False, buf=True,
              salt=0, reduce=None, splits=None, poke=None, pin=False):
    """conv_f32_wgrad on integer data against the f64 weight (and bias) gradient.  poke(x, dy, mask), or with
    pin poke(x, dp, maximum, argmax), may edit the f64 operands."""
    C = hip()
    npix = g.N * g.OH * g.OW
    amp = amp_of(npix)
    x = ints((g.N, g.H, g.W, g.C), amp, 51 + salt)
    if pin:
        dp, mx, arg = _pin_data(g, salt)
        if poke is not None:
            poke(x, dp, mx, arg)
        dy = CR.conv_pool_bwd_ref(dp, mx, arg, g.OH, g.OW)
        a_np, m_np = dp, mx
    else:
        dy0 = ints((g.N, g.OH, g.OW, g.K), amp, 52 + salt)
        m_np = ints(dy0.shape, 2, 53 + salt) if mask else None
        if poke is not None:
            poke(x, dy0, m_np)
        dy = CR.masked_ref(dy0, m_np)
        a_np = dy0
    use_out = out or acc
    prior = ints((g.R, g.S, g.C, g.K), 40, 54 + salt) if use_out else None
    dprior = ints((g.K,), 40, 55 + salt) if dbias else None
    want, _ = CR.conv_wgrad_ref(x, dy, g.R, g.S, **g.kw)
    _, ab = CR.conv_wgrad_ref(_finite_abs(x), _finite_abs(dy), g.R, g.S, **g.kw)
    CR.assert_exact(ab + (np.abs(prior) if acc else 0))
    if acc:
        with np.errstate(invalid="ignore"):
            want = want + prior
    go = Guarded(prior) if use_out else None
    gd = Guarded(dprior) if dbias else None
    x_d, a_d = dev(x, mis_x), dev(a_np, mis_dy)
    m_d = dev(m_np, mis_m) if m_np is not None else None
    use_buf = buf and not pin
    name = f"wgrad_ma{b01(m_np is not None)}_vb{b01(g.C % 4 == 0 and not mis_x)}_pin{b01(pin)}_buf{b01(use_buf)}"
    what = f"wgrad {g} {name}"
    kw = dict(pin_arg=dev(arg, dtype=torch.uint8), out_h=g.OH, out_w=g.OW) if pin else {}
    with hooks(buf=buf, narrow=True, hoist=True, reduce16=True):
        gw = C.conv_f32_wgrad(x_d, a_d, g.R, g.S, *g.bind(), out=go.view if go else None, accumulate=acc,
                              dy_mask=m_d, dbias=gd.view if gd else None, **kw)
    sel = selected(name, reduce, splits)
    same_bits(gw, want, what)
    if go:
        assert gw.data_ptr() == go.view.data_ptr()
        go.check(what)
    if gd:
        db, dab = CR.bias_grad_ref(dy)
        CR.assert_exact(_finite_abs(dy).reshape(-1, g.K).sum(0) + np.abs(dprior))
        with np.errstate(invalid="ignore"):
            same_bits(gd.view, db + (dprior if acc else 0), what + " dbias")
        gd.check(what + " dbias")
    return gw, want, sel
