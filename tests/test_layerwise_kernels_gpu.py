"""The layer-wise optimizer kernels (csrc/kernels/layerwise.hip: chunk sums, per-variable trust ratios, the LARS
and LAMB updates) launch by launch against the f64 references of tests/layerwise_refs.py.

Every operand is a 16-byte-aligned view inside a sentinel-filled buffer, and the slab operands (W, G, the
slots) keep the sentinel in the alignment padding BETWEEN the variables too: every run checks that nothing
but variable elements (and the partials / ratio / norms words) was written.  A norm clip's scale word comes
from ``clip_norm`` over a zero-padded copy of the gradient (it has its own tests, test_clip_kernels_gpu.py,
and sums the whole slab); the layer-wise launches read the sentinel-padded operand.

Layout (layerwise_refs.Case, CH = _C.LAYER_CHUNK): 10 variables of sizes [1, 3, 64, 65, CH - 1, CH, CH + 1,
2 CH + 3, 10, 128] -- a one-thread chunk, a ragged tail, an exact chunk, chunk + 1, a multi-chunk variable --
with variable 2 excluded from adaptation, 3 from decay, 8 all-zero weights, 9 all-zero gradients: every
``where`` branch.  3 steps at lr 0.05, 0.05, 0.0125, the last changed on the device.

Tolerances.  Chunk sums are f64 sums of exact products: relative 2^-40.  |w_i|, LARS's |g'_i| and LARS's ratio
are formed in f64 from such sums of the words the launch itself read (w is read back before the step) and
rounded once: 1 f32 ulp of the f64 value.  LAMB's u is evaluated in f32 and a + wd w can cancel: |u_i| and
the ratio are allowed 4 E_r + 1 ulp, E_r = the CPU f32 path's largest relative ratio error against the f64
reference (|u_i| = |w_i| / ratio carries the same relative error).  Updates are allowed 4 E + 1 ulp per tensor,
E = the CPU f32 path's largest error (``apply_flat`` on CPU tensors) over the 3 steps.  So that E cannot hide
a wrong CPU path, a test fails as ill-conditioned if E(w) > 1e-6 or E_r > 1e-5.
"""
import functools

import numpy as np
import pytest
import torch

import kernel_refs as R
import layerwise_refs as LR

pytestmark = pytest.mark.gpu

PAD = 4
SENT_BITS = 0x4B1D5EED
SENT64 = 0x4B1D5EED4B1D5EED
VARIANTS = [("lars", False), ("lars", True), ("lamb", False)]
VIDS = ["lars", "lars-nesterov", "lamb"]


def _C():
    from tensorflow_distributed_learning_amd.ops import hip

    return hip()


@functools.lru_cache(maxsize=None)
def _case():
    return LR.case(int(_C().LAYER_CHUNK))


class _Slab:
    """A slab operand of the test layout: the view buf[pad : pad + total] of a sentinel-filled buffer, the
    variables' elements set from ``values``, the padding between them left as sentinel."""

    def __init__(self, values, pad=PAD):
        c = _case()
        self.pad, self.n = pad, c.total
        self.buf = torch.full((c.total + 2 * pad + 3,), SENT_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
        self.view = self.buf[pad:pad + c.total]
        assert self.view.data_ptr() % 16 == 0
        self.set(values)

    def set(self, values):
        c = _case()
        host = np.full(c.total, SENT_BITS, dtype=np.int32).view(np.float32)
        host[c.mask] = np.asarray(values, dtype=np.float32)[c.mask]
        self.view.copy_(torch.from_numpy(host))

    def get(self):
        return self.view.cpu().numpy()

    def assert_outside_untouched(self, what):
        c = _case()
        b = self.buf.view(torch.int32).cpu().numpy()
        inner = b[self.pad:self.pad + self.n]
        assert (np.concatenate([b[:self.pad], b[self.pad + self.n:]]) == SENT_BITS).all(), f"{what}: wrote outside"
        assert (inner[~c.mask] == SENT_BITS).all(), f"{what}: wrote into the padding between variables"


class _Words:
    """partials [2 C] f64, ratio [V] and norms [2 V] f32, exactly sized, as aligned views in sentinel buffers."""

    def __init__(self, T):
        self.C, self.V = int(T.C), int(T.V)
        self.pbuf = torch.full((2 * self.C + 4,), SENT64, dtype=torch.int64, device="cuda")
        self.partials = self.pbuf[2:2 + 2 * self.C].view(torch.float64)
        self.rbuf = torch.full((self.V + 2 * PAD + 3,), SENT_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
        self.ratio = self.rbuf[PAD:PAD + self.V]
        self.nbuf = torch.full((2 * self.V + 2 * PAD,), SENT_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
        self.norms = self.nbuf[PAD:PAD + 2 * self.V]
        assert self.partials.data_ptr() % 16 == 0 and self.ratio.data_ptr() % 16 == 0 and self.norms.data_ptr() % 16 == 0

    def snapshot(self):
        return {"partials": self.partials.cpu().numpy().copy(), "ratio": self.ratio.cpu().numpy().copy(),
                "norms": self.norms.cpu().numpy().reshape(-1, 2).copy()}

    def assert_outside_untouched(self, what):
        p = self.pbuf.cpu().numpy()
        assert (np.concatenate([p[:2], p[2 + 2 * self.C:]]) == SENT64).all(), f"{what}: wrote outside partials"
        r = self.rbuf.view(torch.int32).cpu().numpy()
        assert (np.concatenate([r[:PAD], r[PAD + self.V:]]) == SENT_BITS).all(), f"{what}: wrote outside ratio"
        n = self.nbuf.view(torch.int32).cpu().numpy()
        assert (np.concatenate([n[:PAD], n[PAD + 2 * self.V:]]) == SENT_BITS).all(), f"{what}: wrote outside norms"


def _tables(wd=None, adapt=None):
    c = _case()
    T = _C().layer_tables(c.offsets, c.sizes, c.total, c.wd if wd is None else wd, c.adapt if adapt is None else adapt)
    assert T.V == c.V and T.n == c.total and T.C == sum((s + c.CH - 1) // c.CH for s in c.sizes)
    return T


class _Run:
    """The operands of one optimizer run and its launches."""

    def __init__(self, kind, nesterov, mode, pad=PAD, wd=None, adapt=None, grads=None):
        c = _case()
        self.kind, self.nesterov = kind, nesterov
        self.grads = c.grads if grads is None else grads
        self.cn, self.cv = c.clip_consts(mode)
        self.T = _tables(wd, adapt)
        self.words = _Words(self.T)
        zeros = np.zeros(c.total, np.float32)
        self.ops = {"w": _Slab(c.w0, pad), "g": _Slab(self.grads[0], pad)}
        for name in (["momentum"] if kind == "lars" else ["m", "v"]):
            self.ops[name] = _Slab(zeros, pad)
        self.lr = torch.tensor([LR.LR[0]], dtype=torch.float32, device="cuda")
        self.t0 = torch.zeros(1, dtype=torch.float32, device="cuda")
        # the norm clip's operands: the zero-padded gradient, clip_norm's partials and [scale, norm] words
        self.g_clean = torch.zeros(c.total, dtype=torch.float32, device="cuda")
        self.cpart = torch.zeros(max(1, int(_C().clip_partials(c.total))), dtype=torch.float64, device="cuda")
        self.cout = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
        self.gscale = self.cout if self.cn is not None else None

    def set_step(self, k):
        self.ops["g"].set(self.grads[k])
        self.g_clean.copy_(torch.from_numpy(np.ascontiguousarray(self.grads[k], dtype=np.float32)))
        self.lr.fill_(LR.LR[k])  # (changed on the device: the kernels read it there)
        self.t0.fill_(float(k))

    def launch(self, upto=3):
        C, T, o, wds = _C(), self.T, {k: s.view for k, s in self.ops.items()}, self.words
        clip = dict(gscale=self.gscale, clipvalue=self.cv)
        if self.cn is not None:
            C.clip_norm(self.g_clean, self.cpart, self.cout, self.cn, self.cv)
        if self.kind == "lars":
            C.lars_sums(T, o["w"], o["g"], wds.partials, **clip)
            if upto >= 2:
                C.lars_ratio(T, wds.partials, wds.ratio, wds.norms, LR.EETA, LR.LARS_EPS)
            if upto >= 3:
                C.lars_update(T, o["w"], o["g"], o["momentum"], wds.ratio, self.lr, LR.MOM, self.nesterov, **clip)
        else:
            hp = (self.t0, 0, LR.B1, LR.B2, LR.LAMB_EPS)
            C.lamb_sums(T, o["w"], o["g"], o["m"], o["v"], wds.partials, *hp, **clip)
            if upto >= 2:
                C.lamb_ratio(T, wds.partials, wds.ratio, wds.norms)
            if upto >= 3:
                C.lamb_update(T, o["w"], o["m"], o["v"], wds.ratio, self.lr, *hp)

    def scale_word(self):
        return self.cout.cpu().numpy()[0] if self.cn is not None else None

    def check_untouched(self, what):
        for name, s in self.ops.items():
            s.assert_outside_untouched(f"{what}: operand {name}")
        self.words.assert_outside_untouched(what)

    def state(self):
        return {k: s.get() for k, s in self.ops.items() if k != "g"}


def _run(kind, nesterov, mode, steps=3, **kw):
    """``steps`` steps; returns (final {name: f32 slab}, per step {w_before, scale, partials, ratio, norms})."""
    r = _Run(kind, nesterov, mode, **kw)
    log = []
    for k in range(steps):
        r.set_step(k)
        w_before = r.ops["w"].get()
        r.launch()
        torch.cuda.synchronize()
        log.append(dict(r.words.snapshot(), w_before=w_before, scale=r.scale_word()))
        assert (r.ops["g"].get()[_case().mask].view(np.uint32) ==
                np.asarray(r.grads[k], np.float32)[_case().mask].view(np.uint32)).all(), "the gradient is read-only"
    r.check_untouched(f"{kind} nesterov={nesterov} {mode}")
    return r.state(), log


def _conditions(kind, nesterov, mode):
    E, rel = LR.cpu_error(_case().CH, kind, nesterov, mode)
    assert E["w"] <= 1e-6 and rel <= 1e-5, f"ill-conditioned: CPU path E(w) {E['w']:.3e}, ratio error {rel:.3e}"
    return E, rel


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ------------------------------------------------------------------------------------- sums, norms, ratios
@pytest.mark.parametrize("mode", ["none", "both"])
def test_lars_partials_are_the_chunk_sums(mode):
    c = _case()
    r = _Run("lars", False, mode)
    r.set_step(0)
    r.launch(upto=1)
    torch.cuda.synchronize()
    r.check_untouched("lars_sums")
    got = r.words.partials.cpu().numpy().reshape(-1, 2)
    gp = LR.gprime(c.grads[0], r.cv, r.scale_word())
    w = c.w0.astype(np.float64)
    want = []
    for o, s in zip(c.offsets, c.sizes):
        for p in range(0, s, c.CH):
            a, b = w[o + p:o + min(s, p + c.CH)], gp[o + p:o + min(s, p + c.CH)]
            want.append((np.sum(a * a), np.sum(b * b)))
    want = np.array(want)
    assert got.shape == want.shape == (r.T.C, 2)
    assert (np.abs(got - want) <= 2.0 ** -40 * want).all()
    assert (r.state()["w"][c.mask].view(np.uint32) == c.w0[c.mask].view(np.uint32)).all(), "launch 1 writes no weight"


@pytest.mark.parametrize("mode", LR.MODES)
@pytest.mark.parametrize("kind,nesterov", [("lars", True), ("lamb", False)], ids=["lars", "lamb"])
def test_norms_and_ratios_match_f64(kind, nesterov, mode):
    c = _case()
    _, rel = _conditions(kind, nesterov, mode)
    _, log = _run(kind, nesterov, mode)
    ref, ref_ratios, ref_norms = LR.run_ref(c, kind, nesterov, mode, [s["scale"] for s in log])
    _, cv = c.clip_consts(mode)
    for k, s in enumerate(log):
        w = s["w_before"].astype(np.float64)
        nw = np.array([LR._norm(c.span(w, i)) for i in range(c.V)])
        assert (np.abs(s["norms"][:, 0] - nw) <= R.ulp32(nw)).all(), f"step {k}: |w_i|"
        if kind == "lars":
            gp = LR.gprime(c.grads[k], cv, s["scale"])
            _, _, want_r, want_n = LR.lars_step_ref(c, w, gp, np.zeros(c.total), LR.LR[k], nesterov)
            assert (np.abs(want_n[:, 0] - nw) == 0).all()
            err_n = np.abs(s["norms"][:, 1] - want_n[:, 1])
            err_r = np.abs(s["ratio"] - want_r)
            print(f"lars {mode} step {k}: |g'| err {np.max(err_n / R.ulp32(want_n[:, 1])):.3f} ulp, ratio err "
                  f"{np.max(err_r / R.ulp32(want_r)):.3f} ulp")
            assert (err_n <= R.ulp32(want_n[:, 1])).all(), f"step {k}: |g'_i|"
            assert (err_r <= R.ulp32(want_r)).all(), f"step {k}: ratio"
            for i in (LR.NO_ADAPT, LR.ZERO_G) + ((LR.ZERO_W,) if k == 0 else ()):
                assert _bits(s["ratio"])[i] == _bits(np.float32(1.0)), f"step {k}: ratio[{i}] must be exactly 1"
        else:
            want_n, want_r = ref_norms[k][:, 1], ref_ratios[k]
            err_n, err_r = np.abs(s["norms"][:, 1] - want_n), np.abs(s["ratio"] - want_r)
            tol_n, tol_r = 4 * rel * want_n + R.ulp32(want_n), 4 * rel * want_r + R.ulp32(want_r)
            print(f"lamb {mode} step {k}: |u| rel err {np.max(err_n / want_n):.3e}, ratio rel err "
                  f"{np.max(err_r / want_r):.3e} (CPU path {rel:.3e})")
            assert (err_n <= tol_n).all(), f"step {k}: |u_i|"
            assert (err_r <= tol_r).all(), f"step {k}: ratio"
            for i in (LR.NO_ADAPT,) + ((LR.ZERO_W,) if k == 0 else ()):
                assert _bits(s["ratio"])[i] == _bits(np.float32(1.0)), f"step {k}: ratio[{i}] must be exactly 1"


# ------------------------------------------------------------------------------------- updates
@pytest.mark.parametrize("mode", LR.MODES)
@pytest.mark.parametrize("kind,nesterov", VARIANTS, ids=VIDS)
def test_update_matches_f64_reference(kind, nesterov, mode):
    c = _case()
    E, _ = _conditions(kind, nesterov, mode)
    got, log = _run(kind, nesterov, mode)
    ref, _, _ = LR.run_ref(c, kind, nesterov, mode, [s["scale"] for s in log])
    if c.clip_consts(mode)[0] is not None:
        assert all(float(s["scale"]) < 1.0 for s in log), "the norm clip must be active"
    for name, r in ref.items():
        tol = (4.0 * E[name] + R.ulp32(r))[c.mask]
        err = np.abs(got[name].astype(np.float64) - r)[c.mask]
        worst = int(np.argmax(err / tol))
        print(f"{kind} nesterov={nesterov} {mode} {name}: max err {err.max():.3e}, CPU path max {E[name]:.3e}")
        assert (err <= tol).all(), f"{name}[{worst}]: err {err[worst]:.3e} > {tol[worst]:.3e}"
    assert np.abs(got["w"] - c.w0)[c.mask].max() > 1e-3


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip-operands"])
@pytest.mark.parametrize("nesterov", [False, True], ids=["momentum", "nesterov"])
def test_lars_with_everything_excluded_has_sgd_momentum_bits(nesterov, clip):
    c = _case()
    mode = "both" if clip else "none"
    got, log = _run("lars", nesterov, mode, wd=[0.0] * c.V, adapt=[False] * c.V)
    assert all((_bits(s["ratio"]) == _bits(np.float32(1.0))).all() for s in log)
    cn, cv = c.clip_consts(mode)
    C = _C()
    W = torch.from_numpy(c.w0.copy()).cuda()
    V = torch.zeros_like(W)
    lr = torch.zeros(1, device="cuda")
    part = torch.zeros(max(1, int(C.clip_partials(c.total))), dtype=torch.float64, device="cuda")
    out = torch.tensor([1.0, 0.0, 0.0, 0.0], device="cuda")
    for k in range(3):
        G = torch.from_numpy(c.grads[k].copy()).cuda()
        lr.fill_(LR.LR[k])
        if clip:
            C.clip_norm(G, part, out, cn, cv)
        C.sgd_momentum(W, G, V, lr, LR.MOM, nesterov, gscale=out if clip else None, clipvalue=cv)
    torch.cuda.synchronize()
    assert (_bits(got["w"])[c.mask] == _bits(W.cpu().numpy())[c.mask]).all()
    assert (_bits(got["momentum"])[c.mask] == _bits(V.cpu().numpy())[c.mask]).all()


# ------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("kind,nesterov", [("lars", True), ("lamb", False)], ids=["lars", "lamb"])
def test_bits_do_not_depend_on_run_or_address(kind, nesterov):
    a, la = _run(kind, nesterov, "both")
    b, lb = _run(kind, nesterov, "both")
    d, ld = _run(kind, nesterov, "both", pad=8)  # the same data at another buffer offset
    for other, lo in ((b, lb), (d, ld)):
        for name in a:
            assert (_bits(a[name])[_case().mask] == _bits(other[name])[_case().mask]).all(), name
        for k in range(3):
            for word in ("partials", "ratio", "norms"):
                assert (_bits(la[k][word]) == _bits(lo[k][word])).all(), f"step {k}: {word}"


# ------------------------------------------------------------------------------------- non-finite values
def _nan_positions():
    c = _case()
    o, s = c.offsets[7], c.sizes[7]
    return {"first": o, "middle": o + c.CH + 7, "last": o + s - 1}


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_nan_gradient_stays_in_its_variable_and_elements(kind, where):
    c = _case()
    p = _nan_positions()[where]
    g = c.grads[0].copy()
    g[p] = np.nan
    clean, lc = _run(kind, False, "none", steps=1)
    got, lg = _run(kind, False, "none", steps=1, grads=[g])
    s = lg[0]
    assert np.isnan(s["norms"][7, 1]) and not np.isnan(s["norms"][7, 0])
    assert _bits(s["ratio"])[7] == _bits(np.float32(1.0)), "a comparison with a NaN norm is false: ratio 1"
    ref, _, _ = LR.run_ref(c, kind, False, "none", [None], grads=[g], steps=1)
    E, _ = _conditions(kind, False, "none")
    inside = np.zeros(c.total, dtype=bool)
    inside[c.offsets[7]:c.offsets[7] + c.sizes[7]] = True
    for name, r in ref.items():
        assert (np.isnan(got[name]) == np.isnan(r))[c.mask].all(), f"{name}: NaN where the f64 reference has none"
        assert np.isnan(got[name][p]) and np.isnan(got[name][c.mask]).sum() == 1, name
        ok = inside & ~np.isnan(r)
        assert (np.abs(got[name].astype(np.float64) - r)[ok] <= (4.0 * E[name] + R.ulp32(r))[ok]).all(), name
        rest = c.mask & ~inside
        assert (_bits(got[name])[rest] == _bits(clean[name])[rest]).all(), f"{name}: another variable changed"
    others = np.arange(c.V) != 7
    assert (_bits(s["ratio"])[others] == _bits(lc[0]["ratio"])[others]).all()
    assert (_bits(s["norms"])[others] == _bits(lc[0]["norms"])[others]).all()


# ------------------------------------------------------------------------------------- capture
@pytest.mark.parametrize("kind,nesterov", [("lamb", False), ("lars", True)], ids=["lamb", "lars-nesterov"])
def test_captured_step_replays_like_eager(kind, nesterov):
    def run(replay):
        r = _Run(kind, nesterov, "both")
        graph = None
        if replay:
            graph = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=s):
                r.launch()
            torch.cuda.synchronize()
            # (the capture itself runs nothing: the operands still hold the initial state)
        words = []
        for k in range(3):
            r.set_step(k)
            if replay:
                graph.replay()
            else:
                r.launch()
            torch.cuda.synchronize()
            words.append(r.words.snapshot())
        r.check_untouched("capture")
        return r.state(), words

    eager, ew = run(False)
    replayed, rw = run(True)
    for k in range(3):
        for word in ("partials", "ratio", "norms"):
            assert (_bits(ew[k][word]) == _bits(rw[k][word])).all(), f"step {k}: {word}"
    assert len({tuple(_bits(w["ratio"])) for w in ew}) == 3, "the three steps must see three different ratio sets"
    for name in eager:
        assert (_bits(eager[name])[_case().mask] == _bits(replayed[name])[_case().mask]).all(), name


# ------------------------------------------------------------------------------------- bindings
def test_layer_tables_validates_the_layout():
    C = _C()
    CH = int(C.LAYER_CHUNK)
    T = C.layer_tables([0, 64], [10, CH + 1], 64 + CH + 64, [0.0, 0.5], [True, False])
    assert (T.V, T.C, T.n) == (2, 3, 64 + CH + 64)
    assert T.chunks.cpu().tolist() == [[0, 10, 0, 0], [64, CH, 1, 0], [64 + CH, 1, 1, 0]]
    assert T.first_chunk.cpu().tolist() == [0, 1, 3]
    assert T.wd.cpu().tolist() == [0.0, 0.5] and T.adapt.cpu().tolist() == [1, 0]
    assert T.chunks.dtype == torch.int32 and T.chunks.is_cuda
    with pytest.raises(RuntimeError, match="multiple of 4"):
        C.layer_tables([0, 66], [10, 10], 128, [0.0, 0.0], [True, True])
    with pytest.raises(RuntimeError, match="overlaps"):
        C.layer_tables([0, 8], [10, 10], 128, [0.0, 0.0], [True, True])
    with pytest.raises(RuntimeError, match="past the slab"):
        C.layer_tables([0, 64], [10, 65], 128, [0.0, 0.0], [True, True])
    with pytest.raises(RuntimeError, match="not sorted"):
        C.layer_tables([64, 0], [10, 10], 128, [0.0, 0.0], [True, True])
    with pytest.raises(RuntimeError, match="one entry per variable"):
        C.layer_tables([0, 64], [10, 10], 128, [0.0], [True, True])
    with pytest.raises(RuntimeError, match="offset"):
        C.layer_tables([0], [0], 128, [0.0], [True])


def test_launchers_reject_misaligned_short_and_foreign_operands():
    C = _C()
    n = 256
    T = C.layer_tables([0, 64], [10, 100], n, [0.0, 0.0], [True, True])
    other = C.layer_tables([0, 64], [10, 100], n + 64, [0.0, 0.0], [True, True])

    def f32buf(k):
        return torch.zeros(k + 8, dtype=torch.float32, device="cuda")

    w, g, v = (f32buf(n)[4:4 + n] for _ in range(3))
    part = torch.zeros(8, dtype=torch.float64, device="cuda")
    ratio, norms = f32buf(2)[4:6], f32buf(4)[4:8]
    lr = torch.full((1,), 0.1, device="cuda")
    C.lars_sums(T, w, g, part[:4])  # (the well-formed calls)
    C.lars_ratio(T, part[:4], ratio, norms, 0.001, 0.0)
    C.lars_update(T, w, g, v, ratio, lr, 0.9, False)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        C.lars_sums(T, f32buf(n)[1:1 + n], g, part[:4])
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        C.lars_sums(T, w, g, part[1:5])
    with pytest.raises(RuntimeError, match="too short"):
        C.lars_sums(T, w, f32buf(n)[4:4 + n - 4], part[:4])
    with pytest.raises(RuntimeError, match="partials too small"):
        C.lars_sums(T, w, g, part[:2])
    with pytest.raises(RuntimeError, match="float64"):
        C.lars_sums(T, w, g, f32buf(8)[4:8])
    with pytest.raises(RuntimeError, match="built for n"):
        C.lars_sums(T, f32buf(n + 64)[4:4 + n + 64], f32buf(n + 64)[4:4 + n + 64], part[:4])
    with pytest.raises(RuntimeError, match="too short"):
        C.lars_sums(other, w, g, part[:4])
    with pytest.raises(RuntimeError, match="built for n"):
        C.lars_update(T, f32buf(n + 64)[4:4 + n + 64], g, v, ratio, lr, 0.9, False)
    with pytest.raises(RuntimeError, match="ratio too small"):
        C.lars_ratio(T, part[:4], ratio[:1], norms, 0.001, 0.0)
    with pytest.raises(RuntimeError, match="norms too small"):
        C.lamb_ratio(T, part[:4], ratio, norms[:2])
    with pytest.raises(RuntimeError, match="too short"):
        C.lamb_update(T, w, g, f32buf(n)[4:4 + n - 4], ratio, lr, torch.zeros(1, device="cuda"), 0, 0.9, 0.999, 1e-6)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        C.lamb_sums(T, w, g, v, f32buf(n)[2:2 + n], part[:4], torch.zeros(1, device="cuda"), 0, 0.9, 0.999, 1e-6)
    with pytest.raises(TypeError):
        C.lars_sums((T.chunks, T.first_chunk), w, g, part[:4])  # nothing but a LayerTables object is accepted
    torch.cuda.synchronize()


def test_empty_layout_launches_nothing():
    C = _C()
    T = C.layer_tables([], [], 64, [], [])
    assert (T.V, T.C, T.n) == (0, 0, 64)
    bufs = [torch.full((64 + 8,), SENT_BITS, dtype=torch.int32, device="cuda").view(torch.float32) for _ in range(4)]
    w, g, m, v = (b[4:68] for b in bufs)
    part = torch.full((4,), SENT64, dtype=torch.int64, device="cuda").view(torch.float64)
    words = torch.full((8,), SENT_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    lr, t0 = torch.ones(1, device="cuda"), torch.zeros(1, device="cuda")
    C.lars_sums(T, w, g, part)
    C.lars_ratio(T, part, words[:0], words[4:4], 0.001, 0.0)
    C.lars_update(T, w, g, v, words[:0], lr, 0.9, True)
    C.lamb_sums(T, w, g, m, v, part, t0, 0, 0.9, 0.999, 1e-6)
    C.lamb_ratio(T, part, words[:0], words[4:4])
    C.lamb_update(T, w, m, v, words[:0], lr, t0, 0, 0.9, 0.999, 1e-6)
    torch.cuda.synchronize()  # (an empty grid would leave a launch error behind for the next call to find)
    assert (torch.ones(4, device="cuda") + 1).sum().item() == 8.0
    for b in bufs:
        assert (b.view(torch.int32) == SENT_BITS).all()
    assert (part.view(torch.int64) == SENT64).all() and (words.view(torch.int32) == SENT_BITS).all()
