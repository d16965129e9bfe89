"""The W3 stream of the fused MNIST forward (k_fwd_conv: each thread pulls 25 16-byte pieces of its quarter of
W3 into registers while conv1 and conv2 run): which W3 element lands in which w3v[j] of which thread.

Thread (row group rg, columns n4 .. n4+3) of quarter cq must hold in w3v[j] the W3 row of feature
64 j + 16 cq + rg (pool-2 window j, channel 16 cq + rg), columns n4 .. n4+3.  The loads are issued in small
groups between the conv MFMAs, on different paths for the waves with and without conv tiles; a reschedule
that moves a load to another group can give it the wrong j.  The other exact tests use a random W3 in
{-1, 0, 1} with 75 % zeros: two of its rows agree in most columns, so a swapped pair moves few outputs.

Here every W3 row carries a code.  For column group m = n // 4 (the four columns one thread holds) the four
entries w3[r, 4m .. 4m+3] are the balanced base-7 digits (-3 .. 3) of (r + 53 m) mod 2401: pairwise different
over the 1600 rows within EVERY column group, i.e. in every thread's view.  Everything else is
mnist_refs.Coded (integer pixels, weights and biases, power-of-two lr and loss scale, saturated softmax), with
the images selected again for a logit gap >= 128 under this W3, so every sum of the step is exact in f32 and
the kernels' outputs must EQUAL the f64 reference.

Asserted on the host for every case, before any comparison:

* every sum stays below 2^24 and the other conditions of mnist_refs.Coded.check hold;
* the W3 rows are pairwise different in every column group;
* swapping two rows r, s of one quarter changes that quarter's dense1 partial by (P2[i, r] - P2[i, s]) *
  (w3[s, n] - w3[r, n]) in image i, column n: it changes whenever some image of the batch has
  P2[i, r] != P2[i, s].  Two features that agree in every image of the batch (e.g. both closed by the ReLU:
  about 40 % of P2 is 0) cannot be told apart by anything the step stores -- dP2 is masked by P2 > 0 as well
  and dW3 = P2^T dH -- and a single image cannot make 400 features pairwise different.  So "any two rows of
  one quarter" is asserted literally at the full batch b = 64 (whose images are drawn so that it holds), and
  at the smaller batches in the form their few images can meet: in every quarter EVERY pair of windows
  (j, j'), i.e. every pair of w3v indices a thread can confuse, is told apart by some row group and image
  (b >= 1: a swap made on all waves shows in the partial), from b = 17 on also within the two row groups of
  every single wave (a swap confined to one wave shows).  The share of row pairs told apart is printed
  (0.91 - 0.97 at b = 1, 1.0 at b = 64).

Compared bit for bit with the f64 reference: the four quarter partials (part3 after forward_features, head
mode 0), the logits of forward_eval (head mode 2), and after one fused training step (head mode 1, dP2 in
the forward) dH, the per-image part2 rows (through dP2 they see W3 again) and W after the SGD update.
b = 1, 2, 17: the plain block map; 8: the smallest batch with the XCD map; 64: the full batch.  One more
case runs three consecutive SGD steps twice at b = 17 and compares the two runs bit for bit."""
import copy

import numpy as np
import pytest
import torch

import f32_edge_helpers as FE
import mnist_refs as MR
import test_mnist_exact_gpu as TE
from tensorflow_distributed_learning_amd.models import mnist_cnn as M

pytestmark = pytest.mark.gpu

BATCHES = [1, 2, 8, 17, 64]
FULL = 64


def w3_codes():
    """[1600, 128]: w3[r, 4m + t] = digit t (balanced base 7) of (r + 53 m) mod 2401."""
    r = np.arange(1600)[:, None]
    m = np.arange(32)[None, :]
    code = (r + 53 * m) % 2401  # (injective in r for a fixed m: 1600 < 2401)
    w3 = np.empty((1600, 32, 4), np.float64)
    for t in range(4):
        w3[:, :, t] = (code // 7 ** t) % 7 - 3
    return w3.reshape(1600, 128)


def _told_apart(P2q):
    """[400, 400] bool: some image of the batch has P2[i, r] != P2[i, s]."""
    return (P2q[:, :, None] != P2q[:, None, :]).any(0)


class W3Coded:
    """mnist_refs.Coded(b) with the coded W3: the images (3 chunks of b) selected and labelled again by
    Coded's rules under this W3, the f64 reference of each chunk, and the host-side conditions."""

    def __init__(self, b):
        base = MR.coded(b)
        rng = np.random.RandomState(77 + b)
        c = copy.copy(base)
        c.params = list(base.params)
        c.params[4] = w3_codes()
        # |w3| is about 1.7 on average instead of 0.25: w4 = +-1 keeps the logits' sums below 2^24
        c.params[6] = np.sign(base.params[6])
        w1, b1, w2, b2, w3, b3, w4, b4 = c.params
        _, P1, _, _, _ = MR.conv1_pool(base.X, w1, b1)
        _, P2, _, _, _ = MR.conv2_pool(P1, w2, b2)
        H, _ = MR.dense1(P2, w3, b3)
        lg, _ = MR.dense2(H, w4, b4)
        top2 = np.sort(lg, 1)[:, -2:]
        ok = np.flatnonzero(top2[:, 1] - top2[:, 0] >= 128)
        n = len(base.X)
        assert ok.size >= 3 * b, f"b={b}: only {ok.size} of {n} images have a logit gap >= 128"
        # the full batch: the first of eight draws whose chunk 1 tells ANY two rows of each quarter apart
        q = MR.quarter_of_feature(np.arange(1600))
        for draw in range(8):
            c.idx = ok[rng.permutation(ok.size)[:3 * b]].astype(np.int32)
            if b < FULL or all(_told_apart(P2[c.idx[b:2 * b]][:, q == cq])[~np.eye(400, dtype=bool)].all()
                               for cq in range(4)):
                break
        pred = lg.argmax(1)
        Y = (pred + rng.randint(1, 10, n)) % 10
        hit = c.idx[np.arange(3 * b) % 4 == 3]
        Y[hit] = pred[hit]
        c.Y = Y.astype(np.int32)
        self.c, self.b = c, b
        self._ref = {}

    def ref(self, k):
        if k not in self._ref:
            S, AB = self.c.ref(k)
            self.c.check(S, AB)  # every sum below 2^24, saturated softmax, both kinds of label, pool ties
            self._host_conditions(S, AB, k)
            self._ref[k] = (S, AB)
        return self._ref[k]

    def _host_conditions(self, S, AB, k):
        b, w3 = self.b, self.c.params[4]
        assert float(AB.part3.max()) < 2.0 ** 24 and float(AB.dP2.max()) / self.c.scale < 2.0 ** 24
        for m in range(32):
            assert len(np.unique(w3[:, 4 * m:4 * m + 4], axis=0)) == 1600, f"column group {m}: two rows share a code"
        q = MR.quarter_of_feature(np.arange(1600))
        shares = []
        for cq in range(4):
            f = np.flatnonzero(q == cq)  # ascending: position p -> window p // 16, channel 16 cq + p % 16
            assert np.array_equal(f, 64 * (np.arange(400) // 16) + 16 * cq + np.arange(400) % 16)
            P2q, w3q = S.P2[:, f], w3[f]
            T = _told_apart(P2q)
            shares.append(float(T[~np.eye(400, dtype=bool)].mean()))
            # a told-apart pair does change the partial, in every column group (spot check of the algebra on
            # the pairs of one row group)
            Tw = T.reshape(25, 16, 25, 16)
            ch = np.stack([Tw[:, r, :, r] for r in range(16)])  # [row group][window j][window j']
            eye = np.eye(25, dtype=bool)
            bad = np.argwhere(~(ch.any(0) | eye))
            assert len(bad) == 0, f"b={b} chunk {k} quarter {cq}: windows {bad[0].tolist()} carry the same P2 in " \
                                  f"every row group and image"
            if b >= 17:  # per wave: its two row groups
                for w in range(8):
                    bad = np.argwhere(~(ch[2 * w] | ch[2 * w + 1] | eye))
                    assert len(bad) == 0, f"b={b} chunk {k} quarter {cq} wave {w}: windows {bad[0].tolist()} carry " \
                                          f"the same P2 in both row groups in every image"
            if b >= FULL and k == 1:
                bad = np.argwhere(~(T | np.eye(400, dtype=bool)))
                assert len(bad) == 0, f"b={b} quarter {cq}: rows {f[bad[0]].tolist()} carry the same P2 in every image"
            r, s = np.argwhere(T)[:: max(1, int(T.sum()) // 64)].T  # 64 told-apart pairs, swapped for real
            for r1, s1 in zip(r, s):
                sw = w3q.copy()
                sw[[r1, s1]] = sw[[s1, r1]]
                d = (P2q @ sw != P2q @ w3q).reshape(b, 32, 4).any((0, 2))
                assert d.all(), f"quarter {cq}: swapping rows {r1}, {s1} leaves column groups {np.flatnonzero(~d)}"
        print(f"b={b} chunk {k}: share of row pairs told apart per quarter {['%.3f' % s for s in shares]}; "
              f"part3 abs sum {AB.part3.max():.0f}, logits abs sum {AB.logits.max():.0f}")


_cases = {}


def case(b):
    if b not in _cases:
        _cases[b] = W3Coded(b)
    return _cases[b]


def _step(cuda, monkeypatch, b):
    TE._env(monkeypatch, "fused")
    c = case(b).c
    layout = M.mnist_layout()
    W = layout.pack([torch.from_numpy(p).float() for p in c.params], device=cuda)
    G = torch.zeros_like(W)
    lr = torch.tensor([c.lr], device=cuda)
    X = torch.from_numpy(c.X).float().to(cuda)
    Y = torch.from_numpy(c.Y).to(cuda)
    step = M.FusedMnistTrainStep(X, Y, torch.from_numpy(c.idx).to(cuda), W, G, layout, b, 1, lr,
                                 global_batch=c.global_batch)
    TE._named_mode(cuda, step, "fused", b)
    return c, layout, W, G, step


@pytest.mark.parametrize("b", BATCHES)
def test_w3_lands_where_it_belongs(cuda, monkeypatch, b):
    c, layout, W, G, step = _step(cuda, monkeypatch, b)
    S, AB = case(b).ref(1)
    off = b  # chunk 1
    what = f"b={b}"
    W0 = W.clone()

    # ---- head mode 0: the four quarter partials
    TE._poison(step, ["part3", "P2"])
    step._impl.forward_features(off)
    torch.cuda.synchronize()
    V = TE._views(step, b)
    FE.same_bits(V["P2"], S.P2, what + " P2 (features)")
    FE.same_bits(V["part3"], S.part3, what + " part3 (features)")

    # ---- head mode 2: the logits
    step.metrics.zero_()
    logits = torch.full((b * 10,), float("nan"), device=cuda)
    step.forward_eval(off, logits)
    torch.cuda.synchronize()
    FE.same_bits(logits.view(b, 10), S.logits, what + " logits (eval)")
    TE._exact_metrics(step, S, b, what + " eval")

    # ---- head mode 1: one training step with the SGD update
    step.metrics.zero_()
    TE._poison(step, ["P2", "H", "dH", "part1", "part2"])
    step.forward_backward(off)
    step.finalize(True)
    torch.cuda.synchronize()
    step.check()
    V = TE._views(step, b)
    FE.same_bits(V["H"], S.H, what + " H")
    FE.same_bits(V["dH"], S.dH, what + " dH")
    p2 = MR.part2_rows(V["part2"], b, step.fused_bwd)
    assert np.array_equal(p2, S.part2), f"{what} part2: first at (image, row, column) {np.argwhere(p2 != S.part2)[0].tolist()}"
    TE._exact_metrics(step, S, b, what)
    assert not torch.equal(W, W0)
    for (name, _), got, p, g in zip(M.MNIST_CNN_VARIABLES, layout.views(W.cpu()), c.params, S.grads):
        FE.same_bits(got, p - c.lr * g, f"{what} W after SGD: {name}")


def _three_steps(step, W, G, b):
    out = []
    for k in (2, 0, 1):
        step.metrics.zero_()
        step.forward_backward(k * b)
        step.finalize(True)
        torch.cuda.synchronize()
        step.check()
        bufs = step.buffers()
        st = {n: bufs[n].cpu().clone() for n in ("P2", "H", "dH", "dL", "part1", "part2")}
        st["W"] = W.cpu().clone()  # (not the metrics: the loss is summed by atomic adds in arrival order)
        out.append(st)
    return out


def test_w3_three_steps_repeat(cuda, monkeypatch):  # noqa: F811
    """Three consecutive SGD steps at b = 17 (the weights change from step to step, so the sums round and
    depend on every operand), twice from the same W0: the second run equals the first bit for bit."""
    b = 17
    c, layout, W, G, step = _step(cuda, monkeypatch, b)
    W0 = W.clone()
    first = _three_steps(step, W, G, b)
    assert not torch.equal(first[0]["W"], W0.cpu()) and not torch.equal(first[1]["W"], first[0]["W"])
    W.copy_(W0)
    second = _three_steps(step, W, G, b)
    for n, (s0, s1) in enumerate(zip(first, second)):
        for name in s0:
            assert torch.equal(s0[name].view(torch.uint8).view(-1), s1[name].view(torch.uint8).view(-1)), \
                f"step {n}: {name} differs between the two runs"
