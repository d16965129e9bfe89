"""Training through keras.layers.LayerNormalization on the GPU.  The model: Embedding -> LN -> MultiHeadAttention
(causal) -> Add -> LN (rms_scaling) -> Flatten -> Dense, T = 24, dim 16, 6 SGD steps."""
import os
import subprocess
import sys
from unittest import mock

import numpy as np
import pytest
import torch

import attention_refs as AR
import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.ops import attention as A
from tensorflow_distributed_learning_amd.ops import layernorm as LN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, VOCAB, DIM, CLASSES, BATCH, STEPS, LR, EPS = 24, 50, 16, 5, 8, 6, 0.05, 1e-3


def _data():
    g = torch.Generator().manual_seed(0)
    return (torch.randint(0, VOCAB, (STEPS * BATCH, T), generator=g, dtype=torch.int32),
            torch.randint(0, CLASSES, (STEPS * BATCH,), generator=g, dtype=torch.int32))


def _fit(env=None, policy="float32", steps=STEPS):
    """(initial weights, final weights, model) of the fit; eager unless the caller asks for the graph."""
    L = tdl.keras.layers
    with mock.patch.dict(os.environ, dict({"TDL_DISABLE_FUSED": "1", "TDL_GRAPH_STEP": "0"}, **(env or {}))):
        tdl.keras.backend.clear_session()
        tdl.keras.utils.set_random_seed(3)
        tdl.keras.mixed_precision.set_global_policy(policy)
        try:
            with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
                inp = L.Input((T,))
                e = L.Embedding(VOCAB, DIM, name="emb")(inp)
                h = L.LayerNormalization(name="ln1")(e)
                a = L.MultiHeadAttention(2, 16, name="mha")(h, h, use_causal_mask=True)
                n = L.LayerNormalization(rms_scaling=True, name="ln2")(L.Add()([e, a]))
                m = tdl.keras.Model(inp, L.Dense(CLASSES, name="head")(L.Flatten()(n)))
                m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                          optimizer=tdl.keras.optimizers.SGD(learning_rate=LR))
            w0 = [np.array(w, np.float64) for w in m.get_weights()]
            hist = m.fit(tdl.data.Dataset.from_tensor_slices(_data()).batch(BATCH).repeat(), epochs=1,
                         steps_per_epoch=steps, verbose=0)
            assert m._trainer.kind == "generic" and np.isfinite(hist.history["loss"]).all()
            return w0, [np.array(w, np.float64) for w in m.get_weights()], m
        finally:
            tdl.keras.mixed_precision.set_global_policy("float32")


def _fit_f64(w0):
    """The same SGD steps in float64 on the CPU with the torch formulas; weights in the model's order:
    emb, ln1 gamma / beta, the 8 attention weights, ln2 gamma, head kernel / bias."""
    w = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in w0]
    x, y = _data()
    for s in range(STEPS):
        xb, yb = x[s * BATCH:(s + 1) * BATCH].long(), y[s * BATCH:(s + 1) * BATCH].long()
        e = w[0][xb]
        h = LN.layer_norm_torch(e, w[1], w[2], EPS)
        a = AR.layer(w[3:11], h, h, h, lambda q, k, v: A.sdpa_torch(q, k, v, None, True), torch.einsum)
        n = LN.layer_norm_torch(e + a, w[11], None, EPS, rms=True)
        loss = torch.nn.functional.cross_entropy(n.flatten(1) @ w[12] + w[13], yb)
        w = [(p - LR * g).detach().requires_grad_() for p, g in zip(w, torch.autograd.grad(loss, w))]
    return [p.detach().numpy() for p in w]


def _distance(a, b):
    return max(float(np.abs(x - y).max()) for x, y in zip(a, b))


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
def test_fit_runs_on_the_kernels_and_stays_as_close_to_f64_as_the_torch_formula(policy, monkeypatch):
    Lc, seen = tdl.keras.layers.LayerNormalization, []
    orig = Lc._grad_targets
    monkeypatch.setattr(Lc, "_grad_targets", lambda self: seen.append((self.name, orig(self))) or seen[-1][1])
    before, fb, by = LN.CALLS[0], LN.FALLBACKS[0], dict(LN.CALLS_BY_DTYPE)
    w0, wk, m = _fit(policy=policy)
    assert len(w0) == 14 and w0[11].shape == (DIM,) and w0[12].shape == (T * DIM, CLASSES)  # (ln2 has no beta)
    assert LN.CALLS[0] >= before + 2 * STEPS and LN.FALLBACKS[0] == fb, "a fallback ran"
    used = torch.bfloat16 if policy == "mixed_bfloat16" else torch.float32
    assert LN.CALLS_BY_DTYPE[used] > by[used]
    # gamma / beta gradients reach the slab through the direct targets, and the parameters move
    assert len(seen) >= 2 * STEPS and {n for n, _ in seen} == {"ln1", "ln2"}
    for name, t in seen:
        assert t is not None and t[0].dtype == torch.float32 and t[0].numel() == DIM and (t[1] is None) == (name == "ln2")
    assert not any(np.array_equal(wk[i], w0[i]) for i in (1, 2, 11))
    before = LN.CALLS[0]
    w0t, wt, _ = _fit(policy=policy, env={"TDL_LAYERNORM": "torch"})
    assert LN.CALLS[0] == before and all(np.array_equal(a, b) for a, b in zip(w0, w0t))
    ref = _fit_f64(w0)
    dk, dt = _distance(wk, ref), _distance(wt, ref)
    print(f"\n[layernorm fit {policy}] distance to the f64 fit: kernels {dk:.3g}, torch formula {dt:.3g}; "
          f"moved {_distance(ref, w0):.3g}")
    assert _distance(ref, w0) > 1e-3 and dk <= 4 * dt


def test_eager_step_launches_the_hand_written_kernels():
    from tensorflow_distributed_learning_amd.utils.kernel_audit import audit

    _, _, m = _fit(steps=1)  # warm-up (allocations, first-use set-up)
    ds = tdl.data.Dataset.from_tensor_slices(_data()).batch(BATCH).repeat()
    with mock.patch.dict(os.environ, {"TDL_DISABLE_FUSED": "1", "TDL_GRAPH_STEP": "0"}):
        rep = audit(lambda: m.fit(ds, epochs=1, steps_per_epoch=1, verbose=0))
    for kernel in ("k_ln_fwd", "k_ln_bwd", "k_ln_dgb"):
        assert sum(c for n, c in rep["tdl"].items() if kernel in n) == 2, dict(rep["tdl"])
    assert not [n for cat in rep.values() for n in cat if "layer_norm" in n.lower()]


def _graph_fits():
    # in a process of its own, as tests/test_attention_fit_gpu.py has it
    for policy in ("float32", "mixed_bfloat16"):
        before, fb = LN.CALLS[0], LN.FALLBACKS[0]
        _, wg, g = _fit(policy=policy, env={"TDL_GRAPH_STEP": "1"})
        _, we, e = _fit(policy=policy)
        assert len(g._trainer._graphs) >= 1 and len(e._trainer._graphs) == 0, policy
        assert LN.CALLS[0] > before and LN.FALLBACKS[0] == fb, policy
        assert all(np.array_equal(x, y) for x, y in zip(wg, we)), policy


def test_the_step_replays_in_a_captured_graph_and_equals_the_eager_fit():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "capture failed" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]


if __name__ == "__main__":
    _graph_fits()
