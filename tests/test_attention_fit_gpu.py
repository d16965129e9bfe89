"""Training through keras.layers.MultiHeadAttention on the GPU: the kernel fit against the same fit in float64 with the
torch formula (at most 4 x as far from it as the ``TDL_ATTENTION=torch`` fit), and its bit-exact graph replay."""
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
from tensorflow_distributed_learning_amd.ops import conv as CONV

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, VOCAB, DIM, CLASSES, BATCH, STEPS, LR = 24, 50, 16, 5, 8, 6, 0.05


def _data():
    g = torch.Generator().manual_seed(0)
    return (torch.randint(0, VOCAB, (STEPS * BATCH, T), generator=g, dtype=torch.int32),
            torch.randint(0, CLASSES, (STEPS * BATCH,), generator=g, dtype=torch.int32))


def _fit(env=None, policy="float32"):
    """(initial weights, final weights, model) of the 6-step fit; eager unless the caller asks for the graph."""
    L = tdl.keras.layers
    with mock.patch.dict(os.environ, dict({"TDL_DISABLE_FUSED": "1", "TDL_GRAPH_STEP": "0"}, **(env or {}))):
        tdl.keras.backend.clear_session()
        tdl.keras.utils.set_random_seed(3)
        tdl.keras.mixed_precision.set_global_policy(policy)
        try:
            with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
                inp = L.Input((T,))
                e = L.Embedding(VOCAB, DIM, name="emb")(inp)
                a = L.MultiHeadAttention(2, 16, name="mha")(e, e, use_causal_mask=True)
                m = tdl.keras.Model(inp, L.Dense(CLASSES, name="head")(L.Flatten()(L.Add()([e, a]))))
                m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                          optimizer=tdl.keras.optimizers.SGD(learning_rate=LR))
            w0 = [np.array(w, np.float64) for w in m.get_weights()]
            h = m.fit(tdl.data.Dataset.from_tensor_slices(_data()).batch(BATCH).repeat(), epochs=1,
                      steps_per_epoch=STEPS, verbose=0)
            assert m._trainer.kind == "generic" and np.isfinite(h.history["loss"]).all()
            return w0, [np.array(w, np.float64) for w in m.get_weights()], m
        finally:
            tdl.keras.mixed_precision.set_global_policy("float32")


def _fit_f64(w0):
    """The same 6 SGD steps in float64 on the CPU with the torch formula; weights in the model's order."""
    w = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in w0]
    x, y = _data()
    for s in range(STEPS):
        xb, yb = x[s * BATCH:(s + 1) * BATCH].long(), y[s * BATCH:(s + 1) * BATCH].long()
        e = w[0][xb]
        a = AR.layer(w[1:9], e, e, e, lambda q, k, v: A.sdpa_torch(q, k, v, None, True), torch.einsum)
        loss = torch.nn.functional.cross_entropy((e + a).flatten(1) @ w[9] + w[10], yb)
        grads = torch.autograd.grad(loss, w)
        w = [(p - LR * g).detach().requires_grad_() for p, g in zip(w, grads)]
    return [p.detach().numpy() for p in w]


def _distance(a, b):
    return max(float(np.abs(x - y).max()) for x, y in zip(a, b))


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
def test_fit_runs_on_the_kernels_and_stays_as_close_to_f64_as_the_torch_formula(policy):
    before, lib0 = dict(A.CALLS), len(CONV.library_calls())
    w0, wk, m = _fit(policy=policy)
    assert A.CALLS["forward"] >= before["forward"] + STEPS and A.CALLS["backward"] >= before["backward"] + STEPS
    assert A.CALLS["torch"] == before["torch"] and len(CONV.library_calls()) == lib0, "a fallback ran"
    before = dict(A.CALLS)
    w0t, wt, _ = _fit(policy=policy, env={"TDL_ATTENTION": "torch"})
    assert A.CALLS["forward"] == before["forward"] and A.CALLS["torch"] > before["torch"]
    assert all(np.array_equal(a, b) for a, b in zip(w0, w0t))
    ref = _fit_f64(w0)
    dk, dt = _distance(wk, ref), _distance(wt, ref)
    print(f"\n[attention fit {policy}] distance to the f64 fit: kernels {dk:.3g}, torch formula {dt:.3g}; "
          f"moved {_distance(ref, w0):.3g}")
    assert _distance(ref, w0) > 1e-3 and dk <= 4 * dt


def _graph_fits():
    # in a process of its own, as tests/test_conv_transpose_fit_gpu.py has it
    for policy in ("float32", "mixed_bfloat16"):
        before = dict(A.CALLS)
        _, wg, g = _fit(policy=policy, env={"TDL_GRAPH_STEP": "1"})
        _, we, e = _fit(policy=policy)
        assert len(g._trainer._graphs) >= 1 and len(e._trainer._graphs) == 0, policy
        assert A.CALLS["forward"] > before["forward"] and A.CALLS["torch"] == before["torch"], policy
        assert all(np.array_equal(x, y) for x, y in zip(wg, we)), policy


def test_the_step_replays_in_a_captured_graph_and_equals_the_eager_fit():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "capture failed" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]


if __name__ == "__main__":
    _graph_fits()
