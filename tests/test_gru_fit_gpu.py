"""Training through keras.layers.GRU on the GPU.  The model: Embedding -> GRU(32, return_sequences) -> GRU(16) ->
Dense, T = 12, 6 SGD steps."""
import os
import subprocess
import sys
from unittest import mock

import numpy as np
import pytest
import torch

import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.ops import gru as GS
from test_lstm_fit_gpu import BATCH, CLASSES, DIM, LR, STEPS, VOCAB, T, _data, _distance  # the LSTM fit's data and sizes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fit(env=None, policy="float32"):
    """(initial weights, final weights, model) of the fit; eager unless the caller asks for the graph."""
    L = tdl.keras.layers
    with mock.patch.dict(os.environ, dict({"TDL_DISABLE_FUSED": "1", "TDL_GRAPH_STEP": "0"}, **(env or {}))):
        tdl.keras.backend.clear_session()
        tdl.keras.utils.set_random_seed(3)
        tdl.keras.mixed_precision.set_global_policy(policy)
        try:
            with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
                m = tdl.keras.Sequential([L.Input((T,)), L.Embedding(VOCAB, DIM, name="emb"),
                                          L.GRU(32, return_sequences=True, name="gru1"), L.GRU(16, name="gru2"),
                                          L.Dense(CLASSES, name="head")])
                m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                          optimizer=tdl.keras.optimizers.SGD(learning_rate=LR))
            w0 = [np.array(w, np.float64) for w in m.get_weights()]
            hist = m.fit(tdl.data.Dataset.from_tensor_slices(_data()).batch(BATCH).repeat(), epochs=1,
                         steps_per_epoch=STEPS, verbose=0)
            assert m._trainer.kind == "generic" and np.isfinite(hist.history["loss"]).all()
            return w0, [np.array(w, np.float64) for w in m.get_weights()], m
        finally:
            tdl.keras.mixed_precision.set_global_policy("float32")


def _fit_f64(w0):
    """The same SGD steps in float64 on the CPU with the torch formulas; weights in the model's order:
    emb, (kernel, recurrent_kernel, bias [2, 3U]) of each GRU, head kernel / bias."""
    w = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in w0]
    x, y = _data()
    for s in range(STEPS):
        xb, yb = x[s * BATCH:(s + 1) * BATCH].long(), y[s * BATCH:(s + 1) * BATCH].long()
        h1 = GS.gru_torch(w[0][xb] @ w[1] + w[3][0], w[2], w[3][1])[0]
        h2 = GS.gru_torch(h1 @ w[4] + w[6][0], w[5], w[6][1])[1]
        loss = torch.nn.functional.cross_entropy(h2 @ w[7] + w[8], yb)
        w = [(p - LR * g).detach().requires_grad_() for p, g in zip(w, torch.autograd.grad(loss, w))]
    return [p.detach().numpy() for p in w]


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
def test_fit_runs_on_the_kernels_and_stays_as_close_to_f64_as_the_torch_formula(policy):
    before, fb, by = GS.CALLS[0], GS.FALLBACKS[0], dict(GS.CALLS_BY_DTYPE)
    w0, wk, m = _fit(policy=policy)
    assert [a.shape for a in w0[1:4]] == [(DIM, 96), (32, 96), (2, 96)] and len(w0) == 9
    assert GS.CALLS[0] >= before + 2 * STEPS and GS.FALLBACKS[0] == fb, "a fallback ran"
    used = torch.bfloat16 if policy == "mixed_bfloat16" else torch.float32
    assert GS.CALLS_BY_DTYPE[used] > by[used]
    assert not any(np.array_equal(a, b) for a, b in zip(wk, w0))  # every weight moved,
    for i in (3, 6):  # both bias rows of both layers included
        assert not np.array_equal(wk[i][0], w0[i][0]) and not np.array_equal(wk[i][1], w0[i][1])
    before = GS.CALLS[0]
    w0t, wt, _ = _fit(policy=policy, env={"TDL_GRU": "torch"})
    assert GS.CALLS[0] == before and all(np.array_equal(a, b) for a, b in zip(w0, w0t))
    ref = _fit_f64(w0)
    dk, dt = _distance(wk, ref), _distance(wt, ref)
    print(f"\n[gru fit {policy}] distance to the f64 fit: kernels {dk:.3g}, torch formula {dt:.3g}; "
          f"moved {_distance(ref, w0):.3g}")
    assert _distance(ref, w0) > 1e-3 and dk <= 4 * dt


def _graph_fits():
    # in a process of its own, as tests/test_lstm_fit_gpu.py has it
    for policy in ("float32", "mixed_bfloat16"):
        before, fb = GS.CALLS[0], GS.FALLBACKS[0]
        _, wg, g = _fit(policy=policy, env={"TDL_GRAPH_STEP": "1"})
        _, we, e = _fit(policy=policy)
        assert len(g._trainer._graphs) >= 1 and len(e._trainer._graphs) == 0, policy
        assert GS.CALLS[0] > before and GS.FALLBACKS[0] == fb, policy
        assert all(np.array_equal(x, y) for x, y in zip(wg, we)), policy


def test_the_step_replays_in_a_captured_graph_and_equals_the_eager_fit():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "capture failed" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]


if __name__ == "__main__":
    _graph_fits()
