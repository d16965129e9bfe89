"""The fit of tests/test_attention_fit_gpu.py with MultiHeadAttention(2, 16, dropout=0.25): on the DROP kernels, one
ticket per step, at most 4 x as far from the float64 formula fit drawing the same masks as the ``TDL_ATTENTION=torch``
fit is, and bit-exact in a replayed graph."""
import functools
import os
import subprocess
import sys
from unittest import mock

import numpy as np
import pytest
import torch

import attention_dropout_refs as DR
import attention_refs as AR
import tensorflow_distributed_learning_amd as tdl
import test_attention_fit_gpu as F0
from tensorflow_distributed_learning_amd.ops import attention as A, dropout as DO

pytestmark = pytest.mark.gpu
RATE, STEPS, BATCH = 0.25, F0.STEPS, F0.BATCH


def _fit(**kw):
    """F0._fit with the layer's dropout set; (w0, w, the layer): global seed 3, stream = the layer's creation index."""
    with mock.patch.object(tdl.keras.layers, "MultiHeadAttention", functools.partial(tdl.keras.layers.MultiHeadAttention, dropout=RATE)):
        w0, w, m = F0._fit(**kw)
    assert m.get_layer("mha").rng_calls("cuda:0") == STEPS
    return w0, w, m


def _fit_f64(w0, key):
    """F0._fit_f64 with the mask of (key, ticket = step) on the probabilities, in float64."""
    w, (x, y), c = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in w0], F0._data(), DO.keep_scale(RATE)
    for s in range(STEPS):
        xb, yb = x[s * BATCH:(s + 1) * BATCH].long(), y[s * BATCH:(s + 1) * BATCH].long()
        cz, e = c * torch.from_numpy(DR.keep_mask(key, s, RATE, BATCH, 2, F0.T, F0.T)).double(), w[0][xb]
        a = AR.layer(w[1:9], e, e, e, lambda q, k, v: A.sdpa_torch(q, k, v, None, True, dropout=lambda p: p * cz), torch.einsum)
        loss = torch.nn.functional.cross_entropy((e + a).flatten(1) @ w[9] + w[10], yb)
        w = [(p - F0.LR * g).detach().requires_grad_() for p, g in zip(w, torch.autograd.grad(loss, w))]
    return [p.detach().numpy() for p in w]


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
def test_dropout_fit_runs_on_the_kernels_and_stays_as_close_to_f64_as_the_torch_formula(policy):
    before = dict(A.CALLS)
    w0, wk, m = _fit(policy=policy)
    assert A.CALLS["forward"] >= before["forward"] + STEPS and A.CALLS["backward"] >= before["backward"] + STEPS
    assert A.CALLS["torch"] == before["torch"], "a fallback ran"
    w0t, wt, _ = _fit(policy=policy, env={"TDL_ATTENTION": "torch"})
    ref = _fit_f64(w0, DO.stream_key(3, m.get_layer("mha")._rng_stream, 0))
    dk, dt, moved = F0._distance(wk, ref), F0._distance(wt, ref), F0._distance(ref, w0)
    print(f"\n[attention dropout fit {policy}] distance to the f64 fit: kernels {dk:.3g}, torch formula {dt:.3g}; moved {moved:.3g}")
    assert all(np.array_equal(a, b) for a, b in zip(w0, w0t)) and moved > 1e-3 and dk <= 4 * dt


def test_the_dropout_step_replays_in_a_captured_graph_and_equals_the_eager_fit():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, PYTHONPATH=F0.ROOT),
                       capture_output=True, text=True, timeout=300, cwd=F0.ROOT)
    assert r.returncode == 0 and "capture failed" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]


if __name__ == "__main__":  # in a process of its own, as F0 has it
    for policy in ("float32", "mixed_bfloat16"):
        before = dict(A.CALLS)
        (_, wg, g), (_, we, e) = _fit(policy=policy, env={"TDL_GRAPH_STEP": "1"}), _fit(policy=policy)
        assert len(g._trainer._graphs) >= 1 and len(e._trainer._graphs) == 0, policy
        assert A.CALLS["forward"] > before["forward"] and A.CALLS["torch"] == before["torch"], policy
        assert all(np.array_equal(x, y) for x, y in zip(wg, we)), policy
