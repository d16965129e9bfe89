"""Training through keras.layers.Embedding on the GPU kernels: the model, data and sizes of test_lstm_fit_gpu.py
(Embedding -> LSTM(32, return_sequences) -> LSTM(16) -> Dense, T = 12, 6 SGD steps)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tensorflow_distributed_learning_amd.ops import embedding as EM
from test_lstm_fit_gpu import STEPS, _distance, _fit, _fit_f64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
def test_fit_runs_on_the_kernels_and_stays_as_close_to_f64_as_the_torch_formula(policy):
    before, fb, by = EM.CALLS[0], EM.FALLBACKS[0], dict(EM.CALLS_BY_DTYPE)
    w0, wk, m = _fit(policy=policy)
    assert EM.CALLS[0] >= before + STEPS and EM.FALLBACKS[0] == fb, "a fallback ran"
    used = torch.bfloat16 if policy == "mixed_bfloat16" else torch.float32
    assert EM.CALLS_BY_DTYPE[used] > by[used]
    assert not np.array_equal(wk[0], w0[0])  # the emb weight moved
    before = EM.CALLS[0]
    w0t, wt, _ = _fit(policy=policy, env={"TDL_EMBEDDING": "torch"})
    assert EM.CALLS[0] == before and all(np.array_equal(a, b) for a, b in zip(w0, w0t))
    ref = _fit_f64(w0)
    dk, dt = _distance(wk, ref), _distance(wt, ref)
    print(f"\n[embedding fit {policy}] distance to the f64 fit: kernels {dk:.3g}, torch formula {dt:.3g}; "
          f"moved {_distance(ref, w0):.3g}")
    assert _distance(ref, w0) > 1e-3 and dk <= 4 * dt


def _graph_fits():
    # in a process of its own, as tests/test_lstm_fit_gpu.py has it
    for policy in ("float32", "mixed_bfloat16"):
        before, fb = EM.CALLS[0], EM.FALLBACKS[0]
        _, wg, g = _fit(policy=policy, env={"TDL_GRAPH_STEP": "1"})
        _, we, e = _fit(policy=policy)
        assert len(g._trainer._graphs) >= 1 and len(e._trainer._graphs) == 0, policy
        assert EM.CALLS[0] > before and EM.FALLBACKS[0] == fb, policy
        assert all(np.array_equal(x, y) for x, y in zip(wg, we)), policy


def test_the_step_replays_in_a_captured_graph_and_equals_the_eager_fit():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "capture failed" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]


if __name__ == "__main__":
    _graph_fits()
