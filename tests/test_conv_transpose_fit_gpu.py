"""Training through keras.layers.Conv2DTranspose on the GPU (generic engine): the layer runs on the kernels of
csrc/kernels/conv_transpose.hip without a library convolution, in f32 and under ``mixed_bfloat16``, follows the same
fit under ``TDL_CONV_TRANSPOSE=torch`` (F.conv_transpose2d on the GPU), and trains the same from a captured and
replayed whole-step graph.

The batch is centred and scaled to [-1/6, 1/6]: the library run rounds its own dW / db to bf16 (2^-9 relative)
where the kernels keep them f32, and the weight bound under ``mixed_bfloat16`` (a gradient difference of 6e-2 summed
over the fit) leaves room for that only while the layer's gradients stay below 8.  The engine's loss sums the squared
error over an image's 256 pixels, so unit-range images as their own targets give gradients of about 100; centred at
this scale the per-image loss is 256 / 12 / 9 = 2.4, where the cross-entropy of the fit the bounds come from starts.

Tolerances: those of tests/test_grouped_conv_fit_gpu.py for a kernel fit against a library fit (f32: loss rtol 1e-3;
weights rtol 1e-2, atol 2e-3; ``mixed_bfloat16``: loss rtol 3e-2, weights atol 6e-2 x learning rate); a replayed graph
against eager steps as tests/test_depthwise_fit_gpu.py has it (rtol 2e-5, atol 2e-6).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.ops import conv as CONV
from tensorflow_distributed_learning_amd.ops import conv_transpose as CT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the engine's loss is sum(per-pixel MSE) / batch: 256 pixels per image, so 256 x the gradient of the image mean;
# the step is tests/test_grouped_conv_fit_gpu.py's 0.05 on the image-mean loss
LR = 0.05 / 256
BOUNDS = {"float32": (1e-3, 1e-2, 2e-3), "mixed_bfloat16": (3e-2, 0.0, 6e-2 * LR)}  # loss rtol; weights rtol, atol


def _fit(env=None, policy="float32", steps=3, epochs=None):
    # 3 steps, as the fit the weight bounds were set for; eager unless the caller asks for the whole-step graph
    L = tdl.keras.layers
    env = dict({"TDL_DISABLE_FUSED": "1", "TDL_GRAPH_STEP": "0"}, **(env or {}))
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        tdl.keras.backend.clear_session()
        tdl.keras.utils.set_random_seed(3)
        tdl.keras.mixed_precision.set_global_policy(policy)
        g = torch.Generator().manual_seed(0)
        x = (torch.rand(steps * 8, 16, 16, 1, generator=g) - 0.5) / 3  # (see the module docstring)
        with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
            m = tdl.keras.Sequential([L.Conv2D(8, 3, strides=2, padding="same", activation="relu"),
                                      L.Conv2DTranspose(8, 4, strides=2, padding="same", activation="relu"),
                                      L.Conv2D(1, 1)])
            m.compile(loss="mse", optimizer=tdl.keras.optimizers.SGD(learning_rate=LR))
        h = m.fit(tdl.data.Dataset.from_tensor_slices((x, x)).batch(8).repeat(), epochs=epochs or steps,
                  steps_per_epoch=steps // (epochs or steps), verbose=0)
        assert m._trainer.kind == "generic" and np.isfinite(h.history["loss"]).all()
        return m, h.history["loss"]
    finally:
        tdl.keras.mixed_precision.set_global_policy("float32")
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
def test_fit_runs_on_the_kernels_and_follows_the_library_run(policy):
    before = dict(CT.CALLS)
    CONV.reset_library_calls()
    k, lk = _fit(policy=policy)
    assert not CONV.library_calls(), CONV.library_calls()
    assert all(CT.CALLS[n] > before[n] for n in ("forward", "wgrad", "dgrad")), (before, CT.CALLS)
    before = dict(CT.CALLS)
    t, lt = _fit(policy=policy, env={"TDL_CONV_TRANSPOSE": "torch"})
    assert CT.CALLS == before, "TDL_CONV_TRANSPOSE=torch must not run the kernels"
    assert any(d == "conv2d_transpose" for d, _ in CONV.library_calls()), CONV.library_calls()
    CONV.reset_library_calls()
    lr_, wr, wa = BOUNDS[policy]
    print(f"\n[convt fit {policy}] losses {lk} vs {lt}")
    np.testing.assert_allclose(lk, lt, rtol=lr_)
    for v, a, b in zip(k.weights, k.get_weights(), t.get_weights()):
        print(f"[convt fit {policy}] {v.name}: largest weight difference {np.abs(np.asarray(a) - np.asarray(b)).max():.3g}")
        np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=wr, atol=wa, err_msg=v.name)
        assert v.value.dtype == torch.float32


def _graph_fits():
    """Per policy: two fits whose third and later steps replay the captured whole-step graph, and the eager fit."""
    out = {}
    for policy in ("float32", "mixed_bfloat16"):
        before = dict(CT.CALLS)
        CONV.reset_library_calls()
        a, _ = _fit(policy=policy, env={"TDL_GRAPH_STEP": "1"}, steps=6, epochs=1)
        b, _ = _fit(policy=policy, env={"TDL_GRAPH_STEP": "1"}, steps=6, epochs=1)
        e, _ = _fit(policy=policy, steps=6, epochs=1)
        wa, wb, we = ([np.asarray(w, np.float64) for w in m.get_weights()] for m in (a, b, e))
        out[policy] = {"graphs": [len(a._trainer._graphs), len(b._trainer._graphs), len(e._trainer._graphs)],
                       "iterations": int(a._trainer.optimizer.iterations),
                       "kernels_ran": all(CT.CALLS[n] > before[n] for n in before),
                       "library_calls": len(CONV.library_calls()),
                       "same_bits": all(np.array_equal(x, y) for x, y in zip(wa, wb)),
                       "close_to_eager": all(np.allclose(x, y, rtol=2e-5, atol=2e-6) for x, y in zip(wa, we)),
                       "largest_difference_to_eager": max(float(np.abs(x - y).max()) for x, y in zip(wa, we)),
                       "moved": max(float(np.abs(x).max()) for x in wa[1::2])}  # the biases start at zero
    return out


def test_the_step_replays_in_a_captured_graph_and_trains_as_the_eager_steps_do():
    # in a process of its own: the fits above stay eager, as tests/test_grouped_conv_fit_gpu.py's are, so that this
    # process takes no capture stream from its stream pool; the two replicas of tests/test_local_replicas_gpu.py
    # share one GPU on consecutive streams of that pool and need a hardware queue each
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(f"\n[convt graph fit] {res}")
    assert "capture failed" not in r.stderr, r.stderr[-3000:]
    for policy, v in res.items():
        assert v["graphs"][0] >= 1 and v["graphs"][1] >= 1 and v["graphs"][2] == 0, (policy, v)
        assert v["iterations"] == 6 and v["kernels_ran"] and v["library_calls"] == 0 and v["moved"] > 0, (policy, v)
        assert v["same_bits"] and v["close_to_eager"], (policy, v)


if __name__ == "__main__":
    print(json.dumps(_graph_fits()))
