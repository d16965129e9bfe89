"""Training through keras.layers.Conv2D(groups=4) on the GPU (generic engine): the layer runs on the kernels of
csrc/kernels/grouped_conv.hip without a library convolution, in f32 and under ``mixed_bfloat16``, and follows the
same fit under ``TDL_GROUPED_CONV=torch`` (F.conv2d(groups=) on the GPU).

Tolerances: f32 as tests/test_conv_f32_gpu.py compares a kernel fit with a library fit (loss rtol 1e-3; weights
rtol 1e-2, atol 2e-3); ``mixed_bfloat16`` as tests/test_sync_bn_multireplica_gpu.py does (loss rtol 3e-2, weights
atol 6e-2 x learning rate).
"""
import os

import numpy as np
import pytest
import torch

import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.ops import conv as CONV
from tensorflow_distributed_learning_amd.ops import grouped_conv as GC

pytestmark = pytest.mark.gpu

LR = 0.05
BOUNDS = {"float32": (1e-3, 1e-2, 2e-3), "mixed_bfloat16": (3e-2, 0.0, 6e-2 * LR)}  # loss rtol; weights rtol, atol


def _fit(env=None, policy="float32", steps=3):
    L = tdl.keras.layers
    # eager steps (no whole-step graph, so no capture stream is taken from the process's stream pool)
    env = dict({"TDL_DISABLE_FUSED": "1", "TDL_GRAPH_STEP": "0"}, **(env or {}))
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        tdl.keras.backend.clear_session()
        tdl.keras.utils.set_random_seed(3)
        tdl.keras.mixed_precision.set_global_policy(policy)
        g = torch.Generator().manual_seed(0)
        x, y = torch.rand(steps * 8, 10, 10, 1, generator=g), torch.randint(0, 10, (steps * 8,), generator=g)
        with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
            m = tdl.keras.Sequential([L.Conv2D(8, 3, activation="relu"),
                                      L.Conv2D(16, 3, groups=4, padding="same", activation="relu"),
                                      L.GlobalAveragePooling2D(), L.Dense(10)])
            m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                      optimizer=tdl.keras.optimizers.SGD(learning_rate=LR))
        h = m.fit(tdl.data.Dataset.from_tensor_slices((x, y)).batch(8).repeat(), epochs=steps, steps_per_epoch=1,
                  verbose=0)
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
    before = dict(GC.CALLS)
    CONV.reset_library_calls()
    k, lk = _fit(policy=policy)
    assert not CONV.library_calls(), CONV.library_calls()
    assert all(GC.CALLS[n] > before[n] for n in ("forward", "wgrad", "dgrad")), (before, GC.CALLS)
    before = dict(GC.CALLS)
    t, lt = _fit(policy=policy, env={"TDL_GROUPED_CONV": "torch"})
    assert GC.CALLS == before, "TDL_GROUPED_CONV=torch must not run the kernels"
    assert any(d == "conv2d" for d, _ in CONV.library_calls()), CONV.library_calls()
    CONV.reset_library_calls()
    lr_, wr, wa = BOUNDS[policy]
    print(f"\n[gconv fit {policy}] losses {lk} vs {lt}")
    np.testing.assert_allclose(lk, lt, rtol=lr_)
    for v, a, b in zip(k.weights, k.get_weights(), t.get_weights()):
        np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=wr, atol=wa, err_msg=v.name)
        assert v.value.dtype == torch.float32
