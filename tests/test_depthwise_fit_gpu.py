"""Training through keras.layers.DepthwiseConv2D / SeparableConv2D on the GPU (generic engine): the layers run
on the kernels of csrc/kernels/depthwise.hip in eager steps and in captured graphs, without a library
convolution, in f32 and under ``mixed_bfloat16``.

The model: Conv2D(8, 3) -> DepthwiseConv2D(3, same, relu) -> SeparableConv2D(16, 3, strides 2) ->
GlobalAveragePooling2D -> Dense(10) on 10 x 10 x 1 inputs, batch 8, SGD.

The weights after training are compared with the ``TDL_DEPTHWISE=torch`` run (F.conv2d(groups=C) on the GPU) with
the tolerance of test_groupnorm_fit_gpu.py: 4 x the largest difference between that run on the GPU and the same
run on the CPU, plus 1 f32 ulp at the weight's magnitude.
"""
import os

import numpy as np
import pytest
import torch

import tensorflow_distributed_learning_amd as tdl
from kernel_refs import ulp32
from tensorflow_distributed_learning_amd.ops import conv as CONV
from tensorflow_distributed_learning_amd.ops import depthwise as DW

pytestmark = pytest.mark.gpu


def _fit(device="/gpu:0", env=None, policy="float32", steps=3):
    L = tdl.keras.layers
    env = dict({"TDL_DISABLE_FUSED": "1"}, **(env or {}))
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        tdl.keras.backend.clear_session()
        tdl.keras.utils.set_random_seed(3)
        tdl.keras.mixed_precision.set_global_policy(policy)
        g = torch.Generator().manual_seed(0)
        x, y = torch.rand(steps * 8, 10, 10, 1, generator=g), torch.randint(0, 10, (steps * 8,), generator=g)
        with tdl.distribute.MirroredStrategy(devices=[device]).scope():
            i = L.Input(shape=(10, 10, 1))
            h = L.Conv2D(8, 3)(i)
            h = L.DepthwiseConv2D(3, padding="same", activation="relu")(h)
            h = L.SeparableConv2D(16, 3, strides=2)(h)
            m = tdl.keras.Model(i, L.Dense(10)(L.GlobalAveragePooling2D()(h)))
            m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                      optimizer=tdl.keras.optimizers.SGD(learning_rate=0.05))
        h = m.fit(tdl.data.Dataset.from_tensor_slices((x, y)).batch(8).repeat(), epochs=1, steps_per_epoch=steps,
                  verbose=0)
        assert m._trainer.kind == "generic" and np.isfinite(h.history["loss"]).all()
        return m
    finally:
        tdl.keras.mixed_precision.set_global_policy("float32")
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _weights(m):
    return [np.asarray(w, dtype=np.float64) for w in m.get_weights()]


@pytest.mark.parametrize("policy,steps", [("float32", 3), ("mixed_bfloat16", 1)])
def test_weights_match_the_library_run(policy, steps):
    before = dict(DW.CALLS)
    CONV.reset_library_calls()
    k = _fit(policy=policy, steps=steps)
    assert not CONV.library_calls(), CONV.library_calls()
    assert all(DW.CALLS[n] > before[n] for n in before), (before, DW.CALLS)
    before = dict(DW.CALLS)
    t = _fit(policy=policy, steps=steps, env={"TDL_DEPTHWISE": "torch"})
    assert DW.CALLS == before, "TDL_DEPTHWISE=torch must not run the kernels"
    assert any(d == "depthwise_conv2d" for d, _ in CONV.library_calls())
    CONV.reset_library_calls()
    c = _fit(device="/cpu:0", policy=policy, steps=steps, env={"TDL_DEPTHWISE": "torch"})
    wk, wt, wc = _weights(k), _weights(t), _weights(c)
    D = max(float(np.abs(a - b).max()) for a, b in zip(wt, wc))
    worst = max(float(np.abs(a - b).max()) for a, b in zip(wk, wt))
    print(f"\n[dw fit {policy}] library GPU vs CPU: {D:.3e}; kernels vs library on the GPU: {worst:.3e}")
    for v, a, b in zip(k.weights, wk, wt):
        err = np.abs(a - b)
        tol = 4.0 * D + ulp32(b)
        assert (err <= tol).all(), f"{v.name}: {err.max():.3e} > {tol.flat[err.argmax()]:.3e}"
        assert v.value.dtype == torch.float32


def test_the_step_replays_in_a_captured_graph_with_the_same_bits():
    a = _fit(env={"TDL_GRAPH_STEP": "1"}, steps=6)
    assert a._trainer._graphs, "the step was not graph-captured after the warm-up steps"
    b = _fit(env={"TDL_GRAPH_STEP": "1"}, steps=6)
    for wa, wb in zip(a.get_weights(), b.get_weights()):
        assert np.array_equal(np.asarray(wa), np.asarray(wb))
    e = _fit(env={"TDL_GRAPH_STEP": "0"}, steps=6)  # the replayed graph trains as the eager steps do
    for wa, we in zip(_weights(a), _weights(e)):
        np.testing.assert_allclose(wa, we, rtol=2e-5, atol=2e-6)
