"""Training through keras.layers.GroupNormalization on the GPU (generic engine): the layer runs on the
kernels of csrc/kernels/groupnorm.hip in eager steps and in captured graphs, its gamma / beta gradients
reach the gradient slab through the direct targets, evaluate / predict use the same forward, and
``mixed_bfloat16`` takes the bf16 kernels.

The model: Conv2D(8, 3) -> GroupNormalization(4) -> ReLU -> Flatten -> Dense(10) on 8 x 8 x 1 inputs, batch 8,
3 SGD steps.

The weights after the 3 steps are compared with the ``TDL_GROUPNORM=torch`` run (the same function in PyTorch
ops on the GPU).  The tolerance comes from references only: 4 x the largest difference between that
PyTorch-op run on the GPU and the same run on the CPU (same data and seeds: what f32 arithmetic in another
order does to these weights), plus 1 f32 ulp at the weight's magnitude.  Observed (MI355X): recorded in
profiles/groupnorm_cost.txt.
"""
import os

import numpy as np
import pytest
import torch

import tensorflow_distributed_learning_amd as tdl
from kernel_refs import ulp32
from tensorflow_distributed_learning_amd.ops import groupnorm as GN

pytestmark = pytest.mark.gpu

STEPS = 3


def _ds():
    g = torch.Generator().manual_seed(0)
    x, y = torch.rand(STEPS * 8, 8, 8, 1, generator=g), torch.randint(0, 10, (STEPS * 8,), generator=g)
    return tdl.data.Dataset.from_tensor_slices((x, y)).batch(8).repeat()


def _fit(device="/gpu:0", env=None, policy="float32", steps=STEPS):
    L = tdl.keras.layers
    env = dict({"TDL_DISABLE_FUSED": "1"}, **(env or {}))
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        tdl.keras.backend.clear_session()
        tdl.keras.utils.set_random_seed(3)
        tdl.keras.mixed_precision.set_global_policy(policy)
        with tdl.distribute.MirroredStrategy(devices=[device]).scope():
            m = tdl.keras.Sequential([L.Conv2D(8, 3, input_shape=(8, 8, 1)), L.GroupNormalization(groups=4),
                                      L.ReLU(), L.Flatten(), L.Dense(10)])
            m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                      optimizer=tdl.keras.optimizers.SGD(learning_rate=0.05))
        h = m.fit(_ds(), epochs=1, steps_per_epoch=steps, verbose=0)
        assert m._trainer.kind == "generic"
        return m, h
    finally:
        tdl.keras.mixed_precision.set_global_policy("float32")
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _weights(m):
    return [np.asarray(w, dtype=np.float64) for w in m.get_weights()]


def test_fit_runs_the_kernels_in_a_captured_step():
    before = GN.CALLS[0]
    m, h = _fit(env={"TDL_GRAPH_STEP": "1"}, steps=6)
    assert GN.CALLS[0] > before
    assert m._trainer._graphs, "the step was not graph-captured after the warm-up steps"
    assert np.isfinite(h.history["loss"]).all()
    gn = m.layers[1]
    assert [w.name for w in gn.weights] == [f"{gn.name}/gamma:0", f"{gn.name}/beta:0"]
    assert not np.array_equal(gn.gamma.numpy(), np.ones(8)) and not np.array_equal(gn.beta.numpy(), np.zeros(8))
    # the replayed graph trains as the eager steps do
    e, _ = _fit(env={"TDL_GRAPH_STEP": "0"}, steps=6)
    assert not e._trainer._graphs
    for a, b in zip(_weights(m), _weights(e)):
        np.testing.assert_allclose(a, b, rtol=2e-5, atol=2e-6)


def test_eager_step_launches_the_hand_written_kernels():
    from tensorflow_distributed_learning_amd.utils.kernel_audit import audit

    m, _ = _fit(env={"TDL_GRAPH_STEP": "0"}, steps=1)  # warm-up (allocations, first-use set-up)
    ds = _ds()
    old = {k: os.environ.get(k) for k in ("TDL_DISABLE_FUSED", "TDL_GRAPH_STEP")}
    os.environ.update(TDL_DISABLE_FUSED="1", TDL_GRAPH_STEP="0")
    try:
        rep = audit(lambda: m.fit(ds, epochs=1, steps_per_epoch=1, verbose=0))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    print({k: dict(v) for k, v in rep.items() if v})
    mine = {n: c for n, c in rep["tdl"].items() if "k_gn_" in n}
    assert sum(c for n, c in mine.items() if "k_gn_sums" in n) == 2, mine
    assert sum(c for n, c in mine.items() if "k_gn_apply" in n) == 2, mine
    assert sum(c for n, c in mine.items() if "finalize" in n) == 2, mine
    every = [n for cat in rep.values() for n in cat]
    bad = [n for n in every if "group_norm" in n.lower() or "layer_norm" in n.lower()]
    assert not bad, bad


def test_gradients_reach_the_slab_through_the_direct_targets(monkeypatch):
    L = tdl.keras.layers
    seen = []
    orig = L.GroupNormalization._grad_targets

    def spy(self):
        t = orig(self)
        seen.append(t)
        return t

    monkeypatch.setattr(L.GroupNormalization, "_grad_targets", spy)
    a, _ = _fit(env={"TDL_GRAPH_STEP": "0"})
    assert seen and all(t is not None and t[0] is not None and t[1] is not None for t in seen[-STEPS:])
    assert all(t[0].dtype == torch.float32 and t[0].numel() == 8 for t in seen[-STEPS:])
    monkeypatch.setattr(L.GroupNormalization, "_grad_targets", lambda self: None)
    b, _ = _fit(env={"TDL_GRAPH_STEP": "0"})
    # the same kernels and sums; the slab starts at zero, so adding into it or copying into it agree
    for wa, wb in zip(_weights(a), _weights(b)):
        np.testing.assert_allclose(wa, wb, rtol=1e-6, atol=1e-7)
    assert not np.array_equal(a.layers[1].gamma.numpy(), np.ones(8))


def test_weights_match_the_torch_formula_run():
    k, _ = _fit()
    before = GN.CALLS[0]
    t, _ = _fit(env={"TDL_GROUPNORM": "torch"})
    assert GN.CALLS[0] == before, "TDL_GROUPNORM=torch must not run the kernels"
    c, _ = _fit(device="/cpu:0", env={"TDL_GROUPNORM": "torch"})
    wk, wt, wc = _weights(k), _weights(t), _weights(c)
    D = max(float(np.abs(a - b).max()) for a, b in zip(wt, wc))
    worst = max(float(np.abs(a - b).max()) for a, b in zip(wk, wt))
    print(f"\n[gn fit] torch formulas GPU vs CPU: {D:.3e}; kernels vs torch formulas on the GPU: {worst:.3e}")
    assert D > 0.0 or worst == 0.0
    for v, a, b in zip(k.weights, wk, wt):
        err = np.abs(a - b)
        tol = 4.0 * D + ulp32(b)
        assert (err <= tol).all(), f"{v.name}: {err.max():.3e} > {tol.flat[err.argmax()]:.3e}"


def test_evaluate_and_predict_use_the_forward_kernels():
    m, _ = _fit()
    g = torch.Generator().manual_seed(9)
    x, y = torch.rand(20, 8, 8, 1, generator=g), torch.randint(0, 10, (20,), generator=g)
    before = GN.CALLS[0]
    p = np.asarray(m.predict(x, batch_size=8, verbose=0))
    assert GN.CALLS[0] >= before + 3 and p.shape == (20, 10) and np.isfinite(p).all()
    before = GN.CALLS[0]
    ev = m.evaluate(x, y, batch_size=8, verbose=0)
    assert GN.CALLS[0] > before and np.isfinite(np.asarray(ev, dtype=np.float64)).all()
    # per-sample statistics: a sample's prediction does not depend on the batch it sits in
    p1 = np.asarray(m.predict(x[:5], batch_size=5, verbose=0))
    np.testing.assert_allclose(p1, p[:5], rtol=1e-5, atol=1e-6)


def test_mixed_bfloat16_fit_uses_the_bf16_kernels():
    before = dict(GN.CALLS_BY_DTYPE)
    m, h = _fit(policy="mixed_bfloat16")
    assert GN.CALLS_BY_DTYPE[torch.bfloat16] > before[torch.bfloat16]  # (eager and capturing steps; replays do not count)
    assert GN.CALLS_BY_DTYPE[torch.float32] == before[torch.float32]
    assert np.isfinite(h.history["loss"]).all()
    for w in m.get_weights():
        assert np.isfinite(np.asarray(w)).all()
    gn = m.layers[1]
    assert gn.gamma.value.dtype == torch.float32 and gn.beta.value.dtype == torch.float32
