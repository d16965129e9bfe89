"""Gradient clipping without a GPU: the torch path of ``Optimizer.apply_flat`` (the CPU implementation, and
the emulation the GPU tests size their tolerances with) still computes the formulas of ``Optimizer._clip``,
an unbuilt or CPU-built clipped optimizer is not graph-safe, and the fused engine no longer refuses clipping.
"""
import types

import numpy as np
import pytest
import torch

import clip_refs as CR
import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.engine import fused

O = tdl.keras.optimizers
CLIPS = [dict(clipvalue=0.3), dict(clipnorm=0.7), dict(global_clipnorm=0.7), dict(global_clipnorm=0.7, clipvalue=0.3),
         dict(global_clipnorm=1e6)]


@pytest.mark.parametrize("clip", CLIPS, ids=lambda c: "+".join(c))
def test_cpu_apply_flat_clips_by_the_numpy_formula(clip):
    rng = np.random.default_rng(0)
    n = 1000
    w0 = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 0.5).astype(np.float32)
    lr = 0.125  # (a power of two: w - lr * g' rounds once)
    opt = O.SGD(lr, **clip)
    W, G = torch.from_numpy(w0.copy()), torch.from_numpy(g.copy())
    opt.apply_flat(W, G)
    gc, norm, scale = CR.clip_ref(g, clip.get("global_clipnorm") or clip.get("clipnorm"), clip.get("clipvalue"))
    want = w0.astype(np.float64) - lr * gc
    # f32: the norm (a sum of n squares), the scale and the product; far below 1e-5 relative
    np.testing.assert_allclose(W.numpy(), want, rtol=1e-5, atol=1e-6)
    if scale is not None:
        assert (scale < 1.0) == (clip.get("global_clipnorm", 0.7) < 1e5)
    assert opt.iterations == 1
    assert opt._clip_out is None and opt.last_clip_norm is None, "no device buffers on a CPU slab"


def test_cpu_clip_keeps_nan_and_zeroes_on_inf():
    """The two properties of ``_clip`` that TerminateOnNaN depends on, and that the kernels reproduce."""
    g = torch.tensor([1.0, float("nan"), -2.0])
    W = torch.zeros(3)
    O.SGD(1.0, clipnorm=1.0).apply_flat(W, g.clone())
    assert torch.isnan(W).all()
    g = torch.tensor([1.0, float("inf"), -2.0])
    W = torch.ones(3)
    O.SGD(1.0, clipnorm=1.0).apply_flat(W, g.clone())
    assert W[0] == 1 and W[2] == 1 and torch.isnan(W[1])
    g = torch.tensor([float("nan"), float("inf"), -float("inf")])
    W = torch.zeros(3)
    O.SGD(1.0, clipvalue=0.5).apply_flat(W, g.clone())
    assert torch.isnan(W[0]) and W[1] == -0.5 and W[2] == 0.5


@pytest.mark.parametrize("cls", [O.Adam, O.AdamW, O.RMSprop, O.Adagrad])
@pytest.mark.parametrize("clip", [dict(clipnorm=1.0), dict(global_clipnorm=1.0), dict(clipvalue=0.5)],
                         ids=lambda c: "+".join(c))
def test_unbuilt_or_cpu_built_clipped_optimizer_is_not_graph_safe(cls, clip):
    opt = cls(0.01, **clip)
    assert opt._clipped and not opt.graph_safe
    opt.build(128, torch.device("cpu"))
    assert not opt.graph_safe


def test_sgd_graph_safe_stays_constant():
    assert O.SGD(0.01).graph_safe is True and O.SGD(0.01, clipnorm=1.0).graph_safe is True
    assert not O.SGD(0.01)._clipped and O.SGD(0.01, clipvalue=0.0)._clipped


def test_fused_eligibility_does_not_name_clipping(monkeypatch):
    """eligible() with everything in front of the optimizer check stubbed: a clipped optimizer passes it."""
    from tensorflow_distributed_learning_amd import ops
    from tensorflow_distributed_learning_amd.keras import losses

    kernels = types.SimpleNamespace(adam=1, rmsprop=1, adagrad=1, sgd=1, clip_norm=1)
    monkeypatch.setattr(ops, "hip_available", lambda: True)
    monkeypatch.setattr(ops, "hip", lambda: kernels)
    monkeypatch.setattr(fused, "_is_reference_cnn", lambda m: True)
    monkeypatch.delenv("TDL_DISABLE_FUSED", raising=False)

    def model(opt):
        strategy = types.SimpleNamespace(extended=types.SimpleNamespace(device=torch.device("cuda", 0)))
        return types.SimpleNamespace(_get_strategy=lambda: strategy, _dtype_policy=lambda: "float32",
                                     loss=losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt,
                                     compiled_metrics=[])

    for opt in (O.Adam(1e-3, global_clipnorm=1.0), O.SGD(0.05, momentum=0.9, clipnorm=1.0), O.SGD(0.05, clipvalue=0.1),
                O.RMSprop(clipvalue=0.1), O.Adagrad(clipnorm=2.0)):
        assert fused.eligible(model(opt)) is None
    # a stale extension without the clip kernels is named as such, not silently taken
    del kernels.clip_norm
    assert "clip_norm" in fused.eligible(model(O.Adam(1e-3, global_clipnorm=1.0)))
    assert fused.eligible(model(O.Adam(1e-3))) is None


def test_clipped_optimizer_is_never_plain_sgd():
    t = types.SimpleNamespace(optimizer=O.SGD(0.05))
    assert fused.FusedMnistTrainer._plain_sgd.fget(t)
    for opt in (O.SGD(0.05, clipnorm=1.0), O.SGD(0.05, clipvalue=0.1), O.SGD(0.05, momentum=0.9), O.Adam()):
        assert not fused.FusedMnistTrainer._plain_sgd.fget(types.SimpleNamespace(optimizer=opt))
