"""Training through RandomTranslation and RandomFlip on one MI355X (keras/layers.py, ops/augment.py): Sequential
``[RandomTranslation, RandomFlip, Conv2D, MaxPooling2D, Flatten, Dense]`` on 64 images of 8 x 8 x 1, batch 8,
6 SGD steps with ``steps_per_execution=3`` and NO shuffle (every run sees the same batches).  The layers keep
the fit on the generic engine's device-resident input and K-step execution graphs, the replayed graph draws
what eager steps draw (the call counter advances on the device), the step gains no PyTorch indexing kernel,
evaluation ignores the layers, and ``reset_rng`` replays a fit."""
import functools
import os

import numpy as np
import pytest
import torch

import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.ops import augment as A
from tensorflow_distributed_learning_amd.ops import dropout as D

pytestmark = pytest.mark.gpu
K = tdl.keras
L = K.layers
B, STEPS, SPE = 8, 6, 3


class _env:
    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.prev = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.prev.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _xy():
    g = torch.Generator().manual_seed(0)
    return torch.rand(64, 8, 8, 1, generator=g), torch.randint(0, 10, (64,), generator=g)


def _ds():
    """A fresh pipeline over the ONE pair of tensors (so the uploaded columns and the graphs over them stay)."""
    return tdl.data.Dataset.from_tensor_slices(_xy()).cache().batch(B).repeat()


def _model(augment=True):
    K.backend.clear_session()
    K.utils.set_random_seed(3)
    first = [L.RandomTranslation(0.25, 0.25, input_shape=(8, 8, 1)), L.RandomFlip("horizontal")] if augment else []
    conv = L.Conv2D(8, 3, activation="relu", padding="same", **({} if augment else {"input_shape": (8, 8, 1)}))
    with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
        m = K.Sequential(first + [conv, L.MaxPooling2D(), L.Flatten(), L.Dense(10)])
        m.compile(loss=K.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=K.optimizers.SGD(0.05),
                  metrics=["sparse_categorical_accuracy"], steps_per_execution=SPE)
    return m


def _flat(m):
    return torch.cat([torch.as_tensor(w).reshape(-1) for w in m.get_weights()]).cpu()


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _calls(m):
    return [l.rng_calls("cuda:0") for l in m.layers if isinstance(l, (L.RandomTranslation, L.RandomFlip))]


@functools.lru_cache(maxsize=None)
def _fit(mode, augment=True):
    """One fit (cached: the tests share them).  ``graph``: device-resident input and execution graphs;
    ``eager``: the same device path without capture."""
    with _env(TDL_DISABLE_FUSED="0", TDL_GENERIC_DEVICE_DATA="1", TDL_GRAPH_STEP="1",
              TDL_GENERIC_DEVICE_EAGER="1" if mode == "eager" else "0"):
        m = _model(augment)
        h = m.fit(_ds(), epochs=1, steps_per_epoch=STEPS, verbose=0)
    return m, _flat(m), {k: list(v) for k, v in h.history.items()}


def test_gpu_layer_output_is_the_cpu_layer_output():
    x = _xy()[0][:B]
    for make in (lambda: L.RandomTranslation(0.25, 0.25, seed=5),
                 lambda: L.RandomTranslation(0.5, (-0.25, 0.5), fill_mode="constant", fill_value=0.5, seed=5),
                 lambda: L.RandomFlip(seed=5)):
        gpu, cpu = make(), make()
        for call in range(3):
            xg = x.cuda().requires_grad_(True)
            xc = x.clone().requires_grad_(True)
            yg, yc = gpu(xg, training=True), cpu(xc, training=True)
            assert _same(yg.detach().cpu(), yc.detach()), f"{gpu.name} call {call}"
            # and it is the op's reference for this seed and call number
            want = A.augment(x, cpu._spec(8, 8), D.stream_key(5, 0, 0), ticket=call)
            assert _same(yc.detach(), want)
            dy = torch.randn(yc.shape, generator=torch.Generator().manual_seed(call))
            yg.backward(dy.cuda())
            yc.backward(dy)
            assert _same(xg.grad.cpu(), xc.grad)
        assert gpu.rng_calls("cuda:0") == cpu.rng_calls() == 3 and gpu.rng_calls() == 0


def test_execution_graphs_train_like_eager_steps():
    m, w, h = _fit("graph")
    tr = m._trainer
    assert tr.kind == "generic" and m._fused_reason == "model is not the reference CNN"
    assert tr._graph_ok and list(tr._graphs) == [("dev", SPE, B)], f"graph_captured must hold: {list(tr._graphs)}"
    assert tr._X is not None and tr._X.is_cuda, "the input columns must be device-resident"
    assert int(tr.optimizer.iterations) == STEPS and _calls(m) == [STEPS, STEPS]
    e, we, he = _fit("eager")
    assert e._trainer.kind == "generic" and not e._trainer._graphs and _calls(e) == [STEPS, STEPS]
    assert _same(w, we), f"max |dw| = {float((w - we).abs().max()):.3e}"
    assert h == he
    # the layers take part: the same fit without them ends elsewhere
    _, wp, _ = _fit("graph", augment=False)
    assert w.shape == wp.shape and not _same(w, wp)


def test_step_adds_no_torch_indexing_kernel():
    from tensorflow_distributed_learning_amd.utils.kernel_audit import audit

    reps = {}
    for augment in (True, False):
        with _env(TDL_GENERIC_DEVICE_DATA="1", TDL_GRAPH_STEP="1", TDL_GENERIC_DEVICE_EAGER="1"):
            m = _model(augment)
            m.fit(_ds(), epochs=1, steps_per_epoch=SPE, verbose=0)  # warm-up (allocations, first-use set-up)
            reps[augment] = audit(lambda: m.fit(_ds(), epochs=1, steps_per_epoch=SPE, verbose=0))
            assert m._trainer.kind == "generic" and not m._trainer._graphs
    rep, plain = reps[True], reps[False]
    print({k: dict(v) for k, v in rep.items() if v})
    mine = {n: c for n, c in rep["tdl"].items() if "k_augment" in n}
    # the layers sit at the top of the model: their input needs no gradient, so no backward launch exists
    assert sum(mine.values()) == 2 * SPE and all("k_augment_fwd" in n for n in mine), mine
    assert not any("k_augment" in n for n in plain["tdl"])
    extra = {n: c - plain["torch"].get(n, 0) for n, c in rep["torch"].items() if c > plain["torch"].get(n, 0)}
    bad = [n for n in extra if any(s in n.lower() for s in ("index", "gather", "scatter", "flip", "roll"))]
    assert not bad, bad
    assert not extra, f"PyTorch kernels the layers added to the step: {extra}"
    assert not rep["library"], rep["library"]


def test_evaluate_and_predict_ignore_the_layers():
    m, _, _ = _fit("graph")
    calls = _calls(m)
    plain = _model(augment=False)
    plain.build((None, 8, 8, 1))
    plain.set_weights(m.get_weights())
    x, y = _xy()
    pa, pb = m.predict(x, batch_size=B, verbose=0), plain.predict(x, batch_size=B, verbose=0)
    assert np.array_equal(np.asarray(pa), np.asarray(pb))
    ea, eb = m.evaluate(x, y, batch_size=B, verbose=0), plain.evaluate(x, y, batch_size=B, verbose=0)
    assert list(ea) == list(eb)
    assert _calls(m) == calls, "evaluation drew from the layers' streams"


def test_reset_rng_replays_a_fit():
    with _env(TDL_GENERIC_DEVICE_DATA="1", TDL_GRAPH_STEP="1", TDL_GENERIC_DEVICE_EAGER="0"):
        m = _model()
        m.build((None, 8, 8, 1))
        w0 = [np.array(w, copy=True) for w in m.get_weights()]
        m.fit(_ds(), epochs=1, steps_per_epoch=STEPS, verbose=0)
        first = _flat(m)
        assert _calls(m) == [STEPS, STEPS]
        # without the reset the second fit draws calls 6 .. 11 and ends elsewhere
        m.set_weights(w0)
        m.fit(_ds(), epochs=1, steps_per_epoch=STEPS, verbose=0)
        assert _calls(m) == [2 * STEPS, 2 * STEPS] and not _same(_flat(m), first)
        m.set_weights(w0)
        for l in m.layers[:2]:
            l.reset_rng()
        assert _calls(m) == [0, 0]
        m.fit(_ds(), epochs=1, steps_per_epoch=STEPS, verbose=0)
        assert _calls(m) == [STEPS, STEPS]
        assert _same(_flat(m), first), "reset_rng did not replay the draws"
        assert _same(_flat(m), _fit("graph")[1]), "a fresh model with the same seeds ends elsewhere"
