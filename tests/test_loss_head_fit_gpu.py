"""``fit(class_weight=...)``, a sample-weight column and label smoothing end to end on one MI355X: the reference
CNN on 64 synthetic images, batch 16, 4 steps.  Class weights reach the loss, all-ones class weights are the
unweighted fit bit for bit, a class-weight dict is the equivalent sample-weight column bit for bit, a weighted
fit keeps device-resident input and K-step execution graphs (keyed by which weights are present) that replay
like eager steps, the weighted and smoothed head launches hand-written kernels only, stays as close to the torch
formulas as the unweighted head does, and a fused-engine model falls back to the generic engine with a reason.

The data pipelines here do NOT shuffle: every run sees the same batches in the same order.
"""
import numpy as np
import pytest
import torch

import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.models.mnist_cnn import build_mnist_cnn

import kernel_refs as R
import test_fit_gpu as F
from test_accum_fit_gpu import _env

pytestmark = pytest.mark.gpu
K = tdl.keras
B, STEPS = 16, 4
CW = {0: 0.25, 1: 4.0, 2: 0.5, 3: 2.0, 5: 3.0, 7: 0.0, 9: 1.5}  # (4, 6 and 8 are left at 1)


def _table(cw=CW) -> torch.Tensor:
    t = torch.ones(10)
    for c, w in cw.items():
        t[c] = w
    return t


def _xy():
    """The 64 synthetic images [64, 28, 28, 1] and their int64 labels, as tensors."""
    x, y = F._data(64)
    return torch.as_tensor(x), torch.as_tensor(y).long()


def _pipeline(x, y, sw=None):
    cols = (x, y) if sw is None else (x, y, sw)

    def scale(image, *rest):
        return (image.to(torch.float32) / 255,) + rest

    return tdl.data.Dataset.from_tensor_slices(cols).map(scale).cache().batch(B).repeat()


def _train(steps=STEPS, spe=1, graph=True, fused=False, loss=None, metrics="sparse", sw=None, model=None, dense=False,
           ds=None, **fit_kw):
    """``steps`` SGD steps of the reference CNN over the first ``steps`` batches of 16 of 64 synthetic images
    (``ds``: this pipeline instead of a new one over the same images)."""
    g = "1" if graph else "0"
    with _env(TDL_DISABLE_FUSED="0" if fused else "1", TDL_GRAPH=g, TDL_GRAPH_STEP=g):
        x, y = _xy()
        if dense:
            y = torch.nn.functional.one_hot(y, 10).float()
        if model is None:
            K.backend.clear_session()
            K.utils.set_random_seed(3)
            with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
                model = build_mnist_cnn()
                ms = {"sparse": [K.metrics.SparseCategoricalAccuracy()], "dense": [K.metrics.CategoricalAccuracy()],
                      None: None}[metrics]
                model.compile(loss=loss or K.losses.SparseCategoricalCrossentropy(from_logits=True),
                              optimizer=K.optimizers.SGD(0.05), metrics=ms, steps_per_execution=spe)
        ds = ds if ds is not None else _pipeline(x, y, sw)
        h = model.fit(ds, epochs=1, steps_per_epoch=steps, verbose=0, **fit_kw)
        model._last_history = h.history
        return model


def _w(m) -> np.ndarray:
    return m._W.detach().cpu().numpy().copy()


def _same(a, b) -> bool:
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


class _Start(K.callbacks.Callback):
    """The weight slab at the start of fit."""

    def on_train_begin(self, logs=None):
        self.w0 = self.model._W.detach().cpu().numpy().copy()


def test_all_zero_class_weights_leave_the_weights_unchanged():
    """Fails while fit drops class_weight: every row weighs 0, so SGD must not move a weight.  (Also through the
    default engine choice: the compiled model is one the fused MNIST engine takes.)"""
    for fused in (False, True):
        rec = _Start()
        m = _train(fused=fused, class_weight={c: 0.0 for c in range(10)}, callbacks=[rec])
        assert _same(rec.w0, _w(m)), "class_weight was ignored: the weights moved"
        assert m._trainer.kind == "generic" and m._last_history["loss"][-1] == 0.0
    rec = _Start()
    m = _train(callbacks=[rec])
    assert not _same(rec.w0, _w(m)), "the unweighted run must train (the test bites)"


@pytest.mark.parametrize("spe", [1, 2], ids=["step-graphs", "execution-graphs"])
def test_all_ones_class_weight_is_the_unweighted_generic_fit(spe):
    a = _train(spe=spe, class_weight={c: 1.0 for c in range(10)})
    b = _train(spe=spe)
    assert a._trainer.kind == b._trainer.kind == "generic"
    assert _same(_w(a), _w(b))
    assert a._last_history == b._last_history


@pytest.mark.parametrize("spe", [1, 2], ids=["step-graphs", "execution-graphs"])
def test_class_weight_dict_is_the_equivalent_sample_weight_column(spe):
    _, y = _xy()
    a = _train(spe=spe, class_weight=CW)
    b = _train(spe=spe, sw=_table()[y])
    c = _train(spe=spe)
    assert _same(_w(a), _w(b)) and not _same(_w(a), _w(c))
    assert a._last_history == b._last_history


def test_weighted_execution_graph_replays_like_eager_steps():
    """Class weights x a sample-weight column x label smoothing, steps_per_execution = 2: the first execution runs
    eagerly, the second is a captured 2-step graph; the same 4 steps run one at a time without any graph."""
    _, y = _xy()
    sw = torch.rand(64, generator=torch.Generator().manual_seed(5)) * 1.5 + 0.5
    loss = lambda: K.losses.SparseCategoricalCrossentropy(from_logits=True, label_smoothing=0.1)  # noqa: E731
    g = _train(spe=2, class_weight=CW, sw=sw, loss=loss())
    e = _train(spe=1, graph=False, class_weight=CW, sw=sw, loss=loss())
    tr = g._trainer
    assert tr.kind == "generic" and tr._graph_ok and bool(tr._graphs), "graph_captured must be true"
    assert list(tr._graphs) == [("dev", 2, B, ("weights", True, True))], list(tr._graphs)
    assert not e._trainer._graphs
    assert _same(_w(g), _w(e))
    assert g._last_history == e._last_history
    plain = _train(spe=2)
    assert not _same(_w(g), _w(plain))


def test_graph_keys_tell_which_weights_are_present():
    x, y = _xy()
    ds = _pipeline(x, y)  # (ONE pipeline for the first three fits: its cached columns are uploaded once)
    m = _train(spe=2, ds=ds)
    tr = m._trainer
    assert list(tr._graphs) == [("dev", 2, B)]
    _train(spe=2, model=m, ds=ds, class_weight=CW)
    assert m._trainer is tr and sorted(tr._graphs, key=len) == [("dev", 2, B), ("dev", 2, B, ("weights", False, True))]
    table, graphs = tr._cw, dict(tr._graphs)
    _train(spe=2, model=m, ds=ds, class_weight={1: 2.0})  # a later fit updates the ONE table in place
    assert tr._cw is table and table.tolist() == [1, 2, 1, 1, 1, 1, 1, 1, 1, 1]
    assert all(tr._graphs[k] is g for k, g in graphs.items()) and len(tr._graphs) == 2, "the graphs must stay valid"
    _train(spe=2, model=m, sw=_table()[y])  # (another dataset: the graphs over the old columns are gone)
    assert list(tr._graphs) == [("dev", 2, B, ("weights", True, False))]
    # and whole-step graphs of a host pipeline
    with _env(TDL_GENERIC_DEVICE_DATA="0"):
        h = _train(spe=1, steps=4, class_weight=CW)
    assert all(k[-1] == ("weights", False, True) for k in h._trainer._graphs) and h._trainer._graphs


def test_weighted_smoothed_head_launches_hand_written_kernels_only():
    """One weighted, smoothed loss head and its backward, from the logits to dz, under the profiler: no PyTorch and
    no library kernel, for the sparse and for the dense target."""
    from tensorflow_distributed_learning_amd.utils.kernel_audit import audit

    g = torch.Generator().manual_seed(1)
    sw = (torch.rand(B, generator=g) + 0.5).cuda()
    for dense in (False, True):
        loss = (K.losses.CategoricalCrossentropy if dense else K.losses.SparseCategoricalCrossentropy)(
            from_logits=True, label_smoothing=0.1)
        m = _train(steps=2, class_weight=CW, loss=loss, dense=dense, metrics="dense" if dense else "sparse")
        tr = m._trainer
        assert tr._cw_on and tr._cw.is_cuda
        z = torch.randn(B, 10, generator=g).cuda().requires_grad_(True)
        y = torch.randint(0, 10, (B,), generator=g).cuda()
        y = torch.nn.functional.one_hot(y, 10).float() if dense else y
        out = {}

        def step():
            head = tr._fused_head(y, z, sw, tr._cw)
            assert head is not None, "the weighted head was not taken"
            out["loss"] = head(B)
            (out["dz"],) = torch.autograd.grad(out["loss"], z, grad_outputs=tr._seed())

        step()  # (first use)
        rep = audit(step)
        print({k: dict(v) for k, v in rep.items() if v})
        assert not rep["torch"] and not rep["library"] and not rep["other"], rep
        assert list(rep["tdl"].values()) == [1] and "k_xent_head_w" in next(iter(rep["tdl"])), rep["tdl"]
        # what it computed is the torch formula of the same loss
        w = sw * tr._cw[y.argmax(-1) if dense else y]
        zr = z.detach().clone().requires_grad_(True)
        ref = (loss.per_example(y, zr) * w).sum() / B
        (dref,) = torch.autograd.grad(ref, zr)
        torch.testing.assert_close(out["loss"], ref.detach(), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(out["dz"], dref, rtol=1e-4, atol=1e-7)


def test_weighted_head_stays_as_close_to_the_torch_head_as_the_unweighted_one():
    """max |dW| between the fused head and the torch formulas (TDL_FUSED_HEAD=0) after 4 steps: d0 for the unweighted
    pair (existing code only); the class-weighted pair, whose gradients are scaled by at most 4, must stay within
    4 d0 (and never below 4 ulp of |W|)."""
    def pair(**kw):
        on = _w(_train(spe=1, **kw))
        with _env(TDL_FUSED_HEAD="0"):
            off = _w(_train(spe=1, **kw))
        return on, off

    on0, off0 = pair()
    d0 = float(np.abs(on0.astype(np.float64) - off0).max())
    on1, off1 = pair(class_weight=CW)
    d1 = np.abs(on1.astype(np.float64) - off1)
    print(f"loss head vs torch formulas, max |dW| after {STEPS} steps: unweighted d0 = {d0:.3e}, "
          f"class-weighted d1 = {float(d1.max()):.3e}")
    bound = np.maximum(4 * d0, 4 * R.ulp32(on1))
    assert (d1 <= bound).all(), (float(d1.max()), d0)
    assert not _same(on0, on1)


def test_dense_smoothed_weighted_fit_matches_the_torch_formulas():
    """CategoricalCrossentropy(from_logits, label_smoothing) + CategoricalAccuracy + class weights through the
    device-resident path (dense targets are gathered by index_select) against TDL_FUSED_HEAD=0; the bound is
    tests/test_fit_gpu.py's for two f32 evaluation orders of one SGD run (rtol 2e-3, atol 2e-4)."""
    kw = dict(spe=2, dense=True, metrics="dense", class_weight=CW)
    loss = lambda: K.losses.CategoricalCrossentropy(from_logits=True, label_smoothing=0.1)  # noqa: E731
    a = _train(loss=loss(), **kw)
    with _env(TDL_FUSED_HEAD="0"):
        b = _train(loss=loss(), **kw)
    assert a._trainer.kind == "generic" and any(k[0] == "dev" for k in a._trainer._graphs)
    np.testing.assert_allclose(_w(a), _w(b), rtol=2e-3, atol=2e-4)
    for k in a._last_history:
        np.testing.assert_allclose(a._last_history[k], b._last_history[k], rtol=2e-3, atol=2e-4)
    c = _train(loss=loss(), spe=2, dense=True, metrics="dense")
    assert not _same(_w(a), _w(c))


def test_fused_engine_model_falls_back_with_a_reason():
    m = _train(fused=True)
    assert m._trainer.kind == "fused", m._fused_reason
    _train(fused=True, model=m, class_weight=CW)
    assert m._trainer.kind == "generic" and "class_weight" in m._fused_reason
    _, y = _xy()
    m2 = _train(fused=True, sw=_table()[y])
    assert m2._trainer.kind == "generic" and "sample weights" in m2._fused_reason
    assert _same(_w(m2), _w(_train(fused=False, class_weight=CW)))
    m3 = _train(fused=True, loss=K.losses.SparseCategoricalCrossentropy(from_logits=True, label_smoothing=0.1))
    assert m3._trainer.kind == "generic" and "smoothing" in m3._fused_reason
