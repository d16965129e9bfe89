"""``fit(class_weight=...)``, sample weights, sparse label smoothing and the loss config without a GPU: class
weights reach the loss (all-zero weights freeze the model), a class-weight dict is the equivalent sample-weight
column, sparse smoothing is CategoricalCrossentropy on one-hot targets, bad keys raise, and the loss config
survives ``compile_from_config``, also on the clones of a two-device single-process MirroredStrategy."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tensorflow_distributed_learning_amd as tdl

from test_accum_cpu import _cnn, _data

K = tdl.keras
O = K.optimizers


def _fit(x, y, steps=4, B=16, loss=None, strategy=None, metrics=True, **fit_kw):
    """``steps`` SGD steps over consecutive batches of B (no shuffle); returns (model, weights before, after)."""
    K.backend.clear_session()
    K.utils.set_random_seed(7)
    strategy = strategy or tdl.distribute.MirroredStrategy(devices=["/cpu:0"])
    with strategy.scope():
        model = _cnn()
        model.compile(loss=loss or K.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=O.SGD(0.05),
                      metrics=[K.metrics.SparseCategoricalAccuracy()] if metrics else None)
    w0 = [w.copy() for w in model.get_weights()]
    n = steps * B
    h = model.fit(x[:n], y[:n], batch_size=B, epochs=1, shuffle=False, verbose=0, **fit_kw)
    return model, w0, model.get_weights(), h


def _same(a, b):
    return all(np.array_equal(np.asarray(p).view(np.int32), np.asarray(q).view(np.int32)) for p, q in zip(a, b))


def test_all_zero_class_weights_freeze_the_model():
    """Fails while fit drops class_weight: every row weighs 0, so SGD must not move a weight."""
    x, y = _data(64)
    _, w0, w1, h = _fit(x, y, class_weight={c: 0.0 for c in range(10)})
    assert _same(w0, w1), "class_weight was ignored: the weights moved"
    assert h.history["loss"][-1] == 0.0
    _, w0, w1, _ = _fit(x, y)
    assert not _same(w0, w1), "the unweighted run must train (the test bites)"


def test_class_weight_is_the_equivalent_sample_weight():
    x, y = _data(64)
    cw = {0: 0.25, 3: 4.0, 7: 0.0, 9: 1.5}
    table = np.ones(10, dtype=np.float32)
    for c, w in cw.items():
        table[c] = w
    sw = torch.from_numpy(table)[y]
    _, _, wc, hc = _fit(x, y, class_weight=cw)
    _, _, ws, hs = _fit(x, y, sample_weight=sw)
    _, _, wu, _ = _fit(x, y)
    assert _same(wc, ws) and not _same(wc, wu)
    assert hc.history == hs.history  # (loss and the weighted accuracy, too)


def test_class_weight_multiplies_a_sample_weight_column():
    x, y = _data(64)
    sw = torch.rand(64, generator=torch.Generator().manual_seed(1)) + 0.5
    table = torch.ones(10)
    table[2], table[5] = 3.0, 0.5
    _, _, wa, _ = _fit(x, y, class_weight={2: 3.0, 5: 0.5}, sample_weight=sw)
    _, _, wb, _ = _fit(x, y, sample_weight=sw * table[y])
    assert _same(wa, wb)


def test_sparse_label_smoothing_is_categorical_crossentropy_on_one_hot_targets():
    g = torch.Generator().manual_seed(2)
    z = torch.randn(33, 10, generator=g) * 3
    y = torch.randint(0, 10, (33,), generator=g)
    for eps in (0.0, 0.1, 0.5):
        sp = K.losses.SparseCategoricalCrossentropy(from_logits=True, label_smoothing=eps).per_example(y, z)
        cc = K.losses.CategoricalCrossentropy(from_logits=True, label_smoothing=eps).per_example(
            F.one_hot(y, 10).float(), z)
        ref = F.cross_entropy(z.double(), y, reduction="none", label_smoothing=eps)
        # both are f32 evaluations of the same sum of 10 terms of magnitude <= |log p| ~ 20: 1e-5 is ~10 f32 ulp of it
        torch.testing.assert_close(sp, cc, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(sp.double(), ref, rtol=1e-5, atol=1e-5)
    assert K.losses.SparseCategoricalCrossentropy().label_smoothing == 0.0
    # the default is what it was: the plain cross-entropy
    torch.testing.assert_close(K.losses.SparseCategoricalCrossentropy(from_logits=True).per_example(y, z),
                               F.cross_entropy(z, y, reduction="none"), rtol=0, atol=0)


def test_a_smoothed_sparse_fit_is_the_smoothed_one_hot_fit():
    x, y = _data(64)
    _, _, ws, _ = _fit(x, y, loss=K.losses.SparseCategoricalCrossentropy(from_logits=True, label_smoothing=0.1))
    _, _, wc, _ = _fit(x, F.one_hot(y, 10).float(), metrics=False,
                       loss=K.losses.CategoricalCrossentropy(from_logits=True, label_smoothing=0.1))
    _, _, wu, _ = _fit(x, y)
    for a, b, u in zip(ws, wc, wu):  # two f32 formulas of one gradient, 4 SGD steps at lr 0.05
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-6)
    assert not _same(ws, wu)


@pytest.mark.parametrize("bad", [{-1: 1.0}, {10: 1.0}, {1.5: 2.0}, {"3": 1.0}, {True: 1.0}, [1.0] * 10])
def test_bad_class_weight_keys_raise_value_error(bad):
    x, y = _data(32)
    with pytest.raises(ValueError):
        _fit(x, y, steps=2, class_weight=bad)


def test_missing_classes_weigh_one_and_numpy_integer_keys_are_accepted():
    K.backend.clear_session()
    m = _cnn()
    t = m._class_weight_table({np.int64(3): 2.0, 9: 0.5})
    assert t.dtype == torch.float32 and t.tolist() == [1, 1, 1, 2, 1, 1, 1, 1, 1, 0.5]
    assert m._class_weight_table(None) is None


@pytest.mark.parametrize("make", [
    lambda: K.losses.SparseCategoricalCrossentropy(from_logits=True, label_smoothing=0.1),
    lambda: K.losses.SparseCategoricalCrossentropy(from_logits=True, ignore_class=3),
    lambda: K.losses.CategoricalCrossentropy(from_logits=True, label_smoothing=0.2),
    lambda: K.losses.CategoricalCrossentropy(),
], ids=["sparse-smoothed", "sparse-ignore", "dense-logits-smoothed", "dense-default"])
def test_loss_config_survives_compile_from_config(make):
    K.backend.clear_session()
    a, b = _cnn(), _cnn()
    a.compile(loss=make(), optimizer=O.SGD(0.05))
    cfg = a.loss.get_config()
    assert {"from_logits", "label_smoothing", "ignore_class"} <= set(cfg)
    b.compile_from_config(a._compile_config)
    assert type(b.loss) is type(a.loss)
    assert b.loss.from_logits == a.loss.from_logits and b.loss.label_smoothing == a.loss.label_smoothing
    assert getattr(b.loss, "ignore_class", None) == getattr(a.loss, "ignore_class", None)


def test_weighted_metrics_are_appended_to_the_compiled_metrics():
    K.backend.clear_session()
    m = _cnn()
    m.compile(loss=K.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=O.SGD(0.05),
              metrics=["accuracy"], weighted_metrics=[K.metrics.SparseTopKCategoricalAccuracy(k=2)])
    assert [type(x).__name__ for x in m.compiled_metrics] == ["SparseCategoricalAccuracy",
                                                             "SparseTopKCategoricalAccuracy"]


def test_two_cpu_replicas_in_one_process_keep_the_loss_config_and_honour_class_weight():
    x, y = _data(64)
    two = lambda: tdl.distribute.MirroredStrategy(devices=["/cpu:0", "/cpu:1"])  # noqa: E731
    loss = lambda: K.losses.CategoricalCrossentropy(from_logits=True, label_smoothing=0.1)  # noqa: E731
    t = F.one_hot(y, 10).float()
    m, w0, w1, _ = _fit(x, t, loss=loss(), strategy=two(), metrics=False, class_weight={c: 0.0 for c in range(10)})
    assert getattr(m._trainer, "is_group", False) and len(m._local_clones) == 1
    c = m._local_clones[0]
    assert type(c.loss) is K.losses.CategoricalCrossentropy and c.loss.from_logits and c.loss.label_smoothing == 0.1
    assert _same(w0, w1), "a replica ignored class_weight"
    # and a real table trains both replicas like one replica on the whole batch (two summation orders of the mean)
    cw = {1: 2.0, 4: 0.25}
    _, _, wg, _ = _fit(x, t, loss=loss(), strategy=two(), metrics=False, class_weight=cw)
    _, _, ws, _ = _fit(x, t, loss=loss(), metrics=False, class_weight=cw)
    _, _, wu, _ = _fit(x, t, loss=loss(), metrics=False)
    for a, b in zip(wg, ws):
        np.testing.assert_allclose(a, b, rtol=2e-3, atol=2e-4)  # (tests/test_fit_gpu.py's bound for two f32 orders)
    assert not _same(ws, wu)
