"""keras.layers.DepthwiseConv2D / SeparableConv2D on the CPU: values against the float64 loops of
tests/depthwise_refs.py, weight names and shapes, output shapes, config round trips, training inside Sequential
and functional models, and that neither layer is a Conv2D (keras/fusion.py matches on that class)."""
import numpy as np
import pytest
import torch

import depthwise_refs as DR
import tensorflow_distributed_learning_amd as tdl

L = tdl.keras.layers
# kernel, strides, dilation, depth multiplier, padding
GEOS = [((3, 3), (2, 2), (1, 1), 1, "same"), ((3, 3), (1, 1), (2, 2), 1, "valid"), ((2, 3), (1, 1), (1, 1), 2, "same")]


def _x(shape=(2, 7, 6, 3)):
    return np.random.default_rng(0).standard_normal(shape).astype(np.float32)


@pytest.mark.parametrize("k,s,d,dm,padding", GEOS)
def test_depthwise_values_names_and_shapes(k, s, d, dm, padding):
    x = _x()
    layer = L.DepthwiseConv2D(k, strides=s, padding=padding, depth_multiplier=dm, dilation_rate=d, activation="relu",
                              bias_initializer="glorot_uniform", name="dw")
    y = layer(torch.from_numpy(x)).detach().numpy()
    assert [(w.name, tuple(w.shape)) for w in layer.weights] == [("dw/depthwise_kernel:0", k + (3, dm)),
                                                                 ("dw/bias:0", (3 * dm,))]
    pads, oh, ow = DR.geometry(x.shape, k, s, d, padding)
    ref, _ = DR.forward(x, layer.depthwise_kernel.numpy(), layer.bias.numpy(), s, d, pads, oh, ow)
    np.testing.assert_allclose(y, np.maximum(ref, 0.0), rtol=1e-5, atol=1e-5)
    assert layer.compute_output_shape((None,) + x.shape[1:]) == (None, oh, ow, 3 * dm)
    assert not isinstance(layer, L.Conv2D)


@pytest.mark.parametrize("k,s,d,dm,padding", GEOS)
def test_separable_values_names_and_shapes(k, s, d, dm, padding):
    x = _x()
    layer = L.SeparableConv2D(5, k, strides=s, padding=padding, depth_multiplier=dm, dilation_rate=d,
                              bias_initializer="glorot_uniform", name="sep")
    y = layer(torch.from_numpy(x)).detach().numpy()
    assert [(w.name, tuple(w.shape)) for w in layer.weights] == [
        ("sep/depthwise_kernel:0", k + (3, dm)), ("sep/pointwise_kernel:0", (1, 1, 3 * dm, 5)), ("sep/bias:0", (5,))]
    pads, oh, ow = DR.geometry(x.shape, k, s, d, padding)
    mid, _ = DR.forward(x, layer.depthwise_kernel.numpy(), None, s, d, pads, oh, ow)
    ref = mid @ layer.pointwise_kernel.numpy()[0, 0].astype(np.float64) + layer.bias.numpy()
    np.testing.assert_allclose(y, ref, rtol=1e-5, atol=1e-5)
    assert layer.compute_output_shape((None,) + x.shape[1:]) == (None, oh, ow, 5)
    assert not isinstance(layer, L.Conv2D)


def test_config_round_trip_and_registry():
    reg = tdl.keras.regularizers.L2(0.5)
    a = L.DepthwiseConv2D((3, 2), strides=2, padding="same", depth_multiplier=2, activation="relu", use_bias=False,
                          depthwise_regularizer=reg, name="a")
    b = L.DepthwiseConv2D.from_config(a.get_config())
    assert b.get_config() == a.get_config() and b.depthwise_regularizer.l2 == 0.5 and b.kernel_size == (3, 2)
    s = L.SeparableConv2D(4, 3, dilation_rate=2, depth_multiplier=3, pointwise_regularizer=reg, name="s")
    t = L.SeparableConv2D.from_config(s.get_config())
    assert t.get_config() == s.get_config() and t.filters == 4 and t.pointwise_regularizer.l2 == 0.5
    assert L.LAYER_CLASSES["DepthwiseConv2D"] is L.DepthwiseConv2D and "SeparableConv2D" in L.__all__
    from tensorflow_distributed_learning_amd.compat import tf

    assert tf.keras.layers.SeparableConv2D is L.SeparableConv2D and tf.keras.layers.DepthwiseConv2D is L.DepthwiseConv2D
    with pytest.raises(ValueError):
        L.DepthwiseConv2D(3, data_format="channels_first")


def _fit(model):
    g = torch.Generator().manual_seed(0)
    x, y = torch.rand(16, 8, 8, 2, generator=g), torch.randint(0, 4, (16,), generator=g)
    model.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                  optimizer=tdl.keras.optimizers.SGD(learning_rate=0.1))
    before = [w.copy() for w in model.get_weights()]
    h = model.fit(x, y, batch_size=8, epochs=2, verbose=0)
    assert np.isfinite(h.history["loss"]).all()
    assert all(not np.array_equal(a, b) for a, b in zip(before, model.get_weights()))


def test_fit_in_sequential_and_functional_models():
    tdl.keras.utils.set_random_seed(1)
    _fit(tdl.keras.Sequential([L.DepthwiseConv2D(3, padding="same", activation="relu", input_shape=(8, 8, 2)),
                               L.SeparableConv2D(6, 3, strides=2), L.GlobalAveragePooling2D(), L.Dense(4)]))
    i = L.Input(shape=(8, 8, 2))
    h = L.SeparableConv2D(6, 3, padding="same", activation="relu")(i)
    h = L.DepthwiseConv2D(3, strides=2, depth_multiplier=2)(h)
    _fit(tdl.keras.Model(i, L.Dense(4)(L.GlobalAveragePooling2D()(h))))
