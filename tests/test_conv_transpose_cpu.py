"""Conv2DTranspose without a GPU: the layer's size rules and its CPU path (the full F.conv_transpose2d, zero-extended
and cropped) against the float64 scatter-form references of tests/convt_refs.py."""
import numpy as np
import pytest
import torch

import convt_refs as TR
import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.ops import conv_transpose as CT


def _data(case, seed=5):
    shape, F, k, s, d, padding, op, act = case
    geo = TR.geometry(shape, k, s, d, padding, op)
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape), rng.standard_normal(k + (F, shape[3])), rng.standard_normal(F),
            rng.standard_normal((shape[0], geo[0], geo[1], F)), geo)


@pytest.mark.parametrize("case", TR.CASES, ids=TR.IDS)
def test_layer_shape_and_cpu_path_match_the_scatter_form(case):
    shape, F, k, s, d, padding, op, act = case
    x, w, b, _, geo = _data(case)
    tdl.keras.backend.clear_session()
    layer = tdl.keras.layers.Conv2DTranspose(F, k, strides=s, padding=padding, output_padding=op, dilation_rate=d,
                                             activation="relu" if act else None)
    assert layer.compute_output_shape(shape) == (shape[0], geo[0], geo[1], F)
    y = layer(torch.from_numpy(x).float())
    assert tuple(layer.kernel.value.shape) == k + (F, shape[3]) and tuple(y.shape) == (shape[0], geo[0], geo[1], F)
    ref, _ = TR.forward(x, w, b, s, d, geo)
    got = CT.conv2d_transpose(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), s, padding, op, d, act=act)
    torch.testing.assert_close(got.float(), torch.from_numpy(np.maximum(ref, 0) if act else ref).float())


@pytest.mark.parametrize("case", [TR.CASES[4], TR.CASES[6]], ids=[TR.IDS[4], TR.IDS[6]])
def test_cpu_path_gradients(case):
    shape, F, k, s, d, padding, op, act = case
    x, w, b, dy, geo = _data(case)
    xt, wt, bt = (torch.from_numpy(v).requires_grad_() for v in (x, w, b))
    y = CT.conv2d_transpose(xt, wt, bt, s, padding, op, d, act=act)
    y.backward(torch.from_numpy(dy))
    dy_eff = dy * (y.detach().numpy() > 0) if act else dy
    rw, _, rb, _ = TR.wgrad(x, dy_eff, k, s, d, geo)
    for got, ref in ((xt.grad, TR.dgrad(dy_eff, w, shape, s, d, geo)[0]), (wt.grad, rw), (bt.grad, rb)):
        torch.testing.assert_close(got.float(), torch.from_numpy(ref).float())


def test_config_round_trip_and_refusals():
    L = tdl.keras.layers
    tdl.keras.backend.clear_session()
    layer = L.Conv2DTranspose(6, (3, 2), strides=(2, 3), padding="same", output_padding=(1, 2), dilation_rate=(2, 1),
                              activation="relu", use_bias=False)
    twin = L.LAYER_CLASSES["Conv2DTranspose"].from_config(layer.get_config())
    assert twin.get_config() == layer.get_config() and twin.output_padding == (1, 2)
    assert twin.compute_output_shape((2, 5, 7, 3)) == layer.compute_output_shape((2, 5, 7, 3)) == (2, 10, 20, 6)
    assert L.Convolution2DTranspose is L.Conv2DTranspose and "Conv2DTranspose" in L.__all__
    with pytest.raises(ValueError):
        L.Conv2DTranspose(4, 3, strides=2, output_padding=2)
    with pytest.raises(ValueError):
        L.Conv2DTranspose(4, 3, data_format="channels_first")
