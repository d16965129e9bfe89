"""keras.layers.MultiHeadAttention on the CPU (the counted torch-formula path): weights, output against the float64
formula, scores and dropout, config, and each limit of supported()."""
import numpy as np
import pytest
import torch

import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.ops import attention as A
from tensorflow_distributed_learning_amd.ops import hip

import attention_refs as AR

L = tdl.keras.layers


@pytest.mark.parametrize("kind", ["self", "cross", "causal", "empty_row"])
def test_layer_matches_the_f64_formula(kind):
    tdl.keras.utils.set_random_seed(1)
    g = torch.Generator().manual_seed(2)
    x, y, z = torch.randn(2, 6, 12, generator=g), torch.randn(2, 9, 10, generator=g), torch.randn(2, 9, 7, generator=g)
    m = L.MultiHeadAttention(3, 8, value_dim=16, output_shape=5, bias_initializer="random_normal", name="mha")
    before, mask, (qi, vi, ki) = dict(A.CALLS), None, ((x, y, z) if kind == "cross" else (x, x, x))
    if kind == "empty_row":
        mask = (torch.rand(2, 6, 6, generator=g) < 0.6).to(torch.uint8)
        mask[1, 4] = 0
    out = m(qi, vi, key=ki if kind == "cross" else None, attention_mask=mask, use_causal_mask=kind == "causal")
    assert A.CALLS == dict(before, torch=before["torch"] + 1)  # no device counter moved
    assert [(v.name, tuple(v.shape)) for v in m.weights] == [
        ("mha/query/kernel:0", (12, 3, 8)), ("mha/query/bias:0", (3, 8)), ("mha/key/kernel:0", (ki.shape[2], 3, 8)),
        ("mha/key/bias:0", (3, 8)), ("mha/value/kernel:0", (vi.shape[2], 3, 16)), ("mha/value/bias:0", (3, 16)),
        ("mha/attention_output/kernel:0", (3, 16, 5)), ("mha/attention_output/bias:0", (5,))]
    adm = AR.admitted(2, 3, 6, ki.shape[1], kind == "causal", None if mask is None else mask.numpy())
    ref = AR.layer([np.asarray(w, np.float64) for w in m.get_weights()], *(t.double().numpy() for t in (qi, vi, ki)),
                   lambda q, k, v: AR.forward(q, k, v, 8 ** -0.5, adm)[0])
    np.testing.assert_allclose(out.detach().numpy(), ref, rtol=1e-4, atol=1e-5)
    if kind == "empty_row":  # no admitted key: the output bias alone
        np.testing.assert_array_equal(out.detach().numpy()[1, 4], m.get_weights()[7])


def test_scores_dropout_and_config():
    from tensorflow_distributed_learning_amd.compat import tf

    assert tf.keras.layers.MultiHeadAttention is L.LAYER_CLASSES["MultiHeadAttention"]
    m = L.MultiHeadAttention(4, 16, value_dim=8, dropout=0.5, use_bias=False, output_shape=(32,), name="att",
                             kernel_regularizer=tdl.keras.regularizers.l2(0.01))
    cfg = m.get_config()
    assert L.MultiHeadAttention.from_config(cfg).get_config() == cfg and cfg["output_shape"] == 32
    assert "kernel_regularizer" in cfg
    with pytest.raises(ValueError):
        L.MultiHeadAttention(2, 8, attention_axes=(1,))
    a, b = torch.randn(3, 5, 8), torch.randn(3, 7, 8)
    res = m(a, b, return_attention_scores=True)  # inference: no dropout; the scores are the probabilities
    out, scores = res
    assert isinstance(res, tuple) and scores.shape == (3, 4, 5, 7)
    torch.testing.assert_close(scores.sum(dim=3), torch.ones(3, 4, 5))
    torch.testing.assert_close(out, m(a, b))
    torch.manual_seed(0)
    dropped = m(a, b, training=True)  # attention dropout: another function of the same shape
    assert dropped.shape == out.shape and not torch.allclose(dropped, out)


@pytest.mark.parametrize("why", ["D=12", "D=136", "mixed dtypes", "strided innermost axis", "row stride off 16 bytes"])
def test_supported_refuses_each_limit_and_so_does_the_binding(why):
    q, k, v = torch.zeros(2, 5, 3, 16), torch.zeros(2, 7, 3, 16), torch.zeros(2, 7, 3, 16)
    assert A.limits_ok(q, k, v) and A.limits_ok(q, k, v, torch.ones(2, 5, 7, dtype=torch.bool))  # the control
    assert A.limits_ok(*torch.zeros(3, 2, 5, 3, 16).unbind(0)) and not A.supported(q, k, v)  # (views; a CPU tensor)
    if why in ("D=12", "D=136"):
        d = int(why[2:])
        q, k = torch.zeros(2, 5, 3, d), torch.zeros(2, 7, 3, d)
        assert hip().attn_plan(2, 3, 5, 7, 16, 16, False, False)["head_pad"] == 32  # the control
        with pytest.raises(RuntimeError, match="limits"):
            hip().attn_plan(2, 3, 5, 7, d, 16, False, False)
    elif why == "mixed dtypes":
        k = k.bfloat16()
    elif why == "strided innermost axis":
        q = torch.zeros(2, 5, 3, 32)[..., ::2]
    else:
        q = torch.zeros(2, 5, 3, 18)[..., :16]
    assert not A.limits_ok(q, k, v)
