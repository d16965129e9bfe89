"""keras.layers.LSTM on the CPU against torch.nn.LSTM in float64 (same gate order, transposed weights), the
Orthogonal initializer, and the layer's registration."""
import numpy as np
import pytest
import torch

import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.keras import initializers as I

L = tdl.keras.layers
B, T, D, U = 3, 5, 6, 8


@pytest.mark.parametrize("kw", [dict(), dict(return_sequences=True), dict(return_state=True, go_backwards=True),
                                dict(return_sequences=True, return_state=True, use_bias=False)],
                         ids=["last", "sequences", "state-backwards", "all-no-bias"])
@pytest.mark.parametrize("state", [False, True], ids=["zero-state", "initial-state"])
def test_layer_matches_torch_lstm_in_float64(kw, state):
    g = torch.Generator().manual_seed(1)
    x, h0, c0 = (torch.randn(s, generator=g, dtype=torch.float64).requires_grad_() for s in ((B, T, D), (B, U), (B, U)))
    lay = L.LSTM(U, dtype=torch.float64, **kw)
    lay.build((None, T, D))
    ws = [w.value.detach().double().requires_grad_() for w in lay.weights]
    for v, w in zip(lay.weights, ws):  # the layer computes on these float64 leaves
        v._value, v._leaf = w, None
    out = lay(x, initial_state=[h0, c0] if state else None)
    ref = torch.nn.LSTM(D, U, batch_first=True, bias=lay.use_bias).double()
    with torch.no_grad():
        ref.weight_ih_l0.copy_(ws[0].t()), ref.weight_hh_l0.copy_(ws[1].t())
        if lay.use_bias:
            ref.bias_ih_l0.copy_(ws[2]), ref.bias_hh_l0.zero_()
    xr = x.detach().requires_grad_()
    hr, cr = h0.detach().requires_grad_(), c0.detach().requires_grad_()
    o, (h, c) = ref(xr.flip(1) if lay.go_backwards else xr, (hr[None], cr[None]) if state else None)
    want = [o if lay.return_sequences else o[:, -1]] + ([h[0], c[0]] if lay.return_state else [])
    got = out if isinstance(out, list) else [out]
    assert len(got) == len(want)
    cot = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in want]
    sum((a * b).sum() for a, b in zip(got, cot)).backward()
    sum((a * b).sum() for a, b in zip(want, cot)).backward()
    pairs = list(zip(got, want)) + [(x.grad, xr.grad), (ws[0].grad, ref.weight_ih_l0.grad.t()),
                                    (ws[1].grad, ref.weight_hh_l0.grad.t())]
    pairs += [(ws[2].grad, ref.bias_ih_l0.grad)] if lay.use_bias else []
    pairs += [(h0.grad, hr.grad), (c0.grad, cr.grad)] if state else []
    for a, b in pairs:
        assert a.dtype == torch.float64 and torch.allclose(a, b, rtol=0, atol=1e-12)


def test_unit_forget_bias_and_shapes():
    lay = L.LSTM(U)
    lay.build((None, T, D))
    assert [tuple(w.shape) for w in lay.weights] == [(D, 4 * U), (U, 4 * U), (4 * U,)]
    assert [w.name.split("/")[-1].split(":")[0] for w in lay.weights] == ["kernel", "recurrent_kernel", "bias"]
    b = lay.bias.numpy()
    assert (b[U:2 * U] == 1).all() and (np.delete(b, np.s_[U:2 * U]) == 0).all()
    r = lay.recurrent_kernel.numpy().astype(np.float64)  # orthogonal by default: wide, orthonormal rows
    assert np.abs(r @ r.T - np.eye(U)).max() < 1e-6
    plain = L.LSTM(U, unit_forget_bias=False)
    plain.build((None, T, D))
    assert (plain.bias.numpy() == 0).all()


@pytest.mark.parametrize("shape", [(12, 5), (5, 12), (2, 3, 4)], ids=["tall", "wide", "rank3"])
def test_orthogonal(shape):
    q = I.Orthogonal(gain=2.0, seed=7)(shape)
    assert tuple(q.shape) == shape and torch.equal(q, I.get("orthogonal").__class__(2.0, 7)(shape))
    m = q.double().reshape(-1, shape[-1]) / 2.0
    gram = m.t() @ m if m.shape[0] >= m.shape[1] else m @ m.t()
    assert torch.allclose(gram, torch.eye(gram.shape[0], dtype=torch.float64), atol=1e-6)
    assert not torch.equal(q, I.Orthogonal(gain=2.0, seed=8)(shape))


def test_config_registration_and_refusals():
    lay = L.LSTM(U, return_sequences=True, go_backwards=True, recurrent_regularizer="l2", name="rnn")
    cfg = lay.get_config()
    twin = L.LAYER_CLASSES["LSTM"].from_config(cfg)
    assert twin.get_config() == cfg and cfg["units"] == U and cfg["recurrent_initializer"]["class_name"] == "orthogonal"
    from tensorflow_distributed_learning_amd.compat import tf

    assert "LSTM" in L.__all__ and tf.keras.layers.LSTM is L.LSTM
    for kw in (dict(dropout=0.1), dict(recurrent_dropout=0.1), dict(stateful=True), dict(unroll=True)):
        with pytest.raises(ValueError, match="not implemented"):
            L.LSTM(U, **kw)
    with pytest.raises(ValueError, match="not implemented"):
        L.LSTM(U)(torch.zeros(B, T, D), mask=torch.ones(B, T, dtype=torch.bool))
    with pytest.raises(NotImplementedError):
        L.LSTM(U)(L.Input((T, D)), initial_state=[L.Input((U,)), L.Input((U,))])
    outs = L.LSTM(U, return_sequences=True, return_state=True)(L.Input((T, D)))
    assert [o.shape for o in outs] == [(None, T, U), (None, U), (None, U)]
    y = L.LSTM(U, activation="relu")(torch.ones(B, T, D))  # other activations: the formula
    assert y.shape == (B, U) and (y >= 0).all()
