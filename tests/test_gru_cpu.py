"""keras.layers.GRU on the CPU against torch.nn.GRU in float64 (torch's gate order is r, z, n: the column blocks are
permuted; bias row 0 is bias_ih, row 1 bias_hh), reset_after=False against a written-out loop, and the layer's
registration."""
import pytest
import torch

import tensorflow_distributed_learning_amd as tdl

L = tdl.keras.layers
B, T, D, U = 3, 5, 6, 8


def _layer(**kw):
    """A built float64 layer computing on float64 leaves, with non-zero biases."""
    lay = L.GRU(U, dtype=torch.float64, bias_initializer="glorot_uniform", **kw)
    lay.build((None, T, D))
    ws = [w.value.detach().double().requires_grad_() for w in lay.weights]
    for v, w in zip(lay.weights, ws):
        v._value, v._leaf = w, None
    return lay, ws


def _rzn(w):  # column blocks z, r, h -> rows r, z, n of torch's transposed weights
    z, r, h = w.split(U, dim=-1)
    return torch.cat([r, z, h], -1).t() if w.dim() == 2 else torch.cat([r, z, h], -1)


@pytest.mark.parametrize("kw", [dict(), dict(return_sequences=True), dict(return_state=True, go_backwards=True),
                                dict(return_sequences=True, return_state=True, use_bias=False)],
                         ids=["last", "sequences", "state-backwards", "all-no-bias"])
@pytest.mark.parametrize("state", [False, True], ids=["zero-state", "initial-state"])
def test_layer_matches_torch_gru_in_float64(kw, state):
    g = torch.Generator().manual_seed(1)
    x, h0 = (torch.randn(s, generator=g, dtype=torch.float64).requires_grad_() for s in ((B, T, D), (B, U)))
    lay, ws = _layer(**kw)
    out = lay(x, initial_state=[h0] if state else None)
    ref = torch.nn.GRU(D, U, batch_first=True, bias=lay.use_bias).double()
    with torch.no_grad():
        ref.weight_ih_l0.copy_(_rzn(ws[0])), ref.weight_hh_l0.copy_(_rzn(ws[1]))
        if lay.use_bias:
            ref.bias_ih_l0.copy_(_rzn(ws[2][0])), ref.bias_hh_l0.copy_(_rzn(ws[2][1]))
    xr, hr = x.detach().requires_grad_(), h0.detach().requires_grad_()
    o, h = ref(xr.flip(1) if lay.go_backwards else xr, hr[None] if state else None)
    want = [o if lay.return_sequences else o[:, -1]] + ([h[0]] if lay.return_state else [])
    got = out if isinstance(out, list) else [out]
    assert len(got) == len(want)
    cot = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in want]
    sum((a * b).sum() for a, b in zip(got, cot)).backward()
    sum((a * b).sum() for a, b in zip(want, cot)).backward()
    pairs = list(zip(got, want)) + [(x.grad, xr.grad), (_rzn(ws[0].grad), ref.weight_ih_l0.grad),
                                    (_rzn(ws[1].grad), ref.weight_hh_l0.grad)]
    if lay.use_bias:
        pairs += [(_rzn(ws[2].grad[0]), ref.bias_ih_l0.grad), (_rzn(ws[2].grad[1]), ref.bias_hh_l0.grad)]
    pairs += [(h0.grad, hr.grad)] if state else []
    for a, b in pairs:
        assert a.dtype == torch.float64 and torch.allclose(a, b, rtol=0, atol=1e-12)


@pytest.mark.parametrize("kw", [dict(), dict(return_sequences=True, go_backwards=True, use_bias=False)])
def test_reset_before_matches_a_written_out_loop(kw):
    g = torch.Generator().manual_seed(2)
    x, h = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((B, T, D), (B, U)))
    lay, ws = _layer(reset_after=False, **kw)
    assert not lay.use_bias or tuple(lay.bias.shape) == (3 * U,)
    got = lay(x, initial_state=h)
    W, R, b = ws[0], ws[1], (ws[2] if lay.use_bias else torch.zeros(3 * U, dtype=torch.float64))
    hs = []
    for t in (range(T - 1, -1, -1) if lay.go_backwards else range(T)):
        m = x[:, t] @ W + b
        z = torch.sigmoid(m[:, :U] + h @ R[:, :U])
        r = torch.sigmoid(m[:, U:2 * U] + h @ R[:, U:2 * U])
        h = z * h + (1 - z) * torch.tanh(m[:, 2 * U:] + (r * h) @ R[:, 2 * U:])
        hs.append(h)
    assert torch.allclose(got, torch.stack(hs, 1) if lay.return_sequences else h, rtol=0, atol=1e-12)


def test_weights_config_registration_and_refusals():
    lay = L.GRU(U, return_sequences=True, go_backwards=True, recurrent_regularizer="l2", name="rnn")
    lay.build((None, T, D))
    assert [tuple(w.shape) for w in lay.weights] == [(D, 3 * U), (U, 3 * U), (2, 3 * U)]
    assert [w.name.split("/")[-1].split(":")[0] for w in lay.weights] == ["kernel", "recurrent_kernel", "bias"]
    cfg = lay.get_config()
    twin = L.LAYER_CLASSES["GRU"].from_config(cfg)
    assert twin.get_config() == cfg and cfg["units"] == U and cfg["reset_after"] is True
    from tensorflow_distributed_learning_amd.compat import tf

    assert "GRU" in L.__all__ and tf.keras.layers.GRU is L.GRU
    for kw in (dict(dropout=0.1), dict(recurrent_dropout=0.1), dict(stateful=True), dict(unroll=True)):
        with pytest.raises(ValueError, match="not implemented"):
            L.GRU(U, **kw)
    with pytest.raises(ValueError, match="not implemented"):
        L.GRU(U)(torch.zeros(B, T, D), mask=torch.ones(B, T, dtype=torch.bool))
    with pytest.raises(NotImplementedError):
        L.GRU(U)(L.Input((T, D)), initial_state=[L.Input((U,))])
    outs = L.GRU(U, return_sequences=True, return_state=True)(L.Input((T, D)))
    assert [o.shape for o in outs] == [(None, T, U), (None, U)]
    y = L.GRU(U, activation="relu")(torch.ones(B, T, D))  # other activations: the formula
    assert y.shape == (B, U) and (y >= 0).all()
