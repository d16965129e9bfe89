"""MultiHeadAttention's seeded attention dropout on the CPU: the seed and stream rules, the replay, and the formula
path's mask against the numpy stream of tests/attention_dropout_refs.py."""
import numpy as np
import torch

import attention_dropout_refs as DR
import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.ops import attention as A

L = tdl.keras.layers


def test_seed_config_equal_draws_and_replay():
    m, n, x = L.MultiHeadAttention(2, 8, dropout=0.3, seed=11), L.MultiHeadAttention(2, 8, dropout=0.3, seed=11), torch.randn(2, 6, 8)
    cfg = m.get_config()
    assert cfg["seed"] == 11 and L.MultiHeadAttention.from_config(cfg).get_config() == cfg
    first = m(x, x, training=True)
    n(x, x)  # (builds it)
    n.set_weights(m.get_weights())
    assert torch.equal(n(x, x, training=True), first) and not torch.equal(first, m(x, x))
    second = m(x, x, training=True)  # the next ticket: another mask
    assert not torch.equal(second, first) and m.rng_calls() == 2
    m.reset_rng()
    assert torch.equal(m(x, x, training=True), first) and torch.equal(m(x, x, training=True), second)


def test_the_formula_path_draws_the_kernels_mask_and_no_dropout_takes_no_stream_index():
    B, H, T, S, rate = 2, 3, 6, 5, 0.5  # T % 4 = 2: a partial group of rows
    for ticket in (0, 9):
        y, z = A.philox_dropout(rate, DR.KEY, ticket=ticket)(torch.ones(B, H, T, S)), DR.keep_mask(DR.KEY, ticket, rate, B, H, T, S)
        assert np.array_equal(y.numpy(), 2.0 * z) and 0 < z.sum() < z.size
    tdl.keras.backend.clear_session()
    plain, d, drops = L.MultiHeadAttention(2, 8), L.Dropout(0.5), L.MultiHeadAttention(2, 8, dropout=0.1)
    assert plain.get_config()["seed"] is None and (d._rng_stream, drops._rng_stream) == (0, 1)
