"""keras.layers.Embedding on the CPU and the references of tests/embedding_refs.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import embedding_refs as ER
import kernel_refs as R
import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.ops import embedding as EM

L = tdl.keras.layers


def test_the_cpu_layer_is_f_embedding_bit_for_bit_forward_and_gradient():
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 11, (4, 6), generator=g, dtype=torch.int32)
    layer = L.Embedding(11, 8)
    layer(ids)
    table = layer.embeddings.value.detach().clone().requires_grad_()
    want = F.embedding(ids.long(), table)
    assert torch.equal(layer(ids), want) and layer.compute_output_shape((None, 6)) == (None, 6, 8)
    dy = torch.randn(4, 6, 8, generator=g)
    leaf = table.detach().clone().requires_grad_()
    EM.embedding(ids, leaf).backward(dy)  # CPU tensors: the formula path
    want.backward(dy)
    assert torch.equal(leaf.grad, table.grad)
    assert not EM.supported(ids, table) and not EM.supported(ids.float(), table)
    assert not EM.supported(ids, torch.zeros(2, EM.MAX_D + 1))


def test_the_refs_agree_with_an_f64_index_add():
    rng = np.random.default_rng(1)
    ids, dy = rng.integers(-1, 6, 60), rng.standard_normal((60, 5)).astype(np.float32)  # (-1 and 5: outside [0, 5))
    t0 = rng.standard_normal((5, 5)).astype(np.float32)
    ok = (ids >= 0) & (ids < 5)
    ref = torch.zeros(5, 5, dtype=torch.float64).index_add_(0, torch.from_numpy(ids[ok]), torch.from_numpy(dy[ok]).double())
    mag = torch.zeros(5, 5, dtype=torch.float64).index_add_(0, torch.from_numpy(ids[ok]), torch.from_numpy(np.abs(dy[ok])).double())
    # at most 60 additions, each within one ulp of a partial sum no larger than sum |dy| (+ |target|)
    for target in (None, t0):
        want = ref.numpy() + (0 if target is None else target.astype(np.float64))
        bound = 61 * R.ulp32(mag.numpy() + (0 if target is None else np.abs(target)))
        assert (np.abs(ER.fold_ref(ids, dy, 5, target) - want) <= bound).all()
    table = rng.standard_normal((5, 5)).astype(np.float32)
    y = ER.gather_ref(ids, table)
    assert np.array_equal(y[ok], table[ids[ok]]) and not y[~ok].any() and (~ok).any()
    assert np.array_equal(ER.gather_ref(ids, table, bf16=True), R.bf16_rne(y))


def test_mask_zero_raises_and_the_config_round_trips():
    with pytest.raises(NotImplementedError):
        L.Embedding(5, 4, mask_zero=True)
    cfg = L.Embedding(5, 4, embeddings_initializer="zeros", embeddings_regularizer=tdl.keras.regularizers.L1L2(l2=0.01),
                      input_length=7, name="emb").get_config()
    assert L.Embedding.from_config(cfg).get_config() == cfg
    assert cfg["input_dim"] == 5 and cfg["output_dim"] == 4 and cfg["input_length"] == 7 and cfg["mask_zero"] is False
    assert "embeddings_regularizer" not in L.Embedding(5, 4).get_config()
