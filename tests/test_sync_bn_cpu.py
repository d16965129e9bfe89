"""Synchronized batch normalization across replicas on the CPU path (ops/batchnorm.py, PyTorch ops with
float64 sums through the communicator): two replicas whose local batches come from visibly different
distributions train like one replica on the global batch -- and do NOT when the layer is not
synchronized (the control that shows the comparison can fail)."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import tensorflow_distributed_learning_amd as tdl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-4, 1e-6


def _miss(a, b):
    """How far a misses assert_allclose(a, b, RTOL, ATOL): max |a - b| / (ATOL + RTOL |b|) (<= 1 passes)."""
    return float(np.max(np.abs(a - b) / (ATOL + RTOL * np.abs(b))))


def _data():
    """24 samples = 3 global batches of 8; the second half of every batch (the second replica's
    share) is shifted by +3."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(24, 6, 6, 2, generator=g)
    x[(torch.arange(24) % 8) >= 4] += 3.0
    y = torch.randint(0, 3, (24,), generator=g)
    return x, y


def _model(sync):
    L = tdl.keras.layers
    return tdl.keras.Sequential([
        L.Conv2D(4, 3, input_shape=(6, 6, 2)), L.BatchNormalization(synchronized=sync), L.ReLU(), L.Flatten(),
        L.Dense(3)])


def _train(strategy, sync):
    x, y = _data()
    tdl.keras.utils.set_random_seed(11)
    ds = tdl.data.Dataset.from_tensor_slices((x, y)).batch(8)
    with strategy.scope():
        m = _model(sync)
        m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                  optimizer=tdl.keras.optimizers.SGD(learning_rate=0.1))
    m.fit(ds, epochs=1, verbose=0)  # three SGD steps
    return m


def _flat(m):
    return np.concatenate([w.ravel() for w in m.get_weights()]).astype(np.float64)


def test_single_process_two_cpu_replicas_match_one_replica():
    one = _flat(_train(tdl.distribute.MirroredStrategy(devices=["/cpu:0"]), True))
    s = tdl.distribute.MirroredStrategy(devices=["/cpu:0", "/cpu:1"])
    m = _train(s, True)
    for a, b in zip(m.get_weights(), m._local_clones[0].get_weights()):
        assert np.array_equal(a, b), "replicas differ"
    for v0, v1 in zip(m.non_trainable_weights, m._local_clones[0].non_trainable_weights):
        assert torch.equal(v0._value, v1._value), "moving statistics differ between replicas"
    np.testing.assert_allclose(_flat(m), one, rtol=RTOL, atol=ATOL)
    s.shutdown()
    # control: per-replica statistics on the same data are a different model
    s = tdl.distribute.MirroredStrategy(devices=["/cpu:0", "/cpu:1"])
    miss = _miss(_flat(_train(s, False)), one)
    s.shutdown()
    assert miss >= 10.0, miss


BODY = """
import os, sys, numpy as np, torch
sys.path.insert(0, os.path.join(sys.argv[2], "tests"))
import tensorflow_distributed_learning_amd as tdl
from test_sync_bn_cpu import _train
strategy = tdl.distribute.MirroredStrategy()
R, rank = strategy.num_replicas_in_sync, strategy.extended.rank
sync = os.environ["SYNC"] == "1"
m = _train(strategy, sync)
w = np.concatenate([v.ravel() for v in m.get_weights()])
local = np.concatenate([v._value.numpy().ravel() for v in m.non_trainable_weights])
np.save(os.path.join(sys.argv[1], f"w{rank}_{R}_{int(sync)}.npy"), w)
np.save(os.path.join(sys.argv[1], f"nt{rank}_{R}_{int(sync)}.npy"), local)
"""


def _launch(tmp_path, n, sync):
    script = tmp_path / "job.py"
    script.write_text(textwrap.dedent(BODY))
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="",
               TDL_NO_GPU_PARTITION="1", SYNC="1" if sync else "0")
    for k in ("TF_CONFIG", "RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
              "TDL_LAUNCHED"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "tensorflow_distributed_learning_amd.launch", "--nproc-per-node", str(n),
                        str(script), str(tmp_path), ROOT], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.slow
def test_two_processes_match_one_replica(tmp_path):
    _launch(tmp_path, 1, True)
    _launch(tmp_path, 2, True)
    _launch(tmp_path, 2, False)
    one = np.load(tmp_path / "w0_1_1.npy").astype(np.float64)
    w0, w1 = np.load(tmp_path / "w0_2_1.npy"), np.load(tmp_path / "w1_2_1.npy")
    assert np.array_equal(w0, w1), "replicas differ"
    # each replica's own moving statistics (not their ON_READ mean): the same bits everywhere
    assert np.array_equal(np.load(tmp_path / "nt0_2_1.npy"), np.load(tmp_path / "nt1_2_1.npy"))
    np.testing.assert_allclose(w0.astype(np.float64), one, rtol=RTOL, atol=ATOL)
    assert _miss(np.load(tmp_path / "w0_2_0.npy").astype(np.float64), one) >= 10.0


def test_sync_layer_aliases_and_config_round_trip():
    from tensorflow_distributed_learning_amd.compat import tf

    L = tdl.keras.layers
    plain = L.BatchNormalization(momentum=0.9, name="bn")
    assert plain.get_config() == {"name": "bn", "trainable": True, "axis": -1, "momentum": 0.9, "epsilon": 1e-3,
                                  "center": True, "scale": True}
    assert not plain.synchronized
    for cls in (L.SyncBatchNormalization, L.experimental.SyncBatchNormalization,
                tf.keras.layers.SyncBatchNormalization, tf.keras.layers.experimental.SyncBatchNormalization):
        layer = cls(momentum=0.8)
        assert isinstance(layer, L.BatchNormalization) and layer.synchronized
    flagged = tf.keras.layers.BatchNormalization(synchronized=True, epsilon=1e-4)
    cfg = flagged.get_config()
    assert cfg["synchronized"] is True
    again = L.BatchNormalization.from_config(cfg)
    assert again.synchronized and again.epsilon == 1e-4 and again.get_config() == cfg
    m = _model(True)
    m2 = tdl.keras.models.model_from_config(m.get_config_full())
    assert [l.synchronized for l in m2.layers if isinstance(l, L.BatchNormalization)] == [True]
    m3 = tdl.keras.models.model_from_config(_model(False).get_config_full())
    assert [l.synchronized for l in m3.layers if isinstance(l, L.BatchNormalization)] == [False]


def test_single_replica_sync_layer_takes_the_plain_path():
    """One replica: a synchronized layer is an ordinary one (no collective is issued)."""
    from tensorflow_distributed_learning_amd.ops import batchnorm as _bn

    before = _bn.SYNC_EXCHANGES[0]
    a = _flat(_train(tdl.distribute.MirroredStrategy(devices=["/cpu:0"]), True))
    b = _flat(_train(tdl.distribute.MirroredStrategy(devices=["/cpu:0"]), False))
    assert _bn.SYNC_EXCHANGES[0] == before and np.array_equal(a, b)
