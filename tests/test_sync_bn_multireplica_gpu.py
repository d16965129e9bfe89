"""Synchronized batch normalization with REAL peer replica processes sharing the box's GPU: the
statistics exchanges of the HIP kernels (csrc/kernels/bn.hip) ride the xGMI all-reduce kernel inside the
captured whole-step graph, next to the gradient buckets on the side stream.  Two replicas whose local
batches come from different distributions must train like ONE replica on the global batch, f32 and
mixed_bfloat16 -- and must not when the layers are not synchronized (the control)."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

LR = 0.05
BODY = """
import json, os, sys, numpy as np, torch
import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.ops import batchnorm as BN
out = sys.argv[1]
sync = os.environ["SYNC"] == "1"
strategy = tdl.distribute.MirroredStrategy()
R, rank = strategy.num_replicas_in_sync, strategy.extended.rank
comm = strategy.extended.communicator
g = torch.Generator().manual_seed(0)
x = torch.randn(24, 16, 16, 8, generator=g)
x[(torch.arange(24) % 8) >= 4] += 3.0   # the second replica's half of every global batch of 8
y = torch.randint(0, 4, (24,), generator=g)
L = tdl.keras.layers
res = {}
for policy in ("float32", "mixed_bfloat16"):
    tdl.keras.mixed_precision.set_global_policy(policy)
    tdl.keras.utils.set_random_seed(3)
    ds = tdl.data.Dataset.from_tensor_slices((x, y)).batch(8).repeat()
    with strategy.scope():
        inp = L.Input(shape=(16, 16, 8))
        a = L.ReLU()(L.BatchNormalization(momentum=0.5, synchronized=sync)(L.Conv2D(16, 3, padding="same")(inp)))
        b = L.BatchNormalization(momentum=0.5, synchronized=sync)(L.Conv2D(16, 3, padding="same")(a))
        h = L.GlobalAveragePooling2D()(L.ReLU()(L.Add()([b, a])))
        m = tdl.keras.Model(inp, L.Dense(4)(h))
        m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                  optimizer=tdl.keras.optimizers.SGD(learning_rate=@LR@), bucket_bytes=4096)
    before = BN.SYNC_EXCHANGES[0]
    m.fit(ds, epochs=1, steps_per_epoch=3, verbose=0)   # three executions: eager, captured + replayed, replayed
    tr = m._trainer
    w = np.concatenate([v.ravel() for v in m.get_weights()]).astype(np.float64)
    np.save(os.path.join(out, f"w_{policy}_{rank}_{R}_{int(sync)}.npy"), w)
    local = np.concatenate([v._value.detach().cpu().numpy().ravel() for v in m.non_trainable_weights])
    np.save(os.path.join(out, f"nt_{policy}_{rank}_{R}_{int(sync)}.npy"), local)
    res[policy] = {"engine": tr.kind, "algorithm": getattr(comm, "algorithm", comm.name),
                   "graph": len(tr._graphs) >= 1 and tr._graph_ok is True, "bucketed": tr._buckets is not None,
                   "exchanges": BN.SYNC_EXCHANGES[0] - before, "sync_sizes": list(getattr(tr, "_sync_bn_sizes", []))}
json.dump(res, open(os.path.join(out, f"r{rank}_{R}_{int(sync)}.json"), "w"))
""".replace("@LR@", str(LR))


def _run(d, n, sync):
    s = d / "job.py"
    s.write_text(textwrap.dedent(BODY))
    env = dict(os.environ, PYTHONPATH=ROOT, TDL_SHARE_GPU="1", SYNC="1" if sync else "0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "TF_CONFIG", "TDL_LAUNCHED", "MASTER_ADDR",
              "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "tensorflow_distributed_learning_amd.launch", "--nproc-per-node", str(n),
                        str(s), str(d)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "capture failed" not in r.stderr, r.stderr[-3000:]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The three launches every test below reads: one replica, two synchronized, two not."""
    d = tmp_path_factory.mktemp("syncbn")
    _run(d, 1, True)
    _run(d, 2, True)
    _run(d, 2, False)
    return d


def _w(d, policy, rank, R, sync, kind="w"):
    return np.load(d / f"{kind}_{policy}_{rank}_{R}_{int(sync)}.npy")


# f32: the project's R=2-vs-R=1 bound (tests/test_multiproc_gpu.py).  bf16: the BN kernels' bf16 gradient
# tolerance (tests/test_bn_gpu.py: atol 6e-2, rtol 3e-2), a gradient error reaching a weight times lr
BOUNDS = {"float32": (1e-3, 1e-5), "mixed_bfloat16": (3e-2, 6e-2 * LR)}


def _miss(a, b, rtol, atol):
    return float(np.max(np.abs(a - b) / (atol + rtol * np.abs(b))))


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
def test_two_synchronized_replicas_train_like_one(runs, policy):
    res = [json.load(open(runs / f"r{i}_2_1.json"))[policy] for i in range(2)]
    for r in res:
        assert r["engine"] == "generic" and r["algorithm"].startswith("xgmi"), r
        assert r["graph"] and r["bucketed"], r  # the whole step, exchanges included, was captured
        # two layers, forward and backward, in every eager step and in the one capture
        assert r["exchanges"] >= 8 and r["exchanges"] % 4 == 0 and len(r["sync_sizes"]) == 1, r
    assert np.array_equal(_w(runs, policy, 0, 2, True), _w(runs, policy, 1, 2, True)), "replicas diverged"
    # each replica's own moving statistics, not their ON_READ mean
    assert np.array_equal(_w(runs, policy, 0, 2, True, "nt"), _w(runs, policy, 1, 2, True, "nt"))
    rtol, atol = BOUNDS[policy]
    one = _w(runs, policy, 0, 1, True)
    two = _w(runs, policy, 0, 2, True)
    print(f"{policy}: sync R=2 vs R=1 miss {_miss(two, one, rtol, atol):.3g} (<= 1 passes)")
    np.testing.assert_allclose(two, one, rtol=rtol, atol=atol)


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
def test_control_unsynchronized_replicas_do_not(runs, policy):
    res = json.load(open(runs / "r0_2_0.json"))[policy]
    assert res["exchanges"] == 0 and res["sync_sizes"] == [], res
    rtol, atol = BOUNDS[policy]
    miss = _miss(_w(runs, policy, 0, 2, False), _w(runs, policy, 0, 1, True), rtol, atol)
    print(f"{policy}: unsynchronized R=2 vs R=1 miss {miss:.3g}")
    assert miss >= 10.0, miss
