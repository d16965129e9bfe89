"""LARS and LAMB end to end on one MI355X: the reference CNN stays on the fused engine with the three layer-wise
launches inside its captured execution graph and matches the generic engine; the generic engine's whole-step
graph matches eager; a step launches no torch reduction; two replicas form bit-identical trust ratios; a
checkpoint resumes exactly.  Shapes and tolerances are those of tests/test_fit_gpu.py / test_clip_fit_gpu.py
for the same comparisons."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.models.mnist_cnn import build_mnist_cnn

import test_fit_gpu as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
O = tdl.keras.optimizers

CASES = [
    ("lamb", lambda: O.LAMB(1e-3, weight_decay_rate=0.01, exclude_from_weight_decay=["bias"]),
     lambda: O.Adam(1e-3)),
    ("lars-nesterov", lambda: O.LARS(0.05, nesterov=True, weight_decay_rate=1e-4),
     lambda: O.SGD(0.05, momentum=0.9, nesterov=True)),
]


@pytest.mark.parametrize("name,make,plain", CASES, ids=[c[0] for c in CASES])
def test_reference_cnn_trains_layerwise_on_the_fused_engine(name, make, plain):
    mf, hf = F._train_opt(True, make)
    assert mf._trainer.kind == "fused", mf._fused_reason
    assert mf._trainer.capture and mf._trainer._graphs, "the layer-wise step must be captured"
    mg, hg = F._train_opt(False, make)
    assert mg._trainer.kind == "generic"
    assert mf.optimizer.iterations == mg.optimizer.iterations == 8
    # the form of test_reference_cnn_any_optimizer_on_fused_kernels; a step is lr times the trust ratio
    rmax = max(float(mf.optimizer.last_layer_ratios.max()), float(mg.optimizer.last_layer_ratios.max()))
    step = float(mf.optimizer.current_lr()) * rmax
    print(f"{name}: ratios fused {mf.optimizer.last_layer_ratios.cpu().numpy()}, generic "
          f"{mg.optimizer.last_layer_ratios.cpu().numpy()}")
    for a, b in zip(mf.get_weights(), mg.get_weights()):
        off = ~np.isclose(a, b, rtol=5e-3, atol=5e-4)
        assert off.mean() < 1e-3, (name, off.mean())
        assert np.abs(a - b).max() <= 2 * step * 8 + 5e-4, (name, np.abs(a - b).max())
    np.testing.assert_allclose(hf.history["loss"], hg.history["loss"], rtol=2e-3, atol=2e-3)
    # the ratio is active: not every ratio is 1, and the weights differ from the plain optimizer's
    ratios = mf.optimizer.last_layer_ratios.cpu().numpy()
    assert (np.abs(ratios - 1.0) > 1e-3).sum() >= 4, ratios
    mp, _ = F._train_opt(True, plain)
    assert any(np.abs(a - b).max() > 1e-4 for a, b in zip(mf.get_weights(), mp.get_weights()))


def _train_small_resnet(graph, make_opt, steps=8):
    os.environ["TDL_GRAPH_STEP"] = "1" if graph else "0"
    os.environ["TDL_CONV_AUTOTUNE"] = "0"  # (as test_fit_gpu._train_small_resnet: MIOpen immediate mode)
    bench_prev = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = False
    try:
        tdl.keras.backend.clear_session()
        g = torch.Generator().manual_seed(0)
        x = torch.rand(512, 16, 16, 8, generator=g)
        y = torch.randint(0, 10, (512,), generator=g)
        ds = tdl.data.Dataset.from_tensor_slices((x, y)).batch(64).repeat()
        with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
            m = F._small_resnet(1)
            m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=make_opt(),
                      metrics=["sparse_categorical_accuracy"])
        h = m.fit(ds, epochs=2, steps_per_epoch=steps // 2, verbose=0)
        return m, h
    finally:
        os.environ.pop("TDL_GRAPH_STEP", None)
        os.environ.pop("TDL_CONV_AUTOTUNE", None)
        torch.backends.cudnn.benchmark = bench_prev


@pytest.mark.parametrize("name,make", [
    ("lamb", lambda: O.LAMB(1e-3, weight_decay_rate=0.01, exclude_from_weight_decay=["bias", "gamma", "beta"])),
    ("lars", lambda: O.LARS(0.1, weight_decay_rate=1e-4, exclude_from_weight_decay=["bias", "gamma", "beta"])),
], ids=["lamb", "lars"])
def test_generic_whole_step_graph_matches_eager(name, make):
    mg, hg = _train_small_resnet(True, make)
    assert mg._trainer.kind == "generic"
    assert mg.optimizer.graph_safe and mg._trainer._graphable() and len(mg._trainer._graphs) == 1
    me, he = _train_small_resnet(False, make)
    assert not me._trainer._graphs
    assert mg.optimizer.iterations == me.optimizer.iterations == 8
    for a, b in zip(mg.get_weights(), me.get_weights()):
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(hg.history["loss"], he.history["loss"], rtol=1e-4)
    ratios = mg.optimizer.last_layer_ratios.cpu().numpy()
    assert np.isfinite(ratios).all() and (np.abs(ratios - 1.0) > 1e-3).any(), ratios


def test_lamb_apply_flat_launches_no_torch_reduction():
    from tensorflow_distributed_learning_amd.engine.slab import SlabLayout
    from tensorflow_distributed_learning_amd.utils import kernel_audit

    lay = SlabLayout.from_shapes([("a/kernel", (300, 301)), ("a/bias", (301,)), ("b/kernel", (9000,)), ("b/bias", (3,))])
    g = torch.Generator().manual_seed(0)
    W = torch.randn(lay.total, generator=g).cuda()
    G = torch.randn(lay.total, generator=g).cuda()
    opt = O.LAMB(1e-3, weight_decay_rate=0.01, exclude_from_weight_decay=["bias"], global_clipnorm=1.0, clipvalue=0.5)
    opt.set_layout(lay)
    opt.apply_flat(W, G)  # (build, first learning-rate fill)
    res = kernel_audit.audit(lambda: opt.apply_flat(W, G))
    print({k: dict(v) for k, v in res.items()})
    assert not [k for k in res["torch"] if "reduce" in k.lower()], res["torch"]
    named = {**res["tdl"], **res["other"]}
    for kern in ("k_clip_partials", "k_clip_scale", "k_layer_sums_lamb", "k_layer_ratio", "k_lamb_apply"):
        assert sum(c for k, c in named.items() if kern in k) == 1, (kern, res)
    assert not res["library"], res
    assert float(opt.last_clip_norm) > 1.0
    r = opt.last_layer_ratios.cpu().numpy()
    assert r.shape == (4,) and r[1] == 1.0 and r[3] == 1.0 and r[0] != 1.0 and r[2] != 1.0
    assert opt.last_layer_norms.shape == (4, 2)


BODY = """
import json, os, sys, numpy as np, torch
import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.models.mnist_cnn import build_mnist_cnn
from tensorflow_distributed_learning_amd.data.tfds import synthetic_mnist
from tensorflow_distributed_learning_amd.parallel import consistency
out = sys.argv[1]
strategy = tdl.distribute.MirroredStrategy(communication=os.environ.get("JOB_COMM") or None)
R, rank = strategy.num_replicas_in_sync, strategy.extended.rank
tdl.keras.utils.set_random_seed(5)
x, y = synthetic_mnist(256, 2)
ds = tdl.data.Dataset.from_tensor_slices((x.reshape(-1, 28, 28, 1), y))
ds = ds.map(lambda i, l: (i.to(torch.float32) / 255, l)).cache().shuffle(256, seed=9).batch(16).repeat()
with strategy.scope():
    m = build_mnist_cnn()
    opt = tdl.keras.optimizers.LAMB(1e-3, weight_decay_rate=0.01, exclude_from_weight_decay=["bias"])
    m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt,
              metrics=["sparse_categorical_accuracy"], steps_per_execution=1)
ratios = []
cb = tdl.keras.callbacks.LambdaCallback(
    on_batch_end=lambda b, logs=None: ratios.append(opt.last_layer_ratios.view(torch.int32).cpu().tolist()))
h = m.fit(ds, epochs=1, steps_per_epoch=4, verbose=0, callbacks=[cb])
tr = m._trainer
same = consistency.replicas_identical(strategy.extended.communicator, tr.W)
np.save(os.path.join(out, f"w{rank}_{R}.npy"), np.concatenate([v.ravel() for v in m.get_weights()]))
json.dump({"engine": tr.kind, "ratio_bits": ratios, "identical": same, "iterations": int(opt.iterations)},
          open(os.path.join(out, f"r{rank}_{R}.json"), "w"))
"""


@pytest.mark.slow
def test_two_replicas_form_the_same_ratio_bits(tmp_path):
    """2 replica processes sharing the GPU, LAMB on the fused engine: the trust-ratio words are bit-equal on
    both ranks after every step and the replicas' weights stay identical."""
    s = tmp_path / "job.py"
    s.write_text(textwrap.dedent(BODY))
    env = dict(os.environ, PYTHONPATH=ROOT, TDL_SHARE_GPU="1", JOB_COMM="")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "TF_CONFIG"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "tensorflow_distributed_learning_amd.launch", "--nproc-per-node", "2",
                        str(s), str(tmp_path)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    a, b = (json.load(open(tmp_path / f"r{i}_2.json")) for i in range(2))
    assert a["engine"] == b["engine"] == "fused"
    assert a["identical"] and b["identical"] and a["iterations"] == b["iterations"] == 4
    assert len(a["ratio_bits"]) == 4 and all(len(r) == 8 for r in a["ratio_bits"])
    assert a["ratio_bits"] == b["ratio_bits"]
    ratios = np.array(a["ratio_bits"], dtype=np.int32).view(np.float32)
    assert np.isfinite(ratios).all() and (np.abs(ratios - 1.0) > 1e-3).sum() >= 16, ratios
    assert len({tuple(r) for r in a["ratio_bits"]}) == 4, "four steps, four different ratio sets"
    assert np.array_equal(np.load(tmp_path / "w0_2.npy"), np.load(tmp_path / "w1_2.npy"))


def _cnn(make_opt):
    tdl.keras.backend.clear_session()
    tdl.keras.utils.set_random_seed(3)
    with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
        m = build_mnist_cnn()
        m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=make_opt(),
                  metrics=[tdl.keras.metrics.SparseCategoricalAccuracy()], steps_per_execution=4)
    return m


@pytest.mark.parametrize("name,make,plain", CASES, ids=[c[0] for c in CASES])
def test_checkpoint_resumes_exactly(name, make, plain, tmp_path):
    """4 steps, save, restore into a fresh model, 4 more steps == the same two fits on one model (every fit
    starts the unshuffled pipeline at its first batch)."""
    x, y = F._data(512)
    ds = tdl.data.Dataset.from_tensor_slices((x, y)).map(lambda i, l: (i.to(torch.float32) / 255, l)).batch(64).repeat()
    whole = _cnn(make)
    whole.fit(ds, epochs=1, steps_per_epoch=4, verbose=0)
    first = [w.copy() for w in whole.get_weights()]
    path = tdl.train.Checkpoint(model=whole, optimizer=whole.optimizer).save(str(tmp_path / "ck"))
    whole.fit(ds, epochs=1, steps_per_epoch=4, verbose=0)
    assert whole.optimizer.iterations == 8 and whole._trainer.kind == "fused"
    resumed = _cnn(make)
    tdl.train.Checkpoint(model=resumed, optimizer=resumed.optimizer).restore(path)
    assert resumed.optimizer.iterations == 4
    assert all(np.array_equal(a, b) for a, b in zip(first, resumed.get_weights()))
    resumed.fit(ds, epochs=1, steps_per_epoch=4, verbose=0)
    assert resumed.optimizer.iterations == 8 and resumed._trainer.kind == "fused"
    for a, b in zip(whole.get_weights(), resumed.get_weights()):
        assert np.array_equal(a, b)
    for k, v in whole.optimizer.slots().items():
        assert torch.equal(v, resumed.optimizer.slots()[k]), k
    assert any(np.abs(a - b).max() > 1e-4 for a, b in zip(first, resumed.get_weights()))
