"""Gradient clipping end to end on one MI355X: a clipped optimizer keeps the reference CNN on the fused engine
(clip_norm + the update kernel inside the captured execution graph), makes the generic engine's whole-step
graph possible, launches no torch reduction, and keeps two replicas bit-identical.  Shapes and tolerances are
those of tests/test_fit_gpu.py for the same optimizers; the clip constants are chosen so that the clip is
active on every step, which each test asserts from the recorded norm words (a clip that never bites proves
nothing)."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import tensorflow_distributed_learning_amd as tdl

import test_fit_gpu as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CLIPNORM = 0.1  # the reference CNN's gradient norm is > 0.3 during these 8 steps (asserted: _assert_active)
CLIPVALUE = 0.01  # and its largest gradient element well above this


def _record_clips(opt, log):
    """Record, per step of an EAGER run, the norm word (norm clips) and max |g| (clipvalue) on the device."""
    inner = opt.device_clip

    def device_clip(G):
        kw = inner(G)
        log.append((opt.last_clip_norm.clone() if kw.get("gscale") is not None else None, G.abs().max()))
        return kw

    opt.device_clip = device_clip


def _train_cnn(fused, make_opt, graph=True, log=None):
    os.environ["TDL_GRAPH"] = "1" if graph else "0"
    os.environ["TDL_GRAPH_STEP"] = "1" if graph else "0"
    try:
        def make():
            opt = make_opt()
            if log is not None:
                _record_clips(opt, log)
            return opt

        return F._train_opt(fused, make)
    finally:
        os.environ.pop("TDL_GRAPH", None)
        os.environ.pop("TDL_GRAPH_STEP", None)


def _assert_active(log, opt, steps=8):
    assert len(log) == steps
    norm = opt.global_clipnorm or opt.clipnorm
    for k, (n, gmax) in enumerate(log):
        if norm is not None:
            print(f"step {k}: gradient norm {float(n):.4f} (clipnorm {norm})")
            assert float(n) > 1.5 * norm, f"step {k}: norm {float(n)} does not exceed clipnorm {norm} clearly"
        else:
            print(f"step {k}: max |g| {float(gmax):.4f} (clipvalue {opt.clipvalue})")
            assert float(gmax) > 1.5 * opt.clipvalue, f"step {k}: max |g| {float(gmax)} is not clamped"


CASES = [
    ("adam", lambda **kw: tdl.keras.optimizers.Adam(learning_rate=1e-3, **kw), dict(global_clipnorm=CLIPNORM)),
    ("sgd-momentum", lambda **kw: tdl.keras.optimizers.SGD(learning_rate=0.05, momentum=0.9, **kw),
     dict(clipnorm=CLIPNORM)),
    ("sgd-clipvalue", lambda **kw: tdl.keras.optimizers.SGD(learning_rate=0.05, **kw), dict(clipvalue=CLIPVALUE)),
]


@pytest.mark.parametrize("name,make,clip", CASES, ids=[c[0] for c in CASES])
def test_clipped_reference_cnn_trains_on_the_fused_engine(name, make, clip):
    mf, hf = _train_cnn(True, lambda: make(**clip))
    assert mf._trainer.kind == "fused", mf._fused_reason
    assert mf._trainer.capture and mf._trainer._graphs, "the clipped step must be captured"
    mg, hg = _train_cnn(False, lambda: make(**clip))
    assert mg._trainer.kind == "generic"
    assert mf.optimizer.iterations == mg.optimizer.iterations == 8
    if name == "sgd-clipvalue":  # plain SGD: the tolerances of test_fused_engine_selected_and_matches_generic
        for a, b in zip(mf.get_weights(), mg.get_weights()):
            np.testing.assert_allclose(a, b, rtol=2e-3, atol=2e-4)
        np.testing.assert_allclose(hf.history["loss"], hg.history["loss"], rtol=1e-3, atol=6e-3)
    else:  # those of test_reference_cnn_any_optimizer_on_fused_kernels
        lr = float(mf.optimizer.current_lr())
        for a, b in zip(mf.get_weights(), mg.get_weights()):
            off = ~np.isclose(a, b, rtol=5e-3, atol=5e-4)
            assert off.mean() < 1e-3, (name, off.mean())
            assert np.abs(a - b).max() <= 2 * lr * 8 + 5e-4, (name, np.abs(a - b).max())
        np.testing.assert_allclose(hf.history["loss"], hg.history["loss"], rtol=2e-3, atol=2e-3)
    # the clip is active on every step (eager fused run, one read per step) ...
    log = []
    me, _ = _train_cnn(True, lambda: make(**clip), graph=False, log=log)
    assert me._trainer.kind == "fused" and not me._trainer.capture
    _assert_active(log, me.optimizer)
    # ... and it changes the training
    mu, _ = _train_cnn(True, lambda: make())
    assert any(np.abs(a - b).max() > 1e-4 for a, b in zip(mf.get_weights(), mu.get_weights()))


def _train_small_resnet(graph, log=None, steps=8):
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
            opt = tdl.keras.optimizers.Adam(learning_rate=1e-3, global_clipnorm=CLIPNORM)
            if log is not None:
                _record_clips(opt, log)
            m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt,
                      metrics=["sparse_categorical_accuracy"])
        h = m.fit(ds, epochs=2, steps_per_epoch=steps // 2, verbose=0)
        return m, h
    finally:
        os.environ.pop("TDL_GRAPH_STEP", None)
        os.environ.pop("TDL_CONV_AUTOTUNE", None)
        torch.backends.cudnn.benchmark = bench_prev


def test_generic_whole_step_graph_with_clipped_adam_matches_eager():
    mg, hg = _train_small_resnet(True)
    assert mg._trainer.kind == "generic"
    assert mg.optimizer.graph_safe and mg._trainer._graphable() and len(mg._trainer._graphs) == 1
    log = []
    me, he = _train_small_resnet(False, log)
    assert not me._trainer._graphs
    _assert_active(log, me.optimizer)
    assert mg.optimizer.iterations == me.optimizer.iterations == 8
    for a, b in zip(mg.get_weights(), me.get_weights()):
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(hg.history["loss"], he.history["loss"], rtol=1e-4)


def test_clipped_apply_flat_launches_no_torch_reduction():
    from tensorflow_distributed_learning_amd.utils import kernel_audit

    n = 100003
    g = torch.Generator().manual_seed(0)
    W = torch.randn(n, generator=g).cuda()
    G = torch.randn(n, generator=g).cuda()
    opt = tdl.keras.optimizers.Adam(1e-3, global_clipnorm=1.0, clipvalue=0.5)
    opt.apply_flat(W, G)  # (build, first learning-rate fill)
    res = kernel_audit.audit(lambda: opt.apply_flat(W, G))
    print({k: dict(v) for k, v in res.items()})
    assert not [k for k in res["torch"] if "reduce" in k.lower()], res["torch"]
    for kern in ("k_clip_partials", "k_clip_scale", "k_adam"):
        assert sum(c for k, c in res["tdl"].items() if kern in k) == 1, (kern, res)
    assert not res["library"], res
    assert float(opt.last_clip_norm) > 1.0


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
    opt = tdl.keras.optimizers.Adam(1e-3, global_clipnorm=float(os.environ["JOB_CLIPNORM"]))
    m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt,
              metrics=["sparse_categorical_accuracy"], steps_per_execution=1)
norms = []
cb = tdl.keras.callbacks.LambdaCallback(
    on_batch_end=lambda b, logs=None: norms.append(int(opt.last_clip_norm.view(torch.int32).item())))
h = m.fit(ds, epochs=1, steps_per_epoch=4, verbose=0, callbacks=[cb])
tr = m._trainer
same = consistency.replicas_identical(strategy.extended.communicator, tr.W)
np.save(os.path.join(out, f"w{rank}_{R}.npy"), np.concatenate([v.ravel() for v in m.get_weights()]))
json.dump({"engine": tr.kind, "graph": bool(tr.capture and tr.capture_comm), "norm_bits": norms, "identical": same,
           "iterations": int(opt.iterations)}, open(os.path.join(out, f"r{rank}_{R}.json"), "w"))
"""


def _run(tmp_path, n):
    s = tmp_path / "job.py"
    s.write_text(textwrap.dedent(BODY))
    env = dict(os.environ, PYTHONPATH=ROOT, TDL_SHARE_GPU="1", JOB_COMM="", JOB_CLIPNORM=str(CLIPNORM))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "TF_CONFIG"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "tensorflow_distributed_learning_amd.launch", "--nproc-per-node", str(n),
                        str(s), str(tmp_path)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.slow
def test_two_replicas_clip_by_the_same_norm_bits(tmp_path):
    """2 replica processes sharing the GPU, b = 8 each, clipped Adam on the fused engine: the norm word is
    bit-equal on both ranks after every step, the replicas stay identical, and the weights match one replica
    on the same global batches."""
    _run(tmp_path, 1)
    _run(tmp_path, 2)
    one = json.load(open(tmp_path / "r0_1.json"))
    a, b = (json.load(open(tmp_path / f"r{i}_2.json")) for i in range(2))
    assert one["engine"] == a["engine"] == b["engine"] == "fused"
    assert a["identical"] and b["identical"] and a["iterations"] == b["iterations"] == 4
    assert len(a["norm_bits"]) == 4 and a["norm_bits"] == b["norm_bits"]
    norms = np.array(a["norm_bits"], dtype=np.int32).view(np.float32)
    assert (norms > 1.5 * CLIPNORM).all(), norms
    w0, w1, ws = (np.load(tmp_path / f) for f in ("w0_2.npy", "w1_2.npy", "w0_1.npy"))
    assert np.array_equal(w0, w1)
    off = ~np.isclose(w0, ws, rtol=5e-3, atol=5e-4)
    assert off.mean() < 1e-3, off.mean()
    assert np.abs(w0 - ws).max() <= 2 * 1e-3 * 8 + 5e-4
