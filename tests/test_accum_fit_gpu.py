"""Gradient accumulation end to end on one MI355X: the fold both engines run is the numpy fold bit for bit, k
micro-batches of b train like one batch of k b, the accumulating reference CNN stays on the fused engine inside
captured execution graphs keyed by their starting phase, a micro-step that is not the cycle's last launches the
accumulate kernel and nothing else, a checkpoint in the middle of a cycle resumes exactly, and two replicas
exchange gradients once per cycle.

The data pipelines here do NOT shuffle, so k consecutive micro-batches of 16 are exactly one batch of 64.
"""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import accum_refs as AR
import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.models.mnist_cnn import build_mnist_cnn

import test_fit_gpu as F
from test_clip_fit_gpu import CLIPNORM, _record_clips

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
O = tdl.keras.optimizers
SLOT = "gradient_accumulator"


def _pipeline(x, y, B):
    def scale(image, label):
        return image.to(torch.float32) / 255, label

    return tdl.data.Dataset.from_tensor_slices((x, y)).map(scale).cache().batch(B).repeat()


def _env(**kv):
    class _E:
        def __enter__(self):
            self.prev = {k: os.environ.get(k) for k in kv}
            os.environ.update({k: str(v) for k, v in kv.items()})

        def __exit__(self, *a):
            for k, v in self.prev.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    return _E()


def _train(fused, make_opt, B, steps, spe=4, graph=True, hook=None, skip=0, model=None, **env):
    """``steps`` train steps of the reference CNN over consecutive batches of B, from sample ``skip`` on."""
    g = "1" if graph else "0"
    with _env(TDL_DISABLE_FUSED="0" if fused else "1", TDL_GRAPH=g, TDL_GRAPH_STEP=g, **env):
        x, y = F._data(1024)
        if model is None:
            tdl.keras.backend.clear_session()
            tdl.keras.utils.set_random_seed(3)
            with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
                model = build_mnist_cnn()
                opt = make_opt()
                if hook is not None:
                    hook(model, opt)
                model.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt,
                              metrics=[tdl.keras.metrics.SparseCategoricalAccuracy()], steps_per_execution=spe)
        h = model.fit(_pipeline(x[skip:], y[skip:], B), epochs=1, steps_per_epoch=steps, verbose=0)
        return model, h


def _slab(m):
    return m._trainer.W


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "generic"])
def test_engine_fold_and_update_are_exact(fused):
    """Eager run, k = 3, Adam, 6 micro-steps: the gradient each update consumed is the numpy fold of the three
    local gradients recorded before it, bit for bit, and the final weights are those of a second, unaccumulated
    Adam handed the folded slabs at the same step counts."""
    k = 3
    local, folded, first_w = [], [], []

    def hook(model, opt):
        inner = opt.accumulate

        def accumulate(G, t_add=0, **kw):  # (kw: the generic trainer's zero_grad request)
            if not first_w:
                first_w.append(model._W.clone())
            local.append(G.clone())
            last = inner(G, t_add, **kw)
            if last:
                folded.append(G.clone())
            return last

        opt.accumulate = accumulate

    m, _ = _train(fused, lambda: O.Adam(1e-3, gradient_accumulation_steps=k), 16, 6, spe=2, graph=False, hook=hook)
    assert m._trainer.kind == ("fused" if fused else "generic"), getattr(m, "_fused_reason", None)
    assert not m._trainer._graphs or all(g[0] is None for g in m._trainer._graphs.values()), "an eager run"
    assert m.optimizer.iterations == 6 and len(local) == 6 and len(folded) == 2
    for c in range(2):
        want = AR.fold([g.cpu().numpy() for g in local[k * c:k * (c + 1)]], k)
        assert np.abs(want).max() > 0
        assert AR.same_bits(folded[c].cpu().numpy(), want), f"cycle {c}"
    ref = O.Adam(1e-3)
    W = first_w[0].clone()
    for c in range(2):
        ref.iterations = k * c + k - 1
        ref.apply_flat(W, folded[c].clone())
    assert torch.equal(W, _slab(m)), float((W - _slab(m)).abs().max())
    assert not torch.equal(first_w[0], _slab(m))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "generic"])
@pytest.mark.parametrize("make", [lambda **kw: O.SGD(0.05, **kw), lambda **kw: O.SGD(0.05, momentum=0.9, **kw)],
                         ids=["sgd", "sgd-momentum"])
def test_four_micro_batches_of_16_train_like_one_batch_of_64(make, fused):
    """k = 4 x b = 16 over 8 micro-steps against k off, b = 64 over 2 steps on the same samples, on one engine:
    the difference is the f32 summation order of the mean gradient of 64 samples.  Tolerance: ``rtol=2e-3,
    atol=2e-4`` on the weights, what tests/test_fit_gpu.py:52 (test_fused_engine_selected_and_matches_generic,
    the fused-vs-generic plain-SGD comparison) uses for exactly that situation.  The unaccumulated run at
    b = 16 differs from both by more than 1e-4 somewhere, so the comparison bites."""
    kind = "fused" if fused else "generic"
    ma, _ = _train(fused, lambda: make(gradient_accumulation_steps=4), 16, 8)
    mb, _ = _train(fused, make, 64, 2)
    mc, _ = _train(fused, make, 16, 8)
    assert ma._trainer.kind == mb._trainer.kind == mc._trainer.kind == kind, getattr(ma, "_fused_reason", None)
    assert ma.optimizer.iterations == 8 and mb.optimizer.iterations == 2 and mc.optimizer.iterations == 8
    worst = max(np.abs(a - b).max() for a, b in zip(ma.get_weights(), mb.get_weights()))
    print(f"{kind}: max |w(k=4, b=16) - w(b=64)| = {worst:.3g}")
    for a, b in zip(ma.get_weights(), mb.get_weights()):
        np.testing.assert_allclose(a, b, rtol=2e-3, atol=2e-4)
    for other in (ma, mb):
        d = max(np.abs(a - c).max() for a, c in zip(other.get_weights(), mc.get_weights()))
        assert d > 1e-4, d


FUSED_CASES = [
    ("adam", lambda **kw: O.Adam(learning_rate=1e-3, **kw)),
    ("sgd-nesterov", lambda **kw: O.SGD(learning_rate=0.05, momentum=0.9, nesterov=True, **kw)),
    ("lars", lambda **kw: O.LARS(0.05, nesterov=True, weight_decay_rate=1e-4, **kw)),
    ("adam-clipnorm", lambda **kw: O.Adam(learning_rate=1e-3, global_clipnorm=CLIPNORM, **kw)),
]


@pytest.mark.parametrize("name,make", FUSED_CASES, ids=[c[0] for c in FUSED_CASES])
def test_accumulating_reference_cnn_trains_on_the_fused_engine(name, make):
    """k = 2, 8 micro-steps of 64 (tests/test_fit_gpu.py's _train_opt): the accumulating optimizer keeps the
    reference CNN on the fused engine inside captured execution graphs and matches the generic engine, with the
    per-optimizer tolerances of test_reference_cnn_any_optimizer_on_fused_kernels (LARS: of
    test_layerwise_fit_gpu, a step is lr times the trust ratio)."""
    acc = lambda: make(gradient_accumulation_steps=2)  # noqa: E731
    mf, hf = F._train_opt(True, acc)
    assert mf._trainer.kind == "fused", mf._fused_reason
    assert mf._trainer.capture and mf._trainer._graphs, "the accumulating step must be captured"
    assert all(len(key) == 4 and key[3] == 0 for key in mf._trainer._graphs), list(mf._trainer._graphs)
    mg, hg = F._train_opt(False, acc)
    assert mg._trainer.kind == "generic"
    assert mf.optimizer.iterations == mg.optimizer.iterations == 8
    step = float(mf.optimizer.current_lr())
    if name == "lars":
        step *= max(float(mf.optimizer.last_layer_ratios.max()), float(mg.optimizer.last_layer_ratios.max()))
    for a, b in zip(mf.get_weights(), mg.get_weights()):
        off = ~np.isclose(a, b, rtol=5e-3, atol=5e-4)
        assert off.mean() < 1e-3, (name, off.mean())
        assert np.abs(a - b).max() <= 2 * step * 8 + 5e-4, (name, np.abs(a - b).max())
    np.testing.assert_allclose(hf.history["loss"], hg.history["loss"], rtol=2e-3, atol=2e-3)
    # accumulation is what ran: the unaccumulated optimizer ends elsewhere
    mu, _ = F._train_opt(True, make)
    assert any(np.abs(a - b).max() > 1e-4 for a, b in zip(mf.get_weights(), mu.get_weights()))
    if name == "adam-clipnorm":
        # the clip runs on the apply micro-steps only (eager fused run, one norm word per update) and is active
        log = []

        def make_logged():
            opt = acc()
            _record_clips(opt, log)
            return opt

        with _env(TDL_GRAPH="0", TDL_GRAPH_STEP="0"):
            me, _ = F._train_opt(True, make_logged)
        assert me._trainer.kind == "fused" and not me._trainer.capture
        assert len(log) == 4, len(log)
        for i, (n, _) in enumerate(log):
            print(f"apply micro-step {i}: gradient norm {float(n):.4f} (clipnorm {CLIPNORM})")
            assert float(n) > 1.5 * CLIPNORM


def _bits_equal(ma, mb):
    return all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(ma.get_weights(), mb.get_weights()))


def test_fused_execution_graphs_are_keyed_by_phase_and_match_eager():
    """steps_per_execution = 4, k = 3, 8 micro-steps: the two executions start at phases 0 and 1, so two graph
    variants exist.  The weights are bit-identical to the TDL_GRAPH=0 run.  Which case held: on the parent
    commit the unaccumulated fused Adam run (tests/test_fit_gpu.py's _train_opt: 8 steps of 64,
    steps_per_execution = 4) was bit-identical between TDL_GRAPH=1 and TDL_GRAPH=0 on an MI355X (max |dw| = 0,
    recorded in profiles/accum_cost.txt), so the comparison here is exact; rtol=1e-4, atol=1e-5 of
    test_generic_whole_step_graph_with_clipped_adam_matches_eager would have applied had it not been."""
    make = lambda: O.Adam(1e-3, gradient_accumulation_steps=3)  # noqa: E731
    mg, _ = _train(True, make, 16, 8, spe=4)
    tr = mg._trainer
    assert tr.kind == "fused" and tr.capture
    assert {key[3] for key in tr._graphs} == {0, 1}, list(tr._graphs)
    assert all(g[0] is not None for g in tr._graphs.values())
    me, _ = _train(True, make, 16, 8, spe=4, graph=False)
    assert me._trainer.kind == "fused" and not me._trainer.capture
    assert mg.optimizer.iterations == me.optimizer.iterations == 8
    assert torch.equal(mg.optimizer.slots()[SLOT], me.optimizer.slots()[SLOT])
    assert _bits_equal(mg, me), max(np.abs(a - b).max() for a, b in zip(mg.get_weights(), me.get_weights()))


def test_generic_execution_graphs_are_keyed_by_phase_and_match_eager():
    """The generic engine's device-resident executions: ``("dev", K, b, p0)``.  Its first execution at a batch
    size runs eagerly, so 16 micro-steps (starts at phases 0, 1, 2, 0) leave the graphs of phases 1, 2 and 0.
    Bit-identical to the eager host-pipeline run: the unaccumulated Adam run of this model and shape was
    bit-identical between the two modes on the parent commit on an MI355X, so the exact comparison applies
    (rtol=1e-4, atol=1e-5 of test_generic_whole_step_graph_with_clipped_adam_matches_eager otherwise)."""
    make = lambda: O.Adam(1e-3, gradient_accumulation_steps=3)  # noqa: E731
    mg, _ = _train(False, make, 16, 16, spe=4)
    tr = mg._trainer
    assert tr.kind == "generic"
    dev = [key for key in tr._graphs if key[0] == "dev"]
    assert sorted(dev) == [("dev", 4, 16, 0), ("dev", 4, 16, 1), ("dev", 4, 16, 2)], list(tr._graphs)
    me, _ = _train(False, make, 16, 16, spe=4, graph=False)
    assert not me._trainer._graphs and mg.optimizer.iterations == me.optimizer.iterations == 16
    assert _bits_equal(mg, me), max(np.abs(a - b).max() for a, b in zip(mg.get_weights(), me.get_weights()))


def test_generic_per_step_graphs_capture_the_three_modes_and_match_eager():
    """Host pipeline (TDL_GENERIC_DEVICE_DATA=0): one whole-step graph per accumulate mode -- first, middle,
    last -- each captured at its third sighting; 12 micro-steps replay each once.  Bit-identical to the eager run,
    as the unaccumulated per-step graph was on the parent commit (see the test above)."""
    make = lambda: O.Adam(1e-3, gradient_accumulation_steps=3)  # noqa: E731
    mg, _ = _train(False, make, 16, 12, spe=1, TDL_GENERIC_DEVICE_DATA="0")
    tr = mg._trainer
    assert tr.kind == "generic"
    modes = sorted(key[-1][1] for key in tr._graphs if key[-1][0] == "accum")
    assert modes == ["first", "last", "middle"], list(tr._graphs)
    me, _ = _train(False, make, 16, 12, spe=1, graph=False)
    assert not me._trainer._graphs and mg.optimizer.iterations == me.optimizer.iterations == 12
    assert _bits_equal(mg, me), max(np.abs(a - b).max() for a, b in zip(mg.get_weights(), me.get_weights()))


def test_non_apply_micro_step_launches_the_accumulate_kernel_only():
    from tensorflow_distributed_learning_amd.utils import kernel_audit

    n = 100003
    g = torch.Generator().manual_seed(0)
    W = torch.randn(n, generator=g).cuda()
    G = torch.randn(n, generator=g).cuda()
    opt = O.Adam(1e-3, global_clipnorm=1.0, gradient_accumulation_steps=2)
    for _ in range(2):  # (build, first learning-rate fill, one whole cycle)
        opt.apply_flat(W, G)
    assert opt.iterations == 2

    def count(res, kern):
        return sum(c for k, c in res["tdl"].items() if kern in k)

    def micro_step():
        assert opt.accumulate(G) is False
        opt.iterations += 1

    res = kernel_audit.audit(micro_step)
    print({k: dict(v) for k, v in res.items()})
    assert count(res, "k_grad_accum") == 1 and sum(res["tdl"].values()) == 1, res
    assert count(res, "k_adam") == 0 and count(res, "k_clip") == 0
    assert not res["torch"] and not res["library"], res

    def apply_step():
        assert opt.accumulate(G) is True
        opt.apply_flat(W, G, accumulated=True)

    res = kernel_audit.audit(apply_step)
    print({k: dict(v) for k, v in res.items()})
    assert count(res, "k_grad_accum") == 1 and count(res, "k_adam") == 1, res
    assert count(res, "k_clip_partials") == 1 and not res["library"], res
    assert opt.iterations == 4


def test_checkpoint_in_the_middle_of_a_cycle_resumes_bit_exactly():
    """k = 4, eager generic engine: 3 micro-steps, state_dict() + weights into a fresh model and optimizer, 5
    more, against 8 uninterrupted micro-steps."""
    make = lambda: O.Adam(1e-3, gradient_accumulation_steps=4)  # noqa: E731
    full, _ = _train(False, make, 16, 8, spe=1, graph=False)
    first, _ = _train(False, make, 16, 3, spe=1, graph=False)
    st = first.optimizer.state_dict()
    weights = first.get_weights()
    assert st["iterations"] == 3 and SLOT in st["slots"]
    with _env(TDL_DISABLE_FUSED="1"):
        tdl.keras.backend.clear_session()
        with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
            again = build_mnist_cnn()
            again.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=make(),
                          metrics=[tdl.keras.metrics.SparseCategoricalAccuracy()], steps_per_execution=1)
    again.set_weights(weights)
    again.optimizer.load_state_dict(st)
    assert SLOT in again.optimizer.slots() and again.optimizer.iterations == 3
    _train(False, None, 16, 5, spe=1, graph=False, skip=48, model=again)
    assert again._trainer.kind == "generic" and again.optimizer.iterations == full.optimizer.iterations == 8
    assert torch.equal(again.optimizer.slots()[SLOT].cpu(), full.optimizer.slots()[SLOT].cpu())
    assert _bits_equal(again, full), max(np.abs(a - b).max() for a, b in zip(again.get_weights(), full.get_weights()))


BODY = """
import json, os, sys, numpy as np, torch
import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.models.mnist_cnn import build_mnist_cnn
from tensorflow_distributed_learning_amd.data.tfds import synthetic_mnist
from tensorflow_distributed_learning_amd.parallel import consistency
out, tag = sys.argv[1], os.environ["JOB_TAG"]
k = int(os.environ["JOB_ACCUM"]) or None
strategy = tdl.distribute.MirroredStrategy(communication=os.environ.get("JOB_COMM") or None)
R, rank = strategy.num_replicas_in_sync, strategy.extended.rank
comm = strategy.extended.communicator
tdl.keras.utils.set_random_seed(5)
x, y = synthetic_mnist(256, 2)
ds = tdl.data.Dataset.from_tensor_slices((x.reshape(-1, 28, 28, 1), y))
ds = ds.map(lambda i, l: (i.to(torch.float32) / 255, l)).cache().batch(16).repeat()
with strategy.scope():
    m = build_mnist_cnn()
    opt = tdl.keras.optimizers.Adam(1e-3, gradient_accumulation_steps=k)
    m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt,
              metrics=["sparse_categorical_accuracy"], steps_per_execution=1)
calls = []
for name in ("all_reduce", "all_reduce_async", "all_reduce_sgd"):
    inner = getattr(comm, name, None)
    if inner is None:
        continue
    def wrapped(t, *a, _inner=inner, _name=name, **kw):
        calls.append((_name, int(t.numel())))
        return _inner(t, *a, **kw)
    setattr(comm, name, wrapped)
h = m.fit(ds, epochs=1, steps_per_epoch=4, verbose=0)
tr = m._trainer
slab_calls = sum(1 for _, c in calls if c == tr.W.numel())
same = consistency.replicas_identical(comm, tr.W)
np.save(os.path.join(out, f"w{rank}_{tag}.npy"), np.concatenate([v.ravel() for v in m.get_weights()]))
json.dump({"engine": tr.kind, "graph": bool(tr.capture and tr.capture_comm), "identical": same,
           "iterations": int(opt.iterations), "slab_all_reduces": slab_calls, "slab": int(tr.W.numel())},
          open(os.path.join(out, f"r{rank}_{tag}.json"), "w"))
"""


def _run(tmp_path, n, accum, tag, graph=True):
    s = tmp_path / "job.py"
    s.write_text(textwrap.dedent(BODY))
    env = dict(os.environ, PYTHONPATH=ROOT, TDL_SHARE_GPU="1", JOB_COMM="", JOB_ACCUM=str(accum), JOB_TAG=tag)
    if not graph:
        env["TDL_GRAPH"] = "0"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "TF_CONFIG"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "tensorflow_distributed_learning_amd.launch", "--nproc-per-node", str(n),
                        str(s), str(tmp_path)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.slow
def test_two_replicas_exchange_gradients_once_per_cycle(tmp_path):
    """2 replica processes sharing the GPU, b = 8 each, k = 2, 4 micro-steps, Adam on the fused engine (the job
    pattern of test_clip_fit_gpu.test_two_replicas_clip_by_the_same_norm_bits): the replicas stay bit-identical,
    the weights match one replica on the same global batches (that test's bounds), and an eager run all-reduces
    the gradient slab exactly twice, against four times with accumulation off."""
    _run(tmp_path, 1, 2, "one")
    _run(tmp_path, 2, 2, "two")
    _run(tmp_path, 2, 2, "eager", graph=False)
    _run(tmp_path, 2, 0, "off", graph=False)
    one = json.load(open(tmp_path / "r0_one.json"))
    a, b = (json.load(open(tmp_path / f"r{i}_two.json")) for i in range(2))
    assert one["engine"] == a["engine"] == b["engine"] == "fused"
    assert a["identical"] and b["identical"] and a["iterations"] == b["iterations"] == one["iterations"] == 4
    w0, w1, ws = (np.load(tmp_path / f) for f in ("w0_two.npy", "w1_two.npy", "w0_one.npy"))
    assert np.array_equal(w0, w1)
    off = ~np.isclose(w0, ws, rtol=5e-3, atol=5e-4)
    assert off.mean() < 1e-3, off.mean()
    assert np.abs(w0 - ws).max() <= 2 * 1e-3 * 4 + 5e-4
    for r in range(2):
        e = json.load(open(tmp_path / f"r{r}_eager.json"))
        u = json.load(open(tmp_path / f"r{r}_off.json"))
        assert e["engine"] == u["engine"] == "fused" and not e["graph"] and not u["graph"]
        assert e["identical"] and u["identical"]
        assert e["slab_all_reduces"] == 2, e
        assert u["slab_all_reduces"] == 4, u
    assert np.array_equal(np.load(tmp_path / "w0_eager.npy"), np.load(tmp_path / "w1_eager.npy"))
