"""The weight EMA (``use_ema``) end to end on one MI355X, reference CNN, batch 16, at most 12 steps: the average
both engines keep inside their execution graphs is the numpy fold (tests/ema_refs.py) of the per-step weights of
an identical run stepped eagerly one step at a time, the average never perturbs the weights, graphs with
overwrite steps replay like eager steps and are keyed by their phase, ``fit`` ends with the averaged weights, a
checkpoint between two overwrites resumes exactly, plain SGD keeps its in-finalize update, and with gradient
accumulation the average moves on apply micro-steps only.

The data pipelines here do NOT shuffle: every run sees the same batches in the same order.
"""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import ema_refs as ER
import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.models.mnist_cnn import build_mnist_cnn

import test_fit_gpu as F
from test_accum_fit_gpu import _env, _pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
O = tdl.keras.optimizers
SLOT = "ema"
M = 0.9  # (a momentum at which 8 steps move the average visibly)

OPTS = {
    "sgd": lambda **kw: O.SGD(0.05, **kw),
    "sgd-momentum": lambda **kw: O.SGD(0.05, momentum=0.9, **kw),
    "adam": lambda **kw: O.Adam(1e-3, **kw),
    "lamb": lambda **kw: O.LAMB(1e-3, **kw),
}


class Record(tdl.keras.callbacks.Callback):
    """The live weight slab (and the average) at the start of fit and after every execution."""

    def __init__(self):
        super().__init__()
        self.w0, self.ws, self.es, self.its, self.states = None, [], [], [], []

    def on_train_begin(self, logs=None):
        self.w0 = self.model._W.detach().cpu().numpy().copy()

    def on_train_batch_end(self, batch, logs=None):
        opt = self.model.optimizer
        self.ws.append(self.model._W.detach().cpu().numpy().copy())
        self.its.append(int(opt.iterations))
        if SLOT in opt.slots():
            self.es.append(opt.slots()[SLOT].detach().cpu().numpy().copy())


def _train(fused, make_opt, steps, spe=4, graph=True, skip=0, model=None, callbacks=None, **env):
    """``steps`` train steps of the reference CNN over consecutive batches of 16, from sample ``skip`` on."""
    g = "1" if graph else "0"
    with _env(TDL_DISABLE_FUSED="0" if fused else "1", TDL_GRAPH=g, TDL_GRAPH_STEP=g, **env):
        x, y = F._data(1024)
        if model is None:
            tdl.keras.backend.clear_session()
            tdl.keras.utils.set_random_seed(3)
            with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
                model = build_mnist_cnn()
                model.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                              optimizer=make_opt(), metrics=[tdl.keras.metrics.SparseCategoricalAccuracy()],
                              steps_per_execution=spe)
        model.fit(_pipeline(x[skip:], y[skip:], 16), epochs=1, steps_per_epoch=steps, verbose=0,
                  callbacks=callbacks)
        return model


def _w(m) -> np.ndarray:
    return m._W.detach().cpu().numpy()


def _e(m) -> np.ndarray:
    return m.optimizer.slots()[SLOT].detach().cpu().numpy()


def _same(a, b) -> bool:
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "generic"])
@pytest.mark.parametrize("name", list(OPTS))
def test_average_is_the_numpy_fold_of_the_per_step_weights(name, fused):
    """8 steps in executions of 4 (graphs) against the same optimizer stepped eagerly one step at a time, whose
    weights after every step are recorded: E of both runs is the numpy fold of those weights from E = W0, and the
    eager run's last weights are the bits of a run without EMA."""
    kind = "fused" if fused else "generic"
    make = OPTS[name]
    rec = Record()
    eager = _train(fused, lambda: make(use_ema=True, ema_momentum=M), 8, spe=1, graph=False, callbacks=[rec])
    graphs = _train(fused, lambda: make(use_ema=True, ema_momentum=M), 8, spe=4)
    off = _train(fused, make, 8, spe=4)
    assert eager._trainer.kind == graphs._trainer.kind == off._trainer.kind == kind, getattr(graphs, "_fused_reason", 0)
    assert SLOT not in off.optimizer.slots()
    assert len(rec.ws) == 8 and rec.its == list(range(1, 9))
    want = ER.fold(rec.w0, rec.ws, M)
    assert not _same(want, rec.w0) and not _same(want, rec.ws[-1])
    assert _same(rec.ws[-1], _w(off)), "the average perturbed the weights"
    assert ER.same_bits(_e(eager), want), float(np.abs(_e(eager) - want).max())
    assert ER.same_bits(_e(graphs), want), float(np.abs(_e(graphs) - want).max())
    for i in range(8):  # the eager run's average after every step, too
        assert ER.same_bits(rec.es[i], ER.fold(rec.w0, rec.ws[:i + 1], M)), i


@pytest.mark.parametrize("fused,name", [(True, "sgd"), (True, "adam"), (False, "adam")],
                         ids=["fused-sgd", "fused-adam", "generic-adam"])
def test_graphs_with_overwrite_steps_match_eager_and_are_keyed_by_phase(fused, name):
    """f = 3, steps_per_execution = 4, 12 steps: the executions start at step counts 0, 4 and 8, i.e. at overwrite
    phases 0, 1 and 2, and each bakes other steps' overwrites in.  W and E are bit-identical to the eager run."""
    make = lambda: OPTS[name](use_ema=True, ema_momentum=M, ema_overwrite_frequency=3)  # noqa: E731
    mg = _train(fused, make, 12, spe=4)
    me = _train(fused, make, 12, spe=4, graph=False)
    tr = mg._trainer
    assert tr.kind == me._trainer.kind == ("fused" if fused else "generic"), getattr(mg, "_fused_reason", None)
    phases = sorted({k[-1][1] for k in tr._graphs if isinstance(k[-1], tuple) and k[-1][0] == "ema"})
    if fused:
        assert phases == [0, 1, 2], list(tr._graphs)
    else:  # (the generic engine runs its first execution at a batch size eagerly)
        assert phases == [1, 2], list(tr._graphs)
    assert not me._trainer._graphs or all(g[0] is None for g in me._trainer._graphs.values()), "an eager run"
    assert mg.optimizer.iterations == me.optimizer.iterations == 12
    assert _same(_e(mg), _e(me)) and _same(_w(mg), _w(me))
    assert _same(_w(mg), _e(mg))  # (step 12 overwrote, and so did the end of fit)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "generic"])
def test_overwrite_steps_are_taken_at_multiples_of_the_frequency(fused):
    """f = 3, 7 eager steps: after steps 3 and 6 the live weights have the average's bits, after no other."""
    rec = Record()
    _train(fused, lambda: O.Adam(1e-3, use_ema=True, ema_momentum=M, ema_overwrite_frequency=3), 7, spe=1,
           graph=False, callbacks=[rec])
    assert rec.its == list(range(1, 8))
    assert [_same(w, e) for w, e in zip(rec.ws, rec.es)] == [False, False, True, False, False, True, False]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "generic"])
def test_fit_ends_with_the_averaged_weights_and_evaluate_uses_them(fused):
    rec = Record()
    m = _train(fused, lambda: O.SGD(0.05, momentum=0.9, use_ema=True, ema_momentum=M), 8, spe=4, callbacks=[rec])
    live = rec.ws[-1]
    assert not _same(live, _e(m)), "the average equals the live weights: nothing to tell apart"
    assert _same(_w(m), _e(m)), "fit did not end with W = E"
    x, y = F._data(1024)
    with _env(TDL_DISABLE_FUSED="0" if fused else "1"):
        got = m.evaluate(_pipeline(x, y, 16), steps=4, verbose=0, return_dict=True)["loss"]
        averaged = [v.copy() for v in m.get_weights()]
        m._W.copy_(torch.from_numpy(live).to(m._W.device))
        other = m.evaluate(_pipeline(x, y, 16), steps=4, verbose=0, return_dict=True)["loss"]
        m.set_weights(averaged)
        again = m.evaluate(_pipeline(x, y, 16), steps=4, verbose=0, return_dict=True)["loss"]
    # (the fused evaluation adds its per-sample losses with f32 atomics: two evaluations of the same weights agree
    # to the rounding of 64 additions, 64 * 2^-24 < 1e-5 relative, not bit for bit)
    assert abs(got - again) <= 1e-5 * abs(got) and abs(got - other) > 1e-3 * abs(got), (got, again, other)


def test_checkpoint_between_two_overwrites_resumes_bit_exactly():
    """f = 4, eager generic engine, 8 steps; the state after step 6 (live weights and state_dict(), the average in
    it) goes into a fresh model and optimizer, which runs steps 7 and 8 on the same batches."""
    make = lambda: O.Adam(1e-3, use_ema=True, ema_momentum=M, ema_overwrite_frequency=4)  # noqa: E731

    class Snap(tdl.keras.callbacks.Callback):
        st = weights = None

        def on_train_batch_end(self, batch, logs=None):
            if self.model.optimizer.iterations == 6:
                st = self.model.optimizer.state_dict()  # (on the CPU its tensors alias the live slots)
                Snap.st = dict(st, slots={k: v.clone() for k, v in st["slots"].items()})
                Snap.weights = [w.copy() for w in self.model.get_weights()]

    full = _train(False, make, 8, spe=1, graph=False, callbacks=[Snap()])
    st = Snap.st
    assert st["iterations"] == 6 and SLOT in st["slots"]
    with _env(TDL_DISABLE_FUSED="1"):
        tdl.keras.backend.clear_session()
        with tdl.distribute.MirroredStrategy(devices=["/gpu:0"]).scope():
            again = build_mnist_cnn()
            again.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=make(),
                          metrics=[tdl.keras.metrics.SparseCategoricalAccuracy()], steps_per_execution=1)
    again.set_weights(Snap.weights)
    again.optimizer.load_state_dict(st)
    _train(False, None, 2, spe=1, graph=False, skip=96, model=again)
    assert again._trainer.kind == "generic" and again.optimizer.iterations == full.optimizer.iterations == 8
    assert _same(_e(again), _e(full)), "the restored average was not kept"
    assert _same(_w(again), _w(full))


def test_plain_sgd_with_ema_keeps_the_update_inside_finalize():
    """The engine's own path flag: plain SGD + EMA still updates inside the finalize launch (the stand-alone
    kernel follows it); momentum SGD + EMA goes through its update kernel, the average inside."""
    plain = _train(True, lambda: O.SGD(0.05, use_ema=True), 4, spe=4)
    assert plain._trainer.kind == "fused" and plain._trainer._plain_sgd
    assert plain._trainer.update_path == "sgd-in-finalize"
    mom = _train(True, lambda: O.SGD(0.05, momentum=0.9, use_ema=True), 4, spe=4)
    assert mom._trainer.kind == "fused" and mom._trainer.update_path == "update-kernel"
    off = _train(True, lambda: O.SGD(0.05), 4, spe=4)
    assert off._trainer.update_path == "sgd-in-finalize" and SLOT not in off.optimizer.slots()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "generic"])
def test_with_accumulation_the_average_moves_on_apply_micro_steps_only(fused):
    """k = 2, f = 4, 8 eager micro-steps: E changes on micro-steps 2, 4, 6, 8 only and is the numpy step from the
    weights those updates left; micro-steps 4 and 8 overwrite."""
    rec = Record()
    _train(fused, lambda: O.Adam(1e-3, gradient_accumulation_steps=2, use_ema=True, ema_momentum=M,
                                 ema_overwrite_frequency=4), 8, spe=1, graph=False, callbacks=[rec])
    assert rec.its == list(range(1, 9))
    e, w = rec.w0, rec.w0
    for i in range(8):
        if i % 2 == 0:
            assert _same(rec.es[i], e) and _same(rec.ws[i], w), f"micro-step {i + 1} moved E or W"
            continue
        assert not _same(rec.es[i], e), f"apply micro-step {i + 1} left E alone"
        if (i + 1) % 4:
            assert ER.same_bits(rec.es[i], ER.step(e, rec.ws[i], M, 1)[0]), i
            assert not _same(rec.ws[i], rec.es[i])
        else:
            assert _same(rec.ws[i], rec.es[i]), f"micro-step {i + 1} did not overwrite"
        e, w = rec.es[i], rec.ws[i]


BODY = """
import json, os, sys, numpy as np, torch
import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.models.mnist_cnn import build_mnist_cnn
from tensorflow_distributed_learning_amd.data.tfds import synthetic_mnist
from tensorflow_distributed_learning_amd.parallel import consistency
out = sys.argv[1]
strategy = tdl.distribute.MirroredStrategy()
R, rank = strategy.num_replicas_in_sync, strategy.extended.rank
comm = strategy.extended.communicator
tdl.keras.utils.set_random_seed(5)
x, y = synthetic_mnist(256, 2)
ds = tdl.data.Dataset.from_tensor_slices((x.reshape(-1, 28, 28, 1), y))
ds = ds.map(lambda i, l: (i.to(torch.float32) / 255, l)).cache().batch(16).repeat()
with strategy.scope():
    m = build_mnist_cnn()
    opt = tdl.keras.optimizers.SGD(0.05, use_ema=True, ema_momentum=0.9, ema_overwrite_frequency=3)
    m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt,
              metrics=["sparse_categorical_accuracy"], steps_per_execution=4)
m.fit(ds, epochs=1, steps_per_epoch=8, verbose=0)
tr = m._trainer
E = opt.slots()["ema"]
same = bool(consistency.replicas_identical(comm, E)) and bool(consistency.replicas_identical(comm, tr.W))
np.save(os.path.join(out, f"e{rank}.npy"), E.cpu().numpy())
np.save(os.path.join(out, f"w{rank}.npy"), tr.W.cpu().numpy())
json.dump({"engine": tr.kind, "plain": bool(tr._plain_sgd), "path": tr.update_path, "identical": same,
           "iterations": int(opt.iterations)}, open(os.path.join(out, f"r{rank}.json"), "w"))
"""


@pytest.mark.slow
def test_two_replicas_keep_the_same_average(tmp_path):
    """2 replica processes sharing the GPU, b = 8 each, plain SGD + EMA with f = 3, 8 steps in executions of 4 on
    the fused engine: E and W are bit-identical on both ranks, and plain SGD stayed on a plain path."""
    s = tmp_path / "job.py"
    s.write_text(textwrap.dedent(BODY))
    env = dict(os.environ, PYTHONPATH=ROOT, TDL_SHARE_GPU="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "TF_CONFIG"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "tensorflow_distributed_learning_amd.launch", "--nproc-per-node", "2",
                        str(s), str(tmp_path)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    a, b = (json.load(open(tmp_path / f"r{i}.json")) for i in range(2))
    assert a["engine"] == b["engine"] == "fused" and a["plain"] and b["plain"]
    assert a["path"] == b["path"], (a, b)  # (which plain path depends on the communicator the two processes got)
    assert a["identical"] and b["identical"] and a["iterations"] == b["iterations"] == 8
    e0, e1, w0, w1 = (np.load(tmp_path / f) for f in ("e0.npy", "e1.npy", "w0.npy", "w1.npy"))
    assert _same(e0, e1) and _same(w0, w1)
    assert _same(w0, e0)  # (the end of fit stored W = E on both)
