"""LARS and LAMB without a GPU: the CPU formulas of keras/optimizers.py against the f64 references of
tests/layerwise_refs.py on the kernel tests' layout (with the caps on the CPU path's own error that the GPU
tolerances rest on), the exclusion patterns, configuration, the layout contract, the custom-loop path and a
2-process fit.

CH: the device chunk size is a property of the extension; without one the layout is taken at 2048, the value
csrc/kernels/optim.h sets (the CPU path does not depend on it, only the sizes of the layout do).
"""
import json
import os
import subprocess
import sys
import textwrap
import types

import numpy as np
import pytest
import torch

import layerwise_refs as LR
import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.engine import fused
from tensorflow_distributed_learning_amd.engine.slab import SlabLayout

O = tdl.keras.optimizers
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = 2048
E_W_CAP, RATIO_CAP = 1e-6, 1e-5  # a CPU path worse than this is wrong, not merely rounded

VARIANTS = [("lars", False), ("lars", True), ("lamb", False)]


@pytest.mark.parametrize("mode", LR.MODES)
@pytest.mark.parametrize("kind,nesterov", VARIANTS, ids=["lars", "lars-nesterov", "lamb"])
def test_cpu_formulas_match_f64_reference(kind, nesterov, mode):
    c = LR.case(CH)
    assert c.total == 10880  # (41,600 at a chunk of 8192)
    E, rel = LR.cpu_error(CH, kind, nesterov, mode)
    print(f"{kind} nesterov={nesterov} {mode}: E = {E}, relative ratio error {rel:.3e}")
    assert E["w"] <= E_W_CAP, E
    assert rel <= RATIO_CAP, rel
    for name, e in E.items():
        assert e <= 4e-6, (name, e)


def test_reference_ratios_cover_every_branch():
    """The inputs' ratios span 2e-3 ... 100 (LAMB), with the zero-gradient decayed variable at 1 / wd, and no
    ``where`` decision hangs on a rounding: excluded / zero-norm variables have ratio exactly 1."""
    c = LR.case(CH)
    _, rr, norms = LR.run_ref(c, "lamb", False, "none", [None] * 3)
    for k, (r, nm) in enumerate(zip(rr, norms)):
        assert r[LR.NO_ADAPT] == 1.0
        assert abs(r[LR.ZERO_G] - 1.0 / LR.f32(LR.WD)) < 1e-3 * r[LR.ZERO_G]
        if k == 0:  # (the all-zero weights move with ratio 1 in the first step and have a norm from then on)
            assert r[LR.ZERO_W] == 1.0 and nm[LR.ZERO_W, 0] == 0.0
        assert (np.delete(nm[:, 0], LR.ZERO_W) > 1e-3).all() and (nm[:, 1] > 1e-3).all()
    assert np.concatenate(rr).max() > 50
    _, rr, norms = LR.run_ref(c, "lars", False, "none", [None] * 3)
    assert np.concatenate(rr).min() < 1e-2
    for k, (r, nm) in enumerate(zip(rr, norms)):
        assert r[LR.NO_ADAPT] == 1.0 and r[LR.ZERO_G] == 1.0 and nm[LR.ZERO_G, 1] == 0.0
        if k == 0:
            assert r[LR.ZERO_W] == 1.0 and nm[LR.ZERO_W, 0] == 0.0
        others = [i for i in range(c.V) if i not in (LR.NO_ADAPT, LR.ZERO_W, LR.ZERO_G)]
        assert (r[others] < 0.1).all() and (r[others] > 0).all()


def test_nan_gradient_gives_ratio_one_and_stays_in_its_elements():
    c = LR.case(CH)
    for kind in ("lars", "lamb"):
        opt = LR.make_optimizer(c, kind, False, "none")
        g = c.grads[0].copy()
        p = c.offsets[7] + CH + 7
        g[p] = np.nan
        W = torch.from_numpy(c.w0.copy())
        opt.apply_flat(W, torch.from_numpy(g))
        assert opt._cpu_ratios[7] == 1.0
        nan = torch.isnan(W).numpy()
        assert nan[p] and nan.sum() == 1


def test_exclusion_patterns_on_the_reference_cnn_names():
    from tensorflow_distributed_learning_amd.models.mnist_cnn import build_mnist_cnn

    m = build_mnist_cnn()
    m._ensure_slabs()
    offs, sizes, names = m._layout.layer_spans()
    assert len(names) == 8 and sum("bias" in n for n in names) == 4 and sum("kernel" in n for n in names) == 4
    opt = O.LAMB(weight_decay_rate=0.01, exclude_from_weight_decay=["bias"])
    wd, adapt = opt.layer_operands(m._layout)
    assert wd == [0.0 if "bias" in n else 0.01 for n in names]
    assert adapt == ["bias" not in n for n in names], "layer adaptation defaults to the decay list"
    opt = O.LARS(weight_decay_rate=1e-4, exclude_from_weight_decay=["bias"], exclude_from_layer_adaptation=[])
    wd, adapt = opt.layer_operands(m._layout)
    assert adapt == [True] * 8 and wd.count(0.0) == 4
    opt = O.LARS(weight_decay_rate=1e-4, exclude_from_layer_adaptation=[r"dense.*/kernel"])
    wd, adapt = opt.layer_operands(m._layout)
    assert wd == [1e-4] * 8 and adapt == [not ("dense" in n and "kernel" in n) for n in names]
    assert adapt.count(False) == 2


def test_layer_spans():
    lay = SlabLayout.from_shapes([("a", (3, 5)), ("b", ()), ("c", (70,))])
    assert lay.layer_spans() == ([0, 64, 128], [15, 1, 70], ["a", "b", "c"])
    assert lay.total == 256


def test_get_serialize_and_from_config_round_trip():
    assert type(O.get("lars")) is O.LARS and type(O.get("LAMB")) is O.LAMB and O.Lamb is O.LAMB
    a = O.LARS(0.02, momentum=0.8, weight_decay_rate=1e-4, eeta=0.002, epsilon=1e-9, nesterov=True,
               exclude_from_weight_decay=["bias"], exclude_from_layer_adaptation=["bn"], clipnorm=2.0)
    b = O.get(O.serialize(a))
    assert type(b) is O.LARS and b.get_config() == a.get_config()
    assert (b.momentum, b.eeta, b.epsilon, b.nesterov, b.weight_decay_rate) == (0.8, 0.002, 1e-9, True, 1e-4)
    assert b.exclude_from_weight_decay == ["bias"] and b.exclude_from_layer_adaptation == ["bn"] and b.clipnorm == 2.0
    a = O.LAMB(0.003, beta_1=0.8, beta_2=0.99, epsilon=1e-5, weight_decay_rate=0.02, exclude_from_weight_decay=["b"])
    b = O.get(O.serialize(a))
    assert type(b) is O.LAMB and b.get_config() == a.get_config()
    assert (b.beta_1, b.beta_2, b.epsilon, b.weight_decay_rate) == (0.8, 0.99, 1e-5, 0.02)
    assert b.exclude_from_layer_adaptation is None
    d = O.LAMB()
    assert (d.current_lr(), d.beta_1, d.beta_2, d.epsilon, d.weight_decay_rate, d.name) == (
        0.001, 0.9, 0.999, 1e-6, 0.0, "LAMB")
    d = O.LARS()
    assert (d.current_lr(), d.momentum, d.eeta, d.epsilon, d.nesterov, d.name) == (0.01, 0.9, 0.001, 0.0, False, "LARS")
    assert d.weight_decay is None, "the decay is weight_decay_rate, not the decoupled weight_decay"
    assert O.LAMB._needs_step and not O.LARS._needs_step


@pytest.mark.parametrize("cls", [O.LARS, O.LAMB])
def test_layerwise_optimizer_without_a_layout_says_so(cls):
    opt = cls()
    with pytest.raises(ValueError, match="set_layout"):
        opt.build(128, torch.device("cpu"))
    with pytest.raises(ValueError, match="set_layout"):
        opt.apply_flat(torch.zeros(128), torch.zeros(128))
    opt.set_layout(SlabLayout.from_shapes([("a", (100,))]))
    with pytest.raises(ValueError, match="128"):
        opt.build(256, torch.device("cpu"))
    opt.build(128, torch.device("cpu"))
    assert sorted(opt.slots()) == (["momentum"] if cls is O.LARS else ["m", "v"])
    # the base class stores the layout and the existing optimizers ignore it
    sgd = O.SGD(0.1)
    sgd.set_layout(opt._layout)
    sgd.apply_flat(torch.zeros(128), torch.ones(128))


@pytest.mark.parametrize("cls", [O.LARS, O.LAMB])
def test_graph_safe_is_false_when_unbuilt_or_cpu_built(cls):
    opt = cls()
    assert not opt.graph_safe
    opt.set_layout(SlabLayout.from_shapes([("a", (100,))]))
    opt.build(128, torch.device("cpu"))
    assert not opt.graph_safe
    assert opt.last_layer_ratios is None and opt.last_layer_norms is None


def test_fused_eligibility_names_neither_class_as_unsupported(monkeypatch):
    from tensorflow_distributed_learning_amd import ops
    from tensorflow_distributed_learning_amd.keras import losses

    kernels = types.SimpleNamespace(adam=1, rmsprop=1, adagrad=1, sgd=1, clip_norm=1, layer_tables=1)
    monkeypatch.setattr(ops, "hip_available", lambda: True)
    monkeypatch.setattr(ops, "hip", lambda: kernels)
    monkeypatch.setattr(fused, "_is_reference_cnn", lambda m: True)
    monkeypatch.delenv("TDL_DISABLE_FUSED", raising=False)

    def model(opt):
        strategy = types.SimpleNamespace(extended=types.SimpleNamespace(device=torch.device("cuda", 0)))
        return types.SimpleNamespace(_get_strategy=lambda: strategy, _dtype_policy=lambda: "float32",
                                     loss=losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt,
                                     compiled_metrics=[])

    for opt in (O.LARS(0.05, weight_decay_rate=1e-4), O.LAMB(1e-3, weight_decay_rate=0.01), O.LAMB(clipnorm=1.0)):
        assert fused.eligible(model(opt)) is None
        assert not fused.FusedMnistTrainer._plain_sgd.fget(types.SimpleNamespace(optimizer=opt))
    del kernels.layer_tables
    for opt in (O.LARS(), O.LAMB()):
        reason = fused.eligible(model(opt))
        assert "layer_tables" in reason and "rebuild" in reason


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_custom_loop_apply_gradients_equals_apply_flat_on_the_packed_layout(kind):
    from tensorflow_distributed_learning_amd.parallel.values import Variable

    rng = np.random.default_rng(4)
    shapes = [("conv/kernel", (3, 3, 2, 5)), ("conv/bias", (5,)), ("dense/kernel", (70, 3)), ("scalar", ())]
    make = lambda: (O.LARS(0.05, weight_decay_rate=0.01, exclude_from_weight_decay=["bias"], nesterov=True)  # noqa: E731
                    if kind == "lars" else O.LAMB(0.01, weight_decay_rate=0.01, exclude_from_weight_decay=["bias"]))
    w0 = [rng.standard_normal(s).astype(np.float32) for _, s in shapes]
    grads = [[rng.standard_normal(s).astype(np.float32) for _, s in shapes] for _ in range(2)]
    vs = [Variable(torch.from_numpy(w.copy()), name=n) for (n, _), w in zip(shapes, w0)]
    a = make()
    for g in grads:
        a.apply_gradients([(torch.from_numpy(x.copy()), v) for x, v in zip(g, vs)])
    lay = SlabLayout.from_shapes([(v.name, s) for v, (_, s) in zip(vs, shapes)])
    b = make()
    b.set_layout(lay)
    W = lay.pack([torch.from_numpy(w.copy()) for w in w0])
    for g in grads:
        b.apply_flat(W, lay.pack([torch.from_numpy(x.copy()) for x in g]))
    assert a.iterations == b.iterations == 2
    for v, view, w in zip(vs, lay.views(W), w0):
        assert torch.equal(v.read_value().reshape(view.shape), view)
        assert not np.array_equal(view.numpy(), w)
    assert b.layer_operands(lay)[0] == [0.01, 0.0, 0.01, 0.01]


BODY = """
import json, os, sys, numpy as np, torch
import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.compat import tf
from tensorflow_distributed_learning_amd.models.mnist_cnn import build_mnist_cnn
from tensorflow_distributed_learning_amd.data.tfds import synthetic_mnist
out = sys.argv[1]
strategy = tf.distribute.experimental.MultiWorkerMirroredStrategy()
R = strategy.num_replicas_in_sync
tdl.keras.utils.set_random_seed(5)
x, y = synthetic_mnist(128, 2)
ds = tdl.data.Dataset.from_tensor_slices((x.reshape(-1, 28, 28, 1), y))
ds = ds.map(lambda i, l: (i.to(torch.float32) / 255, l)).batch(16 * R)
opts = tdl.data.Options()
opts.experimental_distribute.auto_shard_policy = tdl.data.experimental.AutoShardPolicy.OFF
ds = ds.with_options(opts)
with strategy.scope():
    m = build_mnist_cnn()
    opt = tdl.keras.optimizers.LARS(0.05, weight_decay_rate=1e-4, exclude_from_weight_decay=["bias"])
    m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt)
w0 = np.concatenate([v.ravel() for v in m.get_weights()])
h = m.fit(ds, epochs=1, steps_per_epoch=3, verbose=0)
w = np.concatenate([v.ravel() for v in m.get_weights()])
json.dump({"R": R, "sum": float(np.abs(w).sum()), "first": [float(v) for v in w[:64]], "moved": float(np.abs(w - w0).max()),
           "iterations": int(opt.iterations), "ratios": [float(r) for r in opt._cpu_ratios]},
          open(os.path.join(out, f"out{strategy.extended.rank}.json"), "w"))
"""


@pytest.mark.slow
def test_two_cpu_workers_fit_with_lars_and_end_identical(tmp_path):
    script = tmp_path / "job.py"
    script.write_text(textwrap.dedent(BODY))
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="",
               TDL_NO_GPU_PARTITION="1")
    for k in ("TF_CONFIG", "RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
              "TDL_LAUNCHED"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "tensorflow_distributed_learning_amd.launch", "--local-workers", "2",
                        str(script), str(tmp_path)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    a, b = (json.load(open(tmp_path / f"out{k}.json")) for k in range(2))
    assert a["R"] == b["R"] == 2 and a["iterations"] == b["iterations"] == 3
    assert a["sum"] == b["sum"] and a["first"] == b["first"] and a["ratios"] == b["ratios"]
    assert a["moved"] > 0
    assert len(a["ratios"]) == 8 and a["ratios"].count(1.0) == 4, "the 4 biases are excluded, the kernels adapt"
