"""The weight EMA (``use_ema``) without a GPU: the torch path of ``Optimizer.ema_after`` / ``apply_flat`` is the
numpy step of tests/ema_refs.py bit for bit, the keywords are validated and round-trip through the config,
``use_ema=False`` changes nothing, overwrite steps fall on multiples of the frequency, ``fit`` ends with the
averaged weights, and the generic engine (one replica, and two replicas in one process) trains with it."""
import types

import numpy as np
import pytest
import torch

import ema_refs as ER
import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.engine import execution, fused

from test_accum_cpu import _cnn, _data, _fit, _grads

O = tdl.keras.optimizers
SLOT = "ema"


def _bits(a, b) -> bool:
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


@pytest.mark.parametrize("m", [0.0, 0.5, 0.99, 0.999, 1.0])
def test_cpu_fold_is_the_numpy_step(m):
    """``ema_after`` over slabs with the special values planted: E has numpy's bits, W is left alone (mode 1)."""
    n = 300
    rng = np.random.default_rng(1)
    e0, w0 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    ER.plant_specials([e0, w0], m)
    opt = O.SGD(0.1, use_ema=True, ema_momentum=m)
    W = torch.from_numpy(w0.copy())
    opt.build(n, W.device)
    opt.load_state_dict({"iterations": 0, "slots": {SLOT: torch.from_numpy(e0.copy())}})
    opt.ema_after(W)
    e_ref, _ = ER.step(e0, w0, m, 1)
    assert ER.same_bits(opt.slots()[SLOT].numpy(), e_ref)
    assert _bits(W.numpy(), w0)
    assert np.isnan(e_ref).any() and np.isinf(e_ref).any()


@pytest.mark.parametrize("make", [lambda **kw: O.SGD(0.1, **kw), lambda **kw: O.SGD(0.1, momentum=0.9, **kw),
                                  lambda **kw: O.Adam(1e-2, **kw), lambda **kw: O.RMSprop(1e-2, **kw),
                                  lambda **kw: O.Adagrad(1e-2, **kw)],
                         ids=["sgd", "sgd-momentum", "adam", "rmsprop", "adagrad"])
def test_apply_flat_moves_the_average_and_never_the_weights(make):
    """6 steps through ``apply_flat``: E starts as W0, follows every update as the numpy fold of the weights, and
    the weights are those of the optimizer without EMA."""
    n, m = 257, 0.9
    gs = _grads(n, 6, seed=3)
    w0 = np.random.default_rng(4).standard_normal(n).astype(np.float32)
    a, b = make(use_ema=True, ema_momentum=m), make()
    Wa, Wb = torch.from_numpy(w0.copy()), torch.from_numpy(w0.copy())
    ws = []
    for g in gs:
        a.apply_flat(Wa, torch.from_numpy(g.copy()))
        b.apply_flat(Wb, torch.from_numpy(g.copy()))
        assert _bits(Wa.numpy(), Wb.numpy())
        ws.append(Wa.numpy().copy())
        assert ER.same_bits(a.slots()[SLOT].numpy(), ER.fold(w0, ws, m))
    assert SLOT not in b.slots() and a.iterations == b.iterations == 6
    assert not _bits(a.slots()[SLOT].numpy(), w0) and not _bits(a.slots()[SLOT].numpy(), ws[-1])


@pytest.mark.parametrize("bad", [dict(ema_momentum=-0.1), dict(ema_momentum=1.5), dict(ema_momentum="0.9"),
                                 dict(ema_momentum=True), dict(ema_overwrite_frequency=0),
                                 dict(ema_overwrite_frequency=-2), dict(ema_overwrite_frequency=2.0),
                                 dict(ema_overwrite_frequency=True),
                                 dict(ema_overwrite_frequency=3, gradient_accumulation_steps=2)])
@pytest.mark.parametrize("on", [True, False])
def test_invalid_keywords_raise_value_error(bad, on):
    """(also with use_ema off: the momentum and the frequency are ignored there, but still validated)"""
    for cls in (O.SGD, O.Adam, O.LAMB, O.legacy.RMSprop):
        with pytest.raises(ValueError):
            cls(use_ema=on, **bad)


def test_boundary_keywords_are_accepted():
    O.SGD(use_ema=True, ema_momentum=0, ema_overwrite_frequency=1)
    O.Adam(use_ema=True, ema_momentum=1, ema_overwrite_frequency=None)
    O.Adam(use_ema=True, ema_overwrite_frequency=4, gradient_accumulation_steps=2)
    with pytest.raises(TypeError):
        O.SGD(use_emma=True)


def test_config_round_trip():
    for cls in (O.SGD, O.Adam, O.AdamW, O.RMSprop, O.Adagrad, O.LARS, O.LAMB):
        opt = cls(use_ema=True, ema_momentum=0.95, ema_overwrite_frequency=6)
        cfg = opt.get_config()
        assert (cfg["use_ema"], cfg["ema_momentum"], cfg["ema_overwrite_frequency"]) == (True, 0.95, 6)
        again = cls.from_config(cfg)
        assert (again.use_ema, again.ema_momentum, again.ema_overwrite_frequency) == (True, 0.95, 6)
        assert again.get_config() == cfg
        via = O.get(O.serialize(opt))
        assert type(via) is cls and via.use_ema and via.ema_overwrite_frequency == 6
        d = cls().get_config()
        assert (d["use_ema"], d["ema_momentum"], d["ema_overwrite_frequency"]) == (False, 0.99, None)


def test_off_allocates_no_slot_and_a_fit_is_bit_identical():
    """use_ema=False (with the other two keywords set): no slot, the graph key of the parent commit, and a 5-step
    CPU fit whose weights are the bits of a run without the keywords."""
    tdl.keras.backend.clear_session()
    x, y = _data(128)
    for make in (lambda **kw: O.SGD(0.05, momentum=0.9, **kw), lambda **kw: O.Adam(1e-2, **kw)):
        ma, _ = _fit(x, y, 16, 5, lambda: make(use_ema=False, ema_momentum=0.5, ema_overwrite_frequency=2))
        mb, _ = _fit(x, y, 16, 5, make)
        assert SLOT not in ma.optimizer.slots() and set(ma.optimizer.slots()) == set(mb.optimizer.slots())
        assert ma.optimizer._ema_mode() == 0
        for a, b in zip(ma.get_weights(), mb.get_weights()):
            assert _bits(a, b)
    off = O.Adam(use_ema=False, ema_overwrite_frequency=2)
    assert execution.accum_key(off, ("dev", 4, 16)) == ("dev", 4, 16)
    acc = O.Adam(gradient_accumulation_steps=3)
    acc.iterations = 4
    assert execution.accum_key(acc, ("dev", 4, 16), 1) == ("dev", 4, 16, 2)  # (as on the parent commit)
    assert execution.phase_period(off, 4) == 1 and execution.phase_period(acc, 4) == 3


def test_graph_key_and_modes_follow_the_overwrite_phase():
    opt = O.SGD(0.1, use_ema=True, ema_overwrite_frequency=3)
    assert [opt._ema_mode(t) for t in range(7)] == [1, 1, 2, 1, 1, 2, 1]
    opt.iterations = 4
    assert [opt._ema_mode(t) for t in range(3)] == [1, 2, 1]
    keys = {execution.accum_key(opt, (4, 16, 0), t) for t in (0, 4, 8, 12)}
    assert keys == {(4, 16, 0, ("ema", 1)), (4, 16, 0, ("ema", 2)), (4, 16, 0, ("ema", 0))}
    assert execution.phase_period(opt, 4) == 3 and execution.phase_period(opt, 3) == 1
    assert O.SGD(0.1, use_ema=True)._ema_mode(5) == 1  # (no frequency: never an overwrite step)
    assert execution.accum_key(O.SGD(0.1, use_ema=True), (4, 16, 0)) == (4, 16, 0)
    both = O.SGD(0.1, use_ema=True, ema_overwrite_frequency=4, gradient_accumulation_steps=2)
    both.iterations = 3
    assert execution.accum_key(both, (4, 16, 0)) == (4, 16, 0, ("ema", 3))


def test_overwrite_steps_are_taken_at_the_right_iterations():
    """f = 3 through ``apply_flat`` on the CPU: W = E after updates 3 and 6 and after no other, every E the numpy
    step from the weights the update left."""
    n, m = 129, 0.75
    gs = _grads(n, 7, seed=5)
    w0 = np.random.default_rng(6).standard_normal(n).astype(np.float32)
    opt, ref = O.SGD(0.1, momentum=0.9, use_ema=True, ema_momentum=m, ema_overwrite_frequency=3), O.SGD(0.1, momentum=0.9)
    W, Wr = torch.from_numpy(w0.copy()), torch.from_numpy(w0.copy())
    e = w0.copy()
    for j, g in enumerate(gs):
        opt.apply_flat(W, torch.from_numpy(g.copy()))
        ref.apply_flat(Wr, torch.from_numpy(g.copy()))  # (the same update from the same weights)
        e, w_ref = ER.step(e, Wr.numpy(), m, ER.mode_of(j + 1, 3))
        Wr.copy_(torch.from_numpy(w_ref))
        assert ER.same_bits(opt.slots()[SLOT].numpy(), e), j
        assert _bits(W.numpy(), w_ref), j
        assert _bits(W.numpy(), e) == ((j + 1) % 3 == 0), j


def test_with_accumulation_the_average_moves_on_apply_micro_steps_only():
    n, m = 100, 0.9
    gs = _grads(n, 8, seed=7)
    w0 = np.random.default_rng(8).standard_normal(n).astype(np.float32)
    opt = O.Adam(1e-2, gradient_accumulation_steps=2, use_ema=True, ema_momentum=m, ema_overwrite_frequency=4)
    W = torch.from_numpy(w0.copy())
    e = w0.copy()
    for j, g in enumerate(gs):
        before_w, before_e = W.numpy().copy(), (opt.slots()[SLOT].numpy().copy() if j else w0)
        opt.apply_flat(W, torch.from_numpy(g.copy()))
        if j % 2 == 0:
            assert _bits(W.numpy(), before_w) and _bits(opt.slots()[SLOT].numpy(), before_e), j
            continue
        assert not _bits(opt.slots()[SLOT].numpy(), before_e), j
        assert _bits(W.numpy(), opt.slots()[SLOT].numpy()) == ((j + 1) % 4 == 0), j
    assert opt.iterations == 8


def test_lars_lamb_and_legacy_accept_the_keywords():
    from tensorflow_distributed_learning_amd.engine.slab import SlabLayout

    lay = SlabLayout.from_shapes((("a/kernel", (8, 5)), ("a/bias", (5,)), ("b/kernel", (5, 3))))
    n, m = lay.total, 0.9
    gs = _grads(n, 3, seed=8)
    w0 = np.random.default_rng(9).standard_normal(n).astype(np.float32)
    for cls in (O.LARS, O.LAMB):
        opt, ref = cls(0.1, use_ema=True, ema_momentum=m), cls(0.1)
        opt.set_layout(lay)
        ref.set_layout(lay)
        W, Wr = torch.from_numpy(w0.copy()), torch.from_numpy(w0.copy())
        ws = []
        for g in gs:
            opt.apply_flat(W, torch.from_numpy(g.copy()))
            ref.apply_flat(Wr, torch.from_numpy(g.copy()))
            ws.append(W.numpy().copy())
        assert torch.equal(W, Wr)
        assert ER.same_bits(opt.slots()[SLOT].numpy(), ER.fold(w0, ws, m)), cls.__name__
    for cls in (O.legacy.SGD, O.legacy.Adam, O.legacy.RMSprop, O.legacy.Adagrad):
        opt = cls(use_ema=True, ema_momentum=0.5, ema_overwrite_frequency=2)
        W = torch.from_numpy(w0.copy())
        opt.apply_flat(W, torch.from_numpy(gs[0].copy()))
        assert ER.same_bits(opt.slots()[SLOT].numpy(), ER.step(w0, W.numpy(), 0.5, 1)[0])


def test_finalize_variable_values_for_custom_loops():
    from tensorflow_distributed_learning_amd.parallel.values import Variable

    v = [Variable(torch.ones(3, 2)), Variable(torch.full((4,), 2.0))]
    opt = O.SGD(0.5, use_ema=True, ema_momentum=0.5)
    opt.finalize_variable_values(v)  # (before the first update: a no-op)
    assert float(v[0].read_value().sum()) == 6.0
    opt.apply_gradients([(torch.ones(3, 2), v[0]), (torch.ones(4), v[1])])
    assert np.allclose(v[0].numpy(), 0.5) and np.allclose(v[1].numpy(), 1.5)
    opt.finalize_variable_values(v)
    assert np.allclose(v[0].numpy(), 0.75) and np.allclose(v[1].numpy(), 1.75)
    off = O.SGD(0.5)
    off.apply_gradients([(torch.ones(3, 2), v[0]), (torch.ones(4), v[1])])
    off.finalize_variable_values(v)
    assert np.allclose(v[0].numpy(), 0.25)


def test_cpu_fit_ends_with_the_averaged_weights():
    """The end-of-fit overwrite on the CPU path: W = E bitwise after fit, E the fold of the live weights."""
    tdl.keras.backend.clear_session()
    x, y = _data(128)
    m = 0.9

    class Live(tdl.keras.callbacks.Callback):
        w0, ws = None, []

        def on_train_begin(self, logs=None):
            Live.w0, Live.ws = self.model._W.detach().numpy().copy(), []

        def on_train_batch_end(self, batch, logs=None):
            Live.ws.append(self.model._W.detach().numpy().copy())

    tdl.keras.utils.set_random_seed(7)
    ds = tdl.data.Dataset.from_tensor_slices((x, y)).batch(16).repeat()
    with tdl.distribute.MirroredStrategy(devices=["/cpu:0"]).scope():
        model = _cnn()
        model.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                      optimizer=O.SGD(0.05, momentum=0.9, use_ema=True, ema_momentum=m))
    model.fit(ds, epochs=1, steps_per_epoch=5, verbose=0, callbacks=[Live()])
    E = model.optimizer.slots()[SLOT].numpy()
    assert len(Live.ws) == 5 and ER.same_bits(E, ER.fold(Live.w0, Live.ws, m))
    assert _bits(model._W.numpy(), E) and not _bits(E, Live.ws[-1])
    ref, _ = _fit(x, y, 16, 5, lambda: O.SGD(0.05, momentum=0.9))
    assert _bits(ref._W.numpy(), Live.ws[-1]), "the average perturbed the training"
    flat = np.concatenate([w.ravel() for w in model.get_weights()])
    assert np.isin(flat, E).all()  # (the variables are views of the slab: they hold the averaged values)


def test_cpu_checkpoint_carries_the_average_and_resumes_bit_exactly():
    tdl.keras.backend.clear_session()
    x, y = _data(128)
    make = lambda: O.Adam(1e-2, use_ema=True, ema_momentum=0.9, ema_overwrite_frequency=4)  # noqa: E731

    class Snap(tdl.keras.callbacks.Callback):
        st = weights = None

        def on_train_batch_end(self, batch, logs=None):
            if self.model.optimizer.iterations == 6:
                st = self.model.optimizer.state_dict()  # (on the CPU its tensors alias the live slots)
                Snap.st = dict(st, slots={k: v.clone() for k, v in st["slots"].items()})
                Snap.weights = [w.copy() for w in self.model.get_weights()]

    tdl.keras.utils.set_random_seed(7)
    with tdl.distribute.MirroredStrategy(devices=["/cpu:0"]).scope():
        full = _cnn()
        full.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=make())
    full.fit(tdl.data.Dataset.from_tensor_slices((x, y)).batch(16).repeat(), epochs=1, steps_per_epoch=8, verbose=0,
             callbacks=[Snap()])
    assert Snap.st["iterations"] == 6 and SLOT in Snap.st["slots"]
    with tdl.distribute.MirroredStrategy(devices=["/cpu:0"]).scope():
        again = _cnn()
        again.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=make())
    again.set_weights(Snap.weights)
    again.optimizer.load_state_dict(Snap.st)
    _fit(x[96:], y[96:], 16, 2, None, model=again)
    assert again.optimizer.iterations == full.optimizer.iterations == 8
    assert _bits(again.optimizer.slots()[SLOT].numpy(), full.optimizer.slots()[SLOT].numpy())
    assert _bits(again._W.numpy(), full._W.numpy())


def test_mirrored_two_cpu_devices_in_one_process_stay_identical():
    tdl.keras.backend.clear_session()
    x, y = _data(256)
    make = lambda: O.SGD(0.05, momentum=0.9, use_ema=True, ema_momentum=0.9, ema_overwrite_frequency=4)  # noqa: E731
    s = tdl.distribute.MirroredStrategy(devices=["/cpu:0", "/cpu:1"])
    m, h = _fit(x, y, 32, 6, make, strategy=s)
    assert type(m._trainer).__name__ == "ThreadedGroupTrainer" and m._trainer.kind == "generic"
    (clone,) = m._local_clones
    assert m.optimizer.iterations == clone.optimizer.iterations == 6
    assert clone.optimizer.use_ema and clone.optimizer.ema_overwrite_frequency == 4
    assert _bits(m.optimizer.slots()[SLOT].numpy(), clone.optimizer.slots()[SLOT].numpy())
    for a, b in zip(m.get_weights(), clone.get_weights()):
        assert _bits(a, b), "replicas differ"
    assert _bits(m._W.numpy(), m.optimizer.slots()[SLOT].numpy()) and _bits(clone._W.numpy(), m._W.numpy())
    assert np.isfinite(h.history["loss"]).all()
    s.shutdown()


def test_fused_eligibility_names_a_missing_weight_ema_kernel(monkeypatch):
    """eligible() with everything in front of the optimizer check stubbed (as in tests/test_accum_cpu.py): an EMA
    optimizer passes it, plain SGD + EMA stays plain, and a stale extension without the kernel is named."""
    from tensorflow_distributed_learning_amd import ops
    from tensorflow_distributed_learning_amd.keras import losses

    kernels = types.SimpleNamespace(adam=1, rmsprop=1, adagrad=1, sgd=1, clip_norm=1, grad_accum=1, layer_tables=1,
                                    weight_ema=1)
    monkeypatch.setattr(ops, "hip_available", lambda: True)
    monkeypatch.setattr(ops, "hip", lambda: kernels)
    monkeypatch.setattr(fused, "_is_reference_cnn", lambda m: True)
    monkeypatch.delenv("TDL_DISABLE_FUSED", raising=False)

    def model(opt):
        strategy = types.SimpleNamespace(extended=types.SimpleNamespace(device=torch.device("cuda", 0)))
        return types.SimpleNamespace(_get_strategy=lambda: strategy, _dtype_policy=lambda: "float32",
                                     loss=losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt,
                                     compiled_metrics=[])

    for opt in (O.Adam(1e-3, use_ema=True), O.SGD(0.05, use_ema=True, ema_overwrite_frequency=3),
                O.LAMB(1e-3, use_ema=True), O.SGD(0.05, momentum=0.9, clipnorm=1.0, use_ema=True)):
        assert fused.eligible(model(opt)) is None
    plain = fused.FusedMnistTrainer._plain_sgd.fget
    assert plain(types.SimpleNamespace(optimizer=O.SGD(0.05, use_ema=True)))
    del kernels.weight_ema
    reason = fused.eligible(model(O.Adam(1e-3, use_ema=True)))
    assert "weight_ema" in reason and "rebuild" in reason
    assert fused.eligible(model(O.Adam(1e-3))) is None
    assert fused.eligible(model(O.Adam(1e-3, use_ema=False, ema_momentum=0.5))) is None
