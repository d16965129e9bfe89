"""Gradient accumulation without a GPU: the torch path of ``Optimizer.accumulate`` / ``apply_flat`` is the numpy
fold of tests/accum_refs.py bit for bit, ``iterations`` counts micro-steps, everything but the fold happens on
the cycle's last micro-step only, and the generic engine (one replica, and two replicas in one process) trains
with it."""
import types

import numpy as np
import pytest
import torch

import accum_refs as AR
import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.engine import fused

O = tdl.keras.optimizers
SLOT = "gradient_accumulator"


def _grads(n, count, seed=0, specials=False):
    rng = np.random.default_rng(seed)
    gs = [rng.standard_normal(n).astype(np.float32) for _ in range(count)]
    if specials:
        sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 3.4e38], dtype=np.float32)
        for j, g in enumerate(gs):
            for r in range(len(sp)):
                g[r * len(sp):(r + 1) * len(sp)] = np.roll(sp, r * j)
    return gs


@pytest.mark.parametrize("k", [2, 3, 7])
def test_cpu_fold_is_the_numpy_fold(k):
    """Two cycles through ``accumulate``: the slot and the handed-on gradient have numpy's bits, NaN and Inf
    kept where numpy keeps them."""
    n = 257
    opt = O.SGD(0.1, gradient_accumulation_steps=k)
    gs = _grads(n, 2 * k, seed=k, specials=True)
    a_ref = np.zeros(n, dtype=np.float32)
    for j, g in enumerate(gs):
        G = torch.from_numpy(g.copy())
        mode = AR.mode_of(j % k, k)
        last = opt.accumulate(G)
        assert last == (mode == 2)
        a_ref, g_ref = AR.step(a_ref, g, mode, AR.recip(k))
        assert AR.same_bits(opt.slots()[SLOT].numpy(), a_ref), (k, j)
        assert AR.same_bits(G.numpy(), g_ref), (k, j)
        opt.iterations += 1  # (what apply_flat / the engines do after the fold)
    assert AR.same_bits(g_ref, AR.fold(gs[k:], k))
    assert np.isnan(g_ref).any() and np.isinf(g_ref).any()


def test_iterations_count_micro_steps_and_the_schedule_is_read_at_the_apply_micro_step():
    k, n = 3, 100
    sched = O.schedules.ExponentialDecay(0.5, 2, 0.5)
    opt = O.SGD(sched, gradient_accumulation_steps=k)
    gs = _grads(n, 2 * k, seed=1)
    w0 = np.random.default_rng(2).standard_normal(n).astype(np.float32)
    W = torch.from_numpy(w0.copy())
    want = torch.from_numpy(w0.copy())
    for j, g in enumerate(gs):
        before = W.clone()
        opt.apply_flat(W, torch.from_numpy(g.copy()))
        assert opt.iterations == j + 1
        if j % k != k - 1:
            assert torch.equal(W, before), "a micro-step that is not the cycle's last must not move the weights"
        else:
            cycle = gs[j - k + 1:j + 1]
            lr = float(sched(j))  # iterations before the increment of the apply micro-step: 2, then 5
            assert lr != float(sched(j - k + 1))
            want.add_(torch.from_numpy(AR.fold(cycle, k)), alpha=-lr)
            assert torch.equal(W, want), j


@pytest.mark.parametrize("make", [
    lambda **kw: O.SGD(0.1, momentum=0.9, clipnorm=0.5, **kw),
    lambda **kw: O.AdamW(1e-2, weight_decay=0.1, global_clipnorm=0.5, **kw),
    lambda **kw: O.RMSprop(1e-2, momentum=0.5, clipvalue=0.1, **kw),
    lambda **kw: O.Adagrad(1e-2, **kw),
], ids=["sgd-momentum-clip", "adamw-clip", "rmsprop-clip", "adagrad"])
def test_clip_decay_and_moments_move_on_apply_micro_steps_only(make):
    """A non-apply micro-step leaves the weights and every slot but the accumulator bit-unchanged; the apply
    micro-step is bit-equal to an unaccumulated optimizer handed the folded gradient at the same step count."""
    k, n = 3, 300
    opt, ref = make(gradient_accumulation_steps=k), make()
    gs = _grads(n, 2 * k, seed=3)
    w0 = np.random.default_rng(4).standard_normal(n).astype(np.float32)
    W, Wr = torch.from_numpy(w0.copy()), torch.from_numpy(w0.copy())
    ref.build(n, torch.device("cpu"))
    for j, g in enumerate(gs):
        w_before = W.clone()
        slots_before = {s: v.clone() for s, v in opt.slots().items() if s != SLOT} if j else None
        opt.apply_flat(W, torch.from_numpy(g.copy()))
        if j % k != k - 1:
            assert torch.equal(W, w_before)
            if slots_before is not None:
                for s, v in slots_before.items():
                    assert torch.equal(opt.slots()[s], v), s
        else:
            ref.iterations = j  # (Adam's bias correction reads the micro-step count)
            ref.apply_flat(Wr, torch.from_numpy(AR.fold(gs[j - k + 1:j + 1], k)))
            assert torch.equal(W, Wr), j
            for s, v in ref.slots().items():
                assert torch.equal(opt.slots()[s], v), s
            assert not torch.equal(W, w_before)
    assert opt.iterations == 2 * k


@pytest.mark.parametrize("bad", [0, -1, 2.5, "4"])
def test_invalid_steps_raise_value_error(bad):
    for cls in (O.SGD, O.Adam, O.AdamW, O.RMSprop, O.Adagrad, O.LARS, O.LAMB, O.legacy.SGD, O.legacy.Adam):
        with pytest.raises(ValueError, match="gradient_accumulation_steps"):
            cls(gradient_accumulation_steps=bad)


def test_config_round_trip():
    for cls in (O.SGD, O.Adam, O.AdamW, O.RMSprop, O.Adagrad, O.LARS, O.LAMB):
        a = cls(gradient_accumulation_steps=4)
        cfg = a.get_config()
        assert cfg["gradient_accumulation_steps"] == 4
        b = cls.from_config(cfg)
        assert type(b) is cls and b.gradient_accumulation_steps == 4 and b._accumulating and b.get_config() == cfg
        c = O.get(O.serialize(a))
        assert type(c) is cls and c.gradient_accumulation_steps == 4
        assert cls().get_config()["gradient_accumulation_steps"] is None
        assert not cls.from_config(cls().get_config())._accumulating


@pytest.mark.parametrize("off", [None, 1])
def test_off_allocates_no_slot_and_changes_nothing(off):
    n = 200
    gs = _grads(n, 5, seed=5)
    w0 = np.random.default_rng(6).standard_normal(n).astype(np.float32)
    for make in (lambda **kw: O.SGD(0.1, momentum=0.9, **kw), lambda **kw: O.Adam(1e-2, clipnorm=1.0, **kw)):
        a, b = make(gradient_accumulation_steps=off), make()
        assert not a._accumulating
        Wa, Wb = torch.from_numpy(w0.copy()), torch.from_numpy(w0.copy())
        for g in gs:
            assert a.accumulate(torch.from_numpy(g.copy())) is True
            a.apply_flat(Wa, torch.from_numpy(g.copy()))
            b.apply_flat(Wb, torch.from_numpy(g.copy()))
        assert SLOT not in a.slots() and set(a.slots()) == set(b.slots())
        assert torch.equal(Wa, Wb) and a.iterations == b.iterations == 5


def test_accumulating_optimizer_is_never_plain_sgd():
    plain = fused.FusedMnistTrainer._plain_sgd.fget
    assert plain(types.SimpleNamespace(optimizer=O.SGD(0.05)))
    assert plain(types.SimpleNamespace(optimizer=O.SGD(0.05, gradient_accumulation_steps=1)))
    assert not plain(types.SimpleNamespace(optimizer=O.SGD(0.05, gradient_accumulation_steps=2)))


def test_fused_eligibility_names_a_missing_grad_accum_kernel(monkeypatch):
    """eligible() with everything in front of the optimizer check stubbed (as
    test_clip_cpu.test_fused_eligibility_does_not_name_clipping): an accumulating optimizer passes it, and a
    stale extension without the kernel is named as such."""
    from tensorflow_distributed_learning_amd import ops
    from tensorflow_distributed_learning_amd.keras import losses

    kernels = types.SimpleNamespace(adam=1, rmsprop=1, adagrad=1, sgd=1, clip_norm=1, grad_accum=1)
    monkeypatch.setattr(ops, "hip_available", lambda: True)
    monkeypatch.setattr(ops, "hip", lambda: kernels)
    monkeypatch.setattr(fused, "_is_reference_cnn", lambda m: True)
    monkeypatch.delenv("TDL_DISABLE_FUSED", raising=False)

    def model(opt):
        strategy = types.SimpleNamespace(extended=types.SimpleNamespace(device=torch.device("cuda", 0)))
        return types.SimpleNamespace(_get_strategy=lambda: strategy, _dtype_policy=lambda: "float32",
                                     loss=losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt,
                                     compiled_metrics=[])

    for opt in (O.Adam(1e-3, gradient_accumulation_steps=2), O.SGD(0.05, gradient_accumulation_steps=4),
                O.SGD(0.05, momentum=0.9, clipnorm=1.0, gradient_accumulation_steps=3)):
        assert fused.eligible(model(opt)) is None
    del kernels.grad_accum
    reason = fused.eligible(model(O.Adam(1e-3, gradient_accumulation_steps=2)))
    assert "grad_accum" in reason and "rebuild" in reason
    assert fused.eligible(model(O.Adam(1e-3))) is None
    assert fused.eligible(model(O.Adam(1e-3, gradient_accumulation_steps=1))) is None


# ---------------------------------------------------------------------------------------------- fit (generic engine)
def _cnn():
    L = tdl.keras.layers
    return tdl.keras.Sequential([
        L.Conv2D(8, 3, activation="relu", input_shape=(28, 28, 1)), L.MaxPooling2D(),
        L.Flatten(), L.Dense(16, activation="relu"), L.Dense(10)])


def _data(n=256, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 28, 28, 1, generator=g), torch.randint(0, 10, (n,), generator=g)


def _fit(x, y, B, steps, make_opt, strategy=None, model=None, spe=1):
    """``steps`` train steps over consecutive batches of B (NO shuffle: k batches of b are one batch of k b)."""
    tdl.keras.utils.set_random_seed(7)
    ds = tdl.data.Dataset.from_tensor_slices((x, y)).batch(B).repeat()
    strategy = strategy or tdl.distribute.MirroredStrategy(devices=["/cpu:0"])
    if model is None:
        with strategy.scope():
            model = _cnn()
            model.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=make_opt(),
                          metrics=[tdl.keras.metrics.SparseCategoricalAccuracy()], steps_per_execution=spe)
    h = model.fit(ds, epochs=1, steps_per_epoch=steps, verbose=0)
    return model, h


@pytest.mark.parametrize("make", [lambda **kw: O.SGD(0.05, **kw), lambda **kw: O.SGD(0.05, momentum=0.9, **kw)],
                         ids=["sgd", "sgd-momentum"])
def test_cpu_fit_four_micro_batches_of_16_match_one_batch_of_64(make):
    """k = 4 x b = 16 over 8 micro-steps against k off, b = 64 over 2 steps, the same samples: the mean gradient
    of 64 samples summed in another f32 order.  Tolerance: the one tests/test_fit_gpu.py
    (test_fused_engine_selected_and_matches_generic, ``rtol=2e-3, atol=2e-4``) uses for two f32 summation
    orders of the same SGD run.  An unaccumulated run at b = 16 must differ from both (the test bites)."""
    tdl.keras.backend.clear_session()
    x, y = _data(128)
    ma, ha = _fit(x, y, 16, 8, lambda: make(gradient_accumulation_steps=4))
    mb, _ = _fit(x, y, 64, 2, make)
    mc, _ = _fit(x, y, 16, 8, make)
    assert ma._trainer.kind == "generic" and ma.optimizer.iterations == 8 and mb.optimizer.iterations == 2
    assert len(ha.history["loss"]) == 1 and np.isfinite(ha.history["loss"]).all()
    for a, b in zip(ma.get_weights(), mb.get_weights()):
        np.testing.assert_allclose(a, b, rtol=2e-3, atol=2e-4)
    for other in (ma, mb):
        assert max(np.abs(a - c).max() for a, c in zip(other.get_weights(), mc.get_weights())) > 1e-4


def test_cpu_checkpoint_in_the_middle_of_a_cycle_resumes_bit_exactly():
    """k = 4: 3 micro-steps, state_dict() + weights into a fresh model and optimizer, 5 more, against 8
    uninterrupted micro-steps."""
    tdl.keras.backend.clear_session()
    x, y = _data(128)
    make = lambda: O.Adam(1e-2, gradient_accumulation_steps=4)  # noqa: E731
    full, _ = _fit(x, y, 16, 8, make)
    first, _ = _fit(x, y, 16, 3, make)
    st = first.optimizer.state_dict()
    assert st["iterations"] == 3 and SLOT in st["slots"]
    with tdl.distribute.MirroredStrategy(devices=["/cpu:0"]).scope():
        again = _cnn()
        again.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=make(),
                      metrics=[tdl.keras.metrics.SparseCategoricalAccuracy()])
    again.set_weights(first.get_weights())
    again.optimizer.load_state_dict(st)
    assert again.optimizer.iterations == 3 and SLOT in again.optimizer.slots()
    _fit(x[48:], y[48:], 16, 5, None, model=again)
    assert again.optimizer.iterations == full.optimizer.iterations == 8
    assert torch.equal(again.optimizer.slots()[SLOT], full.optimizer.slots()[SLOT])
    for a, b in zip(again.get_weights(), full.get_weights()):
        assert np.array_equal(a, b)
    # the accumulator mattered: resuming without it does not reproduce the run
    with tdl.distribute.MirroredStrategy(devices=["/cpu:0"]).scope():
        lost = _cnn()
        lost.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=make(),
                     metrics=[tdl.keras.metrics.SparseCategoricalAccuracy()])
    lost.set_weights(first.get_weights())
    st2 = dict(st, slots={s: v for s, v in st["slots"].items() if s != SLOT})
    lost.optimizer.load_state_dict(st2)
    _fit(x[48:], y[48:], 16, 5, None, model=lost)
    assert any(not np.array_equal(a, b) for a, b in zip(lost.get_weights(), full.get_weights()))


def test_lars_and_lamb_accept_the_keyword_and_accumulate():
    from tensorflow_distributed_learning_amd.engine.slab import SlabLayout

    lay = SlabLayout.from_shapes((("a/kernel", (8, 5)), ("a/bias", (5,)), ("b/kernel", (5, 3))))
    n = lay.total
    gs = _grads(n, 4, seed=8)
    w0 = np.random.default_rng(9).standard_normal(n).astype(np.float32)
    for cls in (O.LARS, O.LAMB):
        opt, ref = cls(0.1, gradient_accumulation_steps=2), cls(0.1)
        opt.set_layout(lay)
        ref.set_layout(lay)
        W, Wr = torch.from_numpy(w0.copy()), torch.from_numpy(w0.copy())
        for j, g in enumerate(gs):
            before = W.clone()
            opt.apply_flat(W, torch.from_numpy(g.copy()))
            if j % 2 == 0:
                assert torch.equal(W, before)
            else:
                ref.iterations = j
                ref.apply_flat(Wr, torch.from_numpy(AR.fold(gs[j - 1:j + 1], 2)))
                assert torch.equal(W, Wr), (cls.__name__, j)
        assert opt.iterations == 4 and SLOT in opt.slots()


def test_mirrored_two_cpu_devices_in_one_process_accumulate_and_stay_identical():
    tdl.keras.backend.clear_session()
    x, y = _data(256)
    make = lambda: O.SGD(0.05, momentum=0.9, gradient_accumulation_steps=2)  # noqa: E731
    s = tdl.distribute.MirroredStrategy(devices=["/cpu:0", "/cpu:1"])
    m, h = _fit(x, y, 32, 6, make, strategy=s)
    assert type(m._trainer).__name__ == "ThreadedGroupTrainer" and m._trainer.kind == "generic"
    (clone,) = m._local_clones
    assert m.optimizer.iterations == clone.optimizer.iterations == 6
    assert clone.optimizer.gradient_accumulation_steps == 2 and SLOT in clone.optimizer.slots()
    for a, b in zip(m.get_weights(), clone.get_weights()):
        assert np.array_equal(a, b), "replicas differ"
    assert np.isfinite(h.history["loss"]).all()
    # one replica on the same global batches: the same model up to f32 summation order (the tolerances of
    # test_local_replicas_cpu.test_mirrored_two_cpu_devices_one_process_trains_identical_replicas)
    m1, _ = _fit(x, y, 32, 6, make)
    for a, b in zip(m.get_weights(), m1.get_weights()):
        np.testing.assert_allclose(a, b, rtol=2e-4, atol=2e-5)
    # and accumulation is what ran: the unaccumulated run differs
    m2, _ = _fit(x, y, 32, 6, lambda: O.SGD(0.05, momentum=0.9))
    assert max(np.abs(a - b).max() for a, b in zip(m1.get_weights(), m2.get_weights())) > 1e-4
    s.shutdown()
