"""RandomFlip, RandomCrop and RandomTranslation on the CPU (keras/layers.py, ops/augment.py) against a naive
per-pixel loop written here: it takes its draws word by word from ``philox_words`` and shares no code with
``augment_reference``.  The forward must agree bit for bit (it only moves values), and so must the backward:
the oracle scatters ``dy`` in ascending ``(oh, ow)`` order with f32 adds starting from +0, the order the
kernels' gather form is specified to reproduce."""
import numpy as np
import pytest
import torch

import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.ops import augment as A
from tensorflow_distributed_learning_amd.ops import dropout as D

L = tdl.keras.layers
SHAPES = [(2, 5, 7, 3), (3, 4, 4, 1)]
TICKETS = 4  # calls per case: both flip values and several offsets occur (asserted below)


# ------------------------------------------------------------------------------------------------ the oracle
def _draw(key, ticket, n, spec):
    w = [int(D.philox_words(key, ticket, np.array([4 * n + j], dtype=np.uint64))[0]) for j in range(4)]
    flip_w = (w[0] >> 31) if spec.flip_w else 0
    flip_h = (w[1] >> 31) if spec.flip_h else 0
    off_h = spec.off_h_lo + ((w[2] * spec.off_h_count) >> 32)
    off_w = spec.off_w_lo + ((w[3] * spec.off_w_count) >> 32)
    return flip_h, flip_w, off_h, off_w


def _src(o, flip, off, Lo, L, mode):
    r = (Lo - 1 - o if flip else o) + off
    if 0 <= r < L:
        return r
    if mode == "constant":
        return None
    if mode == "nearest":
        return min(max(r, 0), L - 1)
    if mode == "wrap":
        return r % L
    assert mode == "reflect"
    return -1 - r if r < 0 else 2 * L - 1 - r


def _oracle(x, dy, key, ticket, spec):
    """(y, dx, draws) of one call on f32 numpy arrays, pixel by pixel."""
    N, H, W, C = x.shape
    Ho, Wo = spec.out_h, spec.out_w
    y = np.empty((N, Ho, Wo, C), dtype=np.float32)
    dx = np.zeros((N, H, W, C), dtype=np.float32)
    drawn = []
    for n in range(N):
        fh, fw, oh_, ow_ = d = _draw(key, ticket, n, spec)
        drawn.append(d)
        for oh in range(Ho):
            for ow in range(Wo):
                rh, rw = _src(oh, fh, oh_, Ho, H, spec.fill_mode), _src(ow, fw, ow_, Wo, W, spec.fill_mode)
                if rh is None or rw is None:
                    y[n, oh, ow] = np.float32(spec.fill_value)
                else:
                    y[n, oh, ow] = x[n, rh, rw]
                    for c in range(C):
                        dx[n, rh, rw, c] = np.float32(dx[n, rh, rw, c]) + np.float32(dy[n, oh, ow, c])
    return y, dx, drawn


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _values(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    x.view(-1)[::5] = -0.0  # a sum that starts from +0 turns a lone -0 into +0
    return x


def _check_layer(layer, shape, seed_key):
    """TICKETS training calls of ``layer`` on the CPU, outputs and input gradients against the oracle."""
    N, H, W, C = shape
    spec = layer._spec(H, W)
    seen = []
    for t in range(TICKETS):
        x = _values(shape, 10 + t).requires_grad_(True)
        dy = _values((N, spec.out_h, spec.out_w, C), 20 + t)
        y = layer(x, training=True)
        y.backward(dy)
        want_y, want_dx, drawn = _oracle(x.detach().numpy(), dy.numpy(), seed_key, t, spec)
        assert tuple(y.shape) == want_y.shape
        assert np.array_equal(_bits(y.detach().numpy()), _bits(want_y)), f"{layer.name} call {t}: forward"
        assert np.array_equal(_bits(x.grad.numpy()), _bits(want_dx)), f"{layer.name} call {t}: backward"
        seen += drawn
    assert layer.rng_calls() == TICKETS
    return spec, seen


# ------------------------------------------------------------------------------------------------ 1, 2: the layers
@pytest.mark.parametrize("shape", SHAPES, ids=["2x5x7x3", "3x4x4x1"])
@pytest.mark.parametrize("mode", L.RandomFlip.MODES)
def test_random_flip(shape, mode):
    spec, seen = _check_layer(L.RandomFlip(mode, seed=7), shape, D.stream_key(7, 0, 0))
    fh, fw = {d[0] for d in seen}, {d[1] for d in seen}
    assert fh == ({0, 1} if "vertical" in mode else {0}) and fw == ({0, 1} if "horizontal" in mode else {0})
    assert {d[2:] for d in seen} == {(0, 0)}


@pytest.mark.parametrize("shape", SHAPES, ids=["2x5x7x3", "3x4x4x1"])
@pytest.mark.parametrize("fill_mode", A.FILL_MODES)
@pytest.mark.parametrize("factors", [(0.5, 0.5), (1.0, 1.0), ((1.0, 1.0), (-1.0, -1.0)), ((-1.0, -1.0), (1.0, 1.0)),
                                     ((-1.0, 0.0), (0.3, 1.0))],
                         ids=["half", "full-range", "down-H-left-W", "up-H-right-W", "pairs"])
def test_random_translation(shape, fill_mode, factors):
    N, H, W, C = shape
    layer = L.RandomTranslation(*factors, fill_mode=fill_mode, fill_value=1.5, seed=9)
    spec, seen = _check_layer(layer, shape, D.stream_key(9, 0, 0))
    assert all(spec.off_h_lo <= d[2] < spec.off_h_lo + spec.off_h_count and
               spec.off_w_lo <= d[3] < spec.off_w_lo + spec.off_w_count and d[:2] == (0, 0) for d in seen)
    if factors in ((0.5, 0.5), (1.0, 1.0)):
        assert len({d[2:] for d in seen}) > 3, "the offsets barely vary"
    if isinstance(factors[0], tuple) and abs(factors[0][0]) == abs(factors[0][1]) == 1.0:
        # a shift by the whole image: nothing of it is left, constant fills everything
        assert {abs(d[2]) for d in seen} == {H} and {abs(d[3]) for d in seen} == {W}
        if fill_mode == "constant":
            y = layer(_values(shape, 1), training=True)
            assert (y == 1.5).all()


@pytest.mark.parametrize("shape", SHAPES, ids=["2x5x7x3", "3x4x4x1"])
@pytest.mark.parametrize("size", ["1x1", "full", "inner"])
def test_random_crop(shape, size):
    N, H, W, C = shape
    h, w = {"1x1": (1, 1), "full": (H, W), "inner": (H - 1, W - 2)}[size]
    layer = L.RandomCrop(h, w, seed=3)
    spec, seen = _check_layer(layer, shape, D.stream_key(3, 0, 0))
    assert all(0 <= d[2] <= H - h and 0 <= d[3] <= W - w and d[:2] == (0, 0) for d in seen)
    if size == "full":
        x = _values(shape, 1)
        assert torch.equal(layer(x, training=True), x)
    if size == "1x1":
        assert len({d[2:] for d in seen}) > 3, "the window barely moves"


@pytest.mark.parametrize("fill_mode", A.FILL_MODES)
@pytest.mark.parametrize("off", [(-5, -7), (5, 7), (-4, 6), (0, 0), (2, -3)])
@pytest.mark.parametrize("flips", [(False, False), (True, True)])
def test_reference_backward_at_forced_offsets(fill_mode, off, flips):
    """The op itself (``count = 1`` pins the offset, flips still drawn): extremes in both directions, where
    ``nearest`` piles a run of ``|off| + 1`` pixels on an edge and ``reflect`` reads a pixel up to twice."""
    shape = (2, 5, 7, 3)
    key = D.stream_key(1, 2, 0)
    spec = A.Spec(flip_h=flips[0], flip_w=flips[1], off_h_lo=off[0], off_w_lo=off[1], out_h=5, out_w=7,
                  fill_mode=fill_mode, fill_value=-0.0)
    for t in range(2):
        x = _values(shape, 3).requires_grad_(True)
        dy = _values(shape, 4)
        y = A.augment(x, spec, key, ticket=t)
        y.backward(dy)
        want_y, want_dx, _ = _oracle(x.detach().numpy(), dy.numpy(), key, t, spec)
        assert np.array_equal(_bits(y.detach().numpy()), _bits(want_y))
        assert np.array_equal(_bits(x.grad.numpy()), _bits(want_dx))
        assert np.array_equal(_bits(A.augment_backward_reference(dy.numpy(), key, t, spec, 5, 7)), _bits(want_dx))


def test_other_dtypes_on_the_cpu():
    key = D.stream_key(5, 0, 0)
    spec = A.Spec(flip_w=True, off_h_lo=-2, off_h_count=5, off_w_lo=-3, off_w_count=7, out_h=5, out_w=7,
                  fill_mode="nearest")
    x32, dy32 = _values((2, 5, 7, 3), 1), _values((2, 5, 7, 3), 2)
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        x = x32.to(dt).requires_grad_(True)
        y = A.augment(x, spec, key, ticket=1)
        assert y.dtype == dt
        y.backward(dy32.to(dt))
        want_y, want_dx, _ = _oracle(x.detach().float().numpy(), dy32.to(dt).float().numpy(), key, 1, spec)
        assert torch.equal(y.detach().float(), torch.from_numpy(want_y))  # a copy: exact in every dtype
        assert x.grad.dtype == dt and torch.equal(x.grad, torch.from_numpy(want_dx).to(dt))  # f32 sum, rounded once
    # the constant fill is rounded once to the tensor's dtype
    spec = A.Spec(off_h_lo=5, out_h=5, out_w=7, fill_value=1.00390625 + 2.0 ** -20)
    y = A.augment(x32.to(torch.bfloat16), spec, key, ticket=0)
    assert (y == torch.tensor(1.00390625 + 2.0 ** -20, dtype=torch.float64).to(torch.bfloat16)).all()
    with pytest.raises(TypeError):
        A.augment(torch.zeros(1, 2, 2, 1, dtype=torch.int32), spec, key, ticket=0)


# ------------------------------------------------------------------------------------------------ 3: the draws
def test_draws_of_seed_7():
    key = D.stream_key(7, 0, 0)
    w = D.philox_words(key, 0, np.arange(32, dtype=np.uint64)).reshape(8, 4)
    assert (w[:, 0] >> np.uint64(31)).tolist() == [1, 0, 1, 1, 0, 0, 1, 1]
    assert (w[:, 1] >> np.uint64(31)).tolist() == [0, 0, 0, 0, 0, 0, 1, 1]
    both = A.Spec(flip_h=True, flip_w=True, off_h_count=9, off_w_count=9, out_h=1, out_w=1)
    fh, fw, oh, ow = A.draws(key, 0, 8, both)
    assert fw.tolist() == [1, 0, 1, 1, 0, 0, 1, 1] and fh.tolist() == [0, 0, 0, 0, 0, 0, 1, 1]
    for n in range(8):
        assert _draw(key, 0, n, both) == (fh[n], fw[n], oh[n], ow[n])
    # a disabled flip ignores its word
    off = A.draws(key, 0, 8, both._replace(flip_h=False, flip_w=False))
    assert not off[0].any() and not off[1].any() and off[2].tolist() == oh.tolist()
    # a range of 9 reaches both of its ends on each axis within two calls
    hs = np.concatenate([A.draws(key, t, 8, both)[2] for t in (0, 1)])
    ws = np.concatenate([A.draws(key, t, 8, both)[3] for t in (0, 1)])
    assert hs.min() == 0 and hs.max() == 8 and ws.min() == 0 and ws.max() == 8
    # a count of 1 ignores its word; replicas draw differently
    one = A.draws(key, 0, 8, both._replace(off_h_lo=-3, off_h_count=1))
    assert one[2].tolist() == [-3] * 8
    other = A.draws(D.stream_key(7, 0, 1), 0, 8, both)
    assert any(a.tolist() != b.tolist() for a, b in zip((fh, fw, oh, ow), other))


# ------------------------------------------------------------------------------------------------ 4: the contract
def _layers():
    return [L.RandomFlip("horizontal", seed=4), L.RandomCrop(3, 2, seed=4),
            L.RandomTranslation((-0.5, 0.25), 0.5, fill_mode="wrap", interpolation="nearest", seed=4, fill_value=2.0)]


def test_inference_is_the_identity_or_the_centre_crop():
    x = _values((2, 6, 7, 3), 1)
    for layer in _layers():
        for training in (False, None):
            y = layer(x, training=training)
            if isinstance(layer, L.RandomCrop):
                assert torch.equal(y, x[:, 1:4, 2:4, :])  # top = (6 - 3) // 2, left = (7 - 2) // 2
            else:
                assert y is x
        assert layer.rng_calls() == 0
    assert L.RandomCrop(3, 2).compute_output_shape((None, 6, 7, 3)) == (None, 3, 2, 3)
    assert L.RandomFlip().compute_output_shape((None, 6, 7, 3)) == (None, 6, 7, 3)
    assert L.RandomTranslation(0.1, 0.1).compute_output_shape((None, 6, 7, 3)) == (None, 6, 7, 3)


def test_get_config_round_trips():
    x = _values((2, 6, 8, 3), 1)
    for layer in _layers():
        cfg = layer.get_config()
        twin = L.LAYER_CLASSES[type(layer).__name__].from_config(cfg)
        assert twin.get_config() == cfg
        assert torch.equal(twin(x, training=True), layer(x, training=True))
    cfg = L.RandomTranslation((-0.5, 0.25), 0.5).get_config()
    assert cfg["height_factor"] == [-0.5, 0.25] and cfg["width_factor"] == 0.5 and cfg["fill_mode"] == "reflect" and \
        cfg["interpolation"] == "bilinear" and cfg["seed"] is None and cfg["fill_value"] == 0.0


def test_namespaces():
    from tensorflow_distributed_learning_amd.compat import tf

    pre = L.experimental.preprocessing
    for name in ("RandomFlip", "RandomCrop", "RandomTranslation"):
        cls = getattr(L, name)
        assert L.LAYER_CLASSES[name] is cls and name in L.__all__
        assert getattr(pre, name) is cls and getattr(tf.keras.layers, name) is cls
        assert getattr(tf.keras.layers.experimental.preprocessing, name) is cls


def test_bad_arguments_raise():
    for bad in ("diagonal", "", None):
        with pytest.raises(ValueError):
            L.RandomFlip(bad)
    for h, w in ((0, 2), (2, -1), (2.5, 2)):
        with pytest.raises(ValueError):
            L.RandomCrop(h, w)
    with pytest.raises(ValueError):  # an input smaller than the crop (Keras would resize)
        L.RandomCrop(5, 2)(torch.zeros(1, 4, 4, 1), training=True)
    with pytest.raises(ValueError):
        L.RandomCrop(5, 2)(torch.zeros(1, 4, 4, 1), training=False)
    for hf in (-0.1, 1.5, (0.5, 0.25), (-2.0, 0.0), (0.1, 0.2, 0.3), float("nan")):
        with pytest.raises(ValueError):
            L.RandomTranslation(hf, 0.1)
        with pytest.raises(ValueError):
            L.RandomTranslation(0.1, hf)
    with pytest.raises(ValueError):
        L.RandomTranslation(0.1, 0.1, fill_mode="mirror")
    with pytest.raises(ValueError):
        L.RandomTranslation(0.1, 0.1, interpolation="bicubic")
    with pytest.raises(ValueError):  # [ceil(0.3 * 2), floor(0.4 * 2)] = [1, 0]: no whole-pixel shift
        L.RandomTranslation((0.3, 0.4), 0.0)(torch.zeros(1, 2, 2, 1), training=True)
    with pytest.raises(ValueError):
        L.RandomFlip()(torch.zeros(4, 4, 1), training=True)  # not NHWC
    key = D.stream_key(0, 0, 0)
    for spec in (A.Spec(out_h=5, out_w=4), A.Spec(out_h=4, out_w=4, off_h_lo=-5), A.Spec(out_h=4, out_w=4, off_w_count=6),
                 A.Spec(out_h=4, out_w=4, off_h_count=0), A.Spec(out_h=0, out_w=4),
                 A.Spec(out_h=4, out_w=4, fill_mode="mirror")):
        with pytest.raises(ValueError):
            A.augment(torch.zeros(1, 4, 4, 1), spec, key, ticket=0)
    with pytest.raises(ValueError):
        A.augment(torch.zeros(1, 4, 4, 1), A.Spec(out_h=4, out_w=4), key)  # a CPU input needs a ticket


def test_reset_rng_replays():
    x = _values((3, 6, 8, 2), 1)
    for layer in _layers():
        first = [layer(x, training=True) for _ in range(3)]
        assert layer.rng_calls() == 3
        assert not all(torch.equal(first[0], f) for f in first[1:]), "every call drew the same transform"
        layer.reset_rng()
        assert layer.rng_calls() == 0
        assert all(torch.equal(layer(x, training=True), f) for f in first)
        layer.reset_rng(2)
        assert torch.equal(layer(x, training=True), first[2])


def test_seed_and_stream_rules():
    x = _values((8, 6, 8, 1), 1)
    tdl.keras.backend.clear_session()
    tdl.keras.utils.set_random_seed(11)
    drop = L.Dropout(0.5)  # shares the creation-index counter
    a, b = L.RandomTranslation(0.5, 0.5), L.RandomTranslation(0.5, 0.5)
    assert (drop._rng_stream, a._rng_stream, b._rng_stream) == (0, 1, 2) and a.seed is None
    ya, yb = a(x, training=True), b(x, training=True)
    assert not torch.equal(ya, yb), "two seed=None layers draw alike"
    want = A.augment(x, a._spec(6, 8), D.stream_key(11, 1, 0), ticket=0)
    assert torch.equal(ya, want)
    c, d = L.RandomTranslation(0.5, 0.5, seed=5), L.RandomTranslation(0.5, 0.5, seed=5)
    assert c._rng_stream == d._rng_stream == 0
    assert torch.equal(c(x, training=True), d(x, training=True))
    assert not torch.equal(c(x, training=True), ya)
    # a replica's key differs: the same layer draws differently as replica 1
    from tensorflow_distributed_learning_amd.parallel import strategy as st

    c.reset_rng()
    y0 = c(x, training=True)
    c.reset_rng()
    with st._training_replica(1):
        y1 = c(x, training=True)
    assert torch.equal(y1, A.augment(x, c._spec(6, 8), D.stream_key(5, 0, 1), ticket=0)) and not torch.equal(y0, y1)


def test_dropout_masks_are_what_they_were():
    """Dropout now takes its RNG state from the shared mix-in: its mask for a fixed seed, its counter and its
    stream index are unchanged."""
    tdl.keras.backend.clear_session()
    layer = L.Dropout(0.5, seed=7)
    assert isinstance(layer, L._CallCounterRNG) and layer._rng_stream == 0
    x = torch.ones(4, 8)
    for t in range(2):
        y = layer(x, training=True)
        keep = D.philox_reference(D.stream_key(7, 0, 0), t, 32, D.threshold(0.5)).reshape(4, 8)
        assert np.array_equal((y != 0).numpy(), keep) and set(y.unique().tolist()) <= {0.0, 2.0}
    # the first mask of seed 7, written out: a change of key, stream or word order cannot pass
    first = D.philox_reference(D.stream_key(7, 0, 0), 0, 8, D.threshold(0.5)).astype(int).tolist()
    w = D.philox_words(D.stream_key(7, 0, 0), 0, np.arange(8, dtype=np.uint64))
    assert first == [int(v >= 2 ** 31) for v in w.tolist()]
    assert layer.rng_calls() == 2
    layer.reset_rng()
    assert layer.rng_calls() == 0
    sp = L.SpatialDropout2D(0.5)
    assert sp._rng_stream == 0 and L.Dropout(0.1)._rng_stream == 1
    assert layer.get_config()["seed"] == 7


def test_graph_def_export(tmp_path):
    """RandomFlip / RandomTranslation export as Identity (the saved graph reproduces predict); a model with
    RandomCrop keeps the header-only file, as other unmapped layers do."""
    import os
    import warnings

    from tensorflow_distributed_learning_amd.ckpt import graph_def as GD
    from tensorflow_distributed_learning_amd.ckpt import saved_model_pb as SMP

    def saved(first, name):
        tdl.keras.backend.clear_session()
        m = tdl.keras.Sequential(first + [L.Flatten(), L.Dense(3)])
        m.build((None, 4, 4, 1))
        p = str(tmp_path / name)
        m.save(p)
        with open(os.path.join(p, "saved_model.pb"), "rb") as f:
            mg = SMP.parse_saved_model(f.read())["meta_graphs"][0]
        return m, GD.parse_graph_def(mg["graph_def"])

    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a header-only file would warn
        m, nodes = saved([L.RandomTranslation(0.25, 0.25, input_shape=(4, 4, 1)), L.RandomFlip()], "ok")
    ident = [n for n in nodes.values() if n["op"] == "Identity"]
    assert len(ident) >= 2 and "MatMul" in {n["op"] for n in nodes.values()}
    assert all(not k.startswith("random_crop") for k in nodes)
    with pytest.warns(UserWarning, match="without a TF graph"):
        _, nodes = saved([L.RandomCrop(2, 2, input_shape=(4, 4, 1))], "crop")
    assert nodes == {}


# ------------------------------------------------------------------------------------------------ replicas
def test_two_cpu_replicas_draw_their_own_transforms_and_stay_identical():
    """Single-process MirroredStrategy (the threaded group path): the clone's layer keeps the original's stream,
    each replica counts its own calls and draws from the key of its replica id."""
    g = torch.Generator().manual_seed(0)
    x, y = torch.rand(64, 8, 8, 1, generator=g), torch.randint(0, 10, (64,), generator=g)
    tdl.keras.backend.clear_session()
    tdl.keras.utils.set_random_seed(7)
    s = tdl.distribute.MirroredStrategy(devices=["/cpu:0", "/cpu:1"])
    seen = {}

    class Probe(L.RandomTranslation):
        def call(self, x, training=None):
            out = super().call(x, training=training)
            if training and self._cpu_calls == 1:
                seen[L._replica_id()] = x.detach().clone(), out.detach().clone()
            return out

    L.LAYER_CLASSES["Probe"] = Probe
    try:
        ds = tdl.data.Dataset.from_tensor_slices((x, y)).batch(16).repeat()
        with s.scope():
            L.Dropout(0.5)  # takes stream 0: the probe's is 1, and the clone must inherit it
            m = tdl.keras.Sequential([Probe(0.5, 0.5, input_shape=(8, 8, 1)), L.RandomFlip(),
                                      L.Conv2D(4, 3, activation="relu"), L.Flatten(), L.Dense(10)])
            m.compile(loss=tdl.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                      optimizer=tdl.keras.optimizers.SGD(learning_rate=0.05))
        h = m.fit(ds, epochs=2, steps_per_epoch=3, verbose=0)
    finally:
        del L.LAYER_CLASSES["Probe"]
    assert sorted(seen) == [0, 1]
    probe = m.layers[0]
    assert probe._rng_stream == 1 and m.layers[1]._rng_stream == 2
    spec = probe._spec(8, 8)
    for r in (0, 1):
        xin, out = seen[r]
        assert xin.shape == (8, 8, 8, 1)  # half of the global batch
        assert torch.equal(out, A.augment(xin, spec, D.stream_key(7, 1, r), ticket=0)), f"replica {r}: not its own draw"
    d0, d1 = (A.draws(D.stream_key(7, 1, r), 0, 8, spec) for r in (0, 1))
    assert any(a.tolist() != b.tolist() for a, b in zip(d0, d1)), "the replicas draw one transform"
    clones = m._local_clones
    assert len(clones) == 1 and [l._rng_stream for l in clones[0].layers[:2]] == [1, 2]
    assert [l.rng_calls() for l in m.layers[:2]] == [6, 6] and [l.rng_calls() for l in clones[0].layers[:2]] == [6, 6]
    for a, b in zip(m.get_weights(), clones[0].get_weights()):
        assert np.array_equal(a, b), "replicas differ"
    assert len(h.history["loss"]) == 2 and np.isfinite(h.history["loss"]).all()
    s.shutdown()
