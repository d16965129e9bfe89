"""keras.layers.GroupNormalization on the CPU: construction, weights, config, checkpoints, the compat
namespace, and the PyTorch-op path (values and autograd gradients) against the f64 references of
tests/groupnorm_refs.py on the small shapes of the kernel tests."""
import numpy as np
import pytest
import torch

import groupnorm_refs as GR
import tensorflow_distributed_learning_amd as tdl
from kernel_refs import ulp32

keras = tdl.keras
L = keras.layers
EPS = 1e-3

# [N, P, C], G of tests/test_groupnorm_kernels_gpu.py
SHAPES = [((1, 1, 8), 1), ((1, 1, 8), 8), ((3, 1, 24), 3), ((2, 49, 16), 1), ((2, 49, 16), 4), ((2, 49, 16), 16),
          ((2, 49, 16), -1), ((2, 37 * 41, 8), 2), ((5, 9, 6), 3), ((2, 25, 3), 1), ((2, 16, 2048), 32)]


def test_constructor_validation():
    for bad in (0, -2, 2.5, "4", True):
        with pytest.raises(ValueError):
            L.GroupNormalization(groups=bad)
    with pytest.raises(TypeError):
        L.GroupNormalization(groups=2, momentum=0.9)  # no moving statistics, no such argument
    with pytest.raises(TypeError):
        L.GroupNormalization(groups=2, gamma_constraint=lambda w: w)  # constraints are not implemented: refused
    layer = L.GroupNormalization(groups=3)
    with pytest.raises(ValueError, match="does not divide"):
        layer(torch.zeros(2, 4, 4, 8))
    with pytest.raises(ValueError, match="does not divide"):
        L.GroupNormalization(groups=32)(L.Input(shape=(4, 4, 48)))


def test_default_arguments_and_weight_names():
    layer = L.GroupNormalization(name="gn")
    assert (layer.groups, layer.axis, layer.epsilon, layer.center, layer.scale) == (32, -1, 1e-3, True, True)
    y = layer(torch.randn(2, 3, 3, 64))
    assert y.shape == (2, 3, 3, 64)
    assert [w.name for w in layer.weights] == ["gn/gamma:0", "gn/beta:0"]
    assert [tuple(w.shape) for w in layer.weights] == [(64,), (64,)]
    assert len(layer.trainable_weights) == 2 and not layer.non_trainable_weights  # no moving statistics
    assert np.array_equal(layer.gamma.numpy(), np.ones(64)) and np.array_equal(layer.beta.numpy(), np.zeros(64))


def test_center_and_scale_off():
    x = torch.randn(2, 5, 8)
    for center, scale, names in ((False, True, ["g/gamma:0"]), (True, False, ["g/beta:0"]), (False, False, [])):
        layer = L.GroupNormalization(groups=2, center=center, scale=scale, name="g")
        y = layer(x)
        assert [w.name for w in layer.weights] == names
        ref = GR.gn_fwd_ref(x.numpy()[:, :, :], 2, None, None, EPS)["y"]
        np.testing.assert_allclose(y.numpy(), ref, rtol=0, atol=1e-5)


def test_groups_minus_one_is_instance_norm():
    x = torch.randn(3, 4, 4, 6)
    a = L.GroupNormalization(groups=-1)(x)
    b = L.GroupNormalization(groups=6)(x)
    assert torch.equal(a, b)
    mu = a.reshape(3, 16, 6).mean(dim=1)
    assert mu.abs().max() < 1e-5  # every (sample, channel) plane is centred on its own


def test_training_flag_changes_nothing():
    x = torch.randn(2, 3, 3, 8)
    layer = L.GroupNormalization(groups=4)
    assert torch.equal(layer(x, training=True), layer(x, training=False))


def test_axis_1():
    x = torch.randn(2, 6, 5, 5)  # channels first
    layer = L.GroupNormalization(groups=3, axis=1)
    layer(x)
    g = torch.rand(6) + 0.5
    b = torch.randn(6)
    layer.set_weights([g.numpy(), b.numpy()])
    y = layer(x)
    assert y.shape == x.shape
    ref = GR.gn_fwd_ref(x.permute(0, 2, 3, 1).reshape(2, 25, 6).numpy(), 3, g.numpy(), b.numpy(), EPS)["y"]
    np.testing.assert_allclose(y.permute(0, 2, 3, 1).reshape(2, 25, 6).numpy(), ref, rtol=0, atol=2e-5)
    with pytest.raises(ValueError):
        L.GroupNormalization(groups=1, axis=0)(torch.zeros(2, 4))


def test_get_config_from_config_and_model_config():
    layer = L.GroupNormalization(groups=4, epsilon=1e-5, center=False, name="gn_a")
    cfg = layer.get_config()
    assert cfg["groups"] == 4 and cfg["epsilon"] == 1e-5 and cfg["center"] is False and cfg["scale"] is True
    assert cfg["axis"] == -1 and cfg["name"] == "gn_a"
    again = L.GroupNormalization.from_config(cfg)
    assert again.get_config() == cfg
    assert L.LAYER_CLASSES["GroupNormalization"] is L.GroupNormalization
    assert "gamma_regularizer" not in cfg and "beta_regularizer" not in cfg
    reg = L.GroupNormalization(groups=2, gamma_regularizer=keras.regularizers.L2(0.5),
                               beta_regularizer=keras.regularizers.L1L2(l1=0.25, l2=0.125))
    rcfg = reg.get_config()
    assert rcfg["gamma_regularizer"] == {"class_name": "L1L2", "config": {"l1": 0.0, "l2": 0.5}}
    back = L.GroupNormalization.from_config(rcfg)
    assert (back.gamma_regularizer.l2, back.beta_regularizer.l1, back.beta_regularizer.l2) == (0.5, 0.25, 0.125)
    assert back.get_config() == rcfg
    back(torch.zeros(2, 4))
    assert back.gamma._regularizer is back.gamma_regularizer and back.beta._regularizer is back.beta_regularizer
    m = keras.Sequential([L.Conv2D(8, 3, input_shape=(8, 8, 1)), L.GroupNormalization(groups=-1), L.ReLU(),
                          L.Flatten(), L.Dense(3)])
    m2 = keras.models.model_from_config(m.get_config_full())
    gn = [l for l in m2.layers if isinstance(l, L.GroupNormalization)]
    assert len(gn) == 1 and gn[0].groups == -1
    assert m2(torch.randn(2, 8, 8, 1)).shape == (2, 3)


def test_checkpoint_round_trip(tmp_path):
    def make():
        return keras.Sequential([L.Conv2D(8, 3, input_shape=(8, 8, 1), name="c"),
                                 L.GroupNormalization(groups=4, name="gn"), L.Flatten(name="f"),
                                 L.Dense(3, name="d")])

    m = make()
    gn = m.layers[1]
    rng = np.random.default_rng(0)
    gn.set_weights([rng.random(8).astype(np.float32) + 0.5, rng.standard_normal(8).astype(np.float32)])
    x = torch.randn(2, 8, 8, 1)
    y = m(x)
    m.save_weights(str(tmp_path / "ck"))
    m2 = make()
    m2(x)
    m2.load_weights(str(tmp_path / "ck"))
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(a, b)
    assert torch.equal(m2(x), y)


def test_compat_namespace():
    from tensorflow_distributed_learning_amd.compat import tf

    assert tf.keras.layers.GroupNormalization is L.GroupNormalization
    layer = tf.keras.layers.GroupNormalization(groups=2)
    assert layer(torch.randn(2, 4)).shape == (2, 4)


@pytest.mark.parametrize("shape,G", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}-G{g}" for s, g in SHAPES])
@pytest.mark.parametrize("affine", [True, False])
def test_cpu_path_against_f64(shape, G, affine):
    """The PyTorch-op path and its autograd gradients against the f64 reference.  The bound is that of f32
    arithmetic: the same formulas evaluated by torch in f64 agree with the reference to 1e-9 relative (the
    formulas are right), and the f32 run must stay within 64 f32 ulp of the largest magnitude of each
    output (sums of up to 2^15 f32 terms carry at most ~ sqrt(m) / 2 ulp when pairwise, far below 64)."""
    from tensorflow_distributed_learning_amd.ops import groupnorm as gn

    N, P, C = shape
    G = GR.groups_of(C, G)
    rng = np.random.default_rng(P * 131 + C)
    x = (rng.standard_normal(shape) * 2.0 + 0.5).astype(np.float32)
    dy = rng.standard_normal(shape).astype(np.float32)
    g = (rng.random(C) + 0.5).astype(np.float32) if affine else None
    b = rng.standard_normal(C).astype(np.float32) if affine else None
    f = GR.gn_fwd_ref(x, G, g, b, EPS)
    bw = GR.gn_bwd_ref(dy, x, G, g, EPS)
    for dt, rel in ((torch.float64, 1e-9), (torch.float32, 64 * 2.0 ** -23)):
        tx = torch.from_numpy(x).to(dt).requires_grad_(True)
        tg = torch.from_numpy(g).to(dt).requires_grad_(True) if affine else None
        tb = torch.from_numpy(b).to(dt).requires_grad_(True) if affine else None
        y = gn.group_norm(tx, G, tg, tb, EPS)
        assert y.dtype == dt and y.shape == tx.shape
        y.backward(torch.from_numpy(dy).to(dt))
        pairs = [("y", y.detach(), f["y"]), ("dx", tx.grad, bw["dx"])]
        if affine:
            pairs += [("dgamma", tg.grad, bw["dgamma"]), ("dbeta", tb.grad, bw["dbeta"])]
        for name, got, ref in pairs:
            err = np.abs(got.double().numpy() - ref).max()
            tol = rel * max(np.abs(ref).max(), 1.0)
            assert err <= tol, f"{name} ({dt}): error {err:.3g} > {tol:.3g}"


def test_emulation_tracks_the_reference():
    """The kernel-formula emulation (f64 sums, f32 coefficients) is within a few f32 ulp of the reference,
    and on data with mean 100 / std 0.1 its f32-sum variant is not -- the distinction the GPU tests rely on."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 49, 16)) * 0.1 + 100.0).astype(np.float32)
    g = (rng.random(16) + 0.5).astype(np.float32)
    b = rng.standard_normal(16).astype(np.float32)
    f = GR.gn_fwd_ref(x, 4, g, b, EPS)
    e64 = GR.gn_fwd_emul(x, 4, g, b, EPS)
    e32 = GR.gn_fwd_emul(x, 4, g, b, EPS, sums="f32")
    E = np.abs(e64["y"] - f["y"]).max()
    assert E <= 100.0 * 32.0 * 2.0 ** -23  # |x| ulp(scale): x ~ 100, scale ~ gamma / std < 32
    assert np.abs(e32["y"] - f["y"]).max() > 4 * E + ulp32(f["y"]).max()
    assert np.abs(e64["r"] / f["r"] - 1).max() < 1e-9


def test_resnet50_group_norm_builds_and_runs():
    m = keras.applications.ResNet50(input_shape=(32, 32, 3), classes=10, norm="group")
    gns = [l for l in m.layers if isinstance(l, L.GroupNormalization)]
    assert len(gns) == 53 and all(l.groups == 32 for l in gns)
    assert not any(isinstance(l, L.BatchNormalization) for l in m.layers)
    assert gns[0].name == "conv1_bn"
    with torch.no_grad():
        y = m(torch.randn(1, 32, 32, 3))
    assert y.shape == (1, 10) and torch.isfinite(y).all()
    base = keras.applications.ResNet50(input_shape=(32, 32, 3), classes=10)
    assert sum(isinstance(l, L.BatchNormalization) for l in base.layers) == 53
    m16 = keras.applications.ResNet50(input_shape=(32, 32, 3), classes=10, norm="group", norm_groups=16)
    assert all(l.groups == 16 for l in m16.layers if isinstance(l, L.GroupNormalization))
    with pytest.raises(ValueError):
        keras.applications.ResNet50(input_shape=(32, 32, 3), norm="layer")
