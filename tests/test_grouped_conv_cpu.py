"""Grouped convolution without a GPU: the ResNeXt variant of models/resnet50.ResNet50 and Conv2D(groups=) on the CPU."""
import numpy as np
import torch
import torch.nn.functional as F

import tensorflow_distributed_learning_amd as tdl


def _params(m):
    return sum(int(np.prod(w.shape)) for w in m.get_weights())


def test_resnet50_defaults_are_unchanged():
    tdl.keras.backend.clear_session()
    m = tdl.keras.applications.ResNet50(weights=None)
    assert _params(m) == 25_636_712
    k = m.get_layer("conv2_block1_2_conv")
    assert k.groups == 1 and tuple(k.kernel.value.shape) == (3, 3, 64, 64)
    assert tuple(m.get_layer("conv5_block3_1_conv").kernel.value.shape) == (1, 1, 2048, 512)


def test_resnext50_32x4d_builds_and_runs():
    tdl.keras.backend.clear_session()
    m = tdl.keras.applications.ResNet50(weights=None, groups=32, width_per_group=4, input_shape=(64, 64, 3), classes=10)
    k = m.get_layer("conv2_block1_2_conv")
    assert k.groups == 32 and tuple(k.kernel.value.shape) == (3, 3, 4, 128)
    assert tuple(m.get_layer("conv5_block3_2_conv").kernel.value.shape) == (3, 3, 32, 1024)
    y = m(torch.rand(2, 64, 64, 3, generator=torch.Generator().manual_seed(0)), training=False)
    assert tuple(y.shape) == (2, 10) and torch.isfinite(y).all()


def test_conv2d_groups_on_the_cpu_is_the_library_convolution():
    tdl.keras.backend.clear_session()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 7, 7, 6, generator=g)
    layer = tdl.keras.layers.Conv2D(4, 3, groups=2, padding="same")
    y = layer(x)
    ref = F.conv2d(x.permute(0, 3, 1, 2), layer.kernel.value.permute(3, 2, 0, 1), layer.bias.value, padding=1, groups=2)
    torch.testing.assert_close(y, ref.permute(0, 2, 3, 1))
