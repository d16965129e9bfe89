"""The in-tree gfx950 extension and the native runtime load (no GPU needed): a kernel template whose
host-side launch stub failed to instantiate links fine but leaves an undefined symbol that only
shows at import time (round 4: the LDS-DMA builtin in a templated lambda)."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hip_extension_imports_with_every_entry_point():
    import glob

    if not glob.glob(os.path.join(ROOT, "tensorflow_distributed_learning_amd", "_C*.so")):
        pytest.skip("extension not built (python build_native.py)")
    from tensorflow_distributed_learning_amd.ops import hip

    C = hip()
    for name in ("conv_fwd", "conv_fwd_stats", "conv_dgrad", "conv_dgrad_bn", "conv_dgrad_s2", "conv_wgrad",
                 "conv_wgrad_plans", "conv_force_impl", "conv_selected", "conv_kernel_names", "bn_forward_train", "bn_backward", "gemm_bf16", "MnistStep",
                 "XgmiChannel", "stem_fwd", "maxpool_fwd", "gemm_f32", "conv_f32_fwd", "conv_f32_fwd_pool",
                 "conv_f32_dgrad", "conv_f32_wgrad", "f32_last_selected", "f32_kernel_names", "f32_plan", "f32_reduce16",
                 "f32_buf", "f32_reduce_narrow", "f32_pool_hoist"):
        assert hasattr(C, name), name


def test_native_runtime_imports():
    from tensorflow_distributed_learning_amd import ops

    if not ops.native_available():
        pytest.skip("native runtime not built")
    N = ops.native()
    assert hasattr(N, "RingComm") and hasattr(N.RingComm, "abort")
