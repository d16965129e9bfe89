"""engine/execution.py on the GPU: the pinned staging ring under reuse and growth with copies in flight, and
the update kernels' ``zero_grad`` as ``apply_flat`` reports it."""
import numpy as np
import pytest
import torch

import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.engine import execution as EX

pytestmark = pytest.mark.gpu
O = tdl.keras.optimizers


def test_ring_uploads_survive_reuse_and_growth_without_a_host_sync(cuda):
    """2 slots, 7 uploads: below the minimum size, at it, one past it (growth while the slot's earlier copy
    may be in flight), far past it, tiny again, and both grown buffers reused."""
    rng = np.random.default_rng(0)
    ring = EX.IndexRing(cuda, 2)
    srcs = [rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)
            for n in (8, 1024, 1025, 5000, 3, 5000, 1025)]
    dsts = [torch.zeros(len(s) + 5, dtype=torch.int32, device=cuda) for s in srcs]
    slots = []
    for s, d in zip(srcs, dsts):
        slots.append(ring.next_slot())
        ring.upload(s, d, slots[-1])
    torch.cuda.synchronize(cuda)
    assert slots == [0, 1, 0, 1, 0, 1, 0]
    for s, d in zip(srcs, dsts):
        got = d.cpu().numpy()
        assert np.array_equal(got[:len(s)], s) and not got[len(s):].any(), len(s)
    assert [b.numel() for b in ring.bufs] == [1025, 5000] and all(b.is_pinned() for b in ring.bufs)


def test_ring_reserve_makes_later_uploads_allocation_free(cuda):
    ring = EX.IndexRing(cuda, 2)
    ring.reserve(6000)
    ptrs = [b.data_ptr() for b in ring.bufs]
    assert [b.numel() for b in ring.bufs] == [6000, 6000]
    src = np.arange(5000, dtype=np.int32)
    dst = torch.zeros(5000, dtype=torch.int32, device=cuda)
    for _ in range(2):
        ring.upload(src, dst, ring.next_slot())
    torch.cuda.synchronize(cuda)
    assert [b.data_ptr() for b in ring.bufs] == ptrs
    assert np.array_equal(dst.cpu().numpy(), src)


@pytest.mark.parametrize("make, zeroes", [(lambda: O.SGD(0.1), True), (lambda: O.SGD(0.1, momentum=0.9), True),
                                          (lambda: O.Adam(1e-3), False)], ids=["sgd", "sgd-momentum", "adam"])
def test_apply_flat_reports_whether_its_kernel_zeroed_the_gradient(cuda, make, zeroes):
    """A slab of 1030 floats (no multiple of 4, more than one workgroup), two steps so that the momentum slot
    is read: zero_grad changes G only, never W."""
    n = 1030
    g = torch.Generator().manual_seed(0)
    w0, grads = torch.randn(n, generator=g), [torch.randn(n, generator=g) for _ in range(2)]
    out = {}
    for zero in (False, True):
        opt, W = make(), w0.to(cuda)
        for gr in grads:
            G = gr.to(cuda)
            assert opt.apply_flat(W, G, zero_grad=zero) is (zero and zeroes)
            assert torch.equal(G.cpu(), torch.zeros(n) if zero and zeroes else gr)
        out[zero] = W.cpu()
    assert torch.equal(out[True], out[False]) and not torch.equal(out[True], w0)
