"""The hand-off chain in the middle of the fused MNIST step (k_fwd_conv: dense1 partial -> tagged exchange of
the four quarter partials -> loss head -> dH -> dP2 / dC2 -> conv backward) over CONSECUTIVE SGD steps.

What the chain can get wrong is ordering: a value read before it is written, or a partial that still
carries the previous step's tag.  Such a fault is intermittent and shows as a wrong or a varying bit, so:

* exact: three consecutive SGD steps on ONE step object (chunks 2, 0, 1 of the integer-coded data, so the
  part3t slots are reused with the next tag and hold another chunk's partials), each compared bit for bit
  with the f64 reference: saved state, partial slabs, gradients, and W = W0 - lr G after the update.  W is
  put back to the coded W0 in front of each of these steps: on the updated weights (multiples of
  lr / global batch) the conv2 sums need up to 26 significant bits already at b = 1 (288 products of a P1
  value of up to 2^6 units and a weight of 2^6 units), and an f32 sum that rounds has no order-free f64
  reference.
* repeatable: the same three SGD steps WITHOUT putting W back (the weights change from step to step and
  the data are real-valued from the second step on, so every f32 sum depends on its order), ten times from
  the same W0: W, G, P2, H, dH, dL, part1 and part2 after every step equal the first repetition's bits.
* the error word stays 0 and the loss finite after every step: no poll timed out.

b = 1 and 2: four and eight workgroups, the quarters of an image start far apart; b = 17: the plain block
map (b & 7 != 0); b = 64: the XCD map and every CU of a 256-CU device."""
import numpy as np
import pytest
import torch

import f32_edge_helpers as FE
import mnist_refs as MR
import test_mnist_exact_gpu as TE
from tensorflow_distributed_learning_amd.models import mnist_cnn as M

pytestmark = pytest.mark.gpu

CHUNKS = (2, 0, 1)
REPS = 10
NAMES = ("P2", "H", "dH", "dL", "part1", "part2")


def _fits(cuda, b):
    return 4 * b <= torch.cuda.get_device_properties(cuda).multi_processor_count


def _sgd_step(step, b, k):
    step.metrics.zero_()
    step.forward_backward(k * b)
    step.finalize(True)
    torch.cuda.synchronize()
    step.check()  # the error word
    loss = float(step.metrics[0])
    assert np.isfinite(loss), f"chunk {k}: loss {loss}"


def _state(step, W, G):
    bufs = step.buffers()
    out = {n: bufs[n].cpu().clone() for n in NAMES}
    out["W"], out["G"] = W.cpu().clone(), G.cpu().clone()
    return out


@pytest.mark.parametrize("b", [1, 2, 17, 64])
def test_handoff_consecutive_sgd_steps(cuda, monkeypatch, b):
    if not _fits(cuda, b):
        pytest.skip(f"b={b}: 4b workgroups do not fit the device at once (no fused step)")
    c, layout, W, G, step = TE._coded_step(cuda, monkeypatch, b, 1, "fused")
    assert step.fused_bwd and step.dp2_in_forward
    W0 = W.clone()

    # ---- exact: every step against the f64 reference of its chunk
    for k in CHUNKS:
        S, AB = MR.coded_ref(b, 1, k)  # asserts the exactness conditions
        what = f"b={b} SGD step on chunk {k}"
        W.copy_(W0)
        TE._poison(step, ["P2", "H", "dH", "part1", "part2"])
        _sgd_step(step, b, k)
        TE._exact_saved(step, S, b, True, what)
        TE._exact_grads(layout, G, S, what)
        TE._exact_metrics(step, S, b, what)
        for (name, _), got, p, g in zip(M.MNIST_CNN_VARIABLES, layout.views(W.cpu()), c.params, S.grads):
            FE.same_bits(got, p - c.lr * g, f"{what} W {name}")

    # ---- repeatable: three steps on changing weights, ten times from W0
    first = None
    for rep in range(REPS):
        W.copy_(W0)
        states = []
        for k in CHUNKS:
            _sgd_step(step, b, k)
            states.append(_state(step, W, G))
        assert not torch.equal(states[0]["W"], W0.cpu()) and not torch.equal(states[1]["W"], states[0]["W"])
        if first is None:
            first = states
            continue
        for n, (s0, s1) in enumerate(zip(first, states)):
            for name in s0:
                a0, a1 = s0[name].view(torch.uint8), s1[name].view(torch.uint8)
                assert torch.equal(a0.view(-1), a1.view(-1)), \
                    f"b={b} repetition {rep}, step {n} (chunk {CHUNKS[n]}): {name} differs from the first repetition"
