"""engine/execution.py without a GPU: which executions a run warms, the graph keys of an accumulating
optimizer, and the optimizers' ``zero_grad`` request as an argument (never an attribute set on the side)."""
import pytest
import torch

import tensorflow_distributed_learning_amd as tdl
from tensorflow_distributed_learning_amd.engine import execution as EX

O = tdl.keras.optimizers


@pytest.mark.parametrize("args, want", [
    ((12, 4, 3), [(4, 0), (4, 4), (4, 8)]),
    ((10, 4, 1), [(4, 0), (2, 8)]),
    ((3, 4, 1), [(3, 0)]),
    ((9, 4, 2), [(4, 0), (4, 4), (1, 8)]),
    ((8, 4, 5), [(4, 0), (4, 4)]),
])
def test_execution_starts(args, want):
    assert EX.execution_starts(*args) == want


def test_accum_key():
    assert EX.accum_key(O.SGD(0.1), ("dev", 4, 16)) == ("dev", 4, 16)
    opt = O.SGD(0.1, gradient_accumulation_steps=3)
    opt.iterations = 4
    assert EX.accum_key(opt, ("dev", 4, 16)) == ("dev", 4, 16, 1)
    assert EX.accum_key(opt, ("dev", 4, 16), t_add=2) == ("dev", 4, 16, 0)


@pytest.mark.parametrize("make", [lambda **kw: O.SGD(0.1, **kw), lambda **kw: O.SGD(0.1, momentum=0.9, **kw),
                                  lambda **kw: O.Adam(1e-3, **kw)], ids=["sgd", "sgd-momentum", "adam"])
def test_zero_grad_is_an_argument_and_a_cpu_slab_is_never_zeroed(make):
    g = torch.arange(1.0, 38.0)
    opt = make(gradient_accumulation_steps=2)
    W, G = torch.ones(37), g.clone()
    assert opt.accumulate(G, zero_grad=True) is False
    assert torch.equal(G, g)
    assert opt.apply_flat(W, G, accumulated=True, zero_grad=True) is False  # (a micro-step of its own: counts)
    assert torch.equal(G, g) and not torch.equal(W, torch.ones(37))
    plain = make()
    assert plain.accumulate(G, zero_grad=True) is True and torch.equal(G, g)
    assert plain.apply_flat(W, G, zero_grad=True) is False and torch.equal(G, g)
    for o in (opt, plain):
        assert not hasattr(o, "_zero_grad_after") and not hasattr(o, "_zeroed_grad")
