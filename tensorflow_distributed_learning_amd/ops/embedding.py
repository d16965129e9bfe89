"""Embedding lookup on the hand-written gather / ordered-gradient kernels (csrc/kernels/embedding.hip).

``embedding(ids, table, out_dtype)`` is ``table[ids]``: ``ids [...]`` int32 or int64 (read as they come, no cast
launch), ``table [V, D]`` f32, the result ``[..., D]`` in f32 or bf16 (one round-to-nearest-even per element, or a
plain copy of ``table_bf16``, the trainer's bf16 compute copy of the table: the same bits).

Kernels (csrc/kernels/embedding.h): one forward launch; the backward is a count launch and one owner-computes
launch.  ``dE[v]`` is the f32 left fold of ``dy[n]`` over the tokens with ``ids[n] == v`` in ascending ``n``, started
from the first term, then ``target[v] + s`` once when the gradient is added into a slab view: no sort, no float
atomics, the same bits on every run, reproducible in numpy (tests/embedding_refs.py).  **An id outside ``[0, V)``
is defined on the kernels: a zero row forward, no contribution backward** (``F.embedding`` asserts on the device).

:func:`supported`: non-empty CUDA tensors, 32- or 64-bit integer ids, an f32 table, ``D <= MAX_D``, tensors below
2^31 elements, fewer than ``MAX_WORKGROUPS`` workgroups, and the two measured bounds ``MAX_TOKEN_BLOCKS`` and
``MAX_SCAN`` (where profiles/embedding_cost.txt has the kernels at or below ``F.embedding`` for uniform and skewed ids).  On
a supported GPU input the kernels are the only path (:func:`..ops.hip` raises if the extension is not built).
CPU tensors use :func:`embedding_torch` (``F.embedding``, bit for bit what the layer did before); so do unsupported
GPU inputs (counted in ``FALLBACKS``) and every GPU input under ``TDL_EMBEDDING=torch``.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn.functional as F

from . import hip

MAX_D = 4096
MAX_WORKGROUPS = 1 << 24  # (a launch of 2^32 threads and more is refused by the runtime)
MAX_ELEMS = 1 << 31
# Both from profiles/embedding_cost.txt.  A row's additions are one wave's serial chain, so under a skewed law the
# hottest owner decides the time: N * (64-lane column blocks of a row) at most -- at 2048 the kernels are at 0.55-0.61
# of F.embedding's forward + backward under Zipf(1), at 4096 at 1.5.  And ceil(V / rows_wg) * N at most (every owner
# scans all ids): below the largest product measured, where the kernels are at 0.5-0.63 on uniform ids.
MAX_TOKEN_BLOCKS = 2048
MAX_SCAN = 1 << 24

CALLS = [0]  # forward calls that ran the HIP kernels (tests)
CALLS_BY_DTYPE = {torch.float32: 0, torch.bfloat16: 0}
FALLBACKS = [0]  # GPU calls that took F.embedding without TDL_EMBEDDING=torch asking for it


def use_torch() -> bool:
    return os.environ.get("TDL_EMBEDDING", "") == "torch"


def supported(ids: torch.Tensor, table: torch.Tensor) -> bool:
    if not (ids.is_cuda and table.is_cuda and ids.dtype in (torch.int32, torch.int64) and ids.numel() > 0
            and table.dtype == torch.float32 and table.dim() == 2):
        return False
    N, (V, D) = ids.numel(), table.shape
    if not (1 <= D <= MAX_D and V >= 1 and N * D < MAX_ELEMS and V * D < MAX_ELEMS):
        return False
    p = hip().embed_plan(N, V, D, False)  # (rows_wg and ranges do not depend on the dtype)
    return (max(p["ranges"], p["fwd_blocks"]) < MAX_WORKGROUPS and p["ranges"] * N <= MAX_SCAN
            and N * -(-D // (64 * p["vec"])) <= MAX_TOKEN_BLOCKS)


class _Embedding(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, table, out_bf16, grad_out, anchor, table_bf16):
        K = hip()
        idc = ids.contiguous()
        src = table_bf16 if (out_bf16 and table_bf16 is not None) else table
        y = K.embed_forward(idc, src.detach().contiguous(), out_bf16)
        CALLS[0] += 1
        CALLS_BY_DTYPE[y.dtype] += 1
        ctx.V, ctx.grad_out = table.shape[0], grad_out
        ctx.save_for_backward(idc)
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 6
        (ids,) = ctx.saved_tensors
        if dy.dtype not in (torch.float32, torch.bfloat16):
            dy = dy.float()
        if ctx.grad_out is not None:  # added into the slab view; autograd sees no gradient
            hip().embed_backward(ids, dy.contiguous(), ctx.V, ctx.grad_out)
            return (None,) * 6
        dE = hip().embed_backward(ids, dy.contiguous(), ctx.V, None) if ctx.needs_input_grad[1] else None
        return None, dE, None, None, None, None


def embedding_torch(ids: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """``F.embedding(ids.long(), table)``: the formula path, in the table's dtype."""
    return F.embedding(ids.long(), table)


def embedding(ids: torch.Tensor, table: torch.Tensor, out_dtype: torch.dtype = torch.float32,
              grad_out: Optional[torch.Tensor] = None, anchor: Optional[torch.Tensor] = None,
              table_bf16: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``table[ids]`` as ``out_dtype`` (f32 or bf16) on the kernels; the formula path returns the table's dtype.

    ``grad_out``: the contiguous f32 ``[V, D]`` slab view the GPU backward ADDS the table's gradient into
    (Variable.grad_target).  The ids carry no gradient, so ``table`` is then passed detached and ``anchor``, the
    variable's leaf, makes the backward run.  ``table_bf16``: the trainer's bf16 copy of the table, read instead of
    the f32 table for a bf16 result."""
    if ids.is_cuda and not use_torch():
        if out_dtype in (torch.float32, torch.bfloat16) and supported(ids, table):
            if (grad_out is not None and anchor is not None and anchor.requires_grad and torch.is_grad_enabled()
                    and grad_out.is_contiguous()):
                table = table.detach()
            else:  # no target: the gradient goes to the leaf through autograd
                table, grad_out, anchor = (anchor if anchor is not None else table), None, None
            return _Embedding.apply(ids, table, out_dtype == torch.bfloat16, grad_out, anchor, table_bf16)
        if ids.numel() > 0:
            FALLBACKS[0] += 1
    return embedding_torch(ids, anchor if anchor is not None else table)
