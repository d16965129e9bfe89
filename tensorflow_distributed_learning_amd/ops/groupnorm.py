"""Group normalisation on the hand-written channels-last kernels (csrc/kernels/groupnorm.hip).

``group_norm(x, groups, gamma, beta, eps)`` normalises a ``[N, ..., C]`` tensor per sample over each of
``groups`` groups of ``C / groups`` consecutive channels and all the dimensions between the first and the
last (Wu & He): ``y = gamma * (x - mean) / sqrt(var + eps) + beta`` with the biased variance.  The
statistics belong to one sample, so training and inference are the same computation and the result does
not depend on the batch a sample sits in, on how a global batch is cut over replicas, or on their number.

Kernels (three launches per direction, csrc/kernels/groupnorm.h): per-(sample, channel) sums over the
pixels in f64 and in a fixed order, a finalize that folds them into groups and writes per-(sample,
channel) f32 coefficients, and an elementwise pass ``y = fmaf(x, scale, shift)`` /
``dx = fmaf(A, dy, fmaf(B, x, D))``.  Only ``x`` and the ``[N, G]`` statistics are saved for the backward.
Outputs are the same bits on every run; a sample's ``y`` and ``dx`` bits depend on that sample alone.

:func:`supported`: a non-empty CUDA tensor of at least 2 dimensions, f32 or bf16, ``C % groups == 0``,
``C <= MAX_C``, ``N * C <= MAX_NC`` (the coefficient tables are ``[N, C]`` f32, up to three of them: 192 MiB
at the limit; the finalize walks a group's channels with one wave) and fewer than ``MAX_WORKGROUPS``
workgroups in a streaming pass (only degenerate shapes, such as 2^24 samples of one value, reach that; the
binding refuses them too, since a grid of 2^32 threads does not launch).  On a GPU tensor that is
supported the kernels are the only path (:func:`..ops.hip` raises if the extension is not built); f16 and
f64 GPU tensors go through f32, as the dropout and augment layers do; CPU tensors and unsupported inputs
use PyTorch ops with the same semantics.  ``TDL_GROUPNORM=torch`` forces those formulas on the GPU as well.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import hip

MAX_C = 16384
MAX_NC = 1 << 24
MAX_WORKGROUPS = 1 << 24  # (a launch of 2^32 threads and more is refused by the runtime)

CALLS = [0]  # forward calls that ran the HIP kernels (tests)
CALLS_BY_DTYPE = {torch.float32: 0, torch.bfloat16: 0}


def use_torch() -> bool:
    return os.environ.get("TDL_GROUPNORM", "") == "torch"


def _shape_ok(x: torch.Tensor, groups: int) -> bool:
    if not (x.is_cuda and x.dim() >= 2 and x.numel() > 0):
        return False
    N, C = x.shape[0], x.shape[-1]
    if not (groups >= 1 and C % groups == 0 and C <= MAX_C and N * C <= MAX_NC):
        return False
    # the streaming passes launch N x column blocks x chunks workgroups of 256 threads (f16 / f64 run as f32)
    plan = hip().gn_plan(x.numel() // (N * C), C, x.dtype == torch.bfloat16)
    return N * plan[4] * plan[6] < MAX_WORKGROUPS


def supported(x: torch.Tensor, groups: int) -> bool:
    return _shape_ok(x, groups) and x.dtype in (torch.float32, torch.bfloat16)


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _GroupNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, grad_out):
        C = hip()
        xc = _aligned(x)
        y, stats = C.gn_forward(xc, int(groups), gamma, beta, float(eps))[:2]
        CALLS[0] += 1
        CALLS_BY_DTYPE[xc.dtype] += 1
        ctx.groups = int(groups)
        ctx.has = (gamma is not None, beta is not None)
        ctx.grad_out = grad_out
        ctx.save_for_backward(xc, stats, gamma if gamma is not None else stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        C = hip()
        xc, stats, gamma = ctx.saved_tensors
        has_g, has_b = ctx.has
        go = ctx.grad_out or (None, None)
        dx, dgamma, dbeta = C.gn_backward(_aligned(dy.to(xc.dtype)), xc, ctx.groups, gamma if has_g else None, stats,
                                          go[0] if has_g else None, go[1] if has_b else None)[:3]
        return (dx, dgamma if (has_g and ctx.needs_input_grad[1]) else None,
                dbeta if (has_b and ctx.needs_input_grad[2]) else None, None, None, None)


def group_norm_torch(x: torch.Tensor, groups: int, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor],
                     eps: float) -> torch.Tensor:
    """The same function in differentiable PyTorch ops: f32 arithmetic for f16 / bf16 data, the input's own
    for f32 / f64."""
    N, C = x.shape[0], x.shape[-1]
    ct = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32
    h = x.to(ct).reshape(N, -1, groups, C // groups)
    mean = h.mean(dim=(1, 3), keepdim=True)
    d = h - mean
    var = (d * d).mean(dim=(1, 3), keepdim=True)
    y = (d * torch.rsqrt(var + eps)).reshape(x.shape)
    if gamma is not None:
        y = y * gamma.to(ct)
    if beta is not None:
        y = y + beta.to(ct)
    return y.to(x.dtype)


def group_norm(x: torch.Tensor, groups: int, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor],
               eps: float, grad_out=None) -> torch.Tensor:
    """``x``: ``[N, ..., C]``, channels last; ``gamma`` / ``beta``: f32 ``[C]`` or None (1 / 0).

    ``grad_out = (dgamma_target, dbeta_target)``: f32 slab views the GPU backward ADDS the gamma / beta
    gradients into (Variable.grad_target); gamma / beta are then passed without autograd."""
    groups = int(groups)
    if x.dim() < 2 or groups < 1 or x.shape[-1] % groups != 0:
        raise ValueError(f"group_norm: groups = {groups} must divide the channel count of {tuple(x.shape)}")
    if x.is_cuda and not use_torch():
        if x.dtype in (torch.float16, torch.float64) and _shape_ok(x, groups):
            return group_norm(x.to(torch.float32), groups, gamma, beta, eps, grad_out).to(x.dtype)
        if supported(x, groups):
            if grad_out is not None and x.requires_grad and torch.is_grad_enabled():
                gamma = gamma.detach() if gamma is not None else None
                beta = beta.detach() if beta is not None else None
            else:  # (no backward would reach the kernel that fills the targets through x)
                grad_out = None
            return _GroupNorm.apply(x, gamma, beta, groups, eps, grad_out)
    if x.numel() == 0:
        return x.clone()
    return group_norm_torch(x, groups, gamma, beta, eps)
