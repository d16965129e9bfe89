"""Layer and RMS normalisation on the hand-written row kernels (csrc/kernels/layernorm.hip).

``layer_norm(x, gamma, beta, eps, rms=False)`` normalises ``x`` over its last ``gamma.dim()`` (1 without
parameters, or ``axes``) dimensions, flattened to one row of ``C`` contiguous elements:
``y = gamma * (x - mean) / sqrt(var + eps) + beta`` with the biased variance, or, with ``rms``,
``y = gamma * x / sqrt(mean(x^2) + eps)`` (no centring, no beta).

Kernels (csrc/kernels/layernorm.h): a row is read once and held in the registers of its lanes; the forward is
one launch (f64 centred statistics, ``xhat = fmaf(x, a, b)``, ``y = fmaf(xhat, gamma, beta)``), the backward
two (dx and per-block f64 partials of dgamma / dbeta, then their fold).  Only ``x`` and the ``[R, 2]`` statistics
are saved.  Outputs are the same bits on every run; a row's ``y`` and ``dx`` bits depend on that row alone.

:func:`supported`: a non-empty CUDA tensor, f32 or bf16, ``C <= MAX_C`` (``MAX_C_PER_ELEMENT`` when a row is not a
multiple of 16 bytes) and fewer than ``MAX_WORKGROUPS`` workgroups.  On a GPU tensor that is supported the
kernels are the only path (:func:`..ops.hip` raises if the extension is not built); f16 and f64 GPU tensors go
through f32; CPU tensors and unsupported inputs use PyTorch ops with the same semantics
(:func:`layer_norm_torch`, counted in ``FALLBACKS`` on the GPU).  ``TDL_LAYERNORM=torch`` forces those formulas
on the GPU as well.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import hip

MAX_C = 8192
MAX_C_PER_ELEMENT = 4096
MAX_WORKGROUPS = 1 << 24  # (a launch of 2^32 threads and more is refused by the runtime)

CALLS = [0]  # forward calls that ran the HIP kernels (tests)
CALLS_BY_DTYPE = {torch.float32: 0, torch.bfloat16: 0}
FALLBACKS = [0]  # GPU calls that took the PyTorch formula without TDL_LAYERNORM=torch asking for it


def use_torch() -> bool:
    return os.environ.get("TDL_LAYERNORM", "") == "torch"


def _shape_ok(x: torch.Tensor, axes: int) -> bool:
    if not (isinstance(axes, int) and x.is_cuda and 1 <= axes <= x.dim() and x.numel() > 0):
        return False
    C = 1
    for d in x.shape[x.dim() - axes:]:
        C *= int(d)
    esz = 2 if x.dtype == torch.bfloat16 else 4  # (f16 / f64 run as f32)
    if C > (MAX_C if (C * esz) % 16 == 0 else MAX_C_PER_ELEMENT):
        return False
    R = x.numel() // C
    rows = hip().ln_plan(R, C, esz == 2)["rows_fwd"]  # rows per forward workgroup of 256 threads
    return (R + rows - 1) // rows < MAX_WORKGROUPS


def supported(x: torch.Tensor, axes: int = 1) -> bool:
    """``axes``: how many trailing dimensions are normalised (anything else is not the kernels')."""
    return _shape_ok(x, axes) and x.dtype in (torch.float32, torch.bfloat16)


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _flat_param(p: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if p is None else _aligned(p.reshape(-1))


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, C, eps, rms, grad_out):
        K = hip()
        xc = _aligned(x).view(-1, C)
        g, b = _flat_param(gamma), (None if rms else _flat_param(beta))
        y, stats = K.ln_forward(xc, g, b, float(eps), bool(rms))
        CALLS[0] += 1
        CALLS_BY_DTYPE[xc.dtype] += 1
        ctx.rms = bool(rms)
        ctx.shapes = (x.shape, gamma.shape if gamma is not None else None, beta.shape if beta is not None else None)
        ctx.grad_out = grad_out
        ctx.save_for_backward(xc, stats, g if g is not None else stats)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        K = hip()
        xc, stats, g = ctx.saved_tensors
        xs, gs, bs = ctx.shapes
        has_g, has_b = gs is not None, bs is not None and not ctx.rms
        go = ctx.grad_out or (None, None)
        want = bool((has_g and (ctx.needs_input_grad[1] or go[0] is not None))
                    or (has_b and (ctx.needs_input_grad[2] or go[1] is not None)))
        dx, dg, db = K.ln_backward(_aligned(dy.to(xc.dtype)).view(xc.shape), xc, g if has_g else None, stats, ctx.rms,
                                   go[0].view(-1) if (has_g and go[0] is not None) else None,
                                   go[1].view(-1) if (has_b and go[1] is not None) else None, want)
        return (dx.view(xs), dg.view(gs) if (has_g and ctx.needs_input_grad[1]) else None,
                db.view(bs) if (has_b and ctx.needs_input_grad[2]) else None, None, None, None, None)


def layer_norm_torch(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float,
                     rms: bool = False, axes: Optional[int] = None) -> torch.Tensor:
    """The same function in differentiable PyTorch ops: f32 arithmetic for f16 / bf16 data, the input's own
    for f32 / f64."""
    axes = axes or (gamma.dim() if gamma is not None else beta.dim() if beta is not None else 1)
    dims = tuple(range(x.dim() - axes, x.dim()))
    ct = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32
    h = x.to(ct)
    if rms:
        y = h * torch.rsqrt((h * h).mean(dim=dims, keepdim=True) + eps)
    else:
        d = h - h.mean(dim=dims, keepdim=True)
        y = d * torch.rsqrt((d * d).mean(dim=dims, keepdim=True) + eps)
    if gamma is not None:
        y = y * gamma.to(ct)
    if beta is not None and not rms:
        y = y + beta.to(ct)
    return y.to(x.dtype)


def layer_norm(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float,
               rms: bool = False, grad_out=None, axes: Optional[int] = None) -> torch.Tensor:
    """``x``: ``[..., *S]`` normalised over its trailing dimensions ``S``; ``gamma`` / ``beta``: f32 of shape ``S``
    or None (1 / 0); ``axes = len(S)`` (taken from the parameters when they are given, else 1).

    ``grad_out = (dgamma_target, dbeta_target)``: f32 slab views the GPU backward ADDS the gamma / beta
    gradients into (Variable.grad_target); gamma / beta are then passed without autograd."""
    axes = axes or (gamma.dim() if gamma is not None else beta.dim() if beta is not None else 1)
    for p in (gamma, beta):
        if p is not None and tuple(p.shape) != tuple(x.shape[x.dim() - axes:]):
            raise ValueError(f"layer_norm: parameters of shape {tuple(p.shape)} for an input of shape {tuple(x.shape)}")
    if x.is_cuda and not use_torch():
        if x.dtype in (torch.float16, torch.float64) and _shape_ok(x, axes):
            return layer_norm(x.to(torch.float32), gamma, beta, eps, rms, grad_out, axes).to(x.dtype)
        if supported(x, axes):
            if grad_out is not None and x.requires_grad and torch.is_grad_enabled():
                gamma = gamma.detach() if gamma is not None else None
                beta = beta.detach() if beta is not None else None
            else:  # (no backward would reach the kernel that fills the targets through x)
                grad_out = None
            C = x[(0,) * (x.dim() - axes)].numel()
            return _LayerNorm.apply(x, gamma, beta, C, eps, rms, grad_out)
        if x.numel() > 0:
            FALLBACKS[0] += 1
    if x.numel() == 0:
        return x.clone()
    return layer_norm_torch(x, gamma, beta, eps, rms, axes)
