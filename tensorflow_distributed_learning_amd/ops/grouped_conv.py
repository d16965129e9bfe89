"""Grouped 2-D convolution on the hand-written per-group implicit-GEMM kernels (csrc/kernels/grouped_conv.hip).

``conv2d(x, w_hwio, bias, groups, stride, pads, dil)``: ``x [N,H,W,C]`` f32 or bf16, the Keras kernel
``w [kh,kw,C/groups,F]`` and ``bias [F]`` (f32 in memory), ``pads = (top, bottom, left, right)``; filter ``f``
belongs to group ``f // (F/groups)``.  ``act=1`` fuses ReLU into the forward epilogue and its mask into the
loads of both backward kernels (the mask comes from the saved output).

Kernels (csrc/kernels/grouped_conv.h): per-group implicit GEMMs on ``v_mfma_f32_16x16x4_f32`` with f32
accumulation; bf16 activations are widened in the loader and the weight rounded to bf16 as it is staged into
LDS (what ``kernel.cast(bf16)`` gives the library path).  The weight / bias gradient is a split reduction added
in a fixed order, returned or ADDED into slab views.  No atomics, no library call, the same bits on every run.

:func:`supported`: a non-empty 4-D GPU tensor, f32 or bf16, ``C`` and ``F`` multiples of ``groups``,
``kh*kw*max(C, F)/groups <= 2^20``, ``x`` below 2^31 elements (the binding also checks the output's size and the
strides, and raises).  f16 / f64 GPU tensors go through f32.  CPU tensors, ``TDL_GROUPED_CONV=torch`` and
anything unsupported use :func:`conv2d_torch` (``F.conv2d(groups=)``), counted on the GPU as a library
convolution (``ops.conv.library_calls()``).
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import hip
from . import conv as _conv

MAX_RED = 1 << 20

CALLS = {"forward": 0, "dgrad": 0, "wgrad": 0}  # launches of the HIP kernels (tests)


def use_torch() -> bool:
    return os.environ.get("TDL_GROUPED_CONV", "") == "torch"


def out_size(i, k, s, d, p0, p1):
    return (i + p0 + p1 - (k - 1) * d - 1) // s + 1


def _shape_ok(x, w, groups) -> bool:
    g = int(groups)
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and w.dim() == 4 and g >= 1):
        return False
    if x.numel() == 0 or w.numel() == 0 or x.numel() >= 1 << 31:
        return False
    kh, kw, cg, f = (int(v) for v in w.shape)
    return x.shape[3] % g == 0 and f % g == 0 and cg * g == x.shape[3] and kh * kw * max(cg, f // g) <= MAX_RED


def supported(x, w, groups) -> bool:
    return _shape_ok(x, w, groups) and x.dtype in (torch.float32, torch.bfloat16)


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _f32(t):
    return _aligned(t.detach().float()) if t is not None else None


def _geo(stride, pads, dil):
    return [int(stride[0]), int(stride[1]), int(dil[0]), int(dil[1]), int(pads[0]), int(pads[2])]


def fwd(x, w_hwio, bias, groups, stride, pads, dil=(1, 1), act=0) -> torch.Tensor:
    """``y = conv_g(x, w) + bias`` in x's dtype (``act=1``: ReLU in the epilogue)."""
    oh = out_size(x.shape[1], w_hwio.shape[0], stride[0], dil[0], pads[0], pads[1])
    ow = out_size(x.shape[2], w_hwio.shape[1], stride[1], dil[1], pads[2], pads[3])
    CALLS["forward"] += 1
    return hip().gconv_forward(_aligned(x), _f32(w_hwio), _f32(bias), int(groups), _geo(stride, pads, dil), oh, ow,
                               act=int(act))


def dgrad(dy, w_hwio, groups, hw, stride, pads, dil=(1, 1), dy_mask=None) -> torch.Tensor:
    """Input gradient of :func:`fwd` for an input of spatial size ``hw`` (``dy_mask``: the saved ReLU output)."""
    CALLS["dgrad"] += 1
    return hip().gconv_dgrad(_aligned(dy), _f32(w_hwio), int(groups), hw[0], hw[1], _geo(stride, pads, dil),
                             dy_mask=dy_mask)


def wgrad(x, dy, rs, groups, stride, pads, dil=(1, 1), out=None, accumulate=False, dy_mask=None, dbias=None):
    """f32 ``[kh,kw,C/groups,F]`` weight gradient of :func:`fwd` (added into the f32 ``out`` when ``accumulate``);
    ``dbias``: the bias gradient from the same launches (written, or added into when ``accumulate``)."""
    CALLS["wgrad"] += 1
    return hip().gconv_wgrad(_aligned(x), _aligned(dy), rs[0], rs[1], int(groups), _geo(stride, pads, dil),
                             dy_mask=dy_mask, out=out, accumulate=accumulate, dbias=dbias)


class _GroupedConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, groups, stride, pads, dil, grad_out, anchor=None, act=0, gb_out=None):
        xc, wc = _aligned(x), _f32(w)
        y = fwd(xc, wc, b, groups, stride, pads, dil, act)
        ctx.save_for_backward(xc, wc, y if act else None)
        ctx.geo = (groups, stride, pads, dil)
        ctx.has_b = b is not None
        ctx.grad_out, ctx.gb_out = grad_out, gb_out
        ctx.dtypes = (w.dtype, b.dtype if b is not None else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        groups, stride, pads, dil = ctx.geo
        dy = _aligned(dy.to(x.dtype))
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = dgrad(dy, w, groups, (x.shape[1], x.shape[2]), stride, pads, dil, dy_mask=y)
        rs = (w.shape[0], w.shape[1])
        f32 = dict(dtype=torch.float32, device=dy.device)
        want_db = ctx.has_b and (ctx.gb_out is not None or ctx.needs_input_grad[2])
        if ctx.grad_out is not None:
            # slab targets: dW (and db, from the same launches) added in place
            dbt = ctx.gb_out if ctx.gb_out is not None else (torch.zeros(w.shape[-1], **f32) if want_db else None)
            wgrad(x, dy, rs, groups, stride, pads, dil, out=ctx.grad_out, accumulate=True, dy_mask=y, dbias=dbt)
            if ctx.gb_out is None and want_db:
                db = dbt.to(ctx.dtypes[1])
        elif ctx.needs_input_grad[1] or want_db:
            dbt = torch.empty(w.shape[-1], **f32) if want_db else None
            gw = wgrad(x, dy, rs, groups, stride, pads, dil, dy_mask=y, dbias=dbt)
            if ctx.needs_input_grad[1]:
                dw = gw.to(ctx.dtypes[0])
            if want_db:
                if ctx.gb_out is not None:
                    ctx.gb_out.add_(dbt)
                else:
                    db = dbt.to(ctx.dtypes[1])
        return dx, dw, db, None, None, None, None, None, None, None, None


def conv2d_torch(x, w_hwio, bias=None, groups=1, stride=(1, 1), pads=(0, 0, 0, 0), dil=(1, 1), act=0):
    """The same function in differentiable PyTorch ops: ``F.conv2d(groups=)`` over the permuted view, the
    kernel and bias cast to the data dtype (as Conv2D's library branch does)."""
    if x.is_cuda:
        _conv._lib("conv2d", f"{str(x.dtype).replace('torch.', '')} C={x.shape[-1]} K={w_hwio.shape[-1]} "
                   f"g={groups} {w_hwio.shape[0]}x{w_hwio.shape[1]}/{stride[0]}")
    h = F.pad(x.permute(0, 3, 1, 2), (pads[2], pads[3], pads[0], pads[1]))
    y = F.conv2d(h, w_hwio.to(x.dtype).permute(3, 2, 0, 1), bias.to(x.dtype) if bias is not None else None,
                 stride=tuple(stride), dilation=tuple(dil), groups=int(groups))
    if act:
        y = torch.relu(y)
    return y.permute(0, 2, 3, 1)


def conv2d(x, w_hwio, bias=None, groups=1, stride=(1, 1), pads=(0, 0, 0, 0), dil=(1, 1), grad_out=None, anchor=None,
           act=0, gb_out=None):
    """``grad_out`` / ``gb_out``: f32 slab views (``Variable.grad_target()``) the GPU backward ADDS the kernel /
    bias gradients into; ``w`` / ``bias`` are then taken without autograd, and ``anchor`` -- the variable's own
    tensor -- keeps the backward reachable when ``x`` itself needs no gradient."""
    stride, pads, dil = tuple(int(s) for s in stride), tuple(int(p) for p in pads), tuple(int(d) for d in dil)
    if x.is_cuda and not use_torch():
        if x.dtype in (torch.float16, torch.float64) and _shape_ok(x, w_hwio, groups):
            return conv2d(x.to(torch.float32), w_hwio, bias, groups, stride, pads, dil, grad_out, anchor, act,
                          gb_out).to(x.dtype)
        if supported(x, w_hwio, groups):
            if grad_out is not None and torch.is_grad_enabled():
                w_hwio = w_hwio.detach()
                bias = bias.detach() if (bias is not None and gb_out is not None) else bias
            else:
                grad_out = gb_out = anchor = None
            return _GroupedConv.apply(x, w_hwio, bias, int(groups), stride, pads, dil, grad_out, anchor, int(act),
                                      gb_out)
    return conv2d_torch(x, w_hwio, bias, groups, stride, pads, dil, act)
