"""Depthwise 2-D convolution on the hand-written channels-last kernels (csrc/kernels/depthwise.hip).

``depthwise_conv2d(x, w, bias, strides, pads, dilation, act)``: ``x [N,H,W,C]``, the Keras depthwise kernel
``w [kh,kw,C,dm]`` (always f32), ``bias [C*dm]`` (f32 or None), ``pads = (top, bottom, left, right)``; output
channel ``c*dm + m`` reads input channel ``c``.  ``act=1`` fuses ReLU into the forward epilogue and its mask
into both backward kernels (the mask comes from the saved output).

Kernels (csrc/kernels/depthwise.h): an LDS-staged stencil for the forward and the input gradient -- f32
``fmaf`` chains in ascending tap order, one rounding to the dtype -- and a two-launch f64 reduction for the
weight and bias gradient, which is returned or ADDED into slab views.  No atomics, no library call, the same
bits on every run.

:func:`supported`: a non-empty 4-D CUDA tensor, f32 or bf16, ``kh*kw <= 49``, ``dm <= 8``, ``C*dm <= 16384``,
strides and dilations ``>= 1``, a halo tile within the kernels' LDS budget and fewer than 2^24 workgroups (the
binding checks the same and raises).  On a supported GPU tensor the kernels are the only path
(:func:`..ops.hip` raises if the extension is not built); f16 and f64 GPU tensors go through f32, as the other
layers do; CPU tensors and unsupported inputs use :func:`depthwise_conv2d_torch` (``F.conv2d(groups=C)``),
counted on the GPU as a library convolution (``ops.conv.library_calls()``).  ``TDL_DEPTHWISE=torch`` forces it.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import hip
from . import conv as _conv

MAX_TAPS = 49
MAX_DM = 8
MAX_COUT = 16384

CALLS = {"forward": 0, "dgrad": 0, "wgrad": 0}  # launches of the HIP kernels (tests)


def use_torch() -> bool:
    return os.environ.get("TDL_DEPTHWISE", "") == "torch"


def out_size(i, k, s, d, p0, p1):
    return (i + p0 + p1 - (k - 1) * d - 1) // s + 1


def _geo(strides, dilation, pads):
    return [int(strides[0]), int(strides[1]), int(dilation[0]), int(dilation[1]), int(pads[0]), int(pads[2])]


def _out_hw(x, w, strides, dilation, pads):
    return (out_size(x.shape[1], w.shape[0], strides[0], dilation[0], pads[0], pads[1]),
            out_size(x.shape[2], w.shape[1], strides[1], dilation[1], pads[2], pads[3]))


def _shape_ok(x, w, strides, dilation, pads) -> bool:
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.numel() > 0 and w.dim() == 4):
        return False
    kh, kw, c, dm = (int(v) for v in w.shape)
    if c != x.shape[3] or kh * kw > MAX_TAPS or dm > MAX_DM or c * dm > MAX_COUT or w.numel() == 0:
        return False
    if min(*strides, *dilation) < 1 or min(pads) < 0:
        return False
    oh, ow = _out_hw(x, w, strides, dilation, pads)
    if oh < 1 or ow < 1:
        return False
    try:  # the binding's own checks: the LDS budget at the smallest tile and the grid size
        hip().dw_plan(list(x.shape), kh, kw, dm, oh, ow, _geo(strides, dilation, pads), x.dtype == torch.bfloat16)
    except RuntimeError:
        return False
    return True


def supported(x, w, strides=(1, 1), dilation=(1, 1), pads=(0, 0, 0, 0)) -> bool:
    return _shape_ok(x, w, strides, dilation, pads) and x.dtype in (torch.float32, torch.bfloat16)


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _f32(t):
    return _aligned(t.detach().float()) if t is not None else None


class _Depthwise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, strides, pads, dil, act, grad_out, gb_out, anchor=None):
        xc, wc = _aligned(x), _f32(w)
        geo = _geo(strides, dil, pads)
        oh, ow = _out_hw(x, w, strides, dil, pads)
        y = hip().dw_forward(xc, wc, _f32(b), geo, oh, ow, act=int(act))
        CALLS["forward"] += 1
        ctx.save_for_backward(xc, wc, y if act else None)
        ctx.geo, ctx.has_b = geo, b is not None
        ctx.grad_out, ctx.gb_out = grad_out, gb_out
        ctx.dtypes = (w.dtype, b.dtype if b is not None else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        C = hip()
        xc, wc, y = ctx.saved_tensors
        dy = _aligned(dy.to(xc.dtype))
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = C.dw_dgrad(dy, wc, xc.shape[1], xc.shape[2], ctx.geo, dy_mask=y)
            CALLS["dgrad"] += 1
        want_db = ctx.has_b and (ctx.gb_out is not None or ctx.needs_input_grad[2])
        if ctx.grad_out is not None or ctx.needs_input_grad[1] or want_db:
            # slab targets: dW / db added in place; otherwise returned (a bias gradient alone rides the same launches)
            gw, gb = C.dw_wgrad(xc, dy, wc.shape[0], wc.shape[1], ctx.geo, dy_mask=y, dw_out=ctx.grad_out,
                                db_out=ctx.gb_out, want_db=want_db)[:2]
            CALLS["wgrad"] += 1
            if ctx.grad_out is None and ctx.needs_input_grad[1]:
                dw = gw.to(ctx.dtypes[0])
            if ctx.gb_out is None and want_db:
                db = gb.to(ctx.dtypes[1])
        return dx, dw, db, None, None, None, None, None, None, None


def depthwise_conv2d_torch(x, w, bias=None, strides=(1, 1), pads=(0, 0, 0, 0), dilation=(1, 1), act=0):
    """The same function in differentiable PyTorch ops: ``F.conv2d(groups=C)`` over the permuted view, f32
    arithmetic for f16 / bf16 data, the input's own for f32 / f64."""
    kh, kw, c, dm = w.shape
    ct = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32
    if x.is_cuda:
        _conv._lib("depthwise_conv2d", f"{str(x.dtype).replace('torch.', '')} C={c} dm={dm} {kh}x{kw}/{strides[0]}")
    h = F.pad(x.to(ct).permute(0, 3, 1, 2), (pads[2], pads[3], pads[0], pads[1]))
    wt = w.to(ct).reshape(kh, kw, c * dm).permute(2, 0, 1).unsqueeze(1)  # [C*dm, 1, kh, kw], channel c*dm + m
    y = F.conv2d(h, wt, bias.to(ct) if bias is not None else None, stride=tuple(strides), dilation=tuple(dilation),
                 groups=c)
    if act:
        y = torch.relu(y)
    return y.permute(0, 2, 3, 1).to(x.dtype)


def depthwise_conv2d(x, w, bias=None, strides=(1, 1), pads=(0, 0, 0, 0), dilation=(1, 1), act=0, grad_out=None,
                     gb_out=None, anchor=None):
    """``grad_out`` / ``gb_out``: f32 slab views (``Variable.grad_target()``) the GPU backward ADDS the kernel /
    bias gradients into; ``w`` / ``bias`` are then taken without autograd, and ``anchor`` -- the variable's own
    tensor -- keeps the backward reachable when ``x`` itself needs no gradient."""
    strides, pads, dilation = tuple(int(s) for s in strides), tuple(int(p) for p in pads), tuple(int(d) for d in dilation)
    if x.is_cuda and not use_torch():
        if x.dtype in (torch.float16, torch.float64) and _shape_ok(x, w, strides, dilation, pads):
            return depthwise_conv2d(x.to(torch.float32), w, bias, strides, pads, dilation, act, grad_out, gb_out,
                                    anchor).to(x.dtype)
        if supported(x, w, strides, dilation, pads):
            if grad_out is not None and torch.is_grad_enabled():
                w = w.detach()
                bias = bias.detach() if (bias is not None and gb_out is not None) else bias
            else:
                grad_out = gb_out = anchor = None
            return _Depthwise.apply(x, w, bias, strides, pads, dilation, int(act), grad_out, gb_out, anchor)
    return depthwise_conv2d_torch(x, w, bias, strides, pads, dilation, act)
