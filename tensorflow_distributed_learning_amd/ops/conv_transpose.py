"""Transposed 2-D convolution on the hand-written stride-phase implicit-GEMM kernels (csrc/kernels/conv_transpose.hip).

``conv2d_transpose(x, w, bias, stride, padding, output_padding, dil)``: ``x [N,H,W,C]`` f32 or bf16, the Keras
kernel ``w [kh,kw,F,C]`` (filters before input channels) and ``bias [F]`` (f32 in memory)::

    y[n,oy,ox,f] = b[f] + sum x[n,iy,ix,c] w[i,j,f,c]    over oy = iy sh - pt + i dh, ox = ix sw - pl + j dw

the input gradient of the Conv2D that maps ``[N,OH,OW,F]`` to ``[N,H,W,C]`` with ``w`` as its HWIO kernel.  Sizes
(:func:`out_size`), per axis with ``ke = (k - 1) d + 1``: without ``output_padding`` ``H s + max(ke - s, 0)``
('valid') or ``H s`` ('same'); with ``output_padding = op`` ``(H - 1) s + ke + op`` ('valid') or
``(H - 1) s + ke - 2 (ke // 2) + op`` ('same').  The leading crop ``pt`` is 0 for 'valid' and the leading TF 'same'
pad of the mirrored Conv2D (over ``OH``) for 'same'.  Output pixels no tap reaches hold ``act(b)``.  ``act=1`` fuses
ReLU into the forward epilogue and its mask into the loads of the backward kernels (from the saved output).

Kernels (csrc/kernels/conv_transpose.h): one dense implicit GEMM per stride phase on ``v_mfma_f32_16x16x4_f32``
with f32 accumulation; bf16 activations are widened in the loader and the weight rounded to bf16 as it is staged
into LDS.  The weight / bias gradient is a split reduction added in a fixed order, returned or ADDED into slab
views.  No atomics, no library call, the same bits on every run.

:func:`supported`: a non-empty 4-D GPU tensor, f32 or bf16, ``w [kh,kw,F,C]`` with x's ``C``,
``kh*kw*max(C, F) <= 2^20``, strides up to 8, ``x``, ``w`` and the output below 2^31 elements, dilations and
crops below 65536 and a window extent below 2^28 (the binding's own checks, which raise, mirrored).  f16 / f64 GPU
tensors go through f32.  CPU tensors, ``TDL_CONV_TRANSPOSE=torch`` and anything unsupported use :func:`conv2d_transpose_torch` (the full
``F.conv_transpose2d``, zero-extended and cropped at ``(pt, pl)``), counted on the GPU as a library convolution
(``ops.conv.library_calls()``).
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import hip
from . import conv as _conv

MAX_RED = 1 << 20
MAX_STRIDE = 8

CALLS = {"forward": 0, "dgrad": 0, "wgrad": 0}  # launches of the HIP kernels (tests)


def use_torch() -> bool:
    return os.environ.get("TDL_CONV_TRANSPOSE", "") == "torch"


def out_size(i, k, s, d, padding, op=None):
    """(output size, leading crop) of one axis."""
    ke = (k - 1) * d + 1
    if op is None:
        o = i * s + (max(ke - s, 0) if padding == "valid" else 0)
    else:
        o = (i - 1) * s + ke + op - (2 * (ke // 2) if padding == "same" else 0)
    if padding == "valid":
        return o, 0
    return o, max((-(-o // s) - 1) * s + ke - o, 0) // 2  # the mirrored Conv2D's leading 'same' pad


def _geometry(x, w, stride, padding, output_padding, dil):
    op = output_padding if output_padding is not None else (None, None)
    oh, pt = out_size(int(x.shape[1]), int(w.shape[0]), stride[0], dil[0], padding, op[0])
    ow, pl = out_size(int(x.shape[2]), int(w.shape[1]), stride[1], dil[1], padding, op[1])
    return oh, ow, pt, pl


def _shape_ok(x, w, stride=(1, 1), padding="valid", output_padding=None, dil=(1, 1)) -> bool:
    """The binding's limits (ct_check in csrc/ops_bindings.cpp), so that nothing it would refuse reaches it."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and w.dim() == 4):
        return False
    if x.numel() == 0 or w.numel() == 0 or x.numel() >= 1 << 31 or w.numel() >= 1 << 31:
        return False
    kh, kw, f, c = (int(v) for v in w.shape)
    if c != x.shape[3] or kh * kw * max(c, f) > MAX_RED or not 1 <= min(stride) <= max(stride) <= MAX_STRIDE:
        return False
    oh, ow, pt, pl = _geometry(x, w, stride, padding, output_padding, dil)
    extent = max((int(x.shape[1]) - 1) * stride[0] + (kh - 1) * dil[0],
                 (int(x.shape[2]) - 1) * stride[1] + (kw - 1) * dil[1])
    return (1 <= min(dil) <= max(dil) < 65536 and max(pt, pl) < 65536 and extent < 1 << 28 and 1 <= min(oh, ow)
            and max(oh, ow) < 1 << 28 and int(x.shape[0]) * oh * ow * f < 1 << 31)


def supported(x, w, stride=(1, 1), padding="valid", output_padding=None, dil=(1, 1)) -> bool:
    return _shape_ok(x, w, stride, padding, output_padding, dil) and x.dtype in (torch.float32, torch.bfloat16)


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _f32(t):
    return _aligned(t.detach().float()) if t is not None else None


def _geo(stride, dil, pt, pl):
    return [int(stride[0]), int(stride[1]), int(dil[0]), int(dil[1]), int(pt), int(pl)]


def fwd(x, w, bias, out_hw, stride, lead, dil=(1, 1), act=0) -> torch.Tensor:
    """``y [N, out_hw, F]`` in x's dtype with the leading crop ``lead = (pt, pl)`` (``act=1``: ReLU in the epilogue)."""
    CALLS["forward"] += 1
    return hip().convt_forward(_aligned(x), _f32(w), _f32(bias), _geo(stride, dil, *lead), out_hw[0], out_hw[1],
                               act=int(act))


def dgrad(dy, w, hw, stride, lead, dil=(1, 1), dy_mask=None) -> torch.Tensor:
    """Input gradient of :func:`fwd` for an input of spatial size ``hw`` (``dy_mask``: the saved ReLU output)."""
    CALLS["dgrad"] += 1
    return hip().convt_dgrad(_aligned(dy), _f32(w), hw[0], hw[1], _geo(stride, dil, *lead), dy_mask=dy_mask)


def wgrad(x, dy, rs, stride, lead, dil=(1, 1), out=None, accumulate=False, dy_mask=None, dbias=None):
    """f32 ``[kh,kw,F,C]`` weight gradient of :func:`fwd` (added into the f32 ``out`` when ``accumulate``);
    ``dbias``: the bias gradient from the same call (written, or added into when ``accumulate``)."""
    CALLS["wgrad"] += 1
    return hip().convt_wgrad(_aligned(x), _aligned(dy), rs[0], rs[1], _geo(stride, dil, *lead), dy_mask=dy_mask,
                             out=out, accumulate=accumulate, dbias=dbias)


class _ConvTranspose(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, out_hw, stride, lead, dil, grad_out, anchor=None, act=0, gb_out=None):
        xc, wc = _aligned(x), _f32(w)
        y = fwd(xc, wc, b, out_hw, stride, lead, dil, act)
        ctx.save_for_backward(xc, wc, y if act else None)
        ctx.geo = (stride, lead, dil)
        ctx.has_b = b is not None
        ctx.grad_out, ctx.gb_out = grad_out, gb_out
        ctx.dtypes = (w.dtype, b.dtype if b is not None else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        stride, lead, dil = ctx.geo
        dy = _aligned(dy.to(x.dtype))
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = dgrad(dy, w, (x.shape[1], x.shape[2]), stride, lead, dil, dy_mask=y)
        rs = (w.shape[0], w.shape[1])
        f32 = dict(dtype=torch.float32, device=dy.device)
        want_db = ctx.has_b and (ctx.gb_out is not None or ctx.needs_input_grad[2])
        if ctx.grad_out is not None:
            # slab targets: dW (and db, from the same call) added in place
            dbt = ctx.gb_out if ctx.gb_out is not None else (torch.zeros(w.shape[2], **f32) if want_db else None)
            wgrad(x, dy, rs, stride, lead, dil, out=ctx.grad_out, accumulate=True, dy_mask=y, dbias=dbt)
            if ctx.gb_out is None and want_db:
                db = dbt.to(ctx.dtypes[1])
        elif ctx.needs_input_grad[1] or want_db:
            dbt = torch.empty(w.shape[2], **f32) if want_db else None
            gw = wgrad(x, dy, rs, stride, lead, dil, dy_mask=y, dbias=dbt)
            if ctx.needs_input_grad[1]:
                dw = gw.to(ctx.dtypes[0])
            if want_db:
                if ctx.gb_out is not None:
                    ctx.gb_out.add_(dbt)
                else:
                    db = dbt.to(ctx.dtypes[1])
        return dx, dw, db, None, None, None, None, None, None, None, None


def conv2d_transpose_torch(x, w, bias=None, stride=(1, 1), padding="valid", output_padding=None, dil=(1, 1), act=0):
    """The same function in differentiable PyTorch ops: the full ``F.conv_transpose2d`` (no padding), zero-extended
    to the output size and cropped at ``(pt, pl)``, the kernel and bias cast to the data dtype."""
    oh, ow, pt, pl = _geometry(x, w, stride, padding, output_padding, dil)
    if x.is_cuda:
        _conv._lib("conv2d_transpose", f"{str(x.dtype).replace('torch.', '')} C={x.shape[-1]} F={w.shape[2]} "
                   f"{w.shape[0]}x{w.shape[1]}/{stride[0]} {padding}")
    full = F.conv_transpose2d(x.permute(0, 3, 1, 2), w.to(x.dtype).permute(3, 2, 0, 1), None, stride=tuple(stride),
                              dilation=tuple(dil))
    full = F.pad(full, (0, max(pl + ow - full.shape[3], 0), 0, max(pt + oh - full.shape[2], 0)))
    y = full[:, :, pt:pt + oh, pl:pl + ow].permute(0, 2, 3, 1)
    if bias is not None:
        y = y + bias.to(x.dtype)
    return torch.relu(y) if act else y


def conv2d_transpose(x, w, bias=None, stride=(1, 1), padding="valid", output_padding=None, dil=(1, 1), grad_out=None,
                     anchor=None, act=0, gb_out=None):
    """``grad_out`` / ``gb_out``: f32 slab views (``Variable.grad_target()``) the GPU backward ADDS the kernel /
    bias gradients into; ``w`` / ``bias`` are then taken without autograd, and ``anchor`` -- the variable's own
    tensor -- keeps the backward reachable when ``x`` itself needs no gradient."""
    stride, dil = tuple(int(s) for s in stride), tuple(int(d) for d in dil)
    if x.is_cuda and not use_torch():
        if x.dtype in (torch.float16, torch.float64) and _shape_ok(x, w, stride, padding, output_padding, dil):
            return conv2d_transpose(x.to(torch.float32), w, bias, stride, padding, output_padding, dil, grad_out, anchor,
                                    act, gb_out).to(x.dtype)
        if supported(x, w, stride, padding, output_padding, dil):
            oh, ow, pt, pl = _geometry(x, w, stride, padding, output_padding, dil)
            if grad_out is not None and torch.is_grad_enabled():
                w = w.detach()
                bias = bias.detach() if (bias is not None and gb_out is not None) else bias
            else:
                grad_out = gb_out = anchor = None
            return _ConvTranspose.apply(x, w, bias, (oh, ow), stride, (pt, pl), dil, grad_out, anchor, int(act), gb_out)
    return conv2d_transpose_torch(x, w, bias, stride, padding, output_padding, dil, act)
