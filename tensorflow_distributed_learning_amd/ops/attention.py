"""Scaled-dot-product attention on the fused MFMA kernels of csrc/kernels/attention.hip.

``sdpa(q, k, v, scale=None, causal=False, mask=None)``: ``q [B,T,H,D]``, ``k [B,S,H,D]``, ``v [B,S,H,Dv]`` (f32 or
bf16, any strides on the first three axes: projection outputs and slices of a packed qkv buffer are consumed as
views, no permute or copy is launched) give ``o [B,T,H,Dv]``::

    o[b,i,h] = sum_j softmax_j(scale q[b,i,h] . k[b,j,h]) v[b,j,h]       over the admitted keys j of row i

Key ``j`` is admitted iff ``j < S``, (not ``causal`` or ``j <= i``: Keras' lower-triangular mask, also for
``T != S``) and (no ``mask`` or ``mask[b,(h),i,j] != 0``; a bool / uint8 ``[B,T,S]`` or ``[B,H,T,S]``).  A row without
an admitted key gives ``o = 0`` and zero gradients, never NaN -- Keras gives the mean of ``v`` there, torch NaN.

Kernels (csrc/kernels/attention.h): a flash-style forward that never writes the ``[B,H,T,S]`` matrix and saves only
``o`` and the f32 row normaliser ``lse``; the backward is three launches (delta, dQ by query tile, dK/dV by key
tile) that recompute the probabilities -- no atomics, the same bits on every run.

:func:`supported` mirrors the binding's checks (:func:`limits_ok` is their device-independent part): GPU tensors of
one dtype, f32 or bf16; ``D, Dv <= 128`` and multiples of 8; a contiguous, 16-byte aligned innermost axis with strides that are multiples of 16 bytes; every
tensor below 2^31 elements; ``T, S >= 1``.  f16 / f64 GPU tensors go through f32.  CPU tensors,
``TDL_ATTENTION=torch`` and anything unsupported use :func:`sdpa_torch`, the torch formula in f32 math with the same
zero-row rule, counted in ``CALLS["torch"]``.
"""
from __future__ import annotations

import math
import os

import torch

from . import hip

MAX_HEAD = 128

CALLS = {"forward": 0, "backward": 0, "torch": 0}  # launches of the HIP kernels / torch-formula calls (tests)


def use_torch() -> bool:
    return os.environ.get("TDL_ATTENTION", "") == "torch"


def _operand_ok(t) -> bool:
    """A 4-D tensor below 2^31 elements whose innermost axis is contiguous and whose other strides are multiples of
    16 bytes (whatever its device)."""
    if not (isinstance(t, torch.Tensor) and t.dim() == 4 and 1 <= t.numel() < 1 << 31):
        return False
    per16 = 16 // t.element_size()
    span = sum((n - 1) * s for n, s in zip(t.shape[:3], t.stride()[:3]))
    return t.stride(3) == 1 and span < 1 << 31 and all(s >= 0 and s % per16 == 0 for s in t.stride()[:3])


def limits_ok(q, k, v, mask=None) -> bool:
    """The binding's limits on shapes, dtypes and strides (attn_check in csrc/ops_bindings.cpp) but for f32 / bf16;
    device-independent."""
    if not (_operand_ok(q) and _operand_ok(k) and _operand_ok(v)) or not q.dtype == k.dtype == v.dtype:
        return False
    B, T, H, D = q.shape
    S, Dv = k.shape[1], v.shape[3]
    if k.shape != (B, S, H, D) or v.shape[:3] != (B, S, H) or B > 65535 or H > 65535:
        return False
    if D % 8 or Dv % 8 or not 8 <= min(D, Dv) <= max(D, Dv) <= MAX_HEAD or B * T * H * Dv >= 1 << 31:
        return False
    if mask is not None:
        if not (mask.dtype in (torch.bool, torch.uint8) and tuple(mask.shape) in ((B, T, S), (B, H, T, S))):
            return False
        if min(mask.stride()) < 0 or sum((n - 1) * s for n, s in zip(mask.shape, mask.stride())) >= 1 << 31:
            return False
    return True


def _on_device(q, k, v, mask=None) -> bool:
    return all(t.is_cuda and t.data_ptr() % 16 == 0 for t in (q, k, v)) and (mask is None or mask.is_cuda)


def supported(q, k, v, mask=None) -> bool:
    return (limits_ok(q, k, v, mask) and q.dtype in (torch.float32, torch.bfloat16) and _on_device(q, k, v, mask))


def _u8(mask):
    return mask.view(torch.uint8) if mask is not None and mask.dtype == torch.bool else mask


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, causal, mask):
        CALLS["forward"] += 1
        o, lse = hip().attn_forward(q, k, v, scale, causal, mask)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.args = (scale, causal, mask)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        scale, causal, mask = ctx.args
        CALLS["backward"] += 1
        do = do.to(o.dtype)
        if not (_operand_ok(do) and do.data_ptr() % 16 == 0):
            do = do.contiguous()
            do = do if do.data_ptr() % 16 == 0 else do.clone()
        dq, dk, dv = hip().attn_backward(q, k, v, o, lse, do, scale, causal, mask)
        return dq, dk, dv, None, None, None


def admitted(T, S, causal, mask, device):
    """bool ``[1 or B, 1 or H, T, S]`` of the admitted keys, or None when every key is."""
    adm = None
    if causal:
        adm = (torch.arange(S, device=device)[None, :] <= torch.arange(T, device=device)[:, None])[None, None]
    if mask is not None:
        m = (mask if mask.dim() == 4 else mask[:, None]) != 0
        adm = m if adm is None else adm & m
    return adm


def sdpa_torch(q, k, v, scale=None, causal=False, mask=None, dropout=None, return_scores=False):
    """The same function in differentiable PyTorch ops, f32 math (f64 stays f64), result in q's dtype.  ``dropout``:
    a callable applied to the probabilities (training-time attention dropout)."""
    CALLS["torch"] += 1
    scale = 1.0 / math.sqrt(q.shape[3]) if scale is None else scale
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    s = torch.einsum("bthd,bshd->bhts", q.to(ct), k.to(ct)) * scale
    adm = admitted(q.shape[1], k.shape[1], causal, mask, q.device)
    if adm is not None:
        s = s.masked_fill(~adm, float("-inf"))
        live = adm.any(dim=3, keepdim=True)
        p = torch.softmax(torch.where(live, s, torch.zeros_like(s)), dim=3) * live  # an empty row: p = 0
    else:
        p = torch.softmax(s, dim=3)
    pd = dropout(p) if dropout is not None else p
    o = torch.einsum("bhts,bshe->bthe", pd, v.to(ct)).to(q.dtype)
    return (o, p.to(q.dtype)) if return_scores else o


def sdpa(q, k, v, scale=None, causal=False, mask=None):
    scale = 1.0 / math.sqrt(q.shape[3]) if scale is None else float(scale)
    if q.is_cuda and not use_torch():
        if q.dtype in (torch.float16, torch.float64):
            f = [t.float() for t in (q, k, v)]  # converted once; the limits are those of the f32 copies
            if supported(*f, mask):
                return _Attention.apply(*f, scale, bool(causal), _u8(mask)).to(q.dtype)
        if supported(q, k, v, mask):
            return _Attention.apply(q, k, v, scale, bool(causal), _u8(mask))
    return sdpa_torch(q, k, v, scale, causal, mask)
