"""Scaled-dot-product attention on the fused MFMA kernels of csrc/kernels/attention.hip.

``sdpa(q, k, v, scale=None, causal=False, mask=None, rate=0.0, key=None, state=None, ticket=None)``: ``q [B,T,H,D]``, ``k [B,S,H,D]``, ``v [B,S,H,Dv]`` (f32 or
bf16, any strides on the first three axes: projection outputs and slices of a packed qkv buffer are consumed as
views, no permute or copy is launched) give ``o [B,T,H,Dv]``::

    o[b,i,h] = sum_j softmax_j(scale q[b,i,h] . k[b,j,h]) v[b,j,h]       over the admitted keys j of row i

Key ``j`` is admitted iff ``j < S``, (not ``causal`` or ``j <= i``: Keras' lower-triangular mask, also for
``T != S``) and (no ``mask`` or ``mask[b,(h),i,j] != 0``; a bool / uint8 ``[B,T,S]`` or ``[B,H,T,S]``).  A row without
an admitted key gives ``o = 0`` and zero gradients, never NaN -- Keras gives the mean of ``v`` there, torch NaN.

Kernels (csrc/kernels/attention.h): a flash-style forward that never writes the ``[B,H,T,S]`` matrix and saves only
``o`` and the f32 row normaliser ``lse``; the backward is three launches (delta, dQ by query tile, dK/dV by key
tile) that recompute the probabilities -- no atomics, the same bits on every run.  With ``rate > 0`` the tile kernels
drop probabilities by the seeded Philox stream of ops/dropout.py (``o = (c z P) V``, ``lse`` of the undropped row; the
mask is recomputed in the backward from the saved ticket), and :func:`philox_dropout` draws the same mask for the formula.

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
    """``rate > 0``: the forward kernel takes the ticket from ``state`` and advances it; the ticket tensor is saved
    beside ``o`` and ``lse`` and the backward kernels recompute the mask from it."""

    @staticmethod
    def forward(ctx, q, k, v, scale, causal, mask, rate=0.0, key=None, state=None):
        CALLS["forward"] += 1
        if rate > 0:
            o, lse, ticket = hip().attn_forward(q, k, v, scale, causal, mask, rate, key, state)
            ctx.save_for_backward(q, k, v, o, lse, ticket)
        else:
            o, lse = hip().attn_forward(q, k, v, scale, causal, mask)
            ctx.save_for_backward(q, k, v, o, lse)
        ctx.args = (scale, causal, mask, rate, key)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, *ticket = ctx.saved_tensors
        scale, causal, mask, rate, key = ctx.args
        CALLS["backward"] += 1
        do = do.to(o.dtype)
        if not (_operand_ok(do) and do.data_ptr() % 16 == 0):
            do = do.contiguous()
            do = do if do.data_ptr() % 16 == 0 else do.clone()
        if rate > 0:
            dq, dk, dv = hip().attn_backward(q, k, v, o, lse, do, scale, causal, mask, rate, key, ticket[0])
        else:
            dq, dk, dv = hip().attn_backward(q, k, v, o, lse, do, scale, causal, mask)
        return dq, dk, dv, None, None, None, None, None, None


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


def philox_dropout(rate, key, state=None, ticket=None):
    """The kernels' attention dropout as ``sdpa_torch``'s ``dropout`` callable, on any device: ``p [B,H,T,S]`` is
    padded to ``4 ceil(T / 4)`` rows and laid out as ``[B H, ceil(T / 4), S, 4]``, whose linear index is the kernels'
    mask index (csrc/kernels/attention.h), and goes through :func:`ops.dropout.dropout` with a full-shape mask:
    ``state`` on the GPU, ``ticket`` on the CPU, one ticket per call and the kernels' mask bit for bit."""
    from . import dropout as _do

    def apply(p):
        B, H, T, S = p.shape
        T4 = -(-T // 4)
        x = torch.nn.functional.pad(p, (0, 0, 0, 4 * T4 - T)).reshape(B * H, T4, 4, S).permute(0, 1, 3, 2).contiguous()
        y = _do.dropout(x, rate, key, state=state if p.is_cuda else None, ticket=None if p.is_cuda else ticket)
        return y.permute(0, 1, 3, 2).reshape(B, H, 4 * T4, S)[:, :, :T]

    return apply


def sdpa(q, k, v, scale=None, causal=False, mask=None, rate=0.0, key=None, state=None, ticket=None):
    """``rate > 0``: seeded dropout on the probabilities with the Philox ``key`` (``ops.dropout.stream_key``) and the
    layer's call counter: the int64 ``state = [calls, arrivals]`` tensor of a GPU input's device, which the forward
    kernel (or, on the formula path, the dropout kernel) advances, or the ``ticket`` number of a CPU input."""
    scale = 1.0 / math.sqrt(q.shape[3]) if scale is None else float(scale)
    rate = float(rate)
    if not 0.0 <= rate < 1.0:
        raise ValueError(f"sdpa: the dropout rate must be in [0, 1), got {rate!r}")
    drop = (0.0, None, None)
    if rate > 0:
        if key is None or (state is None if q.is_cuda else ticket is None):
            raise ValueError("sdpa: dropout needs a key and the device state (GPU) or a ticket (CPU)")
        key = (int(key[0]), int(key[1]))
        drop = (rate, key, state)
    if q.is_cuda and not use_torch():
        if q.dtype in (torch.float16, torch.float64):
            f = [t.float() for t in (q, k, v)]  # converted once; the limits are those of the f32 copies
            if supported(*f, mask):
                return _Attention.apply(*f, scale, bool(causal), _u8(mask), *drop).to(q.dtype)
        if supported(q, k, v, mask):
            return _Attention.apply(q, k, v, scale, bool(causal), _u8(mask), *drop)
    return sdpa_torch(q, k, v, scale, causal, mask,
                      dropout=philox_dropout(rate, key, state, ticket) if rate > 0 else None)
