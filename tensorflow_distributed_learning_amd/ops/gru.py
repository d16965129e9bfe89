"""The GRU recurrence on the hand-written scan kernels (csrc/kernels/gru.hip).

``gru_scan(zx, R, b_rec, h0, go_backwards)`` runs the sequential part of a Keras GRU (``reset_after=True``: also
cuDNN's and ``torch.nn.GRU``'s formula) over the projected input ``zx = x W + b_in`` of shape ``[B, T, 3U]`` (gate
columns ``z, r, h``) with the recurrent kernel ``R [U, 3U]`` and the recurrent bias ``b_rec [3U]``::

    mh = h_{t-1} R + b_rec;  z = sigmoid(zx_z + mh_z);  r = sigmoid(zx_r + mh_r);  hh = tanh(zx_h + r mh_h)
    h_t = z h_{t-1} + (1 - z) hh

and returns ``(hs [B, T, U], h_last)``, the sequence in processing order (``go_backwards``: reversed time).

Kernels (csrc/kernels/gru.h): one workgroup per 16 batch rows holds ``h`` in registers and LDS for all ``T`` steps,
one MFMA recurrence per step; the backward is the reverse scan and returns ``dzx`` (what autograd hands to the
projection) and ``dzh``, the gradient of ``mh``.  ``dR = sum_s h_{s-1}^T dzh_s`` is one weight-gradient GEMM over
the time-shifted pair (outside the sequential path), on the GEMMs Dense's backward uses, added into ``r_target``
(``Variable.grad_target``) when given; ``db_rec`` is the column sum of ``dzh`` (a fixed-order f64 kernel), added into
``b_target`` when given.  bf16: ``R`` and every stored ``h_t`` are rounded to bf16; ``b_rec`` and the gate math are f32.

:func:`supported`: a non-empty CUDA ``zx``, f32 or bf16, ``U % 16 == 0``, ``U <= MAX_U``, fewer than 2^31 elements
(of the ``[B, T, 4U]`` tensor saved for the backward).  On such a tensor the kernels are the only path
(:func:`..ops.hip` raises if the extension is not built); f16 / f64 GPU tensors go through f32; CPU tensors, other
shapes, other activations and ``reset_after=False`` (whose kernel would need a second dependent MFMA phase per step)
use :func:`gru_torch` (counted in ``FALLBACKS`` on the GPU).  ``TDL_GRU=torch`` forces the formula on the GPU as well.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import hip
from .lstm import _aligned

MAX_U = 256

CALLS = [0]  # forward calls that ran the HIP kernels (tests)
CALLS_BY_DTYPE = {torch.float32: 0, torch.bfloat16: 0}
FALLBACKS = [0]  # GPU calls that took the PyTorch formula without TDL_GRU=torch asking for it


def use_torch() -> bool:
    return os.environ.get("TDL_GRU", "") == "torch"


def _shape_ok(zx: torch.Tensor) -> bool:
    if not (zx.is_cuda and zx.dim() == 3 and zx.numel() > 0 and zx.shape[2] % 3 == 0):
        return False
    U = zx.shape[2] // 3
    return U % 16 == 0 and U <= MAX_U and zx.numel() // 3 * 4 < 2 ** 31


def supported(zx: torch.Tensor) -> bool:
    return _shape_ok(zx) and zx.dtype in (torch.float32, torch.bfloat16)


def _recurrent_grad(hs, h0, dzh, rev, target):
    """``sum_s hprev_s^T dzh_s`` over the processing steps as one GEMM: f32 ``[U, 3U]``, added into ``target`` when
    given.  None when there is nothing to add (T = 1 without an initial state and a target)."""
    K = hip()
    B, T, U = hs.shape
    dzp = dzh.flip(1) if rev else dzh  # processing order
    if h0 is not None:
        a, b = torch.cat([h0.unsqueeze(1), hs[:, :-1]], 1), dzp
    else:
        a, b = hs[:, :-1], dzp[:, 1:]
    rows = a.shape[0] * a.shape[1]
    if rows == 0:
        return None if target is not None else torch.zeros(U, 3 * U, dtype=torch.float32, device=hs.device)
    a, b = a.reshape(rows, U), b.reshape(rows, 3 * U)
    if hs.dtype == torch.float32:
        a, b = _aligned(a), _aligned(b)
        if target is not None:
            return K.gemm_f32(a, 1, b, 1, out=target, accumulate=True)
        return K.gemm_f32(a, 1, b, 1)
    pad = -rows % 8  # (the bf16 GEMM takes multiples of 8: rows of zeros add nothing)
    if pad:
        a, b = torch.cat([a, a.new_zeros(pad, U)]), torch.cat([b, b.new_zeros(pad, 3 * U)])
    a, b = _aligned(a), _aligned(b)
    if target is not None:
        return K.gemm_bf16(a, 1, b, 1, out=target, accumulate=True)
    return K.gemm_bf16(a, 1, b, 1, out=torch.empty(U, 3 * U, dtype=torch.float32, device=hs.device))


class _GruScan(torch.autograd.Function):
    @staticmethod
    def forward(ctx, zx, R, b_rec, h0, rev, r_target, b_target):
        K = hip()
        zc = zx.contiguous()
        Rc = _aligned(R.detach().to(zc.dtype))
        bc = b_rec.detach().float().contiguous() if b_rec is not None else None
        h0c = h0.detach().to(zc.dtype).contiguous() if h0 is not None else None
        save = any(ctx.needs_input_grad[:4]) or r_target is not None or b_target is not None
        hs, h_last, saved = K.gru_forward(zc, Rc, bc, h0c, bool(rev), save)
        CALLS[0] += 1
        CALLS_BY_DTYPE[zc.dtype] += 1
        ctx.set_materialize_grads(False)
        ctx.rev, ctx.r_target, ctx.b_target = bool(rev), r_target, b_target
        ctx.has_h0 = h0 is not None
        ctx.dtypes = (R.dtype, b_rec.dtype if b_rec is not None else None, h0.dtype if h0 is not None else None)
        if save:
            ctx.save_for_backward(hs, saved, Rc, h0c if h0c is not None else hs.new_empty(0))
        return hs, h_last

    @staticmethod
    def backward(ctx, dhs, dh_last):
        K = hip()
        hs, saved, Rc, h0c = ctx.saved_tensors
        h0c = h0c if ctx.has_h0 else None
        dhs = dhs.to(hs.dtype).contiguous() if dhs is not None else None
        dh_last = dh_last.to(hs.dtype).contiguous() if dh_last is not None else None
        dzx, dzh, dh0 = K.gru_backward(saved, hs, Rc, h0c, dhs, dh_last, ctx.rev, ctx.has_h0)
        dR = db = None
        if ctx.r_target is not None:
            _recurrent_grad(hs, h0c, dzh, ctx.rev, ctx.r_target)
        elif ctx.needs_input_grad[1]:
            dR = _recurrent_grad(hs, h0c, dzh, ctx.rev, None).to(ctx.dtypes[0])
        if ctx.b_target is not None:
            K.gru_bias_grad(dzh, ctx.b_target)
        elif ctx.needs_input_grad[2]:
            db = K.gru_bias_grad(dzh).to(ctx.dtypes[1])
        return (dzx, dR, db, dh0.to(ctx.dtypes[2]) if ctx.has_h0 and ctx.needs_input_grad[3] else None, None, None,
                None)


def gru_torch(zx: torch.Tensor, R: torch.Tensor, b_rec: Optional[torch.Tensor] = None,
              h0: Optional[torch.Tensor] = None, go_backwards: bool = False, activation=torch.tanh,
              recurrent_activation=torch.sigmoid, reset_after: bool = True):
    """The same recurrence in differentiable PyTorch ops: f32 arithmetic for f16 / bf16 data (``R`` and every ``h_t``
    rounded to the data's dtype, as the bf16 kernels do), the input's own for f32 / f64.  ``reset_after=False``:
    ``hh = tanh(zx_h + (r h_{t-1}) R_h)``, without a recurrent bias.  Returns ``(hs, h_last)``."""
    B, T, U = zx.shape[0], zx.shape[1], zx.shape[2] // 3
    low = zx.dtype not in (torch.float32, torch.float64)
    ct = torch.float32 if low else zx.dtype

    def op(t):  # an operand the low-precision kernels round
        return t.to(zx.dtype).to(ct)

    Rc, mx = op(R), zx.to(ct)
    b = b_rec.to(ct) if b_rec is not None and reset_after else None
    h = op(h0) if h0 is not None else mx.new_zeros(B, U)
    hs = []
    for s in range(T):
        m = mx[:, T - 1 - s if go_backwards else s]
        if reset_after:
            mh = h @ Rc if b is None else h @ Rc + b
            z = recurrent_activation(m[:, :U] + mh[:, :U])
            r = recurrent_activation(m[:, U:2 * U] + mh[:, U:2 * U])
            hh = activation(m[:, 2 * U:] + r * mh[:, 2 * U:])
        else:
            mh = h @ Rc[:, :2 * U]
            z = recurrent_activation(m[:, :U] + mh[:, :U])
            r = recurrent_activation(m[:, U:2 * U] + mh[:, U:])
            hh = activation(m[:, 2 * U:] + (r * h) @ Rc[:, 2 * U:])
        h = z * h + (1 - z) * hh
        if low:
            h = op(h)
        hs.append(h)
    hs = torch.stack(hs, 1).to(zx.dtype)
    return hs, hs[:, -1]


def gru_scan(zx: torch.Tensor, R: torch.Tensor, b_rec: Optional[torch.Tensor] = None,
             h0: Optional[torch.Tensor] = None, go_backwards: bool = False, r_target: Optional[torch.Tensor] = None,
             b_target: Optional[torch.Tensor] = None, activation=torch.tanh, recurrent_activation=torch.sigmoid,
             reset_after: bool = True, standard: bool = True):
    """``zx [B, T, 3U]``, ``R [U, 3U]`` (any float dtype: cast to the data's), ``b_rec [3U]`` or None (``reset_after``
    only), ``h0 [B, U]`` or None.  Returns ``(hs, h_last)``.

    ``r_target`` / ``b_target``: the f32 slab views the GPU backward ADDS ``dR`` / ``db_rec`` into
    (``Variable.grad_target``, the bias variable's second row); ``R`` / ``b_rec`` are then passed without autograd.
    ``standard=False``: activations other than tanh / sigmoid (the formula)."""
    if zx.is_cuda and not use_torch() and zx.shape[1] > 0:
        if standard and reset_after:
            if zx.dtype in (torch.float16, torch.float64) and _shape_ok(zx):
                hs, hl = gru_scan(zx.float(), R, b_rec, h0, go_backwards)
                return hs.to(zx.dtype), hl.to(zx.dtype)
            if supported(zx):
                if not (zx.requires_grad and torch.is_grad_enabled()):
                    r_target = b_target = None  # (no backward would reach the kernels that fill the targets through zx)
                if b_rec is None:
                    b_target = None
                return _GruScan.apply(zx, R.detach() if r_target is not None else R,
                                      b_rec.detach() if b_target is not None else b_rec, h0, go_backwards, r_target,
                                      b_target)
        if zx.numel() > 0:
            FALLBACKS[0] += 1
    return gru_torch(zx, R, b_rec, h0, go_backwards, activation, recurrent_activation, reset_after)
