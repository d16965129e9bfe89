"""The LSTM recurrence on the hand-written scan kernels (csrc/kernels/lstm.hip).

``lstm_scan(zx, R, h0, c0, go_backwards)`` runs the sequential part of a Keras LSTM over the projected input
``zx = x W + b`` of shape ``[B, T, 4U]`` (gate columns ``i, f, c, o``) with the recurrent kernel ``R [U, 4U]``::

    z_t = zx_t + h_{t-1} R;  i, f, o = sigmoid(z_i), sigmoid(z_f), sigmoid(z_o);  g = tanh(z_c)
    c_t = f c_{t-1} + i g;   h_t = o tanh(c_t)

and returns ``(hs [B, T, U], h_last, c_last)``, the sequence in processing order (``go_backwards``: reversed time).

Kernels (csrc/kernels/lstm.h): one workgroup per 16 batch rows holds ``c`` in registers and ``h`` in LDS for all
``T`` steps, one MFMA recurrence per step; the backward is the reverse scan and returns ``dzx`` (what autograd hands
to the projection).  ``dR = sum_t h_{t-1}^T dz_t`` is one weight-gradient GEMM over the time-shifted pair
``(hs[:, :-1], dz[:, 1:])`` (two contiguous copies, outside the sequential path), on the GEMMs Dense's backward uses,
added into ``r_target`` (``Variable.grad_target``) when given.  bf16: ``R`` and every stored ``h_t`` are rounded to
bf16; ``c`` and the gate math are f32.

:func:`supported`: a non-empty CUDA ``zx``, f32 or bf16, ``U % 16 == 0``, ``U <= MAX_U``, fewer than 2^31 elements.
On such a tensor the kernels are the only path (:func:`..ops.hip` raises if the extension is not built); f16 / f64 GPU
tensors go through f32; CPU tensors, other shapes and other activations use :func:`lstm_torch` (counted in
``FALLBACKS`` on the GPU).  ``TDL_LSTM=torch`` forces the formula on the GPU as well.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import hip

MAX_U = 256

CALLS = [0]  # forward calls that ran the HIP kernels (tests)
CALLS_BY_DTYPE = {torch.float32: 0, torch.bfloat16: 0}
FALLBACKS = [0]  # GPU calls that took the PyTorch formula without TDL_LSTM=torch asking for it


def use_torch() -> bool:
    return os.environ.get("TDL_LSTM", "") == "torch"


def _shape_ok(zx: torch.Tensor) -> bool:
    if not (zx.is_cuda and zx.dim() == 3 and zx.numel() > 0 and zx.shape[2] % 4 == 0):
        return False
    U = zx.shape[2] // 4
    return U % 16 == 0 and U <= MAX_U and zx.numel() < 2 ** 31


def supported(zx: torch.Tensor) -> bool:
    return _shape_ok(zx) and zx.dtype in (torch.float32, torch.bfloat16)


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _recurrent_grad(hs, h0, dz, rev, target):
    """``sum_s hprev_s^T dz_s`` over the processing steps as one GEMM: f32 ``[U, 4U]``, added into ``target`` when
    given.  None when there is nothing to add (T = 1 without an initial state and a target)."""
    K = hip()
    B, T, U = hs.shape
    dzp = dz.flip(1) if rev else dz  # processing order
    if h0 is not None:
        a, b = torch.cat([h0.unsqueeze(1), hs[:, :-1]], 1), dzp
    else:
        a, b = hs[:, :-1], dzp[:, 1:]
    rows = a.shape[0] * a.shape[1]
    if rows == 0:
        return None if target is not None else torch.zeros(U, 4 * U, dtype=torch.float32, device=hs.device)
    a, b = a.reshape(rows, U), b.reshape(rows, 4 * U)
    if hs.dtype == torch.float32:
        a, b = _aligned(a), _aligned(b)
        if target is not None:
            return K.gemm_f32(a, 1, b, 1, out=target, accumulate=True)
        return K.gemm_f32(a, 1, b, 1)
    pad = -rows % 8  # (the bf16 GEMM takes multiples of 8: rows of zeros add nothing)
    if pad:
        a, b = torch.cat([a, a.new_zeros(pad, U)]), torch.cat([b, b.new_zeros(pad, 4 * U)])
    a, b = _aligned(a), _aligned(b)
    if target is not None:
        return K.gemm_bf16(a, 1, b, 1, out=target, accumulate=True)
    return K.gemm_bf16(a, 1, b, 1, out=torch.empty(U, 4 * U, dtype=torch.float32, device=hs.device))


class _LstmScan(torch.autograd.Function):
    @staticmethod
    def forward(ctx, zx, R, h0, c0, rev, r_target):
        K = hip()
        zc = zx.contiguous()
        Rc = _aligned(R.detach().to(zc.dtype))
        h0c = h0.detach().to(zc.dtype).contiguous() if h0 is not None else None
        c0c = c0.detach().float().contiguous() if c0 is not None else None
        save = any(ctx.needs_input_grad[:4]) or r_target is not None
        hs, h_last, c_last, gates, cs = K.lstm_forward(zc, Rc, h0c, c0c, bool(rev), save)
        CALLS[0] += 1
        CALLS_BY_DTYPE[zc.dtype] += 1
        ctx.set_materialize_grads(False)
        ctx.rev, ctx.r_target = bool(rev), r_target
        ctx.state = (h0 is not None, c0 is not None)
        ctx.dtypes = (R.dtype, h0.dtype if h0 is not None else None, c0.dtype if c0 is not None else None)
        if save:
            none = hs.new_empty(0)
            ctx.save_for_backward(hs, gates, cs, Rc, h0c if h0c is not None else none, c0c if c0c is not None else none)
        return hs, h_last, c_last

    @staticmethod
    def backward(ctx, dhs, dh_last, dc_last):
        K = hip()
        hs, gates, cs, Rc, h0c, c0c = ctx.saved_tensors
        has_h0, has_c0 = ctx.state
        h0c, c0c = (h0c if has_h0 else None), (c0c if has_c0 else None)
        dhs = dhs.to(hs.dtype).contiguous() if dhs is not None else None
        dh_last = dh_last.to(hs.dtype).contiguous() if dh_last is not None else None
        dc_last = dc_last.float().contiguous() if dc_last is not None else None
        want_state = has_h0 or has_c0
        dz, dh0, dc0 = K.lstm_backward(gates, cs, Rc, c0c, dhs, dh_last, dc_last, ctx.rev, want_state)
        dR = None
        if ctx.r_target is not None:
            _recurrent_grad(hs, h0c, dz, ctx.rev, ctx.r_target)
        elif ctx.needs_input_grad[1]:
            dR = _recurrent_grad(hs, h0c, dz, ctx.rev, None).to(ctx.dtypes[0])
        return (dz, dR, dh0.to(ctx.dtypes[1]) if has_h0 and ctx.needs_input_grad[2] else None,
                dc0.to(ctx.dtypes[2]) if has_c0 and ctx.needs_input_grad[3] else None, None, None)


def lstm_torch(zx: torch.Tensor, R: torch.Tensor, h0: Optional[torch.Tensor] = None,
               c0: Optional[torch.Tensor] = None, go_backwards: bool = False, activation=torch.tanh,
               recurrent_activation=torch.sigmoid):
    """The same recurrence in differentiable PyTorch ops: f32 arithmetic for f16 / bf16 data (``R`` and every
    ``h_t`` rounded to the data's dtype, as the bf16 kernels do), the input's own for f32 / f64.  Returns
    ``(hs, h_last, c_last)``, ``c_last`` in the arithmetic's dtype."""
    B, T, U = zx.shape[0], zx.shape[1], zx.shape[2] // 4
    low = zx.dtype not in (torch.float32, torch.float64)
    ct = torch.float32 if low else zx.dtype

    def op(t):  # an operand the low-precision kernels round
        return t.to(zx.dtype).to(ct)

    Rc, z = op(R), zx.to(ct)
    h = op(h0) if h0 is not None else z.new_zeros(B, U)
    c = c0.to(ct) if c0 is not None else z.new_zeros(B, U)
    hs = []
    for s in range(T):
        a = z[:, T - 1 - s if go_backwards else s] + h @ Rc
        i, f, g, o = a.split(U, dim=1)
        c = recurrent_activation(f) * c + recurrent_activation(i) * activation(g)
        h = recurrent_activation(o) * activation(c)
        if low:
            h = op(h)
        hs.append(h)
    hs = torch.stack(hs, 1).to(zx.dtype)
    return hs, hs[:, -1], c


def lstm_scan(zx: torch.Tensor, R: torch.Tensor, h0: Optional[torch.Tensor] = None, c0: Optional[torch.Tensor] = None,
              go_backwards: bool = False, r_target: Optional[torch.Tensor] = None, activation=torch.tanh,
              recurrent_activation=torch.sigmoid, standard: bool = True):
    """``zx [B, T, 4U]``, ``R [U, 4U]`` (any float dtype: cast to the data's), ``h0`` / ``c0 [B, U]`` or None.
    Returns ``(hs, h_last, c_last)``; ``c_last`` is f32 for bf16 data.

    ``r_target``: the f32 slab view the GPU backward ADDS ``dR`` into (``Variable.grad_target``); ``R`` is then passed
    without autograd.  ``standard=False``: activations other than tanh / sigmoid (the formula)."""
    if zx.is_cuda and standard and not use_torch() and zx.shape[1] > 0:
        if zx.dtype in (torch.float16, torch.float64) and _shape_ok(zx):
            hs, hl, cl = lstm_scan(zx.float(), R, h0, c0, go_backwards, None)
            return hs.to(zx.dtype), hl.to(zx.dtype), cl.to(zx.dtype)
        if supported(zx):
            if not (r_target is not None and zx.requires_grad and torch.is_grad_enabled()):
                r_target = None  # (no backward would reach the GEMM that fills the target through zx)
            return _LstmScan.apply(zx, R.detach() if r_target is not None else R, h0, c0, go_backwards, r_target)
        if zx.numel() > 0:
            FALLBACKS[0] += 1
    return lstm_torch(zx, R, h0, c0, go_backwards, activation, recurrent_activation)
