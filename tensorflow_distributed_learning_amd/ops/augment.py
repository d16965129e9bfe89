"""Seeded image augmentation: random flip, crop and whole-pixel translation of an NHWC batch as one
coordinate transform per sample (csrc/kernels/augment.hip, augment.h).

Sample ``n`` of the call with ticket ``t`` draws the four Philox words ``philox_words(key, t, 4 n + j)``,
``j = 0..3`` (the stream, the key and the ticket are those of ops/dropout.py):

* ``flip_w = w0 >> 31`` and ``flip_h = w1 >> 31`` where the flip is enabled, else 0;
* ``off_h = off_h_lo + ((w2 * off_h_count) >> 32)`` and likewise ``off_w`` from ``w3``.

Per axis (height shown) output row ``o`` reads ``r = (flip ? Ho - 1 - o : o) + off``; ``r`` in ``[0, H)`` is
the source row, otherwise the fill mode decides: ``constant`` writes ``fill_value`` (rounded once to the
tensor's dtype), ``nearest`` clamps, ``wrap`` takes ``r mod H``, ``reflect`` mirrors edge-inclusively.  The
forward only moves values, so CPU and GPU agree bit for bit; the backward sums, for every input pixel, the
``dy`` of the output pixels that read it in ascending ``(oh, ow)`` order as f32 adds starting from ``+0`` (bf16
rounds once), which pins its bits as well.  Only the ticket is saved for the backward.

:func:`augment_reference` and :func:`augment_backward_reference` are the numpy form: they ARE the CPU
implementation and the oracle of the GPU tests.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import hip
from .dropout import philox_words

FILL_MODES = ("constant", "nearest", "wrap", "reflect")  # the kernels' fill_mode codes, in order


class Spec(NamedTuple):
    """One transform: which flips are drawn, the offset ranges ``[lo, lo + count)``, the output size and what
    pixels from outside the image are."""
    flip_h: bool = False
    flip_w: bool = False
    off_h_lo: int = 0
    off_h_count: int = 1
    off_w_lo: int = 0
    off_w_count: int = 1
    out_h: int = 0
    out_w: int = 0
    fill_mode: str = "constant"
    fill_value: float = 0.0

    def args(self) -> tuple:
        """The positional ``spec`` arguments of the bindings."""
        return (bool(self.flip_h), bool(self.flip_w), int(self.off_h_lo), int(self.off_h_count), int(self.off_w_lo),
                int(self.off_w_count), int(self.out_h), int(self.out_w), FILL_MODES.index(self.fill_mode),
                float(self.fill_value))


def check_spec(spec: Spec, H: int, W: int) -> None:
    """What the kernels assume (the bindings check the same): an output no larger than the input and
    offsets within ``[-size, size]``, so that one wrap or reflection reaches the image."""
    if spec.fill_mode not in FILL_MODES:
        raise ValueError(f"augment: fill_mode must be one of {FILL_MODES}, got {spec.fill_mode!r}")
    if not (1 <= spec.out_h <= H and 1 <= spec.out_w <= W):
        raise ValueError(f"augment: output {spec.out_h} x {spec.out_w} must be within the input {H} x {W}")
    for lo, count, size in ((spec.off_h_lo, spec.off_h_count, H), (spec.off_w_lo, spec.off_w_count, W)):
        if count < 1 or lo < -size or lo + count - 1 > size:
            raise ValueError(f"augment: offsets [{lo}, {lo + count - 1}] must be a non-empty range within "
                             f"[{-size}, {size}]")


# ------------------------------------------------------------------------------------------------ reference
def draws(key: Tuple[int, int], ticket: int, n: int, spec: Spec):
    """``(flip_h, flip_w, off_h, off_w)`` of samples ``0 .. n - 1``: int64 arrays of length ``n``."""
    w = philox_words(key, ticket, np.arange(4 * int(n), dtype=np.uint64)).reshape(int(n), 4)
    s31, s32 = np.uint64(31), np.uint64(32)
    zero = np.zeros(int(n), dtype=np.int64)
    flip_w = (w[:, 0] >> s31).astype(np.int64) if spec.flip_w else zero
    flip_h = (w[:, 1] >> s31).astype(np.int64) if spec.flip_h else zero
    off_h = int(spec.off_h_lo) + ((w[:, 2] * np.uint64(int(spec.off_h_count))) >> s32).astype(np.int64)
    off_w = int(spec.off_w_lo) + ((w[:, 3] * np.uint64(int(spec.off_w_count))) >> s32).astype(np.int64)
    return flip_h, flip_w, off_h, off_w


def _source(flip: np.ndarray, off: np.ndarray, Lo: int, L: int, mode: str) -> np.ndarray:
    """[n, Lo] source coordinates of one axis, -1 where the fill value goes."""
    o = np.arange(Lo, dtype=np.int64)[None, :]
    r = np.where(flip[:, None] != 0, Lo - 1 - o, o) + off[:, None]
    inside = (r >= 0) & (r < L)
    if mode == "constant":
        out = np.full_like(r, -1)
    elif mode == "nearest":
        out = np.clip(r, 0, L - 1)
    elif mode == "wrap":
        out = np.mod(r, L)
    else:
        out = np.where(r < 0, -1 - r, 2 * L - 1 - r)
    return np.where(inside, r, out)


def _maps(key, ticket, n, H, W, spec):
    check_spec(spec, H, W)
    fh, fw, oh, ow = draws(key, ticket, n, spec)
    return _source(fh, oh, spec.out_h, H, spec.fill_mode), _source(fw, ow, spec.out_w, W, spec.fill_mode)


def augment_reference(x: np.ndarray, key: Tuple[int, int], ticket: int, spec: Spec, fill=None) -> np.ndarray:
    """The forward on a numpy NHWC array of any dtype: a pure gather.  ``fill``: the fill element in ``x``'s
    dtype (default ``spec.fill_value`` cast to it)."""
    N, H, W, _ = x.shape
    rh, rw = _maps(key, ticket, N, H, W, spec)
    valid = (rh >= 0)[:, :, None] & (rw >= 0)[:, None, :]
    y = x[np.arange(N)[:, None, None], np.maximum(rh, 0)[:, :, None], np.maximum(rw, 0)[:, None, :]]
    if not valid.all():
        y[~valid] = np.asarray(spec.fill_value, dtype=x.dtype) if fill is None else fill
    return y


def augment_backward_reference(dy: np.ndarray, key: Tuple[int, int], ticket: int, spec: Spec, H: int,
                               W: int) -> np.ndarray:
    """The backward on a float32 numpy array ``[N, Ho, Wo, C]``: ``dx`` starts at +0 and takes the ``dy`` of every
    output pixel at the input pixel it read, in ascending ``(oh, ow)`` order, as f32 adds."""
    dy = np.ascontiguousarray(dy, dtype=np.float32)
    N, Ho, Wo, C = dy.shape
    rh, rw = _maps(key, ticket, N, H, W, spec)
    dx = np.zeros((N, H, W, C), dtype=np.float32)
    ns = np.arange(N)
    if spec.fill_mode in ("constant", "wrap"):
        # no input pixel is read twice (Ho <= H: one o' = i - off mod H per axis), so the order cannot matter
        valid = (rh >= 0)[:, :, None] & (rw >= 0)[:, None, :]
        n_i, h_i, w_i = np.nonzero(valid)
        dx[n_i, rh[n_i, h_i], rw[n_i, w_i]] = np.float32(0) + dy[n_i, h_i, w_i]
        return dx
    for oh in range(Ho):
        for ow in range(Wo):  # one (oh, ow) touches each sample once: a plain fancy-indexed add
            dx[ns, rh[:, oh], rw[:, ow]] += dy[:, oh, ow]
    return dx


# ------------------------------------------------------------------------------------------------ op
def _cpu_forward(x: torch.Tensor, key, ticket: int, spec: Spec) -> torch.Tensor:
    if x.dtype == torch.float64:  # through f32, as on the GPU
        return _cpu_forward(x.float(), key, ticket, spec).double()
    fill = torch.tensor(spec.fill_value, dtype=torch.float64).to(x.dtype)  # rounded once
    if x.dtype == torch.bfloat16:  # numpy has no bf16: move the bits
        y = augment_reference(x.contiguous().view(torch.int16).numpy(), key, ticket, spec,
                              fill=fill.view(torch.int16).numpy())
        return torch.from_numpy(y).view(torch.bfloat16)
    return torch.from_numpy(augment_reference(x.contiguous().numpy(), key, ticket, spec, fill=fill.numpy()))


def _kernel_dtype(dt):
    return dt if dt in (torch.float32, torch.bfloat16) else torch.float32


class _Augment(torch.autograd.Function):
    """``state``: the layer's device tensor ``[calls, arrivals]`` (GPU; the kernel takes and advances the
    ticket) or None with ``ticket`` an int (CPU).  Saves the ticket alone."""

    @staticmethod
    def forward(ctx, x, state, ticket, key, spec):
        ctx.args = (key, spec, int(x.shape[1]), int(x.shape[2]))
        ctx.in_dtype = x.dtype
        if not x.is_cuda:
            ctx.ticket = int(ticket)
            return _cpu_forward(x.detach(), key, ctx.ticket, spec)
        C = hip()
        xc = x.to(_kernel_dtype(x.dtype)).contiguous()
        if x.dtype == torch.float16:  # the f32 kernel fills with the value already rounded to f16
            spec = spec._replace(fill_value=float(torch.tensor(spec.fill_value, dtype=torch.float64).to(x.dtype)))
        y, t = C.augment_fwd(xc, state, key[0], key[1], *spec.args())
        ctx.save_for_backward(t)
        return y if y.dtype == x.dtype else y.to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        key, spec, H, W = ctx.args
        if not dy.is_cuda:
            # f64 goes through f32 as on the GPU; f16 / bf16 are summed in f32 and rounded once
            dx = torch.from_numpy(augment_backward_reference(dy.to(ctx.in_dtype).float().numpy(), key, ctx.ticket,
                                                             spec, H, W))
            return dx.to(ctx.in_dtype), None, None, None, None
        C = hip()
        (t,) = ctx.saved_tensors
        dt = _kernel_dtype(ctx.in_dtype)
        dx = C.augment_bwd(dy.to(dt).contiguous(), t, key[0], key[1], *spec.args(), H, W)
        return (dx if dx.dtype == ctx.in_dtype else dx.to(ctx.in_dtype)), None, None, None, None


def augment(x: torch.Tensor, spec: Spec, key: Tuple[int, int], state: Optional[torch.Tensor] = None,
            ticket: Optional[int] = None) -> torch.Tensor:
    """The NHWC batch ``x`` through the transform ``spec`` drawn from ``(key, ticket)``: ``[N, out_h, out_w, C]``.
    GPU: ``state`` is the int64 device tensor ``[calls, arrivals]`` whose ``calls`` is the ticket and is advanced
    by the kernel; CPU: ``ticket`` is the call number.  f16 and f64 go through the f32 kernel.  Differentiable
    once; works under ``no_grad``."""
    if not x.is_floating_point():
        raise TypeError(f"augment: floating-point input expected, got {x.dtype}")
    if x.dim() != 4:
        raise ValueError(f"augment: a 4-D NHWC input is expected, got {x.dim()} dimensions")
    if x.is_cuda and state is None:
        raise ValueError("augment: a GPU input needs the layer's device state")
    if not x.is_cuda and ticket is None:
        raise ValueError("augment: a CPU input needs a ticket")
    check_spec(spec, int(x.shape[1]), int(x.shape[2]))
    return _Augment.apply(x, state, ticket, (int(key[0]), int(key[1])), spec)
