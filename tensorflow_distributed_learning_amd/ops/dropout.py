"""Seeded dropout: counter-based Philox masks, recomputed in the backward (csrc/kernels/dropout.hip).

The keep mask of one call is a pure function of ``(key, ticket, mask element index)``:

* ``key = stream_key(seed, stream, replica)``: 64 bits, computed on the host;
* ``ticket``: the call number of the layer on its device.  On the GPU it lives in a small device tensor
  ``state = [calls, arrivals]`` that the forward kernel itself advances (no extra launch, no host sync),
  so a replayed hipGraph draws a fresh mask at every replay; on the CPU it is a Python counter;
* Philox4x32-10 over the counter ``(g_lo, g_hi, t_lo, t_hi)``, ``g = (index + elem_offset) >> 2``, yields
  four 32-bit words for four consecutive mask elements; element ``i`` takes word ``(i + elem_offset) & 3``
  and is DROPPED iff ``word < T``, ``T = int(rate * 2**32)``.

Kept elements are ``x * scale`` (one f32 multiply, ``scale = f32(1 / (1 - rate))``), dropped ones exactly
``+0``.  :func:`philox_reference` is the numpy form of the stream: it IS the CPU implementation, so the
CPU and the GPU produce the same bits, and it is the oracle of the tests.  Only the ticket is saved for
the backward: no mask tensor exists.

``TDL_DROPOUT=torch`` sends the layers back to ``torch.nn.functional.dropout`` (global generator, byte
mask), as an escape hatch.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import hip

_M32 = np.uint64(0xFFFFFFFF)
_M64 = (1 << 64) - 1
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85

_GLOBAL_SEED = [None]


def use_torch() -> bool:
    return os.environ.get("TDL_DROPOUT", "") == "torch"


def set_global_seed(seed: Optional[int]) -> None:
    """The seed of every layer created without one (keras.utils.set_random_seed)."""
    _GLOBAL_SEED[0] = None if seed is None else int(seed)


def global_seed() -> int:
    """The global seed; unset, ``torch.initial_seed()`` at first use (and kept from then on)."""
    if _GLOBAL_SEED[0] is None:
        _GLOBAL_SEED[0] = int(torch.initial_seed())
    return _GLOBAL_SEED[0]


# ------------------------------------------------------------------------------------------------ keys
def _splitmix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def stream_key(seed: int, stream: int, replica: int) -> Tuple[int, int]:
    """The 64-bit Philox key ``(k0, k1)`` of one (seed, layer stream, replica): three chained splitmix64
    steps, ``h = mix(seed); h = mix(h + stream); h = mix(h + replica)``; ``k0`` is the low word.  Each
    step is a bijection of its 64-bit input, so for one seed distinct (stream, replica) pairs collide only
    where ``mix(h1 + stream) + replica`` does, and the tests enumerate seed < 8, stream < 64, replica < 8."""
    h = _splitmix64(int(seed) & _M64)
    h = _splitmix64((h + (int(stream) & _M64)) & _M64)
    h = _splitmix64((h + (int(replica) & _M64)) & _M64)
    return h & 0xFFFFFFFF, h >> 32


def threshold(rate: float) -> int:
    """``T = int(rate * 2**32)``: exact, the scaling is a power of two; 2**32 at rate 1 drops everything."""
    return int(float(rate) * 4294967296.0)


def keep_scale(rate: float) -> float:
    """``1 / (1 - rate)`` computed in double and rounded to f32 (at rate 1 nothing is kept: inf, unused)."""
    return float(np.float32(1.0 / (1.0 - float(rate)))) if rate < 1.0 else math.inf


# ------------------------------------------------------------------------------------------------ reference
def philox4x32_10(key: Tuple[int, int], c0, c1, c2, c3) -> Tuple[np.ndarray, ...]:
    """Philox4x32-10 over arrays of counter words (uint64 arrays holding 32-bit values): four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = m0 * c0  # 32 x 32 -> 64 bits: exact in uint64
        p1 = m1 * c2
        n0 = (p1 >> s32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> s32) ^ c3 ^ np.uint64(k1)
        c1 = p1 & _M32
        c3 = p0 & _M32
        c0, c2 = n0, n2
        k0 = (k0 + PHILOX_W0) & 0xFFFFFFFF
        k1 = (k1 + PHILOX_W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def philox_words(key: Tuple[int, int], ticket: int, index: np.ndarray) -> np.ndarray:
    """The 32-bit word of every (offset) mask index in ``index`` (uint64 array)."""
    index = np.asarray(index, dtype=np.uint64)
    if index.size == 0:
        return np.zeros(index.shape, dtype=np.uint64)
    g = index >> np.uint64(2)
    g0, g1 = int(g.min()), int(g.max())
    if g1 - g0 + 1 <= 2 * index.size:  # a dense range (the usual arange): no sort
        ug = np.arange(g0, g1 + 1, dtype=np.uint64)
        inv = (g - np.uint64(g0)).astype(np.int64)
    else:
        ug, inv = np.unique(g, return_inverse=True)
    t = int(ticket) & _M64
    w = philox4x32_10(key, ug & _M32, ug >> np.uint64(32), np.full(ug.shape, t & 0xFFFFFFFF, dtype=np.uint64),
                      np.full(ug.shape, t >> 32, dtype=np.uint64))
    words = np.stack(w, axis=-1)  # [groups, 4]
    return words[inv.reshape(-1), (index & np.uint64(3)).astype(np.int64).reshape(-1)].reshape(index.shape)


def philox_reference(key: Tuple[int, int], ticket: int, n: int, T: int, elem_offset: int = 0,
                     noise_shape: Optional[Sequence[int]] = None) -> np.ndarray:
    """The KEEP mask (bool) of mask elements ``0 .. n - 1`` for this key and ticket: element ``i`` is kept
    iff its word is ``>= T``.  With ``noise_shape`` the mask is returned in that shape (``n`` is then its
    element count and may be None); it broadcasts against the input as Keras' ``noise_shape`` does."""
    if noise_shape is not None:
        count = int(np.prod([int(d) for d in noise_shape], dtype=np.int64)) if len(noise_shape) else 1
        if n is not None and int(n) != count:
            raise ValueError(f"philox_reference: n = {n} is not the size of noise_shape {tuple(noise_shape)}")
        n = count
    idx = np.arange(int(n), dtype=np.uint64) + np.uint64(int(elem_offset))
    keep = philox_words(key, ticket, idx) >= np.uint64(int(T))
    return keep.reshape(tuple(int(d) for d in noise_shape)) if noise_shape is not None else keep


# ------------------------------------------------------------------------------------------------ op
def _noise_strides(noise_shape: Sequence[int]) -> list:
    out, run = [], 1
    for d in reversed(noise_shape):
        out.append(0 if d == 1 else run)
        run *= int(d)
    return out[::-1]


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _cpu_apply(x: torch.Tensor, key, ticket: int, T: int, scale: float, noise_shape, elem_offset: int):
    shape = tuple(noise_shape) if noise_shape is not None else tuple(x.shape)
    keep = torch.from_numpy(philox_reference(key, ticket, None, T, elem_offset, shape))
    y = (x.to(torch.float32) * torch.tensor(scale, dtype=torch.float32)).to(x.dtype)
    return torch.where(keep, y, torch.zeros((), dtype=x.dtype))


class _Dropout(torch.autograd.Function):
    """``state``: the layer's device tensor ``[calls, arrivals]`` (GPU; the kernel takes and advances the
    ticket) or None with ``ticket`` an int (CPU).  Saves the ticket alone."""

    @staticmethod
    def forward(ctx, x, state, ticket, key, T, scale, noise_shape, elem_offset):
        ctx.args = (key, T, scale, noise_shape, elem_offset)
        ctx.in_dtype = x.dtype
        if not x.is_cuda:
            ctx.ticket = int(ticket)
            return _cpu_apply(x, key, ctx.ticket, T, scale, noise_shape, elem_offset)
        C = hip()
        xc = x if x.dtype in (torch.float32, torch.bfloat16) else x.to(torch.float32)
        ns = _noise_strides(noise_shape) if noise_shape is not None else None
        y, t = C.dropout_fwd(_aligned(xc), state, key[0], key[1], T, scale, ns, elem_offset)
        ctx.save_for_backward(t)
        return y if y.dtype == x.dtype else y.to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        key, T, scale, noise_shape, elem_offset = ctx.args
        if not dy.is_cuda:
            dx = _cpu_apply(dy.to(ctx.in_dtype), key, ctx.ticket, T, scale, noise_shape, elem_offset)
            return dx, None, None, None, None, None, None, None
        C = hip()
        (t,) = ctx.saved_tensors
        dt = ctx.in_dtype if ctx.in_dtype in (torch.float32, torch.bfloat16) else torch.float32
        ns = _noise_strides(noise_shape) if noise_shape is not None else None
        dx = C.dropout_bwd(_aligned(dy.to(dt)), t, key[0], key[1], T, scale, ns, elem_offset)
        return (dx if dx.dtype == ctx.in_dtype else dx.to(ctx.in_dtype)), None, None, None, None, None, None, None


def dropout(x: torch.Tensor, rate: float, key: Tuple[int, int], state: Optional[torch.Tensor] = None,
            ticket: Optional[int] = None, noise_shape: Optional[Sequence[int]] = None, elem_offset: int = 0):
    """``x`` with elements dropped at ``rate`` by the mask of ``(key, ticket)`` and the rest scaled by
    ``1 / (1 - rate)``.  GPU: ``state`` is the int64 device tensor ``[calls, arrivals]`` whose ``calls`` is the
    ticket and is advanced by the kernel; CPU: ``ticket`` is the call number.  ``noise_shape``: the mask's
    shape (entries equal to ``x``'s or 1), None = ``x``'s shape.  Differentiable once; works under
    ``no_grad``."""
    if not x.is_floating_point():
        raise TypeError(f"dropout: floating-point input expected, got {x.dtype}")
    if x.is_cuda and state is None:
        raise ValueError("dropout: a GPU input needs the layer's device state")
    if not x.is_cuda and ticket is None:
        raise ValueError("dropout: a CPU input needs a ticket")
    if noise_shape is not None:
        noise_shape = tuple(int(d) for d in noise_shape)
        if len(noise_shape) != x.dim() or any(d != 1 and d != s for d, s in zip(noise_shape, x.shape)):
            raise ValueError(f"dropout: noise_shape {noise_shape} does not broadcast to {tuple(x.shape)}")
        if noise_shape == tuple(x.shape):
            noise_shape = None
    return _Dropout.apply(x, state, ticket, (int(key[0]), int(key[1])), threshold(rate), keep_scale(rate),
                          noise_shape, int(elem_offset))
