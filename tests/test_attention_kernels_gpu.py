"""The fused attention kernels (csrc/kernels/attention.hip) through the bindings against tests/attention_refs.py, on
operands that are 16-byte aligned views into NaN-filled buffers (a read outside an operand poisons a result)."""
import numpy as np
import pytest
import torch

from tensorflow_distributed_learning_amd.ops import attention as A
from tensorflow_distributed_learning_amd.ops import hip as _C

import attention_refs as AR

pytestmark = pytest.mark.gpu


def _dev(vals, dtype):
    """vals as a 16-byte-aligned view with 16 NaN elements in front of and behind it."""
    vals = np.ascontiguousarray(vals)
    fill = float("nan") if dtype.is_floating_point else 255
    buf = torch.full((vals.size + 32,), fill, dtype=dtype, device="cuda")
    v = buf[16:16 + vals.size].view(vals.shape)
    v.copy_(torch.from_numpy(vals).to(dtype))
    assert v.data_ptr() % 16 == 0
    return v


def _np(t):
    return t.detach().double().cpu().numpy()


def _check(name, got, ref, tol):
    err = np.abs(_np(got) - ref)
    ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f"[attention kernels] {name}: worst error / bound {ratio.max():.3g} (error {err.max():.3g})")
    assert np.isfinite(err).all() and (err <= tol).all(), f"{name}: {int((~(err <= tol)).sum())} elements off"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", AR.CASES, ids=AR.IDS)
def test_kernels_against_f64(case, dtype):
    Ck = _C()
    (B, H, T, S, D, Dv), causal, kind, layout = case
    bf16 = dtype == torch.bfloat16
    (q, k, v, do), mask, scale = AR.inputs(case, bf16)
    if layout == "packed":  # what supported() refuses, the binding's own checks raise for: a base off 16 bytes
        bad = torch.zeros(B * T * H * D + 2, dtype=dtype, device="cuda")[2:].view(B, T, H, D)
        assert not A.supported(bad, bad, bad) and A.supported(bad.clone(), bad.clone(), bad.clone())
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            Ck.attn_forward(bad, bad, bad, scale, causal)
    adm = AR.admitted(B, H, T, S, causal, mask)
    empty = ~adm.any(axis=3)  # [B,H,T]

    # the plan shows that the case hits what it is there for
    plan = Ck.attn_plan(B, H, T, S, D, Dv, bf16, causal)
    assert plan["q_tiles"] == -(-T // 64) and plan["k_tiles"] == -(-S // 64)
    assert (plan["causal_skipped"] > 0) == (causal and S > 64)
    if D == 128:
        assert plan["head_pad"] == 128 and plan["lds_dkv"] == (155136 if not bf16 else 81408) <= 160 * 1024
    assert kind is None or (empty.any() and not adm[..., 64:].any())
    if layout == "steep":
        s = scale * np.einsum("bthd,bshd->bhts", q.astype(np.float64), k.astype(np.float64))
        assert s.max() > 95 and s.min() < -95 and plan["k_tiles"] == 3
        assert (np.diff(s.reshape(B, H, T, 3, 64).max(axis=4), axis=3) > 0).all()

    if layout == "packed":
        buf = _dev(np.stack([q, k, v], axis=2), dtype)  # [B,T,3,H,D]
        qd, kd, vd = buf[:, :, 0], buf[:, :, 1], buf[:, :, 2]
        assert not qd.is_contiguous()
    else:
        qd, kd, vd = _dev(q, dtype), _dev(k, dtype), _dev(v, dtype)
    md = None if mask is None else _dev(mask, torch.uint8)

    o_ref, lse_ref, p = AR.forward(q, k, v, scale, adm)
    tol_o, tol_lse = AR.forward_bounds(q, k, v, scale, adm, p, o_ref, lse_ref, bf16)
    o, lse = Ck.attn_forward(qd, kd, vd, scale, causal, md)
    assert o.dtype == dtype and o.shape == (B, T, H, Dv) and o.is_contiguous() and lse.dtype == torch.float32
    _check("o", o, o_ref, tol_o)
    assert (_np(lse)[empty] == -np.inf).all() and np.isfinite(_np(lse)[~empty]).all()
    _check("lse", lse[torch.from_numpy(~empty).cuda()], lse_ref[~empty], tol_lse[~empty])
    assert (_np(o).transpose(0, 2, 1, 3)[empty] == 0).all()

    # backward from the reference's o and lse, rounded to their dtypes
    o_in = AR.round_bf16(o_ref) if bf16 else o_ref.astype(np.float32)
    lse_in = lse_ref.astype(np.float32)
    refs, tols = AR.backward(q, k, v, o_in, lse_in, do, scale, adm, bf16)
    od, ld, dod = _dev(o_in, dtype), _dev(lse_in, torch.float32), _dev(do, dtype)
    grads = Ck.attn_backward(qd, kd, vd, od, ld, dod, scale, causal, md)
    for name, got, ref, tol in zip(("dq", "dk", "dv"), grads, refs, tols):
        _check(name, got, ref, tol)
    assert (_np(grads[0]).transpose(0, 2, 1, 3)[empty] == 0).all()

    # a second run of all four launches gives the same bits
    again = Ck.attn_forward(qd, kd, vd, scale, causal, md) + Ck.attn_backward(qd, kd, vd, od, ld, dod, scale, causal, md)
    for a, b in zip(again, [o, lse] + grads):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))

