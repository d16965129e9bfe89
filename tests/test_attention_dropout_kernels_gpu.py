"""The DROP instantiations of the fused attention kernels through the bindings: the keep mask read off element for
element against the numpy Philox stream, and o, lse, dq, dk, dv against tests/attention_dropout_refs.py (float64)."""
import numpy as np
import pytest
import torch

import attention_dropout_refs as DR
import attention_refs as AR
from tensorflow_distributed_learning_amd.ops import dropout as DO, hip as _C
from test_attention_kernels_gpu import _check, _dev, _np

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
CASES = {n: AR.CASES[AR.IDS.index(n)] for n in ("tile_plus_one", "cross_odd_heads", "causal", "mask_bhts", "head128", "packed_qkv")}
CASES["partial_group"] = ((1, 1, 18, 16, 16, 16), False, None, "")  # T = 18: the last group of four rows holds two


def _state(calls):
    return torch.tensor([calls, 0], dtype=torch.int64, device="cuda")


@DTYPES
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_the_mask_read_off_the_output_is_the_numpy_stream(causal, dtype):
    """q = 0 and v = onehot(key): o[b,i,h,j] = c z / count_i -- two query tiles, two key tiles, T % 4 = 2."""
    (B, H, T, S, D, Dv), rate, bf16 = (2, 3, 70, 128, 8, 128), 0.5, dtype == torch.bfloat16
    q, k = np.zeros((B, T, H, D), np.float32), AR.inputs(((B, H, S, S, D, D), 0, None, ""), bf16)[0][1]
    v = np.ascontiguousarray(np.broadcast_to(np.eye(S, dtype=np.float32)[None, :, None, :], (B, S, H, Dv)))
    adm = AR.admitted(B, H, T, S, causal, None)
    _, lse_ref, p = AR.forward(q, k, v, 1.0, adm)
    tol_lse = AR.forward_bounds(q, k, v, 1.0, adm, p, np.zeros((B, T, H, Dv)), lse_ref, bf16)[1]
    state, c, one = _state(5), DO.keep_scale(rate), 2.0 ** -8 if bf16 else 2.0 ** -23  # one: a rounding, as AR counts it
    for call in (5, 6):  # the second call: the next ticket and its mask
        o, lse, ticket = _C().attn_forward(_dev(q, dtype), _dev(k, dtype), _dev(v, dtype), 1.0, causal, None, rate, DR.KEY, state)
        assert int(ticket) == call and state.tolist() == [call + 1, 0]
        z, got = DR.keep_mask(DR.KEY, call, rate, B, H, T, S) & adm, _np(o).transpose(0, 2, 1, 3)
        assert np.array_equal(got != 0, z) and 0.4 < z[adm].mean() < 0.6
        assert (np.abs(got - c * z * p) <= 2 * one * c * p).all()
        _check("lse", lse, lse_ref, tol_lse)


@DTYPES
@pytest.mark.parametrize("rate", [0.1, 0.5])
@pytest.mark.parametrize("case", list(CASES.values()), ids=list(CASES))
def test_dropout_kernels_against_f64(case, rate, dtype):
    (B, H, T, S, D, Dv), causal, kind, layout = case
    Ck, bf16, c = _C(), dtype == torch.bfloat16, DO.keep_scale(rate)
    (q, k, v, do), mask, scale = AR.inputs(case, bf16)
    adm = AR.admitted(B, H, T, S, causal, mask)
    empty, z = ~adm.any(axis=3), DR.keep_mask(DR.KEY, 3, rate, B, H, T, S)
    qd, kd, vd = _dev(np.stack([q, k, v], axis=2), dtype).unbind(2) if layout == "packed" else (_dev(a, dtype) for a in (q, k, v))
    o_ref, lse_ref, _, tol_o, tol_lse = DR.forward(q, k, v, scale, adm, z, c, bf16)
    # the backward from the reference's o and lse, rounded to their dtypes, and the forward's ticket tensor
    o_in, lse_in = AR.round_bf16(o_ref) if bf16 else o_ref.astype(np.float32), lse_ref.astype(np.float32)
    md, dod, od, ld = None if mask is None else _dev(mask, torch.uint8), _dev(do, dtype), _dev(o_in, dtype), _dev(lse_in, torch.float32)

    def run():
        o, lse, ticket = Ck.attn_forward(qd, kd, vd, scale, causal, md, rate, DR.KEY, _state(3))
        return [o, lse, ticket] + Ck.attn_backward(qd, kd, vd, od, ld, dod, scale, causal, md, rate, DR.KEY, ticket)

    o, lse, ticket, *grads = run()
    _check("o", o, o_ref, tol_o)
    assert int(ticket) == 3 and (_np(lse)[empty] == -np.inf).all() and (_np(o).transpose(0, 2, 1, 3)[empty] == 0).all()
    _check("lse", lse[torch.from_numpy(~empty).cuda()], lse_ref[~empty], tol_lse[~empty])
    refs, tols = DR.backward(q, k, v, o_in, lse_in, do, scale, adm, z, c, bf16)
    for name, got, ref, tol in zip(("dq", "dk", "dv"), grads, refs, tols):
        _check(name, got, ref, tol)
    assert (_np(grads[0]).transpose(0, 2, 1, 3)[empty] == 0).all()
    for a, b in zip(run(), [o, lse, ticket] + grads):  # from the same call number: the same bits
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
