#!/usr/bin/env python3
"""Checks the rounding bounds of tests/attention_refs.py without the kernels: evaluates the kernels' formulas in plain
f32 numpy on the CPU (log2-domain softmax with scale log2(e) folded in; for bf16, P and dS rounded once to bf16 and
the outputs rounded to bf16) for every test case and prints each result's worst error / bound against the float64
reference.  Every ratio must stay below 1: a bound this straightforward f32 evaluation misses lacks a rounding term.

numpy keeps denormals, so this evaluation does not reach the underflow terms of the bounds (the kernels flush what
falls below 2^-126); those rest on their derivation in tests/attention_refs.py alone.

    python scripts/check_attention_bounds.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import attention_refs as AR  # noqa: E402

F = np.float32
LOG2E, LN2 = F(1.4426950408889634), F(0.6931471805599453)


def evaluate(q, k, v, do, scale, adm, o_in, lse_in, bf16):
    """(o, lse, dq, dk, dv) in f32 arithmetic; the backward from the given o and lse, as the kernels' is."""
    rnd = AR.round_bf16 if bf16 else (lambda x: x)
    cs = F(F(scale) * LOG2E)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.einsum("bthd,bshd->bhts", q, k, dtype=F)
        x = np.where(adm, s * cs, F(-np.inf))
        m = x.max(axis=3, keepdims=True)
        mu = np.where(np.isfinite(m), m, F(0))
        p = np.exp2(x - mu, dtype=F)
        l = p.sum(axis=3, keepdims=True, dtype=F)
        inv = np.where(l > 0, F(1) / np.where(l > 0, l, F(1)), F(0))
        o = rnd(np.einsum("bhts,bshe->bthe", rnd(p), v, dtype=F) * inv.transpose(0, 2, 1, 3))
        lse = np.where(l > 0, (mu + np.log2(l, dtype=F)) * LN2, F(-np.inf))[..., 0]
        l2 = np.where(np.isfinite(lse_in), lse_in * LOG2E, F(np.inf))[..., None]
        pb = np.where(adm, np.exp2(s * cs - l2, dtype=F), F(0))
    delta = np.einsum("bthe,bthe->bht", do, o_in, dtype=F)
    dS = rnd(pb * (np.einsum("bthe,bshe->bhts", do, v, dtype=F) - delta[..., None]))
    dv = rnd(np.einsum("bhts,bthe->bshe", rnd(pb), do, dtype=F))
    dq = rnd(np.einsum("bhts,bshd->bthd", dS, k, dtype=F) * F(scale))
    dk = rnd(np.einsum("bhts,bthd->bshd", dS, q, dtype=F) * F(scale))
    return o, lse, dq, dk, dv


def main():
    worst = 0.0
    for name, case in zip(AR.IDS, AR.CASES):
        (B, H, T, S, D, Dv), causal, _, _ = case
        for bf16 in (False, True):
            (q, k, v, do), mask, scale = AR.inputs(case, bf16)
            adm = AR.admitted(B, H, T, S, causal, mask)
            o_ref, lse_ref, p = AR.forward(q, k, v, scale, adm)
            tol_o, tol_lse = AR.forward_bounds(q, k, v, scale, adm, p, o_ref, lse_ref, bf16)
            o_in = AR.round_bf16(o_ref) if bf16 else o_ref.astype(F)
            lse_in = lse_ref.astype(F)
            refs, tols = AR.backward(q, k, v, o_in, lse_in, do, scale, adm, bf16)
            got = evaluate(q, k, v, do, scale, adm, o_in, lse_in, bf16)
            live = adm.any(axis=3)
            assert (got[1][~live] == -np.inf).all()
            pairs = [(got[0], o_ref, tol_o), (got[1][live], lse_ref[live], tol_lse[live])] + [
                (g, r, t) for g, r, t in zip(got[2:], refs, tols)]
            ratios = [float((np.abs(g.astype(np.float64) - r) / t).max()) for g, r, t in pairs]
            worst = max(worst, *ratios)
            print(f"{name:16s} {'bf16' if bf16 else 'f32 '} " + "  ".join(
                f"{n} {x:.3g}" for n, x in zip(("o", "lse", "dq", "dk", "dv"), ratios)))
    print(f"worst error / bound: {worst:.3g}")
    return 0 if worst <= 1 else 1


if __name__ == "__main__":
    sys.exit(main())
