"""numpy references of the embedding kernels (csrc/kernels/embedding.h): the gather and the ordered f32 fold."""
import numpy as np

import kernel_refs as R


def gather_ref(ids, table, bf16=False):
    """table[ids] (f32 [V, D]) with a zero row for an id outside [0, V): f32 values, or bf16 bits (uint16)."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    ok = (ids >= 0) & (ids < table.shape[0])
    y = np.zeros((ids.size, table.shape[1]), np.float32)
    y[ok] = np.asarray(table, np.float32)[ids[ok]]
    return R.bf16_rne(y) if bf16 else y


def fold_ref(ids, dy, V, target=None):
    """dE [V, D] f32: per row the left fold of dy[n] (f32 values) over ids[n] == v in ascending n, started from the
    first term, one f32 rounding per addition; then target[v] + s for the touched rows of a target, else zeros for
    the untouched rows."""
    ids, dy = np.asarray(ids, dtype=np.int64).reshape(-1), np.asarray(dy, np.float32)
    out = np.zeros((V, dy.shape[1]), np.float32) if target is None else np.array(target, np.float32)
    with np.errstate(all="ignore"):
        for v in np.unique(ids[(ids >= 0) & (ids < V)]):
            rows = dy[ids == v]
            s = rows[0].copy()
            for r in rows[1:]:
                s = s + r
            out[v] = s if target is None else out[v] + s
    return out
