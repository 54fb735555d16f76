"""numpy restatement of the DIRECT BACKWARD rule of max pooling (include/param_amd.h, "MAX POOLING, DIRECT BACKWARD"), per table, on top
of tests/max_rules.py (the request, ``forward`` for ``max_indices``).  ``grads`` / ``args``: lists of T whole-batch ``[B, D_t]`` arrays.

A row's run is its lookups in the slice, in lookup order; a bag's repeats are adjacent there and count once.  The run is cut every
``EXACT_RUN`` lookups from its start; a piece is summed sequentially in fp32 from its first term, the pieces that have a term are added
in order from the first such piece.  A run of at most ``EXACT_RUN`` lookups is one piece: the plain sequential sum."""
import numpy as np

from tests import max_rules as M
from tests import out16_rules as O

EXACT_RUN = 256      # kExactRun in param_amd/csrc/bwd_sorted_apply.h


def sums(rows, dims, indices, offsets, B, grads, args, bag_begin=0, bag_count=None):
    """per table ``(G, won, G64, A64, n)`` ``[rows_t, D_t]``: the rule's fp32 sum, whether the element has a term, the float64 sum of
    the terms, of their magnitudes, and their number"""
    T = len(rows)
    idx = np.asarray(indices).astype(np.int64).reshape(-1)
    hi = B if bag_count is None else bag_begin + bag_count
    start, end = M.bag_bounds(offsets, T, B, idx.size)
    out = []
    for t, (R, D) in enumerate(zip(rows, dims)):
        g, a = np.asarray(grads[t], dtype=np.float32), np.asarray(args[t]).astype(np.int64)
        G, won = np.zeros((R, D), np.float32), np.zeros((R, D), bool)
        G64, A64, n = np.zeros((R, D)), np.zeros((R, D)), np.zeros((R, D), np.int64)
        runs = {}
        for b in range(bag_begin, hi):
            for j in range(int(start[t * B + b]), int(end[t * B + b])):
                runs.setdefault(int(idx[j]), []).append(b)
        with np.errstate(all="ignore"):
            for r, run in runs.items():
                for p0 in range(0, len(run), EXACT_RUN):
                    acc, has = np.zeros(D, np.float32), np.zeros(D, bool)
                    for k in range(p0, min(p0 + EXACT_RUN, len(run))):
                        b = run[k]
                        if k and run[k - 1] == b:
                            continue
                        hit = a[b] == r
                        acc = np.where(hit, np.where(has, acc + g[b], g[b]), acc)
                        has |= hit
                        G64[r] += np.where(hit, g[b].astype(np.float64), 0.0)
                        A64[r] += np.where(hit, np.abs(g[b].astype(np.float64)), 0.0)
                        n[r] += hit
                    G[r] = np.where(has, np.where(won[r], G[r] + acc, acc), G[r])
                    won[r] |= has
        out.append((G, won, G64, A64, n))
    return out


def apply(dst_bits, dtype, G, won, alpha):
    """the destination's bits after the call: ``dst_bits`` uint32 (``dtype`` "f32") or uint16 ("bf16" / "fp16"); an element without a
    term keeps its bits, the others become ``round(widen(dst) + fl32(alpha * G))``"""
    with np.errstate(all="ignore"):
        step = (np.float32(alpha) * G).astype(np.float32)
        if dtype == "f32":
            new = (np.ascontiguousarray(dst_bits).view(np.float32) + step).astype(np.float32).view(np.uint32)
        else:
            new = O.round16((O.widen(dst_bits, dtype) + step).astype(np.float32), dtype)
    return np.where(won, new, dst_bits)
