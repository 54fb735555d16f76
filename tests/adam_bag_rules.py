"""pm_embbag_bwd_adam's rule (include/param_amd.h, FUSED LAZY ADAM) restated in numpy float32: G, the summed gradient of every looked-up
row by the piece rule, then one step of tests/sparse_adam_rules.py.  The kernel is held to this bit for bit (tests/test_gpu_adam_bag.py).
``grads[t]``: float32 ``[B, D_t]``, the gradient of the SUM forward (a mean module's gradient scaled, a 16-bit one widened, by the caller)."""
import numpy as np

from tests import sparse_adam_rules as A

EXACT_RUN = 256      # kExactRun: lookups per piece


def lookups(idx, off, B, t, bag_begin=0, bag_count=None):
    """{row: [bag, ...]} of table t: the bags of the slice ascending, index order inside a bag, a repeat listed as often as it occurs"""
    runs = {}
    for b in range(bag_begin, B if bag_count is None else bag_begin + bag_count):
        for j in range(int(off[t * B + b]), int(off[t * B + b + 1])):
            runs.setdefault(int(idx[j]), []).append(b)
    return runs


def summed_grads(dims, idx, off, B, grads, bag_begin=0, bag_count=None, pads=None):
    """per table (row ids ascending int64 [U_t], G float32 [U_t, D_t]); a table's padding row is left out"""
    out = []
    for t, D in enumerate(dims):
        runs = lookups(idx, off, B, t, bag_begin, bag_count)
        if pads is not None and pads[t] is not None:
            runs.pop(pads[t], None)
        ids = np.array(sorted(runs), dtype=np.int64)
        G = np.zeros((len(ids), D), np.float32)
        for k, r in enumerate(ids):
            pieces = []
            for p0 in range(0, len(runs[r]), EXACT_RUN):      # pieces of 256 lookups from the run's first, each summed from +0.0
                acc = np.zeros(D, np.float32)
                for b in runs[r][p0:p0 + EXACT_RUN]:
                    acc = acc + grads[t][b]
                pieces.append(acc)
            G[k] = pieces[0]
            for p in pieces[1:]:                              # added in ascending order, starting from the first piece
                G[k] = G[k] + p
        out.append((ids, G))
    return out


def step(state, sums, step_no, hyper, dtype="fp32"):
    """state: per table (w, m, v) float32 [R_t, D_t]; returns the new list.  Rows that are not in `sums` keep their bits."""
    return [A.sparse_adam_step(w, ids, G, m, v, step_no, hyper, dtype) for (w, m, v), (ids, G) in zip(state, sums)]
