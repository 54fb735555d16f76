"""Restatement of the fused exact ELEMENT-wise Adagrad update (numpy only, no device), shared by tests/test_elem_adagrad_host.py
(where it is pinned to the live ``torch.optim.Adagrad`` on the CPU) and tests/test_gpu_elem_adagrad.py (where the kernels are held
to it):

    G    = sum over a row's lookups of psw * g            fp32, lookup order, from zero
    gx   = G + wd * w (L2)  |  G (NONE, DECOUPLE)
    s    = s_old + gx * gx                                 one fp32 state value per weight
    w    = w - (lr * gx) / (sqrt(s) + eps)                 NONE, L2     (torch: ``param.addcdiv_(grad, std, value=-lr)``)
    w    = (1 - lr * wd) * w - (lr * G) / (sqrt(s) + eps)  DECOUPLE     (no third-party implementation: restated only)

Only rows some lookup touches change (a fused sparse update; L2 decay reaches touched rows only).

Where the numbers come from:
  * ``STATE_RTOL`` / ``W_RTOL`` / ``W_ATOL`` are the bars the existing torch pin of the row-wise update uses
    (tests/test_gpu_parity.py::test_fused_rowwise_adagrad_equals_torch_adagrad_where_rowwise_is_elementwise).
  * rows looked up more than ``lowp_rules.EXACT_RUN`` times get their gradient sum from ordered chunk partials: ``step_fp64`` returns
    the effect of a sum formed in another order (error <= 1e-5 of the sum of |contributions| per element, the figure
    ``lowp_rules.adagrad_fp64`` uses) on the state and on the weights.
"""
import numpy as np

from oracle import embbag_oracle as O
from tests import lowp_rules as R

EXACT_RUN = R.EXACT_RUN
STATE_RTOL = 1e-6
W_RTOL, W_ATOL = 2e-6, 1e-7
WD_NONE, WD_L2, WD_DECOUPLE = 0, 1, 2


def _lookups(idx, loc_off, g, psw):
    idx = np.asarray(idx, dtype=np.int64)
    B = len(loc_off)
    start, end = O.bag_bounds(loc_off, B, len(idx))
    bag_of = np.repeat(np.arange(B), end - start)
    return idx, bag_of


def grad_sum_f32(rows, idx, loc_off, g, psw=None):
    """(G, count): the fp32 sum of ``psw[j] * g[bag(j)]`` per row, added in lookup order from zero (what the kernels evaluate for
    rows of at most EXACT_RUN lookups, bit for bit), and the number of lookups per row.  ``g`` is the table's [B, D] gradient,
    ``loc_off`` its B (or B + 1) offsets rebased to ``idx``."""
    idx, bag_of = _lookups(idx, loc_off, g, psw)
    g = np.asarray(g, dtype=np.float32)
    contrib = g[bag_of] if psw is None else (np.asarray(psw, dtype=np.float32)[:, None] * g[bag_of]).astype(np.float32)
    G = np.zeros((rows, g.shape[1]), np.float32)
    count = np.bincount(idx, minlength=rows)
    order = np.argsort(idx, kind="stable")
    first = np.concatenate([[0], np.cumsum(count)[:-1]])
    rank = np.arange(len(idx)) - first[idx[order]]             # k-th lookup of its row, in lookup order
    for k in range(int(count.max()) if len(idx) else 0):
        sel = order[rank == k]                                  # one lookup per row: a plain fancy-index add is exact
        G[idx[sel]] = G[idx[sel]] + contrib[sel]
    return G, count


def step_f32(w, s, G, touched, lr, eps, wd=0.0, wd_code=WD_NONE, torch_fused=False):
    """one step in fp32, operation by operation as stated above; returns new (w, s).  ``touched``: boolean per row.
    ``torch_fused``: form ``gx = fma(wd, w, G)`` and ``s = fma(gx, gx, s_old)`` with one rounding each, which is what torch's CPU
    ``grad.add(param, alpha=wd)`` and ``state_sum.addcmul_(grad, grad)`` evaluate; the kernels (built without contraction) and this
    restatement by default round the products first -- the TWO operations in which they depart from torch's bits, by a last place
    (tests/test_special_values_host.py pins every other operation bit for bit through this switch)."""
    w, s, G = (np.asarray(a, dtype=np.float32) for a in (w, s, G))
    lr, eps, wd = np.float32(lr), np.float32(eps), np.float32(wd)
    if wd_code == WD_L2:
        gx = O.fma_f32(wd, w, G) if torch_fused else (G + wd * w).astype(np.float32)
    else:
        gx = G
    s_new = O.fma_f32(gx, gx, s) if torch_fused else (s + gx * gx).astype(np.float32)
    step = ((lr * gx) / (np.sqrt(s_new) + eps)).astype(np.float32)
    kept = ((np.float32(1.0) - lr * wd) * w).astype(np.float32) if wd_code == WD_DECOUPLE else w
    w_new = (kept - step).astype(np.float32)
    t = np.asarray(touched, dtype=bool)[:, None]
    return np.where(t, w_new, w), np.where(t, s_new, s)


def step_fp64(w, s, idx, loc_off, g, psw, lr, eps, wd=0.0, wd_code=WD_NONE):
    """fp64 evaluation of one step of one table and the bound on what a gradient sum formed in another order does to it (the way
    ``lowp_rules.adagrad_fp64`` does it for the row-wise update; element-wise, nothing is averaged over a row and the bound can be
    exact rather than first-order).  With dG = 1e-5 * sum |contributions| the sum's allowance per element:
        state    s = s_old + gx^2:                       ds = (|gx| + dG)^2 - gx^2 = 2 |gx| dG + dG^2
        weights  the step f(gx) = lr gx / (sqrt(s_old + gx^2) + eps) has 0 <= f' <= lr / (sqrt(s_old + gx^2) + eps), largest over
                 [gx - dG, gx + dG] where |gx| is smallest:  dw = lr dG / (sqrt(s_old + max(|gx| - dG, 0)^2) + eps)
        (L2: gx = G + wd w moves one for one with G; DECOUPLE: the shrunk row does not depend on G.)
    Returns (W64, S64, dw, ds, count); the bounds hold no rounding term: the caller adds the fp32 bars."""
    w, s = np.asarray(w, dtype=np.float64), np.asarray(s, dtype=np.float64)
    idx, bag_of = _lookups(idx, loc_off, g, psw)
    pw = np.ones(len(idx)) if psw is None else np.asarray(psw, dtype=np.float64)
    contrib = np.asarray(g, dtype=np.float64)[bag_of] * pw[:, None]
    G, mag = np.zeros(w.shape), np.zeros(w.shape)
    np.add.at(G, idx, contrib)
    np.add.at(mag, idx, np.abs(contrib))
    count = np.bincount(idx, minlength=w.shape[0])
    gx = G + wd * w if wd_code == WD_L2 else G
    S64 = s + gx * gx
    denom = np.sqrt(S64) + eps
    keep = 1.0 - lr * wd if wd_code == WD_DECOUPLE else 1.0
    W64 = keep * w - lr * gx / denom
    t = (count > 0)[:, None]
    W64, S64 = np.where(t, W64, w), np.where(t, S64, s)
    dG = 1e-5 * mag + 1e-30
    ds = 2 * np.abs(gx) * dG + dG * dG
    dw = lr * dG / (np.sqrt(s + np.maximum(np.abs(gx) - dG, 0.0) ** 2) + eps)
    return W64, S64, dw, ds, count
