"""Rules the tests of the 16-bit update paths share (numpy only, no device): the interval a correctly rounded 16-bit result must
lie in, the fp64 evaluation of row-wise Adagrad with the bound for rows whose gradient sum the kernel forms in another order,
and the calibration / correlation statistics of a stochastic store.  Used by tests/test_oracle.py (where the oracle itself is
held to the interval rule), tests/test_gpu_lowp_update.py, tests/test_gpu_many_tables.py and tests/test_gpu_fuzz.py.

Where the numbers come from:
  * ``b = 2e-5 * |w| + 2e-6`` is the bar the fp32 Adagrad kernel meets against the same oracle
    (tests/test_gpu_parity.py::test_fused_rowwise_adagrad_vs_oracle); a round-to-nearest 16-bit store adds half a spacing of
    the table type at the value before rounding.
  * its absolute term suits weights of order one.  For tables far below that the same relative bar is applied to the two terms
    of the update, ``b = 2e-5 * (|w_old| + |w_pre - w_old|)``: kernel and oracle differ in how the sum of squares is reduced
    (fp32 tree against fp64), which moves the step by a relative amount.
  * rows looked up more than 256 times (kExactRun) get their gradient sum from ordered chunk partials: the bound of
    tests/test_gpu_fuzz.py::test_random_adagrad_vs_oracle, derived to first order from an fp64 evaluation.
"""
import numpy as np

from oracle import embbag_oracle as O

EXACT_RUN = 256      # kExactRun in param_amd/csrc/bwd_sorted_apply.h


def tol_b(w_pre, w_old=None):
    """the fp32 part of the tolerance: the project's 2e-5 bar, or (``w_old`` given) its scale-free form"""
    w_pre = np.asarray(w_pre, dtype=np.float64)
    if w_old is None:
        return 2e-5 * np.abs(w_pre) + 2e-6
    w_old = np.asarray(w_old, dtype=np.float64)
    return 2e-5 * (np.abs(w_old) + np.abs(w_pre - w_old))


def nearest_ratio(got, w_pre, code, b):
    """|got - w_pre| / (ulp16(w_pre) / 2 + b) per element: a round-to-nearest store of a value within b of w_pre gives <= 1"""
    got, w_pre = np.asarray(got, dtype=np.float64), np.asarray(w_pre, dtype=np.float64)
    return np.abs(got - w_pre) / (O.ulp16(w_pre, code) / 2 + b)


def adagrad_fp64(w_old, m_old, idx, loc_off, g, psw, lr, eps, wd=0.0, wd_code=0):
    """fp64 evaluation of one exact row-wise Adagrad step of one table and the first-order bound on what a gradient sum formed
    in another order (error <= 1e-5 of the sum of |contributions| per element) does to it.
    Returns (W64, m64, bound_w, bound_m); bound_w has no rounding term and bound_m no relative term: the caller adds those."""
    w_old, m_old = np.asarray(w_old, dtype=np.float64), np.asarray(m_old, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    B = len(loc_off)
    start, end = O.bag_bounds(loc_off, B, len(idx))
    bag_of = np.repeat(np.arange(B), end - start)
    pw = np.ones(len(idx)) if psw is None else np.asarray(psw, dtype=np.float64)
    contrib = np.asarray(g, dtype=np.float64)[bag_of] * pw[:, None]
    G, mag = np.zeros(w_old.shape), np.zeros(w_old.shape)
    np.add.at(G, idx, contrib)
    np.add.at(mag, idx, np.abs(contrib))
    gx = G + wd * w_old if wd_code == 1 else G
    m64 = m_old + (gx ** 2).mean(1)
    mult = lr / (np.sqrt(m64) + eps)
    corr = 1.0 - (mult * wd if wd_code == 1 else np.full_like(mult, lr * wd if wd_code == 2 else 0.0))
    W64 = corr[:, None] * w_old - mult[:, None] * G
    dG = 1e-5 * mag + 1e-30
    dm = (2 * np.abs(gx) * dG).mean(1)                                    # first-order change of the state
    dmult = mult * 0.5 * dm / np.maximum(m64, 1e-30)                      # |d mult / d m| = mult / (2 sqrt(m) (sqrt(m) + eps)) <= this
    shrunk = wd * np.abs(w_old) if wd_code == 1 else 0.0                  # L2: the shrink factor moves with mult
    bound_w = mult[:, None] * dG + dmult[:, None] * (np.abs(G) + shrunk)
    return W64, m64, bound_w, dm


def round_up_stats(got, w_pre, code, b):
    """For a stochastic store: p = the share of the spacing w_pre lies above its lower neighbour, slack = b / spacing, up = the
    stored value is the upper neighbour, inside = the stored value lies in [down16(w_pre - b), up16(w_pre + b)]."""
    got, w_pre = np.asarray(got, dtype=np.float64), np.asarray(w_pre, dtype=np.float64)
    u = O.ulp16(w_pre, code)
    lo = O.down16(w_pre, code)
    p = (w_pre - lo) / u
    inside = (got >= O.down16(w_pre - b, code)) & (got <= O.up16(w_pre + b, code))
    return p, b / u, got > lo, inside


def calibration(p, up, slack, nbins=10):
    """ten equal bins of p: (n, mean p, observed share of round-ups, allowed distance) per bin.  Allowed: five binomial standard
    deviations plus the systematic shift the fp32 tolerance can cause."""
    rows = []
    which = np.minimum((p * nbins).astype(np.int64), nbins - 1)
    for k in range(nbins):
        sel = which == k
        n = int(sel.sum())
        if n == 0:
            rows.append((0, float("nan"), float("nan"), 0.0))
            continue
        pk = p[sel]
        rows.append((n, float(pk.mean()), float(up[sel].mean()), float(5 * np.sqrt((pk * (1 - pk)).sum()) / n + slack[sel].mean())))
    return rows


def calibration_table(rows) -> str:
    out = ["bin      n   expected  observed   allowed"]
    for k, (n, e, o, lim) in enumerate(rows):
        out.append(f"{k:3d} {n:7d}   {e:.4f}    {o:.4f}    {lim:.4f}  {'ok' if n and abs(o - e) <= lim else 'MISS'}")
    return "\n".join(out)


def correlation(a, b) -> float:
    """correlation of two centred indicators (up - p): their expectation is zero by construction, so no mean is removed"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))
