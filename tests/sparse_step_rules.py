"""The rules of pm_sparse_rows_sgd / pm_sparse_rows_adagrad (include/param_amd.h, SPARSE-ROW ADAGRAD AND SGD) restated in numpy float32:
every numpy operation on float32 operands is one fp32 rounding, ``fmaf`` is one rounding of the exact a * b + c, np.sqrt and the
division are correctly rounded.  The kernel is held to this restatement bit for bit (tests/test_gpu_sparse_step.py).  Tables of every
dtype are float32 arrays of representable values."""
import numpy as np

from tests.qrows_rules import fmaf
from tests.sparse_adam_rules import round_to_table


def alpha_of(step, hyper):
    """-(lr / (1 + (step - 1) * lr_decay)) in double precision, rounded ONCE to fp32 (SGD: no lr_decay, so -lr)"""
    return np.float32(-(hyper["lr"] / (1.0 + (step - 1) * hyper.get("lr_decay", 0.0))))


def row_sum_of_squares(g):
    """S of every row of g [U, D] in the kernel's order: G = next_pow2(D / 4) <= 64 lanes; lane l owns columns 4 (pass * G + l) + k; its
    partial adds fl(g * g) to +0 with pass, then k ascending (columns past D hold +0, which changes no partial); xor butterfly, low mask first"""
    U, D = g.shape
    G = 1
    while G < 64 and 4 * G < D:
        G *= 2
    passes = -(-D // (4 * G))
    sq = np.zeros((U, passes * G * 4), dtype=np.float32)
    sq[:, :D] = g * g
    sq = sq.reshape(U, passes, G, 4)
    part = np.zeros((U, G), dtype=np.float32)
    for p in range(passes):
        for k in range(4):
            part = part + sq[:, p, :, k]
    lane, m = np.arange(G), 1
    while m < G:
        part = part + part[:, lane ^ m]
        m *= 2
    assert part.dtype == np.float32 and (part == part[:, :1]).all()       # the same value in every lane
    return part[:, 0]


def sgd_step(w, rows, g, hyper, dtype="fp32"):
    """w [R, D] (values of `dtype`), rows int64 [U] distinct, g [U, D]; returns the new w; rows that are not listed keep their bits"""
    w = w.copy()
    g = -g if hyper.get("maximize", False) else g
    w[rows] = round_to_table(fmaf(alpha_of(1, hyper), g, w[rows]), dtype)
    return w


def adagrad_step(w, rows, g, s, step, hyper, dtype="fp32", rowwise=False):
    """one Adagrad step of one table; s: [R, D], or [R] when rowwise.  Returns the new (w, s)"""
    alpha, eps = alpha_of(step, hyper), np.float32(hyper["eps"])
    w, s = w.copy(), s.copy()
    g = -g if hyper.get("maximize", False) else g
    if rowwise:
        s1 = s[rows] + row_sum_of_squares(g) / np.float32(g.shape[1])
        mult = alpha / (np.sqrt(s1) + eps)
        w[rows], s[rows] = round_to_table(fmaf(mult[:, None], g, w[rows]), dtype), s1
    else:
        s1 = s[rows] + g * g
        w[rows], s[rows] = round_to_table(fmaf(alpha, g / (np.sqrt(s1) + eps), w[rows]), dtype), s1
    assert w.dtype == s.dtype == np.float32
    return w, s
