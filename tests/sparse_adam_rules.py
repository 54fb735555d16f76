"""pm_sparse_rows_adam's rule (include/param_amd.h, SPARSE-ROW ADAM) restated in numpy float32: every numpy operation on float32
operands is one fp32 rounding, nothing is contracted, np.sqrt and the division are correctly rounded.  The kernel is held to this
restatement bit for bit (tests/test_gpu_sparse_adam.py).  Tables of every dtype are float32 arrays of representable values."""
import math

import numpy as np


def step_scalars(step, hyper):
    """(c1, c2, eps, s, d): computed in double precision, each rounded ONCE to fp32"""
    lr, (beta1, beta2), wd = hyper["lr"], hyper["betas"], hyper.get("weight_decay", 0.0)
    s = lr * math.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step)
    return tuple(np.float32(x) for x in (1.0 - beta1, 1.0 - beta2, hyper["eps"], s, 1.0 - lr * wd))


def round_to_table(x, dtype):
    """fp32 -> the table dtype ("fp32" | "bf16" | "fp16"), round to nearest even, as float32 values"""
    if dtype == "fp16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float32)
    if dtype == "bf16":                                     # (finite values: the tests hold no NaN)
        u = x.view(np.uint32).astype(np.uint64)
        return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    return x


def sparse_adam_step(w, rows, g, m, v, step, hyper, dtype="fp32"):
    """one step of one table: w [R, D] (values of `dtype`), rows int64 [U] distinct, g [U, D], m / v [R, D]; float32 throughout.
    Returns new (w, m, v); rows that are not listed keep their bits."""
    c1, c2, eps, s, d = step_scalars(step, hyper)
    w, m, v = w.copy(), m.copy(), v.copy()
    g = -g if hyper.get("maximize", False) else g
    wr, mr, vr = w[rows], m[rows], v[rows]
    w0 = wr * d if hyper.get("weight_decay", 0.0) != 0 else wr
    m1 = mr + (g - mr) * c1
    v1 = vr + (g * g - vr) * c2
    q = m1 / (np.sqrt(v1) + eps)
    w[rows], m[rows], v[rows] = round_to_table(w0 - s * q, dtype), m1, v1
    assert w.dtype == m.dtype == v.dtype == np.float32
    return w, m, v
