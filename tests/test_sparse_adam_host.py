"""Sparse-row Adam without a GPU: the numpy restatement of the rule (tests/sparse_adam_rules.py) against an fp64 evaluation of the same
formulas and against torch.optim.SparseAdam on the CPU, the C entry's refusals, and SparseAdamMI355's constructor and state keys."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from param_amd import _lib
from param_amd.optim import SparseAdamMI355
from tests import sparse_adam_rules as R

ROWS, DIM, LISTED = 12, 8, np.array([11, 0, 5, 3, 8, 2, 7])
EPS32 = 2.0 ** -24


_hyper = lambda wd: {"lr": 1.0e-2, "betas": (0.9, 0.999), "eps": 1.0e-8, "weight_decay": wd}      # noqa: E731


@functools.lru_cache(maxsize=None)
def _trajectory(dtype, wd):
    """three successive steps, the state carried by the restatement: per step (w, m, v before; g; w, m, v after; w64, delta64), where
    w64 and delta64 = s * q are the formulas in fp64 on the step's fp32 inputs, with the scalars in double precision"""
    rng = np.random.default_rng(7)
    hyper = _hyper(wd)
    w = R.round_to_table(rng.standard_normal((ROWS, DIM)).astype(np.float32), dtype)
    m, v = np.zeros_like(w), np.zeros_like(w)
    out = []
    for step in (1, 2, 3):
        g = (rng.choice([-1.0, 1.0], (LISTED.size, DIM)) * 10.0 ** rng.uniform(-4, 2, (LISTED.size, DIM))).astype(np.float32)
        g[rng.random(g.shape) < 0.1] = 0.0                        # both signs, 1e-4 .. 1e2, a few exact zeros
        w1, m1, v1 = R.sparse_adam_step(w, LISTED, g, m, v, step, hyper, dtype)
        lr, (b1, b2) = hyper["lr"], hyper["betas"]
        g64, w64, m64, v64 = (x.astype(np.float64) for x in (g, w[LISTED], m[LISTED], v[LISTED]))
        mn, vn = m64 + (g64 - m64) * (1 - b1), v64 + (g64 * g64 - v64) * (1 - b2)
        delta = lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step) * (mn / (np.sqrt(vn) + hyper["eps"]))
        out.append(((w, m, v), g, (w1, m1, v1), w64 * (1 - lr * wd) - delta, delta))
        w, m, v = w1, m1, v1
    return out


def _bound(w64, delta64, dtype):
    # 16: the at most 14 fp32 roundings on the way to s * q -- four for m' counting c1, five for v' counting c2 (halved by the square
    # root), then sqrt, eps, the add, the division, s and the product -- with room for their second-order terms
    tail = 16 * EPS32 * np.abs(delta64)
    if dtype == "fp32":
        return 3 * EPS32 * np.abs(w64) + tail                     # 3: the decay product, the subtraction, the stored rounding
    e = np.floor(np.log2(np.maximum(np.abs(w64), 1e-300)))        # half an ulp of the table dtype at w64
    return 2.0 ** (e - 8 if dtype == "bf16" else np.maximum(e, -14) - 11) + tail


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_restatement_against_fp64(dtype, wd):
    rest = np.setdiff1d(np.arange(ROWS), LISTED)
    for (w0, _, _), _, (w1, _, _), w64, delta in _trajectory(dtype, wd):
        err = np.abs(w1[LISTED].astype(np.float64) - w64)
        assert (err <= _bound(w64, delta, dtype)).all(), float((err / _bound(w64, delta, dtype)).max())
        assert np.array_equal(w1[rest], w0[rest])                 # rows that are not listed keep their bits


def test_torch_sparse_adam_agrees_within_the_same_bound():
    hyper = _hyper(0.0)
    p = torch.nn.Parameter(torch.zeros(ROWS, DIM))
    opt = torch.optim.SparseAdam([p], lr=hyper["lr"], betas=hyper["betas"], eps=hyper["eps"])
    for step, ((w, m, v), g, _, w64, delta) in enumerate(_trajectory("fp32", 0.0), 1):
        p.data.copy_(torch.from_numpy(w))
        opt.state[p].update(step=step - 1, exp_avg=torch.from_numpy(m.copy()), exp_avg_sq=torch.from_numpy(v.copy()))
        p.grad = torch.sparse_coo_tensor(torch.from_numpy(LISTED)[None], torch.from_numpy(g), (ROWS, DIM)).coalesce()
        opt.step()
        err = np.abs(p.data.numpy()[LISTED].astype(np.float64) - w64)
        assert (err <= _bound(w64, delta, "fp32")).all()


def test_c_entry_refusals_without_a_gpu():
    L = _lib.load()
    good = _lib.pm_sparse_adam(0.1, 0.001, 1e-8, 1e-3, 1.0, 0, 1, 0)
    call = lambda opt, T=1, U=8, max_dim=8, ptr=8, dtype=_lib.PM_F32: L.pm_sparse_rows_adam(                       # noqa: E731
        T, U, max_dim, ptr, dtype, ptr, ptr, ptr, ptr, ptr, ptr, ctypes.byref(opt) if opt else None, None)
    assert call(good, ptr=None) == _lib.PM_ERR_INVALID and b"NULL" in L.pm_last_error() and call(None) == _lib.PM_ERR_INVALID
    assert call(good, dtype=7) == _lib.PM_ERR_INVALID and b"table_dtype" in L.pm_last_error()
    assert call(good, max_dim=6) == _lib.PM_ERR_UNSUPPORTED and b"multiple of 4" in L.pm_last_error()
    assert call(good, U=-1) == _lib.PM_ERR_INVALID
    bad = _lib.pm_sparse_adam(0.1, 0.001, 1e-8, float("inf"), 1.0, 0, 1, 0)                                         # a non-finite lr
    assert call(bad) == _lib.PM_ERR_INVALID and b"finite" in L.pm_last_error()
    assert call(good, U=0, ptr=None) == _lib.PM_OK and call(good, T=0, ptr=None) == _lib.PM_OK


def test_constructor_checks_and_state_keys():
    p = torch.nn.Parameter(torch.zeros(ROWS, DIM))
    with pytest.raises(ValueError, match="Invalid learning rate: -1.0"):
        SparseAdamMI355([p], lr=-1.0)
    with pytest.raises(ValueError, match="Invalid beta parameter at index 1: 1.0"):
        SparseAdamMI355([p], betas=(0.9, 1.0))
    ref = torch.optim.SparseAdam([p])
    p.grad = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.ones(1, DIM), (ROWS, DIM))
    ref.step()
    ours = SparseAdamMI355([p])
    ours.load_state_dict(ref.state_dict())
    assert set(ours.state[p]) == set(ref.state[p]) == {"step", "exp_avg", "exp_avg_sq"}
    p.grad = torch.ones(ROWS, DIM)
    with pytest.raises(RuntimeError, match="SparseAdam does not support dense gradients"):
        ours.step()
