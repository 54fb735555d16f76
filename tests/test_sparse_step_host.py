"""Sparse-row Adagrad and SGD without a GPU: the numpy restatement of the rules (tests/sparse_step_rules.py) against torch's CPU
optimizers on bits, the row-wise rule against an fp64 evaluation of its formulas, the C entries' refusals, and the state's keys."""
import ctypes

import numpy as np
import pytest
import torch

from param_amd import _lib
from param_amd.optim import SparseAdagradMI355, SparseSGDMI355
from tests import sparse_step_rules as R

ROWS, DIM, LISTED = 12, 8, np.array([11, 0, 5, 3, 8, 2, 7])
EPS32 = 2.0 ** -24
HYPER = {"lr": 3.0e-2, "lr_decay": 0.1, "eps": 1.0e-10, "initial_accumulator_value": 0.25}
_bits = lambda x: np.ascontiguousarray(x).view(np.uint32)      # noqa: E731


def _gradient(rng, shape):
    g = (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-4, 2, shape)).astype(np.float32)
    g[rng.random(shape) < 0.1] = 0.0                              # both signs, 1e-4 .. 1e2, a few exact zeros
    return g


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("rule", ["adagrad", "sgd"])
def test_restatement_is_torch_on_bits(rule, maximize):
    rng = np.random.default_rng(7)
    hyper = dict(HYPER, maximize=maximize)
    w = rng.standard_normal((ROWS, DIM)).astype(np.float32)
    s = np.full_like(w, hyper["initial_accumulator_value"])
    p = torch.nn.Parameter(torch.from_numpy(w.copy()))
    opt = (torch.optim.SGD([p], lr=hyper["lr"], maximize=maximize) if rule == "sgd" else
           torch.optim.Adagrad([p], **hyper))
    for step in (1, 2, 3):
        g = _gradient(rng, (LISTED.size, DIM))
        p.grad = torch.sparse_coo_tensor(torch.from_numpy(LISTED)[None], torch.from_numpy(g), (ROWS, DIM)).coalesce()
        opt.step()
        if rule == "sgd":
            w = R.sgd_step(w, LISTED, g, hyper)
        else:
            w, s = R.adagrad_step(w, LISTED, g, s, step, hyper)
            assert np.array_equal(_bits(opt.state[p]["sum"].numpy()), _bits(s)), step
        assert np.array_equal(_bits(p.detach().numpy()), _bits(w)), step


@pytest.mark.parametrize("dim", [8, 12, 520])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_rowwise_restatement_against_fp64(dtype, dim):
    """Bound, with u = 2^-24 and every summand of S positive: S carries (D + 1) u (D products and adds in any order), s' = s + S / D two
    more roundings, the square root halves that and adds one, then eps' add, the division and alpha's own rounding add one each:
    mult is within ((D + 3) / 2 + 4) u, one more u for second-order terms.  mult * g enters the fma exactly; the fma rounds once (u at the
    result) and the table type once more (half an ulp of that type at the result)."""
    rng = np.random.default_rng(11)
    w = R.round_to_table(rng.standard_normal((ROWS, dim)).astype(np.float32), dtype)
    s = np.full(ROWS, HYPER["initial_accumulator_value"], dtype=np.float32)
    rest = np.setdiff1d(np.arange(ROWS), LISTED)
    for step in (1, 2, 3):
        g = _gradient(rng, (LISTED.size, dim))
        w1, s1 = R.adagrad_step(w, LISTED, g, s, step, HYPER, dtype, rowwise=True)
        g64 = g.astype(np.float64)
        s64 = s[LISTED].astype(np.float64) + (g64 * g64).sum(axis=1) / dim
        delta = -(HYPER["lr"] / (1 + (step - 1) * HYPER["lr_decay"])) / (np.sqrt(s64) + HYPER["eps"])[:, None] * g64
        w64 = w[LISTED].astype(np.float64) + delta
        assert (np.abs(s1[LISTED] - s64) <= (dim + 3) * EPS32 * s64).all()
        bound = ((dim + 3) / 2 + 5) * EPS32 * np.abs(delta) + EPS32 * np.abs(w64)
        if dtype != "fp32":
            e = np.floor(np.log2(np.maximum(np.abs(w64) + bound, 1e-300)))       # half an ulp of the table dtype at the result
            bound = bound + 2.0 ** (e - 8 if dtype == "bf16" else np.maximum(e, -14) - 11)
        err = np.abs(w1[LISTED].astype(np.float64) - w64)
        assert (err <= bound).all(), float((err / bound).max())
        assert np.array_equal(w1[rest], w[rest]) and np.array_equal(s1[rest], s[rest])    # rows that are not listed keep their bits
        w, s = w1, s1


def test_c_entry_refusals_without_a_gpu():
    L = _lib.load()

    def adagrad(opt=(-0.01, 1e-10, 0, 0, 1), T=1, U=8, max_dim=8, ptr=8, dtype=_lib.PM_F32):
        o = _lib.pm_sparse_adagrad(*opt, 0) if opt else None
        return L.pm_sparse_rows_adagrad(T, U, max_dim, ptr, dtype, ptr, ptr, ptr, ptr, ptr, ctypes.byref(o) if o else None, None)

    def sgd(opt=(-0.01, 0, 1), T=1, U=8, max_dim=8, ptr=8, dtype=_lib.PM_F32):
        return L.pm_sparse_rows_sgd(T, U, max_dim, ptr, dtype, ptr, ptr, ptr, ptr, *opt, None)

    assert adagrad(opt=None) == _lib.PM_ERR_INVALID and b"opt is NULL" in L.pm_last_error()
    for call, flags, inf in ((adagrad, (-0.01, 1e-10, 2, 0, 1), (-0.01, float("inf"), 0, 0, 1)), (sgd, (-0.01, 0, 2), (float("nan"), 0, 1))):
        assert call(ptr=None) == _lib.PM_ERR_INVALID and b"NULL" in L.pm_last_error()
        assert call(dtype=7) == _lib.PM_ERR_INVALID and b"table_dtype" in L.pm_last_error()
        for max_dim in (6, 4100):
            assert call(max_dim=max_dim) == _lib.PM_ERR_UNSUPPORTED and b"multiple of 4" in L.pm_last_error()
        assert call(opt=flags) == _lib.PM_ERR_INVALID and b"0 or 1" in L.pm_last_error()
        assert call(opt=inf) == _lib.PM_ERR_INVALID and b"finite" in L.pm_last_error()
        assert call(U=-1) == _lib.PM_ERR_INVALID
        assert call(U=0, ptr=None) == _lib.PM_OK and call(T=0, ptr=None) == _lib.PM_OK


def test_constructor_checks_and_state_keys():
    p = torch.nn.Parameter(torch.zeros(ROWS, DIM))
    with pytest.raises(ValueError, match="Invalid learning rate: -1.0"):
        SparseAdagradMI355([p], lr=-1.0)
    with pytest.raises(ValueError, match="Invalid lr_decay value: -0.5"):
        SparseAdagradMI355([p], lr_decay=-0.5)
    with pytest.raises(ValueError, match="Invalid learning rate: -1.0"):
        SparseSGDMI355([p], lr=-1.0)
    ref, ours = torch.optim.Adagrad([p], initial_accumulator_value=0.5), SparseAdagradMI355([p], initial_accumulator_value=0.5)
    assert set(ours.state[p]) == set(ref.state[p]) == {"step", "sum"} and torch.equal(ours.state[p]["sum"], ref.state[p]["sum"])
    assert tuple(SparseAdagradMI355([p], rowwise=True).state[p]["sum"].shape) == (ROWS,)
    assert SparseSGDMI355([p], lr=0.1).state_dict()["state"] == {}


@pytest.mark.parametrize("rule", ["adagrad", "sgd"])
def test_state_dict_moves_both_ways_and_torch_steps_on_ours(rule):
    """load_state_dict replaces the param groups with the saved ones: ours loaded from torch's must still resolve its own options, and
    torch's loaded from ours must find every key its step reads (the GPU direction: tests/test_gpu_sparse_step.py)"""
    p = torch.nn.Parameter(torch.zeros(ROWS, DIM))
    make = ((lambda c: c([p], lr=0.5)) if rule == "sgd" else (lambda c: c([p], lr=0.5, lr_decay=0.1, initial_accumulator_value=0.5)))
    ours, ref = make(SparseSGDMI355 if rule == "sgd" else SparseAdagradMI355), make(torch.optim.SGD if rule == "sgd" else torch.optim.Adagrad)
    ours.load_state_dict(ref.state_dict())
    assert ours.param_groups[0]["maximize"] is False and ours.param_groups[0].get("rowwise", False) is False
    p.grad = torch.ones(ROWS, DIM)
    with pytest.raises(RuntimeError, match="does not support dense gradients"):       # step() reads the loaded group without a KeyError
        ours.step()
    assert rule == "sgd" or int(ours.state[p]["step"]) == 0                            # a refused step leaves the state as it was
    ref.load_state_dict(ours.state_dict())
    g = np.full((LISTED.size, DIM), 2.0, dtype=np.float32)
    p.grad = torch.sparse_coo_tensor(torch.from_numpy(LISTED)[None], torch.from_numpy(g), (ROWS, DIM)).coalesce()
    ref.step()
    hyper = {"lr": 0.5, "lr_decay": 0.1, "eps": 1e-10}
    w = np.zeros((ROWS, DIM), dtype=np.float32)
    want = R.sgd_step(w, LISTED, g, hyper) if rule == "sgd" else R.adagrad_step(w, LISTED, g, np.full_like(w, 0.5), 1, hyper)[0]
    assert np.array_equal(_bits(p.detach().numpy()), _bits(want))
    bad = ref.state_dict()
    bad["param_groups"][0]["weight_decay"] = 0.1
    ours.load_state_dict(bad)
    with pytest.raises(RuntimeError, match="weight_decay"):
        ours.step()
