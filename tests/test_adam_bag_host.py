"""AdamBatchedEmbeddingBagMI355 without a GPU: constructor checks and state keys, the C entry's refusals and empty request, the two
exported symbols, and the numpy restatement (tests/adam_bag_rules.py) against torch.optim.SparseAdam on the CPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from param_amd import AdamBatchedEmbeddingBagMI355, BatchedEmbeddingBagMI355, _lib
from tests import adam_bag_rules as R
from tests.test_sparse_adam_host import _bound      # the torch comparison's bound, reused


def test_constructor_checks_and_state():
    kw = dict(device="cpu", init=None)
    m = AdamBatchedEmbeddingBagMI355([10, 20], [8, 16], **kw)
    assert m.optimizer == "adam" and int(m.step) == 0 and m.step.dtype == torch.int64 and isinstance(m, BatchedEmbeddingBagMI355)
    assert tuple(m.exp_avg_table(1).shape) == tuple(m.exp_avg_sq_table(1).shape) == (20, 16) and tuple(m.exp_avg_table(0).shape) == (10, 8)
    assert m.exp_avg.dtype == m.exp_avg_sq.dtype == torch.float32 and m.exp_avg.numel() == m.exp_avg_sq.numel() == 10 * 8 + 20 * 16
    assert {"exp_avg", "exp_avg_sq", "step"} <= set(m.state_dict()) and "momentum" not in m.state_dict()
    assert AdamBatchedEmbeddingBagMI355([10], [8], dtype=torch.bfloat16, **kw).exp_avg.dtype == torch.float32      # the state is always fp32
    for bad in (dict(optimizer="adagrad"), dict(layout="blocked", block_bags=2), dict(stochastic_rounding=True), dict(weight_decay_mode="l2"),
                dict(betas=(0.9, 1.0)), dict(learning_rate=0.0)):
        with pytest.raises(ValueError):
            AdamBatchedEmbeddingBagMI355([10, 20], [8, 8], **kw, **bad)
    with pytest.raises(ValueError, match="1024 tables"):
        AdamBatchedEmbeddingBagMI355([4] * 1025, 8, **kw)
    with pytest.raises(ValueError, match="multiple of 8"):
        AdamBatchedEmbeddingBagMI355([10], [12], dtype=torch.float16, **kw)
    with pytest.raises(ValueError):      # the parent still refuses the name
        BatchedEmbeddingBagMI355([10], [8], optimizer="adam", **kw)
    idx, off = torch.zeros(4, dtype=torch.int64), torch.arange(5, dtype=torch.int64)
    for call in (lambda: m.adagrad_step_(None, idx, off), lambda: m.sequence_optimizer_step_(None, idx, off),
                 lambda: m.optimizer_step_(None, idx, off, per_sample_weights=torch.ones(4)), lambda: m(idx, off, torch.ones(4)),
                 lambda: m.forward_sequence(idx, off)):
        with pytest.raises(ValueError, match="lazy Adam"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.optimizer_step_(torch.zeros(2, 24), idx, off)
    assert int(m.step) == 0      # a refused call does not count


def _op(**kw):
    op = _lib.pm_embbag_batch()
    op.num_tables, op.weight_dtype, op.index_dtype, op.max_dim, op.batch, op.bag_count, op.num_indices, op.out_stride = 1, _lib.PM_F32, _lib.PM_I64, 8, 4, 4, 100, 8
    op.tables = op.rows = op.dims = op.out_offsets = op.indices = op.offsets = 16      # non-null dummies, never dereferenced on the host
    for k, v in kw.items():
        setattr(op, k, v)
    return op


@pytest.mark.parametrize("load", [_lib.load, _lib.load_alternates])
def test_c_entry_refusals_and_empty_request_without_a_gpu(load):
    L = load()
    assert hasattr(L, "pm_embbag_bwd_adam") and hasattr(L, "pm_embbag_bwd_adam_workspace")
    good = _lib.pm_sparse_adam(0.1, 0.001, 1e-8, 1e-3, 1.0, 0, 1, 0)

    def call(op, opt=good, grad=16, gd=_lib.PM_F32, td=_lib.PM_F32, state=16, ws=16, ws_bytes=1 << 40, max_rows=1000):
        return L.pm_embbag_bwd_adam(ctypes.byref(op) if op else None, grad, gd, 16, td, state, state, None, ctypes.byref(opt) if opt else None,
                                    max_rows, ws, ws_bytes, None)
    U, I = _lib.PM_ERR_UNSUPPORTED, _lib.PM_ERR_INVALID
    assert call(None) == I
    assert call(_op(per_sample_weights=16)) == U and b"per_sample_weights" in L.pm_last_error()
    assert call(_op(grad_block_shift=1, grad_block_extra=64, batch=4)) == U and b"blocked" in L.pm_last_error()
    assert call(_op(num_indices=1 << 32)) == U and b"2^32" in L.pm_last_error()
    assert call(_op(num_tables=1025)) == U
    assert L.pm_embbag_bwd_adam_workspace(ctypes.byref(_op(num_tables=1025)), 1000) == U
    assert call(_op(), gd=7) == I and b"grad_dtype" in L.pm_last_error()
    assert call(_op(), td=7) == I
    assert call(_op(max_dim=6)) == U and b"multiple of 4" in L.pm_last_error()
    assert call(_op(), max_rows=0) == I
    assert call(_op(), opt=None) == I and b"opt is NULL" in L.pm_last_error()
    assert call(_op(), opt=_lib.pm_sparse_adam(0.1, 0.001, 1e-8, float("nan"), 1.0, 0, 1, 0)) == I and b"finite" in L.pm_last_error()
    assert call(_op(), opt=_lib.pm_sparse_adam(0.1, 0.001, 1e-8, 1e-3, 1.0, 2, 1, 0)) == I and b"maximize" in L.pm_last_error()
    assert call(_op(), state=None) == I and b"exp_avg" in L.pm_last_error()
    assert call(_op(), grad=None) == I
    assert call(_op(), grad=8) == I and b"aligned" in L.pm_last_error()
    assert call(_op(), ws=None, ws_bytes=0) == I and b"workspace" in L.pm_last_error()
    # an empty request: PM_OK without a device, whatever the pointers
    assert call(_op(num_indices=0), grad=None, state=None, ws=None, ws_bytes=0) == _lib.PM_OK
    assert call(_op(bag_count=0), grad=None, state=None, ws=None, ws_bytes=0) == _lib.PM_OK


def test_rules_agree_with_torch_sparse_adam():
    """one table, no row looked up twice: G is the bag's gradient, and one step of the rule is torch.optim.SparseAdam's within the bound
    tests/test_sparse_adam_host.py holds both to (against the formulas in fp64)"""
    rng = np.random.default_rng(3)
    rows, D, B = 40, 8, 6
    hyper = {"lr": 1.0e-2, "betas": (0.9, 0.999), "eps": 1.0e-8, "weight_decay": 0.0}
    idx = rng.permutation(rows)[:17].astype(np.int64)
    off = np.array([0, 3, 3, 8, 9, 15, 17], np.int64)
    g = rng.standard_normal((B, D)).astype(np.float32)
    w = rng.standard_normal((rows, D)).astype(np.float32)
    (ids, G), = R.summed_grads([D], idx, off, B, [g])
    assert np.array_equal(ids, np.sort(idx)) and np.array_equal(G, g[np.searchsorted(off, np.argsort(idx), side="right") - 1])
    (w1, m1, v1), = R.step([(w, np.zeros_like(w), np.zeros_like(w))], [(ids, G)], 1, hyper)
    p = torch.nn.Parameter(torch.from_numpy(w.copy()))
    opt = torch.optim.SparseAdam([p], lr=hyper["lr"], betas=hyper["betas"], eps=hyper["eps"])
    p.grad = torch.sparse_coo_tensor(torch.from_numpy(ids)[None], torch.from_numpy(G), (rows, D)).coalesce()
    opt.step()
    g64 = G.astype(np.float64)
    delta = hyper["lr"] * math.sqrt(1 - 0.999) / (1 - 0.9) * (g64 * 0.1 / (np.sqrt(g64 * g64 * 0.001) + hyper["eps"]))
    w64 = w[ids].astype(np.float64) - delta
    for got in (w1, p.data.numpy()):
        assert (np.abs(got[ids].astype(np.float64) - w64) <= _bound(w64, delta, "fp32")).all()
    rest = np.setdiff1d(np.arange(rows), ids)
    assert np.array_equal(w1[rest], w[rest]) and not m1[rest].any() and not v1[rest].any()
