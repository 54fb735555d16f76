"""Fused exact element-wise Adagrad, the parts that need no GPU: the two C entry points are declared, bound and exported; their
host-side validation answers before any HIP call; the operator plug-in maps ``"exact_adagrad"``; and the numpy restatement the GPU
tests hold the kernels to (tests/elem_adagrad_rules.py) is pinned to the live ``torch.optim.Adagrad`` on the CPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from param_amd import _lib
from tests import elem_adagrad_rules as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pm_embbag_bwd_sorted_adagrad_elem", "pm_embbag_bwd_fused_adagrad_elem")


def test_header_declares_and_both_libraries_export_the_two_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "param_amd.h")).read(), flags=re.S)
    product = re.sub(r"#ifdef PM_ALTERNATES.*?#endif", "", src, flags=re.S)
    L, A = _lib.load(), _lib.load_alternates()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", product), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(L, name) and hasattr(A, name), name
    # the ABI version did not move: a client that needs the new calls finds out at symbol resolution
    assert L.pm_abi_version() == 8 and A.pm_abi_version() == 8 and _lib.PM_ABI_VERSION == 8
    assert ctypes.sizeof(_lib.pm_embbag_batch) == 144
    # the options struct serves both flavours and says so
    assert re.search(r"BOTH fused Adagrad flavours", open(os.path.join(ROOT, "include", "param_amd.h")).read())


def _request(T=1, max_dim=8):
    op = _lib.pm_embbag_batch()
    op.num_tables, op.weight_dtype, op.index_dtype, op.max_dim = T, _lib.PM_F32, _lib.PM_I64, max_dim
    op.tables = op.rows = op.dims = op.out_offsets = 8      # non-null dummies, never dereferenced on the host
    op.batch, op.bag_begin, op.bag_count, op.num_indices, op.indices, op.offsets = 4, 0, 4, 100, 8, 8
    return op


@pytest.mark.parametrize("which", NEW)
def test_argument_validation_without_gpu(which):
    """Host-side validation paths return error codes before any HIP call (a valid-looking pointer is never dereferenced on the host)."""
    L = _lib.load()
    fn = getattr(L, which)
    fused = "fused" in which
    good = _lib.pm_rowwise_adagrad(0.01, 1e-8, 0.0, _lib.PM_WD_NONE, 0, 0, 0)
    big = 1 << 40
    call = lambda op, state=8, opt=good, ws=8, ws_bytes=big, dtype=_lib.PM_F32: fn(          # noqa: E731
        ctypes.byref(op), 8, 8, dtype, state, None if opt is None else ctypes.byref(opt), 1000, ws, ws_bytes, None)
    op = _request()
    # NULL state
    assert call(op, state=None) == _lib.PM_ERR_INVALID
    assert b"state" in L.pm_last_error()
    # NULL options, unknown weight-decay mode
    assert call(op, opt=None) == _lib.PM_ERR_INVALID
    assert b"options" in L.pm_last_error()
    bad = _lib.pm_rowwise_adagrad(0.01, 1e-8, 0.0, 7, 0, 0, 0)
    assert call(op, opt=bad) == _lib.PM_ERR_INVALID
    assert b"weight_decay_mode" in L.pm_last_error()
    # NULL / short workspace
    assert call(op, ws=None, ws_bytes=0) == _lib.PM_ERR_INVALID
    assert b"workspace" in L.pm_last_error()
    assert call(op, ws=8, ws_bytes=16) == _lib.PM_ERR_INVALID
    assert b"workspace" in L.pm_last_error()
    # the width limit: one column pass, 64 lanes x 4 (fp32) / 8 (16-bit) columns
    for dtype, lim in ((_lib.PM_F32, 256), (_lib.PM_BF16, 512), (_lib.PM_F16, 512)):
        wide = _request(max_dim=lim + 8)
        wide.weight_dtype = dtype
        assert call(wide, dtype=dtype) == _lib.PM_ERR_UNSUPPORTED, (dtype, lim)
        assert b"element-wise Adagrad needs max_dim <= " + str(lim).encode() in L.pm_last_error()
    # more than 1024 tables in one call
    assert call(_request(T=1025)) == _lib.PM_ERR_UNSUPPORTED
    assert b"1024 tables" in L.pm_last_error()
    # an empty request has nothing to launch: PM_OK without a device, whatever else is missing
    empty = _request()
    empty.num_indices = 0
    assert call(empty, state=None, ws=None, ws_bytes=0) == _lib.PM_OK
    if fused:      # the fused call validates what its APPLY half needs before the sort half could launch anything
        assert fn(ctypes.byref(op), None, 8, _lib.PM_F32, 8, ctypes.byref(good), 1000, 8, big, None) == _lib.PM_ERR_INVALID
        assert b"grad" in L.pm_last_error()
        assert fn(ctypes.byref(op), 8, 8, 7, 8, ctypes.byref(good), 1000, 8, big, None) == _lib.PM_ERR_INVALID
        assert b"dtype" in L.pm_last_error()
    # the row-wise calls still name their own argument
    assert L.pm_embbag_bwd_fused_adagrad(ctypes.byref(op), 8, 8, _lib.PM_F32, None, ctypes.byref(good), 1000, 8, big, None) == _lib.PM_ERR_INVALID
    assert b"momentum" in L.pm_last_error()


def test_operator_name_mapping_needs_no_device():
    from param_amd.compute.python.split_table_batched_embeddings_ops import optimizer_name

    class OptimType:                      # fbgemm's spelling: an enum member whose value is the name
        class _M:
            def __init__(self, v):
                self.value = v

            def __str__(self):
                return "OptimType." + self.value.upper()
        EXACT_ADAGRAD, EXACT_ROWWISE_ADAGRAD, EXACT_SGD = _M("exact_adagrad"), _M("exact_row_wise_adagrad"), _M("exact_sgd")

    for name in ("exact_adagrad", "EXACT_ADAGRAD", "adagrad", "OptimType.EXACT_ADAGRAD", OptimType.EXACT_ADAGRAD):
        assert optimizer_name(name) == "adagrad", name
    for name in ("sgd", "exact_sgd", OptimType.EXACT_SGD):
        assert optimizer_name(name) == "sgd", name
    for name in ("exact_row_wise_adagrad", "exact_rowwise_adagrad", "rowwise_adagrad", "row_wise_adagrad", OptimType.EXACT_ROWWISE_ADAGRAD):
        assert optimizer_name(name) == "rowwise_adagrad", name
    for name in ("adam", "lamb", "partial_rowwise_adam", "exact_adagrad_v2", ""):
        with pytest.raises(ValueError):
            optimizer_name(name)


def test_module_accepts_the_new_optimizer_name_and_refuses_unknown_ones():
    """constructor checks only (CPU tensors; nothing is launched)"""
    from param_amd import BatchedEmbeddingBagMI355

    m = BatchedEmbeddingBagMI355([10, 20], [8, 16], device="cpu", init=None, optimizer="adagrad")
    assert m.optimizer == "adagrad" and m.momentum is None
    assert tuple(m.momentum_table(1).shape) == (20, 16) and tuple(m.momentum_table(0).shape) == (10, 8)
    assert m.momentum.numel() == 10 * 8 + 20 * 16 and m.momentum.dtype.is_floating_point and float(m.momentum.abs().sum()) == 0.0
    assert "momentum" in m.state_dict()
    r = BatchedEmbeddingBagMI355([10, 20], [8, 16], device="cpu", init=None, optimizer="rowwise_adagrad")
    assert tuple(r.momentum_table(1).shape) == (20,) and r.momentum.numel() == 30
    with pytest.raises(ValueError):
        BatchedEmbeddingBagMI355([10], [8], device="cpu", init=None, optimizer="adam")


def _zipf_request(rng, rows, B, L):
    """table-major TBE request with Zipf(1.4) duplicates; the last five rows of every table are never hit"""
    idx = np.concatenate([np.minimum(rng.zipf(1.4, B * L) - 1, r - 6).astype(np.int64) for r in rows])
    off = np.arange(len(rows) * B + 1, dtype=np.int64) * L
    return idx, off


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_restatement_is_pinned_to_torch_adagrad(wd):
    """Three steps, two tables of different widths, general (unequal) columns and gradients, Zipf duplicates (up to ~100 hits
    per row), some rows never hit.  torch.optim.Adagrad (initial_accumulator_value = 0, lr_decay = 0) is fed the TOUCHED rows
    only, its state injected through ``opt.state[p]["sum"]``, so that L2 decay reaches touched rows only, as a fused sparse
    update does.  Bars: state rtol 1e-6, weights rtol 2e-6 / atol 1e-7 (the existing torch pin's)."""
    import torch

    rng = np.random.default_rng(5)
    rows, dims, B, L, lr, eps = [300, 50], [16, 64], 64, 5, 0.05, 1e-6
    code = E.WD_L2 if wd else E.WD_NONE
    W = [rng.standard_normal((r, d)).astype(np.float32) for r, d in zip(rows, dims)]
    W0 = [w.copy() for w in W]
    S = [np.zeros_like(w) for w in W]
    Wt, St = [w.copy() for w in W], [np.zeros_like(w) for w in W]
    most = 0
    for step in range(3):
        idx, off = _zipf_request(rng, rows, B, L)
        for t, (r, d) in enumerate(zip(rows, dims)):
            g = rng.standard_normal((B, d)).astype(np.float32)
            ti, to = idx[off[t * B]:off[(t + 1) * B]], off[t * B:(t + 1) * B] - off[t * B]
            G, count = E.grad_sum_f32(r, ti, to, g)
            most = max(most, int(count.max()))
            assert count[-5:].sum() == 0 and (count == 0).sum() > 5
            W[t], S[t] = E.step_f32(W[t], S[t], G, count > 0, lr, eps, wd, code)
            hit = np.nonzero(count)[0]
            p = torch.nn.Parameter(torch.from_numpy(Wt[t][hit].copy()))
            opt = torch.optim.Adagrad([p], lr=lr, eps=eps, initial_accumulator_value=0.0, lr_decay=0.0, weight_decay=wd)
            opt.state[p]["sum"] = torch.from_numpy(St[t][hit].copy())
            p.grad = torch.from_numpy(G[hit].copy())
            opt.step()
            Wt[t][hit], St[t][hit] = p.detach().numpy(), opt.state[p]["sum"].numpy()
    assert most >= 30                                       # real duplicates
    for t in range(2):
        ds = np.abs(S[t] - St[t]) / np.maximum(np.abs(St[t]), 1e-30)
        dw = np.abs(W[t] - Wt[t]) / (E.W_RTOL * np.abs(Wt[t]) + E.W_ATOL)
        print(f"wd={wd} table {t}: state max rel diff {ds.max():.3g} (bar {E.STATE_RTOL}), weights max diff / bar {dw.max():.3g}")
        assert np.allclose(S[t], St[t], rtol=E.STATE_RTOL, atol=0), t
        assert np.allclose(W[t], Wt[t], rtol=E.W_RTOL, atol=E.W_ATOL), t
        assert np.array_equal(W[t][-5:], W0[t][-5:]) and not S[t][-5:].any()
        assert (np.abs(W[t] - W0[t]) > 0).any()


def test_fp64_restatement_agrees_with_the_fp32_one_and_bounds_reordered_sums():
    """``step_fp64`` is the same update in fp64 (within the fp32 bars of ``step_f32``), and its bound covers a gradient sum formed
    in another order: here the worst the rule allows, every |contribution| moved by 1e-5 of itself, either way."""
    rng = np.random.default_rng(9)
    r, d, B, L, lr, eps = 40, 16, 32, 6, 0.05, 1e-6
    idx = rng.integers(0, r - 3, B * L)
    off = np.arange(B, dtype=np.int64) * L
    g = rng.standard_normal((B, d)).astype(np.float32)
    psw = rng.uniform(0.5, 1.5, B * L).astype(np.float32)
    w, s = rng.standard_normal((r, d)).astype(np.float32), rng.uniform(0.0, 2.0, (r, d)).astype(np.float32)
    for code, wd in ((E.WD_NONE, 0.0), (E.WD_L2, 0.01), (E.WD_DECOUPLE, 0.01)):
        G, count = E.grad_sum_f32(r, idx, off, g, psw)
        w32, s32 = E.step_f32(w, s, G, count > 0, lr, eps, wd, code)
        W64, S64, dw, ds, c64 = E.step_fp64(w, s, idx, off, g, psw, lr, eps, wd, code)
        assert np.array_equal(count, c64)
        assert np.allclose(s32, S64, rtol=4 * E.STATE_RTOL, atol=0) and np.allclose(w32, W64, rtol=4 * E.W_RTOL, atol=4 * E.W_ATOL)
        assert np.array_equal(w32[count == 0], w[count == 0]) and np.array_equal(s32[count == 0], s[count == 0])
        # the same step from a perturbed sum stays inside the bound (slack: fp64 rounding of the evaluation itself)
        for sign in (1.0, -1.0):
            W2, S2, _, _, _ = E.step_fp64(w, s, idx, off, g.astype(np.float64) * (1 + sign * 1e-5 * np.sign(g.astype(np.float64))), psw, lr, eps, wd, code)
            assert (np.abs(W2 - W64) <= dw * (1 + 1e-9) + 1e-15).all() and (np.abs(S2 - S64) <= ds * (1 + 1e-9) + 1e-13).all()
