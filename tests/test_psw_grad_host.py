"""Gradient of per_sample_weights, the parts that need no GPU: ``pm_embbag_psw_grad`` is declared, bound and exported; its
host-side validation answers before any HIP call; and the numpy restatement the GPU tests hold the kernel to
(tests/psw_grad_rules.py) is pinned to live ``torch.nn.functional.embedding_bag(..., per_sample_weights=w)`` autograd on the CPU
and to the fp64 value, both within the derived bar."""
import ctypes
import os
import re

import numpy as np
import pytest

from param_amd import _lib
from tests import psw_grad_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pm_embbag_psw_grad"


def test_header_declares_and_both_libraries_export_the_symbol():
    text = open(os.path.join(ROOT, "include", "param_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    product = re.sub(r"#ifdef PM_ALTERNATES.*?#endif", "", src, flags=re.S)
    L, A = _lib.load(), _lib.load_alternates()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*const\s+pm_embbag_batch\s*\*\s*op\s*,\s*const\s+float\s*\*\s*grad\s*,\s*float\s*\*\s*out\s*,"
                     r"\s*pm_stream_t\s+stream\s*\)", product)
    assert NAME in _lib.EXPORTED_SYMBOLS
    assert hasattr(L, NAME) and hasattr(A, NAME)
    assert L.pm_abi_version() == 8 and A.pm_abi_version() == 8 and _lib.PM_ABI_VERSION == 8
    assert ctypes.sizeof(_lib.pm_embbag_batch) == 144
    # the header states the formula's reference sites
    assert "_embedding_bag_per_sample_weights_backward" in text and "indice_weights" in text
    assert "split_table_batched_embeddings_ops.py:318-324" in text


def _request(T=1, max_dim=8):
    op = _lib.pm_embbag_batch()
    op.num_tables, op.weight_dtype, op.index_dtype, op.max_dim = T, _lib.PM_F32, _lib.PM_I64, max_dim
    op.tables = op.rows = op.dims = op.out_offsets = 8      # non-null dummies, never dereferenced on the host
    op.batch, op.bag_begin, op.bag_count, op.num_indices, op.indices, op.offsets = 4, 0, 4, 100, 8, 8
    op.out_stride = max_dim
    return op


def test_argument_validation_without_gpu():
    """every refusal is made on the host, before any HIP call (the dummy pointers are never dereferenced)"""
    L = _lib.load()
    fn = L.pm_embbag_psw_grad
    call = lambda op, grad=8, out=8: fn(None if op is None else ctypes.byref(op), grad, out, None)      # noqa: E731
    # what make_params checks
    assert call(None) == _lib.PM_ERR_INVALID
    op = _request()
    op.index_dtype = 3
    assert call(op) == _lib.PM_ERR_INVALID and b"index_dtype" in L.pm_last_error()
    op = _request()
    op.bag_count = 5
    assert call(op) == _lib.PM_ERR_INVALID and b"bag_begin/bag_count" in L.pm_last_error()
    op = _request()
    op.offsets = None
    assert call(op) == _lib.PM_ERR_INVALID and b"offsets" in L.pm_last_error()
    op = _request(max_dim=6)
    assert call(op) == _lib.PM_ERR_UNSUPPORTED and b"multiple of 4" in L.pm_last_error()
    op = _request()
    op.weight_dtype = 7
    assert call(op) == _lib.PM_ERR_INVALID and b"dtype" in L.pm_last_error()
    # NULL grad / NULL out
    assert call(_request(), grad=None) == _lib.PM_ERR_INVALID
    assert b"grad" in L.pm_last_error()
    assert call(_request(), out=None) == _lib.PM_ERR_INVALID
    assert b"out" in L.pm_last_error()
    # the blocked-gradient rules, in pm_embbag_bwd_fused's words
    for mutate in (lambda o: setattr(o, "grad_block_extra", 64), lambda o: (setattr(o, "grad_block_shift", 3), setattr(o, "grad_block_extra", 64)),
                   lambda o: setattr(o, "grad_block_shift", 40)):
        op, twin = _request(), _request()
        mutate(op)
        mutate(twin)
        assert call(op) == _lib.PM_ERR_INVALID
        msg = L.pm_last_error()
        assert L.pm_embbag_bwd_fused(ctypes.byref(twin), 8, 8, _lib.PM_F32, 1.0, 1000, 8, 1 << 40, None) == _lib.PM_ERR_INVALID
        assert msg == L.pm_last_error() and msg
    # the width limit: 64 lanes x 4 (fp32) / 8 (16-bit) columns
    for dtype, lim in ((_lib.PM_F32, 256), (_lib.PM_BF16, 512), (_lib.PM_F16, 512)):
        wide = _request(max_dim=lim + 8)
        wide.weight_dtype = dtype
        assert call(wide) == _lib.PM_ERR_UNSUPPORTED, (dtype, lim)
        assert b"pm_embbag_psw_grad" in L.pm_last_error() and str(lim).encode() in L.pm_last_error()
    # an empty request has nothing to launch: PM_OK without a device (out may be NULL when there are no lookups)
    empty = _request()
    empty.num_indices = 0
    assert call(empty, out=None) == _lib.PM_OK
    empty = _request()
    empty.bag_count = 0
    assert call(empty) == _lib.PM_OK


def _ragged(rng, B, rows, lo=0, hi=5):
    """bag lengths lo .. hi with an empty first and an empty last bag"""
    lens = rng.integers(lo, hi + 1, B)
    lens[0] = lens[-1] = 0
    lens[B // 2] = hi
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rng.integers(0, rows, int(off[-1])).astype(np.int64), off


def _case(D, values="float32", seed=0, B=37, rows=61):
    rng = np.random.default_rng(1000 * D + seed)
    idx, off = _ragged(rng, B, rows)
    W = rng.standard_normal((rows, D)).astype(np.float32)
    if values == "bfloat16":
        W = R.to_bf16_values(W)
    elif values == "float16":
        W = R.to_fp16_values(W)
    g = rng.standard_normal((B, D)).astype(np.float32)
    return idx, off, W, g


@pytest.mark.parametrize("D", [4, 16, 64, 128, 256])
def test_restatement_is_pinned_to_torch_autograd_and_fp64(D):
    import torch
    import torch.nn.functional as F

    B = 37
    idx, off, W, g = _case(D)
    psw = torch.from_numpy(np.random.default_rng(D).standard_normal(idx.size).astype(np.float32)).requires_grad_(True)
    out = F.embedding_bag(torch.from_numpy(idx), torch.from_numpy(W), torch.from_numpy(off[:B]), mode="sum", per_sample_weights=psw)
    out.backward(torch.from_numpy(g))
    tg = psw.grad.numpy()
    mine, written, exact, bar = R.restate([W], idx, off, B, [g], 4)
    assert written.all() and idx.size > B                              # every lookup, none left out
    rt = np.abs(tg.astype(np.float64) - exact) / bar
    rm = np.abs(mine.astype(np.float64) - exact) / bar
    print(f"D={D}: n={idx.size} torch max |err| / bar {rt.max():.3g}, restatement {rm.max():.3g}")
    assert (rt <= 1.0).all() and (rm <= 1.0).all()
    # teeth: a result with one column dropped leaves the bar
    bags = R.lookups_of_request(off, 1, B, idx.size)[2]
    rd = np.abs(mine.astype(np.float64) - g[bags, D - 1].astype(np.float64) * W[idx, D - 1] - exact) / bar
    print(f"D={D}: one column dropped: median |err| / bar {np.median(rd):.3g}")
    assert np.median(rd) > 1.0


@pytest.mark.parametrize("values", ["bfloat16", "float16"])
@pytest.mark.parametrize("D", [8, 128, 512])
def test_restatement_of_16_bit_valued_tables_is_within_the_bar_of_fp64(D, values):
    B = 37
    idx, off, W, g = _case(D, values)
    mine, written, exact, bar = R.restate([W], idx, off, B, [g], 8)
    assert written.all()
    rm = np.abs(mine.astype(np.float64) - exact) / bar
    bags = R.lookups_of_request(off, 1, B, idx.size)[2]
    rd = np.abs(mine.astype(np.float64) - g[bags, D - 1].astype(np.float64) * W[idx, D - 1] - exact) / bar
    print(f"D={D} {values}: restatement max |err| / bar {rm.max():.3g}; one column dropped: median {np.median(rd):.3g}")
    assert (rm <= 1.0).all()
    assert np.median(rd) > 1.0


def test_value_does_not_depend_on_the_group_width():
    """x + 0 == x and a partial is never -0: padding the lanes to any wider power of two gives the same bits"""
    rng = np.random.default_rng(3)
    for D, V in ((4, 4), (16, 4), (24, 4), (64, 4), (8, 8), (40, 8)):
        G, W = rng.standard_normal((50, D)).astype(np.float32), rng.standard_normal((50, D)).astype(np.float32)
        W[:5] = -0.0
        a = R.dot_rule(G, W, V)
        for wide in (64 * V, 16 * V):
            if wide < D:
                continue
            Gp, Wp = np.zeros((50, wide), np.float32), np.zeros((50, wide), np.float32)
            Gp[:, :D], Wp[:, :D] = G, W
            assert R.same_bits(a, R.dot_rule(Gp, Wp, V)), (D, V, wide)
        assert not np.signbit(a[:5]).any()
