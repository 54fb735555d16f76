"""The coalesced sparse gradient's argument checks (ABI v8: pm_embbag_sparse_grad_workspace / _count / pm_embbag_sparse_grad) and
the Python layer's shape and layout errors -- host-side paths that return before any HIP call, so no GPU is needed."""
import ctypes

import pytest
import torch

from param_amd import _lib

FAKE = 0x1000          # a non-NULL "device pointer": the checks below return before anything is dereferenced or launched


def _op(T=2, max_dim=64, dtype=_lib.PM_F32, n=100, batch=10):
    op = _lib.pm_embbag_batch()
    op.num_tables, op.weight_dtype, op.index_dtype, op.max_dim = T, dtype, _lib.PM_I64, max_dim
    op.batch, op.num_indices, op.bag_begin, op.bag_count = batch, n, 0, batch
    op.tables = op.rows = op.dims = op.out_offsets = FAKE
    op.indices = op.offsets = FAKE
    op.out_stride = T * max_dim
    return op


def _err(L):
    return L.pm_last_error().decode()


def test_abi_version_is_8():
    L = _lib.load()
    assert _lib.PM_ABI_VERSION == 8 and L.pm_abi_version() == 8
    for name in ("pm_embbag_sparse_grad_workspace", "pm_embbag_sparse_grad_count", "pm_embbag_sparse_grad"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)


def test_workspace_covers_the_sorted_backwards():
    L = _lib.load()
    for T, n in ((1, 1), (2, 100), (48, 48 * 8192 * 20), (1024, 5000)):
        op = _op(T=T, n=n)
        sorted_ws = L.pm_embbag_bwd_sorted_workspace(ctypes.byref(op), 10_000_000)
        sparse_ws = L.pm_embbag_sparse_grad_workspace(ctypes.byref(op), 10_000_000)
        assert sorted_ws > 0 and sparse_ws >= sorted_ws + 4 * n, (T, n, sorted_ws, sparse_ws)


def test_null_and_bad_arguments_are_refused():
    L = _lib.load()
    s = None
    assert L.pm_embbag_sparse_grad_workspace(None, 100) == _lib.PM_ERR_INVALID
    assert L.pm_embbag_sparse_grad_count(None, 100, FAKE, 1 << 40, FAKE, s) == _lib.PM_ERR_INVALID
    assert L.pm_embbag_sparse_grad(None, FAKE, 100, FAKE, 1 << 40, FAKE, FAKE, s) == _lib.PM_ERR_INVALID
    op = _op()
    assert L.pm_embbag_sparse_grad_workspace(ctypes.byref(op), 0) == _lib.PM_ERR_INVALID          # max_rows
    assert L.pm_embbag_sparse_grad_count(ctypes.byref(op), 100, FAKE, 1 << 40, None, s) == _lib.PM_ERR_INVALID
    assert "unique_counts" in _err(L)
    assert L.pm_embbag_sparse_grad(ctypes.byref(op), None, 100, FAKE, 1 << 40, FAKE, FAKE, s) == _lib.PM_ERR_INVALID
    assert L.pm_embbag_sparse_grad(ctypes.byref(op), FAKE, 100, FAKE, 1 << 40, None, FAKE, s) == _lib.PM_ERR_INVALID
    assert L.pm_embbag_sparse_grad(ctypes.byref(op), FAKE, 100, FAKE, 1 << 40, FAKE, None, s) == _lib.PM_ERR_INVALID
    # workspace too small / NULL
    assert L.pm_embbag_sparse_grad_count(ctypes.byref(op), 100, FAKE, 16, FAKE, s) == _lib.PM_ERR_INVALID
    assert "workspace too small" in _err(L)
    assert L.pm_embbag_sparse_grad(ctypes.byref(op), FAKE, 100, None, 1 << 40, FAKE, FAKE, s) == _lib.PM_ERR_INVALID
    # mismatched request: bag slice outside the batch, bad index dtype, bad table dtype
    bad = _op()
    bad.bag_begin, bad.bag_count = 5, 10
    assert L.pm_embbag_sparse_grad_workspace(ctypes.byref(bad), 100) == _lib.PM_ERR_INVALID
    bad = _op()
    bad.index_dtype = _lib.PM_F32
    assert L.pm_embbag_sparse_grad_count(ctypes.byref(bad), 100, FAKE, 1 << 40, FAKE, s) == _lib.PM_ERR_INVALID
    bad = _op(dtype=7)
    assert L.pm_embbag_sparse_grad(ctypes.byref(bad), FAKE, 100, FAKE, 1 << 40, FAKE, FAKE, s) == _lib.PM_ERR_INVALID


def test_count_and_apply_need_a_sort_of_the_request_on_the_workspace():
    """No sort was recorded for this workspace address: refused on the host, nothing launched."""
    L = _lib.load()
    op = _op()
    assert L.pm_embbag_sparse_grad_count(ctypes.byref(op), 100, FAKE, 1 << 40, FAKE, None) == _lib.PM_ERR_INVALID
    assert "pm_embbag_sort_indices has not been called" in _err(L)
    assert L.pm_embbag_sparse_grad(ctypes.byref(op), FAKE, 100, FAKE, 1 << 40, FAKE, FAKE, None) == _lib.PM_ERR_INVALID


def test_limits_of_the_sorted_path_are_inherited():
    L = _lib.load()
    s = None
    op = _op(T=1025, n=10250)
    for rc in (L.pm_embbag_sparse_grad_workspace(ctypes.byref(op), 100),
               L.pm_embbag_sparse_grad_count(ctypes.byref(op), 100, FAKE, 1 << 40, FAKE, s),
               L.pm_embbag_sparse_grad(ctypes.byref(op), FAKE, 100, FAKE, 1 << 40, FAKE, FAKE, s)):
        assert rc == _lib.PM_ERR_UNSUPPORTED
        assert "1024 tables" in _err(L)
    op = _op(n=1 << 32)
    assert L.pm_embbag_sparse_grad_workspace(ctypes.byref(op), 100) == _lib.PM_ERR_UNSUPPORTED
    op = _op(batch=1 << 32, n=100)
    assert L.pm_embbag_sparse_grad_workspace(ctypes.byref(op), 100) == _lib.PM_ERR_UNSUPPORTED
    # max_dim: a multiple of 4 (the fp32 value rows) -- and of 8 for 16-bit tables, as everywhere
    for dt, dim in ((_lib.PM_F32, 6), (_lib.PM_F32, 0), (_lib.PM_BF16, 12), (_lib.PM_F16, 4)):
        op = _op(max_dim=dim, dtype=dt)
        assert L.pm_embbag_sparse_grad_workspace(ctypes.byref(op), 100) == _lib.PM_ERR_UNSUPPORTED, (dt, dim)
        assert L.pm_embbag_sparse_grad_count(ctypes.byref(op), 100, FAKE, 1 << 40, FAKE, s) == _lib.PM_ERR_UNSUPPORTED
        assert L.pm_embbag_sparse_grad(ctypes.byref(op), FAKE, 100, FAKE, 1 << 40, FAKE, FAKE, s) == _lib.PM_ERR_UNSUPPORTED
    for dt, dim in ((_lib.PM_F32, 4), (_lib.PM_F32, 1024), (_lib.PM_BF16, 8), (_lib.PM_F16, 512)):
        assert L.pm_embbag_sparse_grad_workspace(ctypes.byref(_op(max_dim=dim, dtype=dt)), 100) > 0, (dt, dim)


def test_python_layer_refuses_cpu_tensors():
    import param_amd

    m = param_amd.BatchedEmbeddingBagMI355([10, 20], 8, device="cpu", init=None)
    with pytest.raises(RuntimeError, match="ROCm device"):
        m.sparse_grad(torch.zeros(2, 16), torch.tensor([1, 2]), torch.tensor([0, 1, 1, 2]), batch=2)


@pytest.fixture
def no_device_check(monkeypatch):
    """lets the host-side argument checks of the Python layer run on CPU tensors (they come before any library call)"""
    from param_amd import embedding_bag

    monkeypatch.setattr(embedding_bag, "_require_device", lambda t, what: None)


def test_python_layer_checks_grad_shape_and_dtype(no_device_check):
    import param_amd

    idx, off = torch.tensor([1, 2, 3, 4]), torch.tensor([0, 1, 2, 3])
    m = param_amd.BatchedEmbeddingBagMI355([10, 20], [8, 16], device="cpu", init=None)
    for g in (torch.zeros(2, 16), torch.zeros(2, 24, dtype=torch.bfloat16), torch.zeros(3, 24), torch.zeros(2, 2, 8)):
        with pytest.raises(ValueError, match="grad must be float32 of shape"):
            m.sparse_grad(g, idx, off, batch=2)
    t = param_amd.BatchedEmbeddingBagMI355([10, 20], 8, device="cpu", init=None, layout="tbd")
    with pytest.raises(ValueError, match=r"shape \(2, 2, 8\)"):
        t.sparse_grad(torch.zeros(2, 16), idx, off, batch=2)
    b = param_amd.BatchedEmbeddingBagMI355([10, 20], 8, device="cpu", init=None, layout="blocked", block_bags=2)
    with pytest.raises(ValueError, match=r"shape \(1, 2, 2, 8\)"):
        b.sparse_grad(torch.zeros(2, 16), idx, off, batch=2)


def test_python_layer_checks_layout_and_request(no_device_check):
    import param_amd

    # "tbd" / "blocked" need one common dim; "blocked" needs a power-of-two block of bags that divides the batch
    with pytest.raises(ValueError, match="one common embedding dim"):
        param_amd.BatchedEmbeddingBagMI355([10, 20], [8, 16], device="cpu", init=None, layout="tbd").sparse_grad(
            torch.zeros(2, 2, 8), torch.tensor([1, 2]), torch.tensor([0, 1, 1, 2]), batch=2)
    b = param_amd.BatchedEmbeddingBagMI355([10, 20], 8, device="cpu", init=None, layout="blocked", block_bags=4)
    with pytest.raises(ValueError, match="not a multiple of block_bags"):
        b.sparse_grad(torch.zeros(2, 16), torch.tensor([1, 2]), torch.tensor([0, 1, 1, 2]), batch=2)
    m = param_amd.BatchedEmbeddingBagMI355([10, 20], 8, device="cpu", init=None)
    with pytest.raises(TypeError, match="int64 or both int32"):
        m.sparse_grad(torch.zeros(2, 16), torch.tensor([1, 2], dtype=torch.int32), torch.tensor([0, 1, 1, 2]), batch=2)
    with pytest.raises(ValueError, match="offsets has"):
        m.sparse_grad(torch.zeros(2, 16), torch.tensor([1, 2]), torch.tensor([0, 1, 1]), batch=2)
