"""What the sorted apply entry points say about a workspace no sort was recorded for -- host-side refusals that return before any
HIP call, so no GPU is needed.  (The sparse-gradient calls are pinned the same way in test_sparse_grad_host.py.)"""
import ctypes

import pytest

from param_amd import _lib

FAKE = 0x1000          # a non-NULL "device pointer": the checks below return before anything is dereferenced or launched
BIG = 1 << 40          # bytes the "workspace" claims to have
MAX_ROWS = 1000


def _op(dtype=_lib.PM_F32):
    op = _lib.pm_embbag_batch()
    op.num_tables, op.weight_dtype, op.index_dtype, op.max_dim = 2, dtype, _lib.PM_I64, 64
    op.batch, op.num_indices, op.bag_begin, op.bag_count = 10, 100, 0, 10
    op.tables = op.rows = op.dims = op.out_offsets = FAKE
    op.indices = op.offsets = FAKE
    op.out_stride = 2 * 64
    return op


def _opt():
    return _lib.pm_rowwise_adagrad(0.01, 1.0e-8, 0.0, _lib.PM_WD_NONE, 0, 0, 0)


# name -> the call with every argument valid, on `workspace` of `nbytes` bytes (the request's table dtype is `dt`)
APPLIES = {
    "pm_embbag_bwd_sorted":
        lambda L, op, dt, ws, nbytes: L.pm_embbag_bwd_sorted(ctypes.byref(op), FAKE, FAKE, dt, 1.0, MAX_ROWS, ws, nbytes, None),
    "pm_embbag_bwd_sorted_adagrad":
        lambda L, op, dt, ws, nbytes: L.pm_embbag_bwd_sorted_adagrad(ctypes.byref(op), FAKE, FAKE, dt, FAKE, 0.01, 1.0e-8, MAX_ROWS, ws,
                                                                     nbytes, None),
    "pm_embbag_bwd_sorted_adagrad_ex":
        lambda L, op, dt, ws, nbytes: L.pm_embbag_bwd_sorted_adagrad_ex(ctypes.byref(op), FAKE, FAKE, dt, FAKE, ctypes.byref(_opt()),
                                                                        MAX_ROWS, ws, nbytes, None),
    "pm_embbag_bwd_sorted_adagrad_elem":
        lambda L, op, dt, ws, nbytes: L.pm_embbag_bwd_sorted_adagrad_elem(ctypes.byref(op), FAKE, FAKE, dt, FAKE, ctypes.byref(_opt()),
                                                                          MAX_ROWS, ws, nbytes, None),
}


@pytest.mark.parametrize("dtype", [_lib.PM_F32, _lib.PM_BF16, _lib.PM_F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", sorted(APPLIES))
def test_an_apply_needs_a_sort_of_the_request_on_the_workspace(name, dtype):
    L = _lib.load()
    op = _op(dtype)
    need = L.pm_embbag_bwd_sorted_workspace(ctypes.byref(op), MAX_ROWS)
    assert need > 0
    # a workspace that is too small (or NULL) is refused BEFORE the question whether it was sorted
    for ws, nbytes in ((FAKE, need - 1), (FAKE, 0), (None, BIG)):
        assert APPLIES[name](L, op, dtype, ws, nbytes) == _lib.PM_ERR_INVALID
        err = L.pm_last_error().decode()
        assert f"workspace too small: need {need} bytes" in err and "pm_embbag_sort_indices" not in err, err
    # large enough, never sorted
    for nbytes in (need, BIG):
        assert APPLIES[name](L, op, dtype, FAKE, nbytes) == _lib.PM_ERR_INVALID
        assert "pm_embbag_sort_indices has not been called" in L.pm_last_error().decode()


def test_pairs_and_status_need_a_recorded_sort():
    L = _lib.load()
    op = _op()
    vp = ctypes.c_void_p
    keys, vals, cnt, kb, tsh = vp(), vp(), vp(), ctypes.c_int32(), ctypes.c_int32()
    assert L.pm_embbag_sorted_pairs(ctypes.byref(op), MAX_ROWS, FAKE, ctypes.byref(keys), ctypes.byref(vals), ctypes.byref(cnt),
                                    ctypes.byref(kb), ctypes.byref(tsh)) == _lib.PM_ERR_INVALID
    assert "no sort has been recorded" in L.pm_last_error().decode()
    st = _lib.pm_sort_status()
    assert L.pm_embbag_sort_status(ctypes.byref(op), MAX_ROWS, FAKE, ctypes.byref(st), None) == _lib.PM_ERR_INVALID
    assert "no sort has been recorded" in L.pm_last_error().decode()
