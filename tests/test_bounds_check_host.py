"""bounds_check_mode, the parts that need no GPU: the numpy restatement of the rule (tests/bounds_rules.py) has the properties the
rule was chosen for -- a clean request comes back unchanged, a repaired one passes the conditions of ``embbag_check_kernel``, repairing
twice changes nothing --; ``pm_embbag_bounds_check`` / ``pm_embbag_bounds_check_scratch`` are declared, bound and exported by both
libraries with the ABI where it was; every host-side refusal answers before a HIP call; the modules validate the mode before they
allocate and, with the default mode, never reach the sanitiser."""
import ctypes
import os
import re

import numpy as np
import pytest

from param_amd import _lib
from tests import bounds_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _shapes(rng):
    T = int(rng.integers(1, 6))
    B = int(rng.integers(0, 9))
    rows = [int(r) for r in rng.integers(1, 40, T)]
    empty = [t for t in range(T) if rng.random() < 0.25]
    max_len = int(rng.integers(0, 4))              # 0: N = 0
    return T, B, rows, empty, max_len


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("closed", [False, True])
def test_rule_properties_over_random_requests(dtype, closed):
    rng = np.random.default_rng(7 + closed)
    seen = {"n0": 0, "b0": 0, "empty_table": 0, "bad": 0}
    for _ in range(400):
        T, B, rows, empty, max_len = _shapes(rng)
        idx, off = R.clean_request(rng, rows, B, max_len, dtype, closed, empty_tables=empty)
        seen["n0"] += idx.size == 0
        seen["b0"] += B == 0
        seen["empty_table"] += bool(empty) and B > 0
        # clean: unchanged, zero report, no violation
        i1, o1, rep = R.repair(idx, off, rows, T, B)
        assert _same(i1, idx) and _same(o1, off) and rep == (0, 0, None, None)
        assert R.check_errors(idx, off, rows, T, B) == 0
        # corrupted: repaired output passes the check kernel's conditions; the rule is idempotent
        ci, co = R.corrupt(rng, idx, off, rows, int(rng.integers(0, 4)), int(rng.integers(0, 4)))
        i2, o2, rep2 = R.repair(ci, co, rows, T, B)
        assert i2.dtype == ci.dtype and o2.dtype == co.dtype
        assert R.check_errors(i2, o2, rows, T, B) == 0
        if B == 0:
            assert _same(i2, ci) and _same(o2, co) and rep2 == (0, 0, None, None)      # nothing is repaired
        else:
            assert int(o2[0]) == 0 and (np.diff(o2[:T * B].astype(np.int64)) >= 0).all() and (not closed or int(o2[-1]) == idx.size)
        assert rep2[0] == int((i2 != ci).sum())                                      # rows >= 1: a replaced entry was not 0
        assert rep2[1] == int((o2 != co).sum())
        seen["bad"] += bool(rep2[0] or rep2[1])
        i3, o3, rep3 = R.repair(i2, o2, rows, T, B)
        assert _same(i3, i2) and _same(o3, o2) and rep3 == (0, 0, None, None)
    assert all(v > 10 for v in seen.values()), seen


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("closed", [False, True])
def test_hand_worked_every_defect(dtype, closed):
    idx, off, rows, T, B, want_idx, want_off, want_rep = R.every_defect_case(closed, dtype)
    got_idx, got_off, rep = R.repair(idx, off, rows, T, B)
    assert _same(got_idx, want_idx) and _same(got_off, want_off) and rep == want_rep
    assert R.check_errors(idx, off, rows, T, B) > 0 and R.check_errors(got_idx, got_off, rows, T, B) == 0
    assert list(R.report_array(rep)) == [5, 5 if closed else 4, 1, 0]


def test_hand_worked_small_cases():
    a = lambda v: np.array(v, dtype=np.int64)      # noqa: E731
    # an early oversized offset: everything behind it becomes N, every lookup falls into table 0, table 1 is empty
    i, o, rep = R.repair(a([1, 50, 2]), a([0, 9, 1, 2]), [2, 100], 2, 2)
    assert i.tolist() == [1, 0, 0] and o.tolist() == [0, 3, 3, 3] and rep == (2, 3, 1, 1)
    # no lookups: the offsets are still repaired, the trailing entry included
    i, o, rep = R.repair(a([]), a([0, 4, -1, 2, 9]), [3, 3], 2, 2)
    assert i.size == 0 and o.tolist() == [0, 0, 0, 0, 0] and rep == (0, 4, None, 1)
    # no bags: nothing is repaired, not even the trailing entry
    i, o, rep = R.repair(a([7, -7]), a([5]), [3], 1, 0)
    assert i.tolist() == [7, -7] and o.tolist() == [5] and rep == (0, 0, None, None)
    # an index that is already the replacement value is fine (rows >= 1); a clean leading empty table
    i, o, rep = R.repair(a([0, 3, 0]), a([0, 0, 0, 1, 3]), [9, 3], 2, 2)
    assert i.tolist() == [0, 0, 0] and o.tolist() == [0, 0, 0, 1, 3] and rep == (1, 0, 1, None)
    assert R.report_dict(rep) == {"bad_indices": 1, "bad_offsets": 0, "first_bad_index": 1, "first_bad_offset": None}
    assert R.report_array(rep).tolist() == [1, 0, 1, R.NONE] and R.NONE == _lib.PM_BOUNDS_NONE == 2**63 - 1


def test_header_binding_and_both_libraries_carry_the_symbols():
    text = open(os.path.join(ROOT, "include", "param_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    product = re.sub(r"#ifdef PM_ALTERNATES.*?#endif", "", src, flags=re.S)
    assert re.search(r"\bint64_t\s+pm_embbag_bounds_check_scratch\s*\(\s*const\s+pm_embbag_batch\s*\*\s*op\s*\)", product)
    assert re.search(r"\bint\s+pm_embbag_bounds_check\s*\(\s*const\s+pm_embbag_batch\s*\*\s*op\s*,\s*int32_t\s+mode\s*,\s*int64_t\s*\*\s*d_report\s*,"
                     r"\s*void\s*\*\s*d_scratch\s*,\s*int64_t\s+scratch_bytes\s*,\s*pm_stream_t\s+stream\s*\)", product)
    defines = dict(re.findall(r"#define\s+(PM_BOUNDS_[A-Z_]+)\s+(\S+)", product))
    assert defines == {"PM_BOUNDS_FATAL": "1", "PM_BOUNDS_WARNING": "2", "PM_BOUNDS_IGNORE": "3", "PM_BOUNDS_LAST_OFFSET": "0x100",
                       "PM_BOUNDS_NONE": "INT64_MAX", "PM_BOUNDS_OFFSETS_PER_WG": str(_lib.PM_BOUNDS_OFFSETS_PER_WG)}
    assert (_lib.PM_BOUNDS_FATAL, _lib.PM_BOUNDS_WARNING, _lib.PM_BOUNDS_IGNORE, _lib.PM_BOUNDS_LAST_OFFSET) == (1, 2, 3, 0x100)
    L, A = _lib.load(), _lib.load_alternates()
    for name in ("pm_embbag_bounds_check_scratch", "pm_embbag_bounds_check"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name) and hasattr(A, name)
    assert L.pm_embbag_bounds_check.argtypes is not None and L.pm_embbag_bounds_check_scratch.restype is ctypes.c_int64
    assert L.pm_abi_version() == 8 and A.pm_abi_version() == 8 and _lib.PM_ABI_VERSION == 8
    assert ctypes.sizeof(_lib.pm_embbag_batch) == 144
    assert "#define PM_ABI_VERSION 8" in text


def _request(T=2, B=4, N=100, idt=None):
    op = _lib.pm_embbag_batch()
    op.num_tables, op.weight_dtype, op.index_dtype, op.max_dim = T, _lib.PM_F32, _lib.PM_I64 if idt is None else idt, 8
    op.tables = op.rows = op.dims = op.out_offsets = 8      # non-null dummies, never dereferenced on the host
    op.batch, op.bag_begin, op.bag_count, op.num_indices, op.indices, op.offsets = B, 0, B, N, 8, 8
    op.out_stride = 8
    return op


def test_every_refusal_is_made_on_the_host():
    L = _lib.load()
    fn, size = L.pm_embbag_bounds_check, L.pm_embbag_bounds_check_scratch
    W = _lib.PM_BOUNDS_WARNING
    call = lambda op, mode=W, rep=8, scr=8, nbytes=1 << 20: fn(None if op is None else ctypes.byref(op), mode, rep, scr, nbytes, None)      # noqa: E731
    # what make_params refuses, for both calls
    assert call(None) == _lib.PM_ERR_INVALID and size(None) == _lib.PM_ERR_INVALID
    op = _request()
    op.index_dtype = 3
    assert call(op) == _lib.PM_ERR_INVALID and b"index_dtype" in L.pm_last_error()
    assert size(ctypes.byref(op)) == _lib.PM_ERR_INVALID
    op = _request()
    op.num_tables = 0
    assert call(op) == _lib.PM_ERR_INVALID and b"num_tables" in L.pm_last_error()
    op = _request()
    op.offsets = None
    assert call(op) == _lib.PM_ERR_INVALID and b"offsets" in L.pm_last_error()
    op = _request()
    op.bag_count = 0                                           # bag_begin / bag_count are ignored: offsets are still needed
    op.offsets = None
    assert call(op) == _lib.PM_ERR_INVALID and b"offsets" in L.pm_last_error()
    # unknown mode
    for mode in (0, 4, -1, 7 | _lib.PM_BOUNDS_LAST_OFFSET, 0x200 | W):
        assert call(_request(), mode=mode) == _lib.PM_ERR_INVALID, mode
        assert b"unknown mode" in L.pm_last_error()
    # NULL report outside IGNORE
    for mode in (_lib.PM_BOUNDS_FATAL, W, W | _lib.PM_BOUNDS_LAST_OFFSET):
        assert call(_request(), mode=mode, rep=None) == _lib.PM_ERR_INVALID and b"d_report" in L.pm_last_error()
    # short / NULL scratch; the text names the size the query gives
    op = _request(T=3, B=5000)
    need = size(ctypes.byref(op))
    assert need == ((3 * 5000 + _lib.PM_BOUNDS_OFFSETS_PER_WG - 1) // _lib.PM_BOUNDS_OFFSETS_PER_WG + 3 + 1) * 8
    assert call(op, nbytes=need - 1) == _lib.PM_ERR_INVALID and b"scratch" in L.pm_last_error() and str(need).encode() in L.pm_last_error()
    assert call(op, scr=None) == _lib.PM_ERR_INVALID and b"scratch" in L.pm_last_error()
    assert call(op, mode=_lib.PM_BOUNDS_IGNORE, rep=None, nbytes=0) == _lib.PM_ERR_INVALID and b"scratch" in L.pm_last_error()
    # pointers off their element, int32 offsets that cannot hold N
    op = _request()
    op.indices = 12
    assert call(op) == _lib.PM_ERR_INVALID and b"aligned" in L.pm_last_error()
    op = _request(N=1 << 31, idt=_lib.PM_I32)
    assert call(op) == _lib.PM_ERR_INVALID and b"2^31" in L.pm_last_error()
    assert call(_request(), rep=12) == _lib.PM_ERR_INVALID and b"aligned" in L.pm_last_error()


def test_an_empty_request_succeeds_without_a_device():
    L = _lib.load()
    op = _request(B=0)                                          # no bags: nothing is repaired, nothing launched
    assert L.pm_embbag_bounds_check_scratch(ctypes.byref(op)) == 0
    for mode in (_lib.PM_BOUNDS_FATAL, _lib.PM_BOUNDS_WARNING, _lib.PM_BOUNDS_IGNORE | _lib.PM_BOUNDS_LAST_OFFSET):
        assert L.pm_embbag_bounds_check(ctypes.byref(op), mode, 8, None, 0, None) == _lib.PM_OK
    op.num_indices = 0
    assert L.pm_embbag_bounds_check(ctypes.byref(op), _lib.PM_BOUNDS_IGNORE, None, None, 0, None) == _lib.PM_OK


def test_mode_names():
    import enum

    from param_amd.embedding_bag import bounds_check_mode_name as name

    class BoundsCheckMode(enum.IntEnum):                      # fbgemm_gpu's enum, restated
        FATAL = 0
        WARNING = 1
        IGNORE = 2
        NONE = 3

    for want in ("fatal", "warning", "ignore", "none"):
        member = BoundsCheckMode[want.upper()]
        assert name(want) == name(want.upper()) == name(want.title()) == name(member) == name(int(member)) == want
    assert name(None) == "none"
    for bad in ("", "fatl", 4, -1, 1.0, True, object()):
        with pytest.raises(ValueError, match="bounds_check_mode"):
            name(bad)


def test_constructors_reject_an_unknown_mode_before_allocating():
    import param_amd

    # (tables of 2^50 bytes: reaching the allocation would be another error)
    with pytest.raises(ValueError, match="bounds_check_mode"):
        param_amd.BatchedEmbeddingBagMI355([1 << 40] * 4, 256, device="cpu", bounds_check_mode="loud")
    with pytest.raises(ValueError, match="bounds_check_mode"):
        param_amd.EmbeddingBagMI355(1 << 40, 256, device="cpu", bounds_check_mode=9)
    m = param_amd.BatchedEmbeddingBagMI355([4], 4, device="cpu", init=None)
    assert m.bounds_check_mode == "none" and m.bounds_report() is None
    assert param_amd.BatchedEmbeddingBagMI355([4], 4, device="cpu", init=None, bounds_check_mode="WARNING").bounds_check_mode == "warning"
    assert param_amd.EmbeddingBagMI355(4, 4, device="cpu", bounds_check_mode=2).bounds_check_mode == "ignore"


class _Recorder:
    """stands in for the loaded library: every entry point returns 0 and is written down"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


@pytest.mark.parametrize("mode", ["none", "ignore", "warning"])
def test_lookup_reaches_the_sanitiser_only_with_a_mode(monkeypatch, mode):
    import torch

    import param_amd
    from param_amd import embedding_bag as eb

    rec = _Recorder()
    monkeypatch.setattr(eb, "_require_device", lambda t, what: None)
    monkeypatch.setattr(eb, "_stream_ptr", lambda: 0)
    monkeypatch.setattr(_lib, "load", lambda: rec)
    m = param_amd.BatchedEmbeddingBagMI355([5, 6], 4, device="cpu", init=None, fused_update=False, bounds_check_mode=mode)
    idx = torch.tensor([0, 1, 2, 3], dtype=torch.int64)
    off = torch.tensor([0, 1, 2, 3, 4], dtype=torch.int64)
    m.lookup(idx, off)
    m(idx, off[:4])
    names = [c[0] for c in rec.calls]
    if mode == "none":
        assert names == ["pm_embbag_fwd", "pm_embbag_fwd"]
        return
    assert names == ["pm_embbag_bounds_check_scratch", "pm_embbag_bounds_check", "pm_embbag_fwd"] * 2
    flags = [c[1][1] for c in rec.calls if c[0] == "pm_embbag_bounds_check"]
    code = {"ignore": _lib.PM_BOUNDS_IGNORE, "warning": _lib.PM_BOUNDS_WARNING}[mode]
    assert flags == [code | _lib.PM_BOUNDS_LAST_OFFSET, code]           # [T*B+1] offsets, then [T*B]
    reports = [c[1][2] for c in rec.calls if c[0] == "pm_embbag_bounds_check"]
    assert all(r is None for r in reports) if mode == "ignore" else all(reports)
