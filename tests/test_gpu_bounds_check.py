"""bounds_check_mode on the device (``pytest -m gpu``): ``pm_embbag_bounds_check`` through ``sanitize_`` / ``forward`` / ``lookup`` of
the modules, arrays and report compared BIT FOR BIT with the numpy restatement of the rule (tests/bounds_rules.py).

No lookup, sort or apply kernel is launched on a request before the existing ``check()`` (``pm_embbag_check``, which is safe on any
contents) has returned zero errors for it: every repaired request is handed to ``check()``, and the lookups of this file go through
a ``_fwd`` that calls it first -- a sanitiser bug shows as a failed assertion, not as a fault.
"""
import numpy as np
import pytest
import torch

from param_amd import _lib
from tests import bounds_rules as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPW = _lib.PM_BOUNDS_OFFSETS_PER_WG
NP = {"int32": np.int32, "int64": np.int64}
both_dtypes = pytest.mark.parametrize("dtype", ["int32", "int64"])
both_forms = pytest.mark.parametrize("closed", [False, True], ids=["TB", "TB+1"])


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    import param_amd

    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    param_amd.load_library()
    yield


@pytest.fixture(autouse=True)
def _lookups_are_checked_first(monkeypatch):
    """every lookup of this file: ``check()`` between the sanitiser and the kernel (raises IndexError on a violation)"""
    from param_amd import embedding_bag as eb

    real = eb._fwd

    def checked(ts, indices, offsets, B, *args, **kw):
        eb.check_request(ts, indices, offsets, B)
        return real(ts, indices, offsets, B, *args, **kw)

    monkeypatch.setattr(eb, "_fwd", checked)


_modules = {}


def _module(rows, dim=4, **kw):
    import param_amd

    key = (tuple(rows), dim, tuple(sorted(kw.items())))
    if key not in _modules:
        kw.setdefault("fused_update", False)
        _modules[key] = param_amd.BatchedEmbeddingBagMI355(list(rows), dim, device=DEV, init="normal", seed=3, **kw)
    return _modules[key]


def _dev(a):
    return torch.from_numpy(a).to(DEV)


def _same(t, a):
    got = t.cpu().numpy()
    return got.dtype == a.dtype and got.shape == a.shape and got.tobytes() == a.tobytes()


def _run(rows, idx, off, B, mode, m=None):
    """``sanitize_`` of copies of the arrays on the device -> (indices tensor, offsets tensor, report dict or None)"""
    m = m or _module(rows)
    d_idx, d_off = _dev(idx), _dev(off)
    if mode == "fatal":
        try:
            m.sanitize_(d_idx, d_off, batch=B, mode=mode)
            raised = False
        except IndexError as e:
            raised = str(e)
        rep = m.bounds_report()
        assert bool(raised) == bool(rep["bad_indices"] or rep["bad_offsets"])
        if raised:
            assert f"{rep['bad_indices']} out-of-range indices" in raised and f"{rep['bad_offsets']} invalid offsets" in raised
    else:
        m.sanitize_(d_idx, d_off, batch=B, mode=mode)
        rep = m.bounds_report()
        assert (rep is None) == (mode == "ignore")
    return d_idx, d_off, rep


def _expect(rows, idx, off, B, modes=("warning", "ignore", "fatal"), what=""):
    """every mode against the rule: repaired arrays and report bit for bit, the dry run untouched with the same report, and the
    repaired request passes the device's own check()"""
    T = len(rows)
    want_idx, want_off, want = R.repair(idx, off, rows, T, B)
    assert R.check_errors(want_idx, want_off, rows, T, B) == 0
    m = _module(rows)
    for mode in modes:
        d_idx, d_off, rep = _run(rows, idx, off, B, mode, m)
        if mode == "fatal":
            assert _same(d_idx, idx) and _same(d_off, off), (what, mode)
        else:
            bad_i = np.nonzero(d_idx.cpu().numpy() != want_idx)[0][:5]
            bad_o = np.nonzero(d_off.cpu().numpy() != want_off)[0][:5]
            assert _same(d_idx, want_idx) and _same(d_off, want_off), (what, mode, bad_i, bad_o)
            m.check(d_idx, d_off, batch=B)
        if mode != "ignore":
            assert rep == R.report_dict(want), (what, mode)
    return want


@both_dtypes
@both_forms
def test_clean_request_is_unchanged_in_every_mode(dtype, closed):
    rng = np.random.default_rng(1)
    rows = [5, 50, 7, 3000]
    idx, off = R.clean_request(rng, rows, 33, 5, NP[dtype], closed, empty_tables=(2,))
    assert _expect(rows, idx, off, 33) == (0, 0, None, None)
    m = _module(rows)
    for mode in ("warning", "ignore", "fatal"):
        d_idx, d_off, _ = _run(rows, idx, off, 33, mode, m)
        assert _same(d_idx, idx) and _same(d_off, off)


@both_dtypes
@both_forms
def test_every_defect(dtype, closed):
    idx, off, rows, T, B, want_idx, want_off, want = R.every_defect_case(closed, NP[dtype])
    assert _expect(rows, idx, off, B) == want
    d_idx, d_off, rep = _run(rows, idx, off, B, "warning")
    assert _same(d_idx, want_idx) and _same(d_off, want_off) and rep == R.report_dict(want)      # the hand-written arrays


@both_dtypes
@both_forms
def test_fatal_is_a_dry_run_with_the_warning_report(dtype, closed):
    rng = np.random.default_rng(2)
    rows = [11, 1000, 13]
    idx, off = R.clean_request(rng, rows, 300, 6, NP[dtype], closed)
    idx, off = R.corrupt(rng, idx, off, rows, 9, 5)
    _, _, warn = _run(rows, idx, off, 300, "warning")
    d_idx, d_off, fatal = _run(rows, idx, off, 300, "fatal")
    assert warn == fatal and warn["bad_indices"] > 0 and warn["bad_offsets"] > 0
    assert _same(d_idx, idx) and _same(d_off, off)
    # the report is overwritten by every call, never accumulated
    m = _module(rows)
    clean_idx, clean_off, _ = R.repair(idx, off, rows, 3, 300)
    m.sanitize_(_dev(clean_idx), _dev(clean_off), batch=300, mode="warning")
    assert m.bounds_report() == R.report_dict((0, 0, None, None))


@both_dtypes
@pytest.mark.parametrize("defect", ["spike_at_1", "dip_at_second_workgroup", "spike_at_workgroup_end"])
def test_carry_across_scan_workgroups(dtype, defect):
    rng = np.random.default_rng(3)
    rows, B = [4, 400, 40], OPW + 1
    T = len(rows)
    assert T * B >= 3 * OPW + 1
    idx, off = R.clean_request(rng, rows, B, 2, NP[dtype], True)
    N = idx.size
    if defect == "spike_at_1":
        off[1] = N + 7                      # everything behind becomes N: every lookup falls into bag 0 (table 0)
    elif defect == "dip_at_second_workgroup":
        off[OPW] = 0                        # the first entry of the second workgroup's range
    else:
        off[OPW - 1] = off[2 * OPW + 5]     # the last entry of the first workgroup: carried through the whole second one
    want = _expect(rows, idx, off, B, what=defect)
    if defect == "spike_at_1":
        closed_off = R.repair(idx, off, rows, T, B)[1]
        assert (closed_off[1:] == N).all() and want[1] >= T * B - 20 and want[0] > N // 2
    elif defect == "dip_at_second_workgroup":
        assert want[1] == 1 and want[3] == OPW
    else:
        assert want[1] > OPW // 2 and want[3] == OPW      # (the spike itself keeps its value: what follows it changes)


@both_dtypes
@pytest.mark.parametrize("defect", ["near_the_end", "spike_at_the_start"])
def test_more_partials_than_the_scan_workgroup_has_threads(dtype, defect):
    rng = np.random.default_rng(4)
    rows, B = [1000], 1024 * OPW + 5
    idx, off = R.clean_request(rng, rows, B, 1, NP[dtype], True)
    N = idx.size
    if defect == "near_the_end":
        off[B - 3] = -1
        off[B - 700] = N + 1
        idx[N - 2] = 1000
    else:
        off[5] = N // 2                     # carried over half of the partials: across rounds of the second-level scan
        idx[N // 2 + 1] = -1
    want = _expect(rows, idx, off, B, modes=("warning", "fatal"), what=defect)
    assert want[1] > (600 if defect == "near_the_end" else B // 4) and want[0] >= 1


@both_dtypes
@both_forms
def test_more_tables_than_fit_the_lds(dtype, closed):
    rng = np.random.default_rng(5)
    T, B = 1100, 2
    rows = [3 + t % 7 for t in range(T)]
    idx, off = R.clean_request(rng, rows, B, 3, NP[dtype], closed, min_len=1, empty_tables=(7, 8, 500))
    idx[0] = rows[0]                        # table 0
    idx[-1] = -5                            # table 1099
    idx[idx.size // 2] = 100
    off[2 * 300] = 0                        # a table border that has to be repaired before the tables are told apart
    want = _expect(rows, idx, off, B)
    assert want[0] >= 3 and want[2] == 0 and want[1] == 1


@both_dtypes
def test_table_borders_inside_a_vector(dtype):
    """pooling 3: table t starts at lookup 21 t, inside a 16-byte vector for most t; indices valid for the neighbour only"""
    rng = np.random.default_rng(6)
    rows, B = [10, 100, 10, 100, 10], 7
    idx, off = R.clean_request(rng, rows, B, 3, NP[dtype], True, min_len=3)
    assert idx.size == 5 * 21
    idx[20], idx[21] = 50, 50               # border 21: the last lookup of table 0 (bad), the first of table 1 (fine)
    idx[41], idx[42] = 99, 99               # border 42: table 1 (fine), table 2 (bad)
    idx[62], idx[63] = 10, 10               # border 63: table 2 (bad: == rows), table 3 (fine)
    want = _expect(rows, idx, off, B)
    assert want == (3, 0, 20, None)
    got = R.repair(idx, off, rows, 5, B)[0]
    assert got[[20, 21, 41, 42, 62, 63]].tolist() == [0, 50, 99, 0, 0, 10]


@both_dtypes
@pytest.mark.parametrize("shift", [1, 3])
def test_index_pointer_off_the_vector(dtype, shift):
    """a slice of a larger tensor: the pointer is element-aligned only and N is no multiple of the vector; the elements around the
    slice are not touched"""
    rng = np.random.default_rng(7)
    rows, B = [9, 90000], 3000
    idx, off = R.clean_request(rng, rows, B, 7, NP[dtype], False)
    vec = 16 // idx.itemsize
    if idx.size % vec == 0:                 # one lookup fewer: the last bag gets shorter
        idx = idx[:-1]
    N = idx.size
    assert N % vec and N > 16 * 256 * vec   # more than one workgroup of the index pass
    idx, off = R.corrupt(rng, idx, off, rows, 40, 3)
    idx[0], idx[N - 1] = -1, 90000          # the scalar head and tail
    want_idx, want_off, want = R.repair(idx, off, rows, 2, B)
    m = _module(rows)
    big = torch.full((N + shift + 5,), -77, dtype=getattr(torch, dtype), device=DEV)
    d_idx = big[shift:shift + N]
    d_idx.copy_(torch.from_numpy(idx))
    assert d_idx.data_ptr() % 16 != 0 and d_idx.is_contiguous()
    d_off = _dev(off)
    m.sanitize_(d_idx, d_off, batch=B, mode="warning")
    assert m.bounds_report() == R.report_dict(want) and want[2] == 0
    assert _same(d_idx, want_idx) and _same(d_off, want_off)
    assert (big[:shift] == -77).all() and (big[shift + N:] == -77).all()
    m.check(d_idx, d_off, batch=B)


@both_dtypes
def test_no_lookups_and_no_bags(dtype):
    rows = [5, 6]
    a = lambda v: np.array(v, dtype=NP[dtype])      # noqa: E731
    assert _expect(rows, a([]), a([0, 4, -1, 2, 9]), 2) == (0, 4, None, 1)            # N = 0: the offsets are still repaired
    # B = 0: nothing is repaired, nothing is launched; the module's report is the zero report
    m = _module(rows)
    d_idx, d_off = _dev(a([7, -7])), _dev(a([5]))
    m.sanitize_(d_idx, d_off, batch=0, mode="warning")
    assert m.bounds_report() == R.report_dict((0, 0, None, None)) and d_idx.tolist() == [7, -7] and d_off.tolist() == [5]


@both_dtypes
def test_end_to_end_through_the_modules(dtype):
    import param_amd

    rng = np.random.default_rng(8)
    rows, B, T = [50, 7, 300], 64, 3
    idx, off = R.clean_request(rng, rows, B, 6, NP[dtype], True)
    idx, off = R.corrupt(rng, idx, off, rows, 12, 4)
    want_idx, want_off, want = R.repair(idx, off, rows, T, B)
    assert want[0] > 0 and want[1] > 0
    kw = dict(device=DEV, init="normal", seed=9, learning_rate=0.5)
    warn = param_amd.BatchedEmbeddingBagMI355(rows, 8, bounds_check_mode="WARNING", **kw)
    plain = param_amd.BatchedEmbeddingBagMI355(rows, 8, **kw)
    same_tables = lambda: all(torch.equal(warn.table(t), plain.table(t)) for t in range(T))      # noqa: E731  (the slab has padding)
    assert plain.bounds_check_mode == "none" and same_tables()
    # forward (autograd glue and all) of the corrupted request == forward of the numpy-repaired one; check() runs in between
    outs, reports = [], []
    for _ in range(2):                                  # two runs on copies: identical bits and reports
        d_idx, d_off = _dev(idx), _dev(off)
        out = warn(d_idx, d_off)
        outs.append(out)
        reports.append(warn.bounds_report())
        assert _same(d_idx, want_idx) and _same(d_off, want_off)
    ref = plain(_dev(want_idx), _dev(want_off))
    assert reports[0] == reports[1] == R.report_dict(want)
    assert torch.equal(outs[0], outs[1]) and outs[0].detach().cpu().numpy().tobytes() == ref.detach().cpu().numpy().tobytes()
    fatal_tables = [warn.table(0).clone()]
    # the backward sees the repaired tensors: the same fused update as the plain module's on the repaired request
    g = torch.randn_like(ref)
    outs[1].backward(g)
    ref.backward(g)
    assert same_tables() and not torch.equal(warn.table(0), fatal_tables[0])       # (updated, and equal)
    # fatal: IndexError, nothing written, no lookup issued
    fatal = param_amd.BatchedEmbeddingBagMI355(rows, 8, bounds_check_mode="fatal", fused_update=False, **kw)
    d_idx, d_off = _dev(idx), _dev(off)
    with pytest.raises(IndexError, match=f"{want[0]} out-of-range indices .first at position {want[2]}., {want[1]} invalid offsets"):
        fatal.lookup(d_idx, d_off)
    assert _same(d_idx, idx) and _same(d_off, off) and fatal.bounds_report() == R.report_dict(want)
    assert torch.equal(fatal.lookup(_dev(want_idx), _dev(want_off)), ref.detach())
    # the single-table module: offsets [B]
    one = param_amd.EmbeddingBagMI355(40, 8, device=DEV, bounds_check_mode="ignore")
    i1, o1 = R.clean_request(rng, [40], 20, 4, NP[dtype], False)
    c1, co1 = R.corrupt(rng, i1, o1, [40], 5, 2)
    w1, wo1, _ = R.repair(c1, co1, [40], 1, 20)
    d_i, d_o = _dev(c1), _dev(co1)
    with torch.no_grad():
        got = one(d_i, d_o)
    assert _same(d_i, w1) and _same(d_o, wo1) and one.bounds_report() is None
    plain_one = param_amd.EmbeddingBagMI355(40, 8, device=DEV, _weight=one.weight.data)
    with torch.no_grad():
        assert torch.equal(got, plain_one(_dev(w1), _dev(wo1)))
