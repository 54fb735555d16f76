"""The batched sequence backward on the GPU (``pytest -m gpu``): ``pm_embseq_*`` behind ``BatchedEmbeddingBagMI355.sequence_*``.

The base request is T = 3 tables of rows (60, 5000, 17), B = 1100 ragged bags of 0 .. 4 lookups: the middle table holds more than
4096 lookups (several radix tiles, the look-back), the small ones many short runs across chunk and tile borders; variants leave the
first, the middle or the last table without a lookup; int64 and int32.  The sort is held to its contract, the dense gradient to the
numpy rule (tests/sequence_grad_rules.py) bit for bit, a row hotter than the exact run to the fp64 sum, and the optimizers to the
route the package had before -- one ``optimizer_step_`` per table on the request "one bag per lookup" -- bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from tests import embedding_rules as E
from tests import sequence_grad_rules as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
ROWS = (60, 5000, 17)
T, B = 3, 1100
EXACT_RUN = 256      # kExactRun of the sorted apply: a row looked up more often is summed as ordered chunk partials


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    import param_amd

    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    param_amd.load_library()


def _bits(t):
    t = t.detach().contiguous()
    if t.element_size() == 2:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


_REQ = {}


def _request(empty=None, dtype=np.int64):
    """(indices, offsets [T * B + 1]) of the base request, built once per variant and never modified: bags of 0 .. 4 lookups; the
    middle table's bags are 4 long but for fifty of them (> 4096 lookups); ``empty``: that table owns no lookup"""
    key = (empty, np.dtype(dtype).name)
    if key not in _REQ:
        rng = np.random.default_rng(100 + (0 if empty is None else 1 + empty))
        lens = rng.integers(0, 5, T * B)
        lens[B:2 * B] = 4
        lens[B + rng.choice(B, 50, replace=False)] = rng.integers(0, 4, 50)
        if empty is not None:
            lens[empty * B:(empty + 1) * B] = 0
        off = np.concatenate([[0], np.cumsum(lens)])
        idx = np.concatenate([rng.integers(0, ROWS[t], int(off[(t + 1) * B] - off[t * B])) for t in range(T)])
        assert empty == 1 or off[2 * B] - off[B] > 4096
        for t in range(T):
            n_t = int(off[(t + 1) * B] - off[t * B])
            assert n_t == 0 or np.bincount(idx[off[t * B]:off[(t + 1) * B]]).max() <= EXACT_RUN
        _REQ[key] = (idx.astype(dtype), off.astype(dtype))
    return _REQ[key]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _module(D, dtype=torch.float32, rows=ROWS, **kw):
    import param_amd

    kw.setdefault("fused_update", False)
    return param_amd.BatchedEmbeddingBagMI355(list(rows), D, dtype=dtype, device=DEV, init="normal", seed=21, **kw)


_GRAD = {}


def _grad(n, D, seed=0):
    key = (n, D, seed)
    if key not in _GRAD:
        _GRAD[key] = np.random.default_rng(300 + seed).standard_normal((n, D)).astype(np.float32)
    return _GRAD[key]


_RULE = {}


def _rule(empty, D, pads=None, slice=(0, None)):
    """the numpy rule on the base request and its gradient: computed once per case, shared, never modified"""
    key = (empty, D, None if pads is None else tuple(pads), slice)
    if key not in _RULE:
        idx, off = _request(empty)
        _RULE[key] = S.dense_grad(ROWS, [D] * T, idx, off[:-1], B, _grad(idx.size, D), pads, slice)
    return _RULE[key]


def _wbits(m):
    """the bits of every table of a module (the slab itself has uninitialised padding between the tables)"""
    return np.concatenate([_bits(m.table(t)).reshape(-1) for t in range(len(m.rows))])


def _same(got, want):
    return all(np.array_equal(_bits(g), np.ascontiguousarray(w, dtype=np.float32).view(np.uint32)) for g, w in zip(got, want))


# ---- 1. the sort's contract -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("empty,dtype,sl", [(None, np.int64, (0, None)), (0, np.int32, (0, None)), (1, np.int64, (0, None)),
                                            (2, np.int32, (0, None)), (None, np.int32, (100, 700)), (2, np.int64, (100, 700))])
def test_sort_contract(empty, dtype, sl):
    """per table keys ascending; within equal keys the values are ascending lookup positions of exactly that table and row; the pair
    count is the slice's lookups"""
    from param_amd import embedding_bag as EB

    idx_h, off_h = _request(empty, dtype)
    idx, off = _dev(idx_h), _dev(off_h)
    m = _module(8)
    m.sequence_sort_indices(idx, off, batch=B, bag_begin=sl[0], bag_count=sl[1])
    k, v, tshift = EB.sorted_pairs(m._tables(), idx, off, B, None, sl[0], sl[1])
    k, v = k.cpu().numpy().astype(np.int64), v.cpu().numpy().view(np.uint32).astype(np.int64)
    tab, inside = E.in_slice(off_h[:-1], T, B, idx_h.size, sl[0], sl[1])
    assert k.size == v.size == int(inside.sum())
    assert np.array_equal(np.sort(v), np.nonzero(inside)[0])                     # every position of the slice exactly once
    assert np.array_equal(k >> tshift, tab[v]) and np.array_equal(k & ((1 << tshift) - 1), idx_h[v].astype(np.int64))
    dk, dv = np.diff(k), np.diff(v)
    assert (dk >= 0).all() and (dv[dk == 0] > 0).all()
    st = m.sort_status(idx, off, batch=B, bag_begin=sl[0], bag_count=sl[1])
    assert st["pairs_sorted"] == k.size and st["hybrid_launched"] == 0


# ---- 2. the dense gradient is the rule, bit for bit -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("D", [8, 128])
def test_dense_grad_equals_the_rule(D, kind):
    idx_h, off_h = _request()
    m = _module(D, TDT[kind])
    got = m.sequence_dense_grad(_dev(_grad(idx_h.size, D)), _dev(idx_h), _dev(off_h), batch=B)
    assert [tuple(g.shape) for g in got] == [(r, D) for r in ROWS] and all(g.dtype == torch.float32 for g in got)
    assert _same(got, _rule(None, D))


@pytest.mark.parametrize("empty,dtype", [(0, np.int64), (1, np.int32), (2, np.int64), (None, np.int32)])
def test_dense_grad_with_a_table_that_owns_no_lookup(empty, dtype):
    idx_h, off_h = _request(empty, dtype)
    got = _module(8).sequence_dense_grad(_dev(_grad(idx_h.size, 8)), _dev(idx_h), _dev(off_h), batch=B)
    want = _rule(empty, 8)
    assert _same(got, want) and (empty is None or not want[empty].any())


def test_dense_grad_out_accumulates_and_padding_rows_keep_their_bits():
    D, pads = 8, [5, None, 0]
    idx_h, off_h = _request()
    assert (idx_h[:off_h[B]] == 5).any() and (idx_h[off_h[2 * B]:] == 0).any()
    rng = np.random.default_rng(31)
    init = [rng.standard_normal((r, D)).astype(np.float32) for r in ROWS]
    init[0][5, :] = np.nan                                                       # what a padding row holds comes back as it was
    m = _module(D, padding_idx=pads)
    outs = [_dev(a) for a in init]
    got = m.sequence_dense_grad(_dev(_grad(idx_h.size, D)), _dev(idx_h), _dev(off_h), batch=B, out=outs)
    assert all(g is o for g, o in zip(got, outs))
    want = S.dense_grad(ROWS, [D] * T, idx_h, off_h[:-1], B, _grad(idx_h.size, D), pads, init=init)
    assert _same(got, want)
    assert np.array_equal(_bits(got[0][5]), init[0][5].view(np.uint32)) and np.array_equal(_bits(got[2][0]), init[2][0].view(np.uint32))
    # fresh buffers: the padding rows stay zero
    fresh = m.sequence_dense_grad(_dev(_grad(idx_h.size, D)), _dev(idx_h), _dev(off_h), batch=B)
    assert _same(fresh, _rule(None, D, pads)) and not fresh[0][5].any() and not fresh[2][0].any()


def test_a_row_hotter_than_the_exact_run():
    """one row of the middle table gets 300 lookups: every other row bit for bit, the hot row within 1e-5 * sum |contribution| of
    the fp64 sum (the bar of tests/test_gpu_parity.py and _check_grad_rows in tests/test_gpu_embedding.py)"""
    D, hot = 128, 7
    idx_h, off_h = (a.copy() for a in _request())
    lo, hi = int(off_h[B]), int(off_h[2 * B])
    at = lo + np.random.default_rng(32).choice(hi - lo, 300, replace=False)
    idx_h[lo:hi][idx_h[lo:hi] == hot] = hot + 1
    idx_h[at] = hot
    assert (idx_h[lo:hi] == hot).sum() == 300 > EXACT_RUN
    g = _grad(idx_h.size, D)
    got = _module(D).sequence_dense_grad(_dev(g), _dev(idx_h), _dev(off_h), batch=B)
    want = S.dense_grad(ROWS, [D] * T, idx_h, off_h[:-1], B, g)
    cold = np.arange(ROWS[1]) != hot
    assert _same([got[0], got[1].cpu()[torch.from_numpy(cold)], got[2]], [want[0], want[1][cold], want[2]])
    sel = np.sort(at)
    exact, mag = g[sel].astype(np.float64).sum(axis=0), np.abs(g[sel]).astype(np.float64).sum(axis=0)
    assert (np.abs(got[1][hot].cpu().numpy().astype(np.float64) - exact) <= 1e-5 * mag).all()


def test_batch_slice_reads_nothing_outside():
    """bag_begin = 100, bag_count = 700: the gradient rows of positions outside the slice hold NaN; the result is the rule's and
    holds no NaN"""
    D, sl = 8, (100, 700)
    idx_h, off_h = _request()
    _, inside = E.in_slice(off_h[:-1], T, B, idx_h.size, *sl)
    g = _grad(idx_h.size, D).copy()
    g[~inside] = np.nan
    assert inside.any() and not inside.all()
    m = _module(D)
    m.weights.data.zero_()
    m.sequence_scatter_add_(_dev(g), _dev(idx_h), _dev(off_h), 1.0, batch=B, bag_begin=sl[0], bag_count=sl[1])
    got = [m.table(t) for t in range(T)]
    assert _same(got, _rule(None, D, None, sl)) and not any(torch.isnan(x).any() for x in got)


def test_c_abi_with_a_row_stride():
    """grad_row_stride = D + 4 with NaN in the pad columns equals the contiguous call bit for bit"""
    from param_amd import _lib
    from param_amd import embedding_bag as EB

    D = 8
    idx_h, off_h = _request()
    idx, off = _dev(idx_h), _dev(off_h)
    m = _module(D)
    ts = m._tables()
    wide = np.full((idx_h.size, D + 4), np.nan, dtype=np.float32)
    wide[:, :D] = _grad(idx_h.size, D)
    gw = _dev(wide)
    outs = [torch.zeros(r, D, device=DEV) for r in ROWS]
    d_ptrs = torch.tensor([o.data_ptr() for o in outs], dtype=torch.int64, device=DEV)
    op = ts.request(idx, off, B, None, 0, None)
    ws = EB._workspace(ts, op)
    rc = _lib.load().pm_embseq_bwd_fused(ctypes.byref(op), gw.data_ptr(), D + 4, d_ptrs.data_ptr(), _lib.PM_F32, 1.0, max(ROWS),
                                         ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, _lib.load().pm_last_error()
    contiguous = m.sequence_dense_grad(_dev(_grad(idx_h.size, D)), idx, off, batch=B)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs, contiguous))
    assert _same(outs, _rule(None, D))


# ---- 3. the optimizers against the route the package had: one call per table, one bag per lookup -------------------------------------

def _one_table_route(M, idx_h, off_h, grads, **kw):
    """per table t a one-table module with M's weight bits, stepped with the EXISTING ``optimizer_step_`` on ``offsets = arange(n_t)``,
    ``batch = n_t`` and the table's gradient rows, once per gradient -> [(table, state or None)] per table"""
    import param_amd

    res = []
    for t in range(T):
        lo, hi = int(off_h[t * B]), int(off_h[(t + 1) * B])
        one = param_amd.BatchedEmbeddingBagMI355([ROWS[t]], M.dims[0], dtype=M.weights.dtype, device=DEV, init=None, fused_update=False, **kw)
        one.table(0).copy_(M.table(t))
        idx, arange = _dev(idx_h[lo:hi]), torch.arange(hi - lo, dtype=torch.int64, device=DEV)
        for g in grads:
            one.optimizer_step_(g[lo:hi].contiguous(), idx, arange, batch=hi - lo)
        res.append((one.table(0).clone(), None if one.momentum is None else one.momentum_table(0).clone()))
    return res


CONFIGS = [("sgd", None), ("rowwise_adagrad", None), ("rowwise_adagrad", "l2"), ("rowwise_adagrad", "decouple"), ("adagrad", None)]


@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("optimizer,wd_mode", CONFIGS, ids=[f"{o}-{w}" for o, w in CONFIGS])
def test_optimizer_step_equals_the_one_table_route(optimizer, wd_mode, kind):
    """two consecutive steps; every table and every state buffer bit-identical.  No row exceeds 256 lookups (asserted on the host
    when the request is built), so both sides sum sequentially and the comparison needs no tolerance."""
    D = 16
    idx_h, off_h = _request()
    for t in range(T):
        assert np.bincount(idx_h[off_h[t * B]:off_h[(t + 1) * B]]).max() <= EXACT_RUN
    kw = dict(optimizer=optimizer, learning_rate=0.05, eps=1e-6, weight_decay=0.01 if wd_mode else 0.0, weight_decay_mode=wd_mode)
    M = _module(D, TDT[kind], **kw)
    grads = [_dev(_grad(idx_h.size, D, s)) for s in (1, 2)]
    want = _one_table_route(M, idx_h, off_h, grads, **kw)
    before = [M.table(t).clone() for t in range(T)]
    idx, off = _dev(idx_h), _dev(off_h)
    for g in grads:
        M.sequence_optimizer_step_(g, idx, off, batch=B)
    for t, (w, s) in enumerate(want):
        assert np.array_equal(_bits(M.table(t)), _bits(w)), (t, "table")
        assert not np.array_equal(_bits(M.table(t)), _bits(before[t]))
        if s is None:
            assert M.momentum is None
        else:
            assert np.array_equal(_bits(M.momentum_table(t)), _bits(s)) and s.any(), (t, "state")


@pytest.mark.parametrize("optimizer", ["rowwise_adagrad", "adagrad"])
def test_stochastic_rounding_is_reproducible_and_table_0_is_the_one_table_route(optimizer):
    D = 16
    idx_h, off_h = _request()
    kw = dict(optimizer=optimizer, learning_rate=0.05, stochastic_rounding=True)
    A, C, N = _module(D, torch.bfloat16, **kw), _module(D, torch.bfloat16, **kw), _module(D, torch.bfloat16, **{**kw, "stochastic_rounding": False})
    g, idx, off = _dev(_grad(idx_h.size, D, 3)), _dev(idx_h), _dev(off_h)
    want0 = _one_table_route(A, idx_h, off_h, [g], **kw)[0]
    for mod in (A, C, N):
        mod.sequence_optimizer_step_(g, idx, off, batch=B)
    assert np.array_equal(_wbits(A), _wbits(C)) and np.array_equal(_bits(A.momentum), _bits(C.momentum))
    assert not np.array_equal(_wbits(A), _wbits(N))          # the draws did something
    assert np.array_equal(_bits(A.table(0)), _bits(want0[0])) and np.array_equal(_bits(A.momentum_table(0)), _bits(want0[1]))


# ---- 4. presorted, and the workspace's record of what it holds ------------------------------------------------------------------------

def test_presorted_equals_fused_and_the_two_kinds_of_sort_do_not_mix():
    from param_amd import _lib

    D = 8
    idx_h, off_h = _request()
    idx, off, g = _dev(idx_h), _dev(off_h), _dev(_grad(idx_h.size, D))
    a, b = _module(D), _module(D)
    a.sequence_scatter_add_(g, idx, off, -0.5, batch=B)
    b.sequence_sort_indices(idx, off, batch=B)
    b.sequence_scatter_add_(g, idx, off, -0.5, batch=B, presorted=True)
    assert np.array_equal(_wbits(a), _wbits(b))
    for opt in ("rowwise_adagrad", "adagrad"):
        a, b = _module(D, optimizer=opt), _module(D, optimizer=opt)
        a.sequence_optimizer_step_(g, idx, off, batch=B)
        b.sequence_sort_indices(idx, off, batch=B)
        b.sequence_optimizer_step_(g, idx, off, batch=B, presorted=True)
        assert np.array_equal(_wbits(a), _wbits(b)) and np.array_equal(_bits(a.momentum), _bits(b.momentum))
    # a pooled apply after a sequence sort, and a sequence apply after a pooled sort: refused on the host, nothing is written
    pooled = torch.zeros(B, T * D, device=DEV)
    keep = _wbits(b)
    b.sequence_sort_indices(idx, off, batch=B)
    with pytest.raises(_lib.ParamAmdError, match="sequence sort"):
        b.scatter_add_(pooled, idx, off, 1.0, batch=B, presorted=True)
    with pytest.raises(_lib.ParamAmdError, match="sequence sort"):
        b.adagrad_step_(pooled, idx, off, batch=B, presorted=True)
    b.sort_indices(idx, off, batch=B)
    with pytest.raises(_lib.ParamAmdError, match="pooled sort"):
        b.sequence_scatter_add_(g, idx, off, 1.0, batch=B, presorted=True)
    with pytest.raises(_lib.ParamAmdError, match="pooled sort"):
        b.sequence_optimizer_step_(g, idx, off, batch=B, presorted=True)
    torch.cuda.synchronize()
    assert np.array_equal(_wbits(b), keep)
    c = _module(D)
    with pytest.raises(_lib.ParamAmdError, match="pm_embseq_sort_indices has not been called"):
        c.sequence_scatter_add_(g, idx, off, 1.0, batch=B, presorted=True)


def test_presorted_is_refused_on_a_workspace_another_table_set_sorted_on():
    """The library keeps its record of the last sort by the workspace's ADDRESS, and torch's caching allocator hands the block of a
    freed workspace to the next one of its size.  Modelled without the allocator: module ``c`` is given the very workspace tensor on which
    module ``a`` has sorted the same request tensors.  ``c`` has sorted nothing: ``presorted=True`` is refused for it, sequence and
    pooled, although the library's record under that address fits the call; after a sort of its own the call goes through."""
    from param_amd import _lib

    D = 8
    idx_h, off_h = _request()
    idx, off, g = _dev(idx_h), _dev(off_h), _dev(_grad(idx_h.size, D))
    pooled = torch.ones(B, T * D, device=DEV)
    for sequence in (True, False):
        a, c = _module(D), _module(D)
        if sequence:
            a.sequence_sort_indices(idx, off, batch=B)
        else:
            a.sort_indices(idx, off, batch=B)
        c._tables()._ws = a._tables()._ws
        keep = _wbits(c)
        with pytest.raises(_lib.ParamAmdError, match="pm_embseq_sort_indices has not been called" if sequence else
                           "pm_embbag_sort_indices has not been called"):
            if sequence:
                c.sequence_scatter_add_(g, idx, off, 1.0, batch=B, presorted=True)
            else:
                c.scatter_add_(pooled, idx, off, 1.0, batch=B, presorted=True)
        assert c._tables()._ws.data_ptr() == a._tables()._ws.data_ptr()
        torch.cuda.synchronize()
        assert np.array_equal(_wbits(c), keep)
        if sequence:
            c.sequence_sort_indices(idx, off, batch=B)
            c.sequence_scatter_add_(g, idx, off, 1.0, batch=B, presorted=True)
        else:
            c.sort_indices(idx, off, batch=B)
            c.scatter_add_(pooled, idx, off, 1.0, batch=B, presorted=True)
        assert not np.array_equal(_wbits(c), keep)


# ---- 5. autograd ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,optimizer", [("f32", "sgd"), ("f32", "rowwise_adagrad"), ("bf16", "adagrad")])
def test_forward_sequence_backward_is_the_optimizer_step(kind, optimizer):
    D = 16
    idx_h, off_h = _request()
    idx, off = _dev(idx_h), _dev(off_h)
    out = "bf16" if kind == "bf16" else None
    a = _module(D, TDT[kind], optimizer=optimizer, fused_update=True, output_dtype=out)
    b = _module(D, TDT[kind], optimizer=optimizer, fused_update=True, output_dtype=out)
    g32 = _dev(_grad(idx_h.size, D, 4))
    g = g32.to(torch.bfloat16) if out else g32
    y = a.forward_sequence(idx, off, batch=B)
    assert y.requires_grad and y.dtype == (torch.bfloat16 if out else torch.float32) and tuple(y.shape) == (idx_h.size, D)
    rows = b.lookup_sequence(idx, off, batch=B)
    assert np.array_equal(_bits(y), _bits(rows))
    y.backward(g)
    b.sequence_optimizer_step_(g.float() if out else g, idx, off, batch=B)
    assert np.array_equal(_wbits(a), _wbits(b)) and not np.array_equal(_wbits(a), _wbits(_module(D, TDT[kind])))
    if optimizer != "sgd":
        assert np.array_equal(_bits(a.momentum), _bits(b.momentum)) and a.momentum.any()
    if out:      # the caller's 16-bit gradient is only read
        assert np.array_equal(_bits(g), _bits(g32.to(torch.bfloat16)))
    with torch.no_grad():
        assert not a.forward_sequence(idx, off, batch=B).requires_grad


# ---- 6. more tables than one sorted call takes -------------------------------------------------------------------------------------------

def test_dense_grad_1100_tables():
    """1100 tables x 8 rows x D 8, B = 2 (the shape of test_lookup_sequence_1100_tables): two table ranges, the second one's gradient
    rows start at its first lookup position"""
    Tn, Bn, D = 1100, 2, 8
    rng = np.random.default_rng(9)
    rows = [8] * Tn
    lens = rng.integers(0, 4, Tn * Bn)
    lens[Bn * 7:Bn * 9] = 0                                                        # two tables without lookups
    off_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx_h = rng.integers(0, 8, int(off_h[-1])).astype(np.int64)
    g = rng.standard_normal((idx_h.size, D)).astype(np.float32)
    m = _module(D, rows=rows)
    got = m.sequence_dense_grad(_dev(g), _dev(idx_h), _dev(off_h), batch=Bn)
    want = S.dense_grad(rows, [D] * Tn, idx_h, off_h[:-1], Bn, g)
    assert np.array_equal(_bits(torch.stack(got)), np.stack(want).view(np.uint32))
    assert want[1050].any() and not want[7].any()
    with pytest.raises(ValueError, match="presorted=True takes requests of at most 1024 tables"):
        m.sequence_scatter_add_(_dev(g), _dev(idx_h), _dev(off_h), 1.0, batch=Bn, presorted=True)
    with pytest.raises(ValueError, match="at most 1024 tables"):
        m.sequence_sort_indices(_dev(idx_h), _dev(off_h), batch=Bn)


# ---- 7. nothing that exists reaches the new entry points --------------------------------------------------------------------------------

NEW = ("pm_embseq_sort_indices", "pm_embseq_bwd_sorted", "pm_embseq_bwd_fused", "pm_embseq_bwd_sorted_adagrad", "pm_embseq_bwd_fused_adagrad")


def test_existing_methods_never_call_the_sequence_entry_points(monkeypatch):
    import param_amd
    from param_amd import _lib

    real = _lib.load()
    seen = []

    class Raising:
        def __getattr__(self, name):
            if name in NEW:
                raise AssertionError(f"{name} reached from a pre-existing method")
            return getattr(real, name)

    monkeypatch.setattr(_lib, "load", lambda: Raising())
    D, Bs = 16, 40
    rng = np.random.default_rng(12)
    lens = rng.integers(0, 5, T * Bs)
    off_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx_h = np.concatenate([rng.integers(0, ROWS[t], int(off_h[(t + 1) * Bs] - off_h[t * Bs])) for t in range(T)]).astype(np.int64)
    idx, off = _dev(idx_h), _dev(off_h)
    grad = torch.randn(Bs, T * D, device=DEV)
    psw = torch.rand(idx_h.size, device=DEV)
    for opt in ("sgd", "rowwise_adagrad", "adagrad"):
        m = _module(D, optimizer=opt)
        m.scatter_add_(grad, idx, off, -0.1, batch=Bs)
        m.scatter_add_(grad, idx, off, -0.1, per_sample_weights=psw, batch=Bs)
        m.adagrad_step_(grad, idx, off, batch=Bs)
        m.optimizer_step_(grad, idx, off, batch=Bs)
        m.sort_indices(idx, off, batch=Bs)
        m.optimizer_step_(grad, idx, off, batch=Bs, presorted=True)
        m.dense_grad(grad, idx, off, batch=Bs)
        m.sparse_grad(grad, idx, off, batch=Bs)
        m.per_sample_weights_grad(grad, idx, off, batch=Bs)
        f = _module(D, optimizer=opt, fused_update=True)
        f(idx, off).backward(grad)
    for sparse in (False, True):
        e = param_amd.EmbeddingMI355(50, D, device=DEV, sparse=sparse)
        e(idx[:100] % 50).sum().backward()
        b = param_amd.EmbeddingBagMI355(50, D, device=DEV, sparse=sparse)
        b(idx[:100] % 50, off[:10].clamp(max=100)).sum().backward()

    class Counting:
        def __getattr__(self, name):
            if name in NEW:
                seen.append(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "load", lambda: Counting())
    g = torch.randn(idx_h.size, D, device=DEV)
    m = _module(D, optimizer="adagrad")
    m.sequence_sort_indices(idx, off, batch=Bs)
    m.sequence_scatter_add_(g, idx, off, 1.0, batch=Bs, presorted=True)
    m.sequence_scatter_add_(g, idx, off, 1.0, batch=Bs)
    m.sequence_sort_indices(idx, off, batch=Bs)
    m.sequence_optimizer_step_(g, idx, off, batch=Bs, presorted=True)
    m.sequence_optimizer_step_(g, idx, off, batch=Bs)
    assert set(seen) == set(NEW)
