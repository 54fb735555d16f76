"""The direct backward of max pooling on the GPU (``pytest -m gpu``): ``dense_grad`` / ``scatter_add_`` with ``method="direct"``
(``pm_embbag_max_bwd``) against the numpy restatement of its rule (tests/max_direct_rules.py), on bits.  Three small tables, ragged
bags with empty ones, a bag that holds its arg-max row twice, a tie between two rows, a bag whose later rows win no column.  Then the
constructed requests of tests/max_direct_cases.py under hand-written ``max_indices``: a bag's repeat across a piece cut and across a
tile border, pieces and a run that win nothing, a run start four tiles back, a run from sorted position 0, hot runs in every table and
gradient type, under ``tbd``, a slice and a padding row, with mixed dims up to D = 2048, and 8-byte sort keys through the C call.  Hot
rows need no tolerance either: the rule restates the piece cuts."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import max_direct_cases as C
from tests import max_direct_rules as R
from tests import max_rules as M
from tests import out16_rules as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
ROWS, B = (40, 17, 300), 24
TOP, NEG0, NAN, SUB = 10, 11, 12, 13      # a row that wins every column of its bag, and three that follow it there and win none
OUT = 14                                  # a row looked up by bag 2 alone, which it wins: outside the batch slice 5 .. 15
TILE = 1024                               # kMbTile: sorted pairs per workgroup of the main kernel


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype=dtype)


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy().view(np.uint32 if t.element_size() == 4 else np.uint16)


@functools.lru_cache(maxsize=None)
def _case(dims, pads=(None, None, None), tdt="f32"):
    """tables (multiples of 1/8 with the special rows), the request, whole-batch gradients (multiples of 1/16: exact in 16 bits) and the
    rule's max_indices; computed once per shape and left unchanged"""
    rng = np.random.default_rng(sum(dims))
    sub = np.float32(2.0 ** -20 if tdt == "fp16" else 2.0 ** -130)
    tabs, idx, off = [], [], []
    for t, (r, d) in enumerate(zip(ROWS, dims)):
        w = (rng.integers(-80, 81, size=(r, d)) / 8.0).astype(np.float32)
        w[5] = w[4]
        w[TOP], w[NEG0], w[NAN], w[SUB], w[OUT] = 50.0, -0.0, np.nan, sub, 60.0
        if pads[t] is not None:
            w[pads[t]] = -0.0
        tabs.append(w)
        p = 9 if pads[t] is None else pads[t]
        bags = [[4, 5], [9, 3, 9], [OUT, TOP, SUB, NEG0], [], [p, 6], [p], [TOP, NEG0, NAN, SUB], [5, 4, 9]]
        while len(bags) < B:
            n = (0, 1, 2, 3, 5)[len(bags) % 5]
            bags.append([int(x) for x in rng.integers(0, r, size=n) if x not in (NEG0, NAN, SUB, OUT)])
        for bag in bags:
            off.append(len(idx))
            idx += bag
    idx, off = np.array(idx, np.int64), np.array(off, np.int64)
    grads = [(rng.integers(-64, 65, size=(B, d)) / 16.0).astype(np.float32) for d in dims]
    _, args = M.forward(tabs, idx, off, B, list(pads))
    assert (args[0][1] == 9).any() and (args[0][0] == 4).all() and (args[0][2] == OUT).all() and (args[0][3] == -1).all()
    assert (args[0][6] == TOP).all()
    return tabs, idx, off, grads, args


def _module(dims, tabs, tdt="f32", layout="bd", pads=None, out16=None):
    import param_amd

    m = param_amd.MaxBatchedEmbeddingBagMI355(list(ROWS), list(dims), dtype=TDT[tdt], device=DEV, init=None, layout=layout, padding_idx=pads,
                                              output_dtype=out16, fused_update=False)
    for t, w in enumerate(tabs):
        m.table(t).copy_(_dev(w).to(TDT[tdt]))
    return m


def _join(parts, layout, dtype):
    return _dev(np.stack(parts) if layout == "tbd" else np.concatenate(parts, axis=1), dtype)


def _want_dense(dims, idx, off, nb, grads, args):
    return [R.apply(np.zeros(G.shape, np.uint32), "f32", G, won, 1.0) for G, won, _, _, _ in R.sums(ROWS, dims, idx, off, nb, grads, args)]


@pytest.mark.parametrize("layout,idt", [("bd", torch.int64), ("tbd", torch.int32)])
@pytest.mark.parametrize("gdt", ["f32", "bf16", "fp16"])
@pytest.mark.parametrize("D", [8, 32, 128, 512])
def test_dense_grad_direct_on_bits(D, gdt, layout, idt):
    dims = (D, D, D)
    tabs, idx_h, off_h, grads, args = _case(dims)
    m = _module(dims, tabs, layout=layout, out16=None if gdt == "f32" else TDT[gdt])
    idx, off, g = _dev(idx_h, idt), _dev(off_h, idt), _join(grads, layout, TDT[gdt])
    _, saved = m.lookup(idx, off, batch=B, return_max_indices=True)
    want = _want_dense(dims, idx_h, off_h, B, grads, args)
    sorted_ = m.dense_grad(g, idx, off, batch=B, method="sorted", max_indices=saved)
    for arg in (saved, None):
        got = m.dense_grad(g, idx, off, batch=B, method="direct", max_indices=arg)
        for t in range(3):
            assert np.array_equal(_bits(got[t]), want[t]), (t, arg is None)
            assert np.array_equal(_bits(got[t]), _bits(sorted_[t])), ("sorted", t)


@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("tdt", ["f32", "bf16", "fp16"])
def test_scatter_add_direct_keeps_rows_without_a_term(tdt, sliced):
    dims, pads = (32, 32, 32), (None, 2, None)
    tabs, idx_h, off_h, grads, args = _case(dims, pads, tdt)
    m = _module(dims, tabs, tdt, pads=list(pads))
    before = [_bits(m.table(t)).copy() for t in range(3)]
    b0, nb = (5, 11) if sliced else (0, B)
    m.scatter_add_(_join(grads, "bd", torch.float32), _dev(idx_h), _dev(off_h), alpha=-0.5, batch=B, bag_begin=b0, bag_count=nb, method="direct")
    for t, (G, won, _, _, _) in enumerate(R.sums(ROWS, dims, idx_h, off_h, B, grads, args, b0, nb)):
        after = _bits(m.table(t))
        assert np.array_equal(after, R.apply(before[t], tdt, G, won, -0.5)), t
        assert won[TOP].all() and won[OUT].all() != sliced and not won[[NEG0, NAN, SUB]].any()      # (bag 6 lies inside the slice, bag 2 outside)
        assert np.array_equal(after[[NEG0, NAN, SUB]], before[t][[NEG0, NAN, SUB]])
        if pads[t] is not None:
            assert (idx_h == pads[t]).any() and np.array_equal(after[pads[t]], before[t][pads[t]])


def test_mixed_dims_direct():
    dims = (8, 128, 32)
    tabs, idx_h, off_h, grads, args = _case(dims)
    m = _module(dims, tabs)
    idx, off, g = _dev(idx_h), _dev(off_h), _join(grads, "bd", torch.float32)
    got = m.dense_grad(g, idx, off, batch=B, method="direct")
    for t, want in enumerate(_want_dense(dims, idx_h, off_h, B, grads, args)):
        assert np.array_equal(_bits(got[t]), want), t
    with pytest.raises(ValueError, match="one common embedding dim"):
        m.dense_grad(g, idx, off, batch=B, method="sorted")


@pytest.mark.parametrize("L", [255, 256, 257, 1500])
def test_run_lengths_across_the_tile_border(L):
    """row 7 of table 1 is looked up by L bags and wins each; its run starts 100 pairs in front of a tile border of the main kernel.  Row 3 of
    table 2 has a run of 300 whose second piece starts inside the tile of its head."""
    import param_amd

    nb, D = L + 1100, 8
    n0 = (TILE - 100 - nb) % TILE                       # bags of table 1 that look up row 0: their pairs precede the run
    rows_of = [[1] * nb, [7] * L + [0] * n0 + [12] * (nb - L - n0), [3] * 300 + [5] * (nb - 300)]
    idx_h, off_h = np.array(sum(rows_of, []), np.int64), np.arange(3 * nb, dtype=np.int64)
    assert (nb + n0) % TILE == TILE - 100 and (2 * nb) % TILE < TILE - 256
    rng = np.random.default_rng(L)
    grads = [rng.standard_normal((nb, D)).astype(np.float32) for _ in range(3)]
    args = [np.repeat(np.array(r, np.int32)[:, None], D, axis=1) for r in rows_of]      # a bag of one lookup: that row wins
    m = param_amd.MaxBatchedEmbeddingBagMI355(list(ROWS), D, device=DEV, init=None, fused_update=False)
    idx, off, g = _dev(idx_h), _dev(off_h), _dev(np.concatenate(grads, axis=1))
    got = m.dense_grad(g, idx, off, batch=nb, method="direct")
    res = R.sums(ROWS, (D, D, D), idx_h, off_h, nb, grads, args)
    for t, (G, won, _, _, _) in enumerate(res):
        assert np.array_equal(_bits(got[t]), R.apply(np.zeros(G.shape, np.uint32), "f32", G, won, 1.0)), t
    _, _, G64, A64, n = res[1]
    row = got[1][7].cpu().numpy()
    assert (n[7] == L).all()
    if L <= R.EXACT_RUN:
        seq = grads[1][0].copy()
        for b in range(1, L):
            seq = seq + grads[1][b]
        assert np.array_equal(M.bits(row), M.bits(seq))
    else:
        print("max |direct - float64|", np.abs(row - G64[7]).max(), "bound", (L * 2.0 ** -24 * A64[7]).min())
        assert (np.abs(row.astype(np.float64) - G64[7]) <= L * 2.0 ** -24 * A64[7]).all()
        again = m.dense_grad(g, idx, off, batch=nb, method="direct")
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, again))


def test_c_refusals():
    from param_amd import _lib

    dims = (8, 8, 8)
    tabs, idx_h, off_h, grads, _ = _case(dims)
    m = _module(dims, tabs)
    idx, off, g = _dev(idx_h), _dev(off_h), _join(grads, "bd", torch.float32)
    _, arg = m.lookup(idx, off, batch=B, return_max_indices=True)
    ts, L = m._tables(), _lib.load()
    op = _lib.pm_embbag_batch.from_buffer_copy(ts.request(idx, off, B, None, 0, None))
    need = L.pm_embbag_max_bwd_workspace(ctypes.byref(op), max(ROWS))
    assert need > L.pm_embbag_bwd_sorted_workspace(ctypes.byref(op), max(ROWS)) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    psw = torch.ones(idx_h.size, device=DEV)

    def call(o=op, a=arg.data_ptr(), nbytes=need):
        return L.pm_embbag_max_bwd(ctypes.byref(o), g.data_ptr(), _lib.PM_F32, a, ts.d_ptrs.data_ptr(), _lib.PM_F32, 1.0, max(ROWS), ws.data_ptr(),
                                   nbytes, None)

    before = [_bits(m.table(t)).copy() for t in range(3)]
    weighted, blocked = _lib.pm_embbag_batch.from_buffer_copy(op), _lib.pm_embbag_batch.from_buffer_copy(op)
    weighted.per_sample_weights, blocked.table_group = psw.data_ptr(), 1
    assert call(weighted) == _lib.PM_ERR_UNSUPPORTED and b"unweighted" in L.pm_last_error()
    assert call(blocked) == _lib.PM_ERR_UNSUPPORTED and b"blocked" in L.pm_last_error()
    assert call(a=None) == _lib.PM_ERR_INVALID and b"NULL" in L.pm_last_error()
    assert call(nbytes=need - 1) == _lib.PM_ERR_INVALID and b"workspace" in L.pm_last_error()
    torch.cuda.synchronize()
    assert all(np.array_equal(_bits(m.table(t)), before[t]) for t in range(3))
    assert call() == _lib.PM_OK


# ---- hot runs against the piece cuts, the tile borders and the key width (tests/max_direct_cases.py builds and checks the requests) ------

def _hot_case(name):
    return {"repeat100": lambda: C.repeat(263), "repeat768": lambda: C.repeat(85), "nothing": C.nothing, "far": C.far, "zero": C.zero,
            "sliced": C.sliced, "mixed": C.mixed}[name]()


def _hot_module(c, tdt="f32", layout="bd", out16=None):
    import param_amd

    pads = list(c.pads) if any(p is not None for p in c.pads) else None
    m = param_amd.MaxBatchedEmbeddingBagMI355(list(C.ROWS), list(c.dims), dtype=TDT[tdt], device=DEV, init=None, layout=layout, padding_idx=pads,
                                              output_dtype=out16, fused_update=False)
    rng = np.random.default_rng(77)
    for t, (r, d) in enumerate(zip(C.ROWS, c.dims)):
        w = (rng.integers(-80, 81, size=(r, d)) / 8.0).astype(np.float32)      # exact in 16 bits
        w[7, 0] = -0.0
        m.table(t).copy_(_dev(w).to(TDT[tdt]))
    return m


def _hot_grads(c, gdt):
    return c.grads if gdt == "f32" else [O.widen(O.round16(g, gdt), gdt) for g in c.grads]


def _hot_dense(c, gdt="f32", layout="bd", idt=torch.int64):
    """dense_grad(method="direct") under the case's hand-written max_indices == the rule on bits, twice"""
    grads = _hot_grads(c, gdt)
    m = _hot_module(c, layout=layout, out16=None if gdt == "f32" else TDT[gdt])
    idx, off = _dev(c.idx, idt), _dev(c.off, idt)
    g, arg = _join(grads, layout, TDT[gdt]), _join(c.args, layout, torch.int32)
    res = R.sums(C.ROWS, c.dims, c.idx, c.off, c.B, grads, c.args)
    want = [R.apply(np.zeros(G.shape, np.uint32), "f32", G, won, 1.0) for G, won, _, _, _ in res]
    for call in range(2):
        got = m.dense_grad(g, idx, off, batch=c.B, method="direct", max_indices=arg)
        for t in range(3):
            assert np.array_equal(_bits(got[t]), want[t]), (t, call, np.argwhere(_bits(got[t]) != want[t])[:4].tolist())
    return res


@pytest.mark.parametrize("name", ["repeat100", "repeat768", "nothing", "far", "zero", "mixed"])
def test_hot_runs_against_the_cuts_on_bits(name):
    """repeat100 / repeat768: a bag's repeat across a piece cut, inside a tile and where the cut is a tile border; nothing: pieces, the
    first one included, and a whole run that win no column; far: a run start four tiles back; zero: a run from sorted position 0;
    mixed: dims (8, 2048, 32) with hot runs in the narrow and the wide table"""
    c = _hot_case(name)
    res = _hot_dense(c)
    for (t, row), n in c.hot().items():
        assert res[t][4][row].max() <= n and n > R.EXACT_RUN
    if name == "nothing":
        assert not res[2][1][3].any() and not res[1][1][7, 7] and M.bits(res[1][0][7])[0] == 0x80000000


@pytest.mark.parametrize("kind,dt", [("table", "f32"), ("table", "bf16"), ("table", "fp16"), ("grad", "f32"), ("grad", "bf16"), ("grad", "fp16")])
def test_hot_runs_in_every_element_type(kind, dt):
    """the request whose pieces 0 and 2 win nothing: 16-bit gradients through ``output_dtype`` and ``dense_grad``; fp32, bf16 and fp16
    tables through ``scatter_add_`` with alpha = -0.5, where the run that wins nothing and the column that nobody wins keep their bits
    and the -0.0 sum of column 0 meets a stored -0.0"""
    c = C.nothing()
    if kind == "grad":
        _hot_dense(c, gdt=dt)
        return
    m = _hot_module(c, tdt=dt)
    before = [_bits(m.table(t)).copy() for t in range(3)]
    idx, off, g, arg = _dev(c.idx), _dev(c.off), _join(c.grads, "bd", torch.float32), _join(c.args, "bd", torch.int32)
    res = R.sums(C.ROWS, c.dims, c.idx, c.off, c.B, c.grads, c.args)
    zero16 = 0x80000000 if dt == "f32" else 0x8000
    assert before[1][7, 0] == zero16
    for call in range(2):
        m.scatter_add_(g, idx, off, alpha=-0.5, batch=c.B, method="direct", max_indices=arg)
        for t, (G, won, _, _, _) in enumerate(res):
            after = _bits(m.table(t))
            assert np.array_equal(after, R.apply(before[t], dt, G, won, -0.5)), (t, call)
        assert np.array_equal(_bits(m.table(2))[3], before[2][3]) and _bits(m.table(1))[7, 7] == before[1][7, 7] and _bits(m.table(1))[7, 0] == 0
        for t in range(3):
            m.table(t).copy_(_dev(before[t].view(np.int32 if dt == "f32" else np.int16)).view(TDT[dt]))


def test_hot_runs_under_tbd_a_slice_and_a_padding_row():
    """layout tbd with int32 indices; the slice cuts one hot run to 257 pairs and another to 256; 300 padded lookups in the slice leave
    the device fewer pairs than the request has lookups"""
    c = C.sliced()
    b0, nb = c.slice
    m = _hot_module(c, layout="tbd")
    before = [_bits(m.table(t)).copy() for t in range(3)]
    idx, off = _dev(c.idx, torch.int32), _dev(c.off, torch.int32)
    g, arg = _join(c.grads, "tbd", torch.float32), _join(c.args, "tbd", torch.int32)
    res = R.sums(C.ROWS, c.dims, c.idx, c.off, c.B, c.grads, c.args, b0, nb)
    assert (res[1][4][7] == 257).all() and (res[2][4][3] == 256).all() and (res[0][4][9] == 300).all() and not res[0][1][5].any()
    for call in range(2):
        m.scatter_add_(g, idx, off, alpha=-0.5, batch=c.B, bag_begin=b0, bag_count=nb, method="direct", max_indices=arg)
        for t, (G, won, _, _, _) in enumerate(res):
            assert np.array_equal(_bits(m.table(t)), R.apply(before[t], "f32", G, won, -0.5)), (t, call)
        for t in range(3):
            m.table(t).copy_(_dev(before[t].view(np.int32)).view(torch.float32))


@pytest.mark.parametrize("name", ["case", "repeat100"])
def test_eight_byte_keys(name):
    """``pm_embbag_max_bwd`` with a ``max_rows`` of 2^30: three tables take 2 + 30 key bits and one spare, so the sort plan says 8-byte
    keys and the kernels load ``uint64`` keys (``key64``).  The bits equal the rule's and the 4-byte-key run's."""
    from param_amd import _lib

    if name == "case":
        dims = (8, 8, 8)
        tabs, idx_h, off_h, grads, args = _case(dims)
        m, nb = _module(dims, tabs), B
    else:
        c = C.repeat(263)
        dims, idx_h, off_h, grads, args, nb = c.dims, c.idx, c.off, c.grads, c.args, c.B
        m = _hot_module(c)
    idx, off, g, arg = _dev(idx_h), _dev(off_h), _join(grads, "bd", torch.float32), _join(args, "bd", torch.int32)
    ts, L = m._tables(), _lib.load()
    op = _lib.pm_embbag_batch.from_buffer_copy(ts.request(idx, off, nb, None, 0, None))
    op.fixed_pooling = 0
    want = [R.apply(np.zeros(G.shape, np.uint32), "f32", G, won, 1.0) for G, won, _, _, _ in R.sums(ROWS, dims, idx_h, off_h, nb, grads, args)]
    small = m.dense_grad(g, idx, off, batch=nb, method="direct", max_indices=arg)
    for max_rows, key_bytes in ((max(ROWS), "4"), (1 << 30, "8")):
        buf = ctypes.create_string_buffer(512)
        assert L.pm_embbag_sort_plan(ctypes.byref(op), max_rows, 1, buf, 512) == _lib.PM_OK, L.pm_last_error()
        assert dict(kv.split("=") for kv in buf.value.decode().split())["key_bytes"] == key_bytes
        need = L.pm_embbag_max_bwd_workspace(ctypes.byref(op), max_rows)
        assert 0 < need < 1 << 30, need
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        for call in range(2):
            outs = [torch.zeros(r, d, device=DEV) for r, d in zip(ROWS, dims)]
            ptrs = torch.tensor([o.data_ptr() for o in outs], dtype=torch.int64, device=DEV)
            assert L.pm_embbag_max_bwd(ctypes.byref(op), g.data_ptr(), _lib.PM_F32, arg.data_ptr(), ptrs.data_ptr(), _lib.PM_F32, 1.0, max_rows,
                                       ws.data_ptr(), need, None) == _lib.PM_OK, L.pm_last_error()
            torch.cuda.synchronize()
            for t in range(3):
                assert np.array_equal(_bits(outs[t]), want[t]), (key_bytes, t, call)
                assert np.array_equal(_bits(outs[t]), _bits(small[t])), (key_bytes, t, "the module's 4-byte-key run")
