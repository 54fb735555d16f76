"""PRUNED TABLES on the GPU: ``pm_embbag_fwd_qrows_pruned`` and ``pm_embedding_gather_qrows_pruned`` through the modules'
``index_remapping=``, compared as BITS (a) against tests/pruned_rules.py -- delete the pruned lookups, remap the rest, then
tests/qmixed_rules.py -- and (b) against the module WITHOUT pruning over the same physical bytes, fed the request that the host deleted
and remapped: no new arithmetic.  Three tables of logical rows (97, 40, 300), the middle one not pruned; the requests' conditions -- how
much is pruned, an all-pruned bag, a bag with nothing pruned, pruned lookups first and last in a tile -- are asserted, so that no case
passes by pruning nothing.  One reference per request, shared by the index types, layouts and output types that must give the same bits."""
import functools

import numpy as np
import pytest
import torch

from oracle import rowquant
from tests import out16_rules as O
from tests import pruned_rules as P
from tests import qgather_rules as Q
from tests import qrows_rules as R
from tests.test_gpu_qgather import TDT, bits_of, same, unroll_knob
from tests.test_gpu_qrows import DEV, IDT, assert_same, dev, float_tables, module, split_bd, tuning

pytestmark = pytest.mark.gpu
LOGICAL, B = (97, 40, 300), 37
FORMATS = [(4, 8, 4), (8, 4, 8), (8, 8, 8), (4, 4, 4)]
FMT = pytest.mark.parametrize("bits", FORMATS, ids=["484", "848", "888", "444"])
TILE = 256                                  # lookup positions per workgroup of the un-pooled kernel


def remap_of(keep):
    return np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)


def keeps(seed, logical, pruned_tables):
    """per table a bool mask over its logical rows (about 55 % kept), or None"""
    rng = np.random.default_rng(seed)
    return [(rng.random(n) < 0.55) if t in pruned_tables else None for t, n in enumerate(logical)]


def pruned_request(seed, logical, masks, nbags, lens=None):
    """(indices int64 over the LOGICAL rows, offsets int64 [T * nbags + 1], psw fp32): ragged bags of 0 .. 9 lookups; of every pruned
    table the first and the last lookup are pruned (first / last of a pooled tile, whatever the tile: a tile belongs to one table), one
    bag is all pruned and one non-empty bag has nothing pruned; a pruned lookup of a live bag weighs +Inf"""
    rng = np.random.default_rng(seed)
    T = len(logical)
    lens = rng.integers(0, 10, T * nbags) if lens is None else np.asarray(lens, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tab = np.repeat(np.arange(T), lens.reshape(T, nbags).sum(axis=1))
    idx = (rng.random(int(lens.sum())) * np.asarray(logical)[tab]).astype(np.int64)
    psw = (rng.standard_normal(idx.size) * 1.5).astype(np.float32)
    for t, k in enumerate(masks):
        if k is None:
            continue
        kept, dropped = np.nonzero(k)[0], np.nonzero(~k)[0]
        a, e = off[t * nbags], off[(t + 1) * nbags]
        idx[a], idx[e - 1] = dropped[0], dropped[-1]
        own = range(t * nbags, (t + 1) * nbags)
        ends = [b for b in own if off[b] <= a < off[b + 1] or off[b] <= e - 1 < off[b + 1]]      # the bags of those two lookups
        bags = [b for b in own if lens[b] >= 2 and b not in ends]
        for b, pool in ((bags[0], dropped), (bags[1], kept)):
            idx[off[b]:off[b + 1]] = rng.choice(pool, lens[b])
        live = [b for b in own if lens[b] >= 3 and b not in bags[:2]][0]      # its first lookup is pruned and weighs +Inf, its second is kept
        idx[off[live]], idx[off[live] + 1] = dropped[1], kept[0]
        psw[off[live]] = np.inf
    return idx, off, psw


def check_conditions(remaps, idx, off, nbags, share=True):
    """what the issue asks of every request, asserted: no case passes by pruning nothing"""
    phys = P.physical(remaps, idx, off, nbags)
    pruned = phys < 0
    firsts = [j for j in range(0, idx.size, TILE)]
    lasts = [min(j + TILE, idx.size) - 1 for j in firsts]
    assert pruned[firsts].any() and pruned[lasts].any()               # un-pooled tiles of 256 positions
    for t, r in enumerate(remaps):
        a, e = off[t * nbags], off[(t + 1) * nbags]
        if r is None:
            assert not pruned[a:e].any()
            continue
        assert pruned[a] and pruned[e - 1]                            # pooled tiles: the table's first tile begins, its last ends pruned
        if share:
            assert 0.30 <= pruned[a:e].mean() <= 0.60, (t, pruned[a:e].mean())
        per_bag = [pruned[off[b]:off[b + 1]] for b in range(t * nbags, (t + 1) * nbags)]
        assert any(p.size and p.all() for p in per_bag) and any(p.size and not p.any() for p in per_bag)
    return pruned


@functools.lru_cache(maxsize=None)
def case(bits, dim, seed=1):
    """(physical rows, physical tables, remaps, request, pruned positions) of the main request"""
    masks = keeps(100 + seed, LOGICAL, (0, 2))
    remaps = [None if k is None else remap_of(k) for k in masks]
    rows = tuple(n if k is None else int(k.sum()) for n, k in zip(LOGICAL, masks))
    qt = [rowquant.quantize_rows(x, b) for x, b in zip(float_tables(200 + dim, rows, (dim,) * 3), bits)]
    idx, off, psw = pruned_request(300 + seed, LOGICAL, masks, B)
    pruned = check_conditions(remaps, idx, off, B)
    assert np.isinf(psw[pruned]).sum() == 2 and np.isfinite(psw[~pruned]).all() and idx.size > TILE
    return rows, qt, remaps, idx, off, psw, pruned


def tremaps(remaps):
    return [None if r is None else torch.from_numpy(r) for r in remaps]


def pmodule(rows, dims, bits, qt, remaps, **kw):
    m = module(list(rows), list(dims), list(bits), qt, index_remapping=tremaps(remaps), **kw)
    assert m.pruned and m.rows == list(rows) and m._tables().d_bits is not None
    return m


# ---- the main grid: pooled -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [64, 128])
@FMT
def test_pooled_main_grid(bits, dim):
    rows, qt, remaps, idx, off, psw, _ = case(bits, dim)
    dims = (dim,) * 3
    want = {w: P.forward(qt, dims, bits, remaps, idx, off, B, psw if w else None) for w in (False, True)}
    assert all(np.isfinite(x).all() for x in want[True])              # the +Inf weights sit on pruned lookups: they reach no bag
    cidx, coff, cw, _ = P.compact(remaps, idx, off, B, psw)
    for odt in ("fp32", "bf16", "fp16"):
        for layout in ("bd", "tbd"):
            m = pmodule(rows, dims, bits, qt, remaps, layout=layout, output_dtype=TDT[odt])
            plain = module(list(rows), list(dims), list(bits), qt, layout=layout, output_dtype=TDT[odt])
            assert m.logical_rows == list(LOGICAL) and not plain.pruned
            for it in ("i32", "i64"):
                d_idx, d_off = dev(idx, IDT[it]), dev(off, IDT[it])
                for w in (False, True):
                    out = m(d_idx, d_off, dev(psw) if w else None)
                    assert out.dtype == TDT[odt] and not out.requires_grad
                    got = bits_of(out)
                    per_table = list(got) if layout == "tbd" else [got[:, t * dim:(t + 1) * dim] for t in range(3)]
                    for t in range(3):
                        assert same(per_table[t], want[w][t], odt), (bits, dim, odt, layout, it, w, t)
                    # no new arithmetic: the module without pruning over the physical bytes, fed the deleted-and-remapped request
                    ref = plain(dev(cidx, IDT[it]), dev(coff, IDT[it]), dev(cw) if w else None)
                    assert np.array_equal(bits_of(ref), got), (bits, dim, odt, layout, it, w)
            # the geometry reported is the per-table-format plan's for the same request, which is what was launched
            assert m.plan(d_idx, d_off) == plain_mixed_plan(m, d_idx, d_off)


def plain_mixed_plan(m, d_idx, d_off, psw=None):
    from param_amd import _lib
    return _lib.embbag_qrows_mixed_plan(m._tables().request(d_idx, d_off, B, psw, 0, None, forward=True), {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[m.output_dtype])


@pytest.mark.parametrize("bits", [(4, 8, 4), (8, 4, 8)], ids=["484", "848"])
def test_pooled_out_and_batch_slice(bits):
    dim = 64
    rows, qt, remaps, idx, off, psw, _ = case(bits, dim)
    dims = (dim,) * 3
    m = pmodule(rows, dims, bits, qt, remaps)
    d_idx, d_off, d_w = dev(idx), dev(off), dev(psw)
    buf = torch.full((B, 3 * dim), float("nan"), device=DEV)
    assert m.lookup(d_idx, d_off, d_w, out=buf) is buf
    assert_same(split_bd(buf, dims), P.forward(qt, dims, bits, remaps, idx, off, B, psw), "out=")
    for begin, count in ((0, 5), (11, 20), (30, 7), (5, 0)):
        want = P.forward(qt, dims, bits, remaps, idx, off, B, psw, begin, count)
        buf = torch.full((B, 3 * dim), -7.0, device=DEV)
        m.lookup(d_idx, d_off, d_w, out=buf, bag_begin=begin, bag_count=count)
        outside = np.ones(B, dtype=bool)
        outside[begin:begin + count] = False
        assert (buf.cpu().numpy()[outside] == -7.0).all()
        assert_same([x[begin:begin + count] for x in split_bd(buf, dims)], want, f"slice {begin}+{count}")


# ---- the unstaged path -----------------------------------------------------------------------------------------------------------------

def test_pooled_unstaged_path_at_both_unrolls():
    logical, bits, dims, nb = (1000, 900), (8, 4), (128, 128), 4
    masks = keeps(7, logical, (0, 1))
    remaps = [remap_of(k) for k in masks]
    rows = tuple(int(k.sum()) for k in masks)
    qt = [rowquant.quantize_rows(x, b) for x, b in zip(float_tables(3, rows, dims), bits)]
    idx, off, psw = pruned_request(8, logical, masks, nb, lens=(1500,) * 8)      # four bags of 1500 lookups per table
    pruned = check_conditions(remaps, idx, off, nb)                   # (of each table's four bags one is all pruned, one all kept)
    psw[np.nonzero(pruned)[0][::7]] = np.inf
    want_u = P.forward(qt, dims, bits, remaps, idx, off, nb)
    want_w = P.forward(qt, dims, bits, remaps, idx, off, nb, psw)
    assert all(np.isfinite(x).all() for x in want_w)
    m = pmodule(rows, dims, bits, qt, remaps)
    for it in ("i32", "i64"):
        d_idx, d_off = dev(idx, IDT[it]), dev(off, IDT[it])
        for u in (2, 4):
            with tuning(unroll=u):
                p = m.plan(d_idx, d_off, batch=nb)
                assert p["tiles_per_table"] == 1 and p["idx_cap"] < 6000 and p["unroll"] == u      # 6000 lookups per tile: not staged
                assert_same(split_bd(m.lookup(d_idx, d_off, batch=nb), dims), want_u, f"unstaged {it} u{u}")
                assert m.plan(d_idx, d_off, dev(psw), batch=nb)["idx_cap"] < 6000
                assert_same(split_bd(m.lookup(d_idx, d_off, dev(psw), batch=nb), dims), want_w, f"unstaged weighted {it} u{u}")


# ---- un-pooled -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [64, 128])
@FMT
def test_sequence_main_grid(bits, dim):
    rows, qt, remaps, idx, off, _, pruned = case(bits, dim)
    dims = (dim,) * 3
    want, written = P.gather(qt, dim, bits, remaps, idx, off, B)
    table, _ = Q.owners(off, 3, B, idx.size)
    assert written.all() and len(set(table[:TILE].tolist())) >= 2 and not want[pruned].any()      # tile 0 straddles a table border
    cidx, coff, _, kept = P.compact(remaps, idx, off, B)
    for odt in ("fp32", "bf16", "fp16"):
        m = pmodule(rows, dims, bits, qt, remaps, layout="tbd", output_dtype=TDT[odt])
        plain = module(list(rows), list(dims), list(bits), qt, layout="tbd", output_dtype=TDT[odt])
        for it in ("i32", "i64"):
            d_idx, d_off = dev(idx, IDT[it]), dev(off, IDT[it])
            out = m.lookup_sequence(d_idx, d_off)
            assert out.shape == (idx.size, dim) and out.dtype == TDT[odt] and not out.requires_grad
            got = bits_of(out)
            assert same(got, want, odt), (bits, dim, odt, it)
            assert not got[pruned].any()                              # +0.0 of the output dtype: all bits clear
            ref = bits_of(plain.lookup_sequence(dev(cidx, IDT[it]), dev(coff, IDT[it])))
            assert np.array_equal(ref, got[kept]), (bits, dim, odt, it)
        buf = torch.full((idx.size, dim), float("nan"), device=DEV, dtype=TDT[odt])
        assert m.lookup_sequence(d_idx, d_off, out=buf) is buf and same(bits_of(buf), want, odt)
    # the geometry reported is the per-table-format plan's, tables of one format included: eight columns per lane
    from param_amd import _lib
    p = m.sequence_plan(d_idx, d_off)
    assert p == _lib.embedding_gather_qrows_mixed_plan(m._tables().request(d_idx, d_off, B, None, 0, None, forward=True))
    assert p["vec"] == 8 and p["group_lanes"] == dim // 8 and p["grid"] == 2 and p["lds_borders"] == 1
    for knob in (1, 2, 4, 8):                                        # every rows-in-flight value
        with unroll_knob(knob):
            assert m.sequence_plan(d_idx, d_off)["unroll"] == knob
            assert same(bits_of(m.lookup_sequence(d_idx, d_off)), want, "fp16"), (bits, dim, knob)
    # a batch slice: rows outside it keep the sentinel; pruned positions inside it are zeros
    m32 = pmodule(rows, dims, bits, qt, remaps)
    for begin, count in ((0, 5), (11, 20), (30, 7), (5, 0)):
        want_s, written = P.gather(qt, dim, bits, remaps, idx, off, B, begin, count)
        buf = torch.full((idx.size, dim), -7.0, device=DEV)
        m32.lookup_sequence(dev(idx), dev(off), out=buf, bag_begin=begin, bag_count=count)
        got = buf.cpu().numpy()
        assert (got[~written] == -7.0).all() and R.same_f32(got[written], want_s[written]), (begin, count)
        assert count == 0 or ((written & pruned).any() and not got[written & pruned].any())


def test_sequence_column_passes():
    """D = 1024: lane groups of 64 lanes take two column passes; pruned rows are zeros in both"""
    bits, dim = (4, 8, 4), 1024
    rows, qt, remaps, idx, off, _, pruned = case(bits, dim)
    want, _ = P.gather(qt, dim, bits, remaps, idx, off, B)
    for odt in ("fp32", "bf16"):
        m = pmodule(rows, (dim,) * 3, bits, qt, remaps, output_dtype=TDT[odt])
        assert m.sequence_plan(dev(idx), dev(off))["col_passes"] == 2
        got = bits_of(m.lookup_sequence(dev(idx), dev(off)))
        assert same(got, want, odt) and not got[pruned].any() and got[~pruned].any(axis=1).all()
    # ... and the pooled lookup of the same request through its LDS burst of 1024 floats per row
    psw = case(bits, dim)[5]
    assert m.plan(dev(idx), dev(off))["stage_out"] == 1024
    out = bits_of(m.lookup(dev(idx), dev(off), dev(psw)))
    for t, w in enumerate(P.forward(qt, (dim,) * 3, bits, remaps, idx, off, B, psw)):
        assert same(out[:, t * dim:(t + 1) * dim], w, "bf16"), t


@pytest.mark.parametrize("first", [8, 4])
def test_sequence_many_tables(first):
    """tables of 3 lookups each, alternating format, three of every four pruned, D = 8: 100 tables -- borders and formats from LDS, a tile
    straddles 85 table borders -- and 300 -- beyond the LDS borders, from global memory"""
    for T in (100, 300):
        logical, bits = (11,) * T, tuple((first, 12 - first)[t % 2] for t in range(T))
        rng = np.random.default_rng(70 + T)
        masks = [None if t % 4 == 2 else rng.random(11) < 0.55 for t in range(T)]
        for k in masks:
            if k is not None:
                k[:2] = (True, False)
        remaps = [None if k is None else remap_of(k) for k in masks]
        rows = tuple(11 if k is None else int(k.sum()) for k in masks)
        qt = [rowquant.quantize_rows(x, b) for x, b in zip(float_tables(71, rows, (8,) * T), bits)]
        idx = rng.integers(0, 11, 3 * T).astype(np.int64)
        idx[0] = idx[TILE - 1] = idx[TILE] = idx[-1] = 1              # pruned: 0, 255, 256 and the last position belong to pruned tables
        off = np.arange(0, 3 * T + 1, 3, dtype=np.int64)
        table, _ = Q.owners(off, T, 1, idx.size)
        pruned = P.physical(remaps, idx, off, 1) < 0
        assert all(remaps[table[j]] is not None and pruned[j] for j in (0, TILE - 1, TILE, idx.size - 1))
        assert 0.30 <= pruned[np.isin(table, [t for t in range(T) if remaps[t] is not None])].mean() <= 0.60
        want, written = P.gather(qt, 8, bits, remaps, idx, off, 1)
        assert written.all() and len(set(table[:TILE].tolist())) >= 85
        m = pmodule(rows, (8,) * T, bits, qt, remaps, layout="tbd")
        p = m.sequence_plan(dev(idx), dev(off))
        assert p["lds_borders"] == (1 if T == 100 else 0) and p["grid"] == -(-3 * T // TILE) > 1 and p["group_lanes"] == 8
        for it in ("i32", "i64"):
            got = m.lookup_sequence(dev(idx, IDT[it]), dev(off, IDT[it])).cpu().numpy()
            assert R.same_f32(got, want) and not got[pruned].any(), (T, it)
        # pooled: bags of three, many all pruned or empty of kept rows
        out = m(dev(idx), dev(off)).cpu().numpy()
        assert out.shape == (T, 1, 8)
        assert_same([out[t] for t in range(T)], P.forward(qt, (8,) * T, bits, remaps, idx, off, 1), f"T = {T}")


# ---- bounds check ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [(4, 8, 4), (8, 8, 8)], ids=["484", "888"])
def test_bounds_check_reads_the_logical_rows(bits):
    dim = 64
    rows, qt, remaps, idx, off, psw, _ = case(bits, dim)
    dims = (dim,) * 3
    assert rows[0] < 90 < LOGICAL[0] and rows[2] < 290 < LOGICAL[2]
    ok_idx = idx.copy()
    ok_idx[1], ok_idx[off[2 * B] + 1] = 90, 290                       # in [rows_t, logical_rows_t): beyond the storage, inside the index space
    bad_idx = ok_idx.copy()
    bad_idx[4], bad_idx[off[2 * B] + 3] = LOGICAL[0], LOGICAL[2] + 5  # at and beyond logical_rows_t
    fixed = bad_idx.copy()
    fixed[4] = fixed[off[2 * B] + 3] = 0                              # repaired to 0, which is then remapped like any other index
    for mode in ("ignore", "warning"):
        m = pmodule(rows, dims, bits, qt, remaps, bounds_check_mode=mode)
        d_idx = dev(ok_idx)
        assert_same(split_bd(m.lookup(d_idx, dev(off), dev(psw)), dims), P.forward(qt, dims, bits, remaps, ok_idx, off, B, psw), f"{mode}: accepted")
        assert np.array_equal(d_idx.cpu().numpy(), ok_idx) and (mode == "ignore" or m.bounds_report()["bad_indices"] == 0)
        d_idx = dev(bad_idx)
        out = m.lookup(d_idx, dev(off), dev(psw))
        assert np.array_equal(d_idx.cpu().numpy(), fixed) and (mode == "ignore" or m.bounds_report()["bad_indices"] == 2)
        assert_same(split_bd(out, dims), P.forward(qt, dims, bits, remaps, fixed, off, B, psw), f"{mode}: repaired")
        d_idx = dev(bad_idx)
        seq = m.lookup_sequence(d_idx, dev(off))
        assert np.array_equal(d_idx.cpu().numpy(), fixed) and R.same_f32(seq.cpu().numpy(), P.gather(qt, dim, bits, remaps, fixed, off, B)[0])
        d_idx = dev(bad_idx)
        m.sanitize_(d_idx, dev(off))
        assert np.array_equal(d_idx.cpu().numpy(), fixed)
    fatal = pmodule(rows, dims, bits, qt, remaps, bounds_check_mode="fatal")
    assert_same(split_bd(fatal.lookup(dev(ok_idx), dev(off), dev(psw)), dims), P.forward(qt, dims, bits, remaps, ok_idx, off, B, psw), "fatal: accepted")
    assert R.same_f32(fatal.lookup_sequence(dev(ok_idx), dev(off)).cpu().numpy(), P.gather(qt, dim, bits, remaps, ok_idx, off, B)[0])
    for call in (fatal.lookup, fatal.lookup_sequence):
        d_idx = dev(bad_idx)
        with pytest.raises(IndexError, match="2 out-of-range indices"):
            call(d_idx, dev(off))
        assert np.array_equal(d_idx.cpu().numpy(), bad_idx)


# ---- the single-table modules ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b", [8, 4])
def test_single_table_modules(b):
    from param_amd import QuantizedEmbeddingBagMI355, QuantizedEmbeddingMI355

    dim, logical, nb = 64, 300, 12
    mask = keeps(31, (logical,), (0,))[0]
    rm, rows = remap_of(mask), int(mask.sum())
    q = rowquant.quantize_rows(float_tables(32 + b, (rows,), (dim,))[0], b)
    idx, off, psw = pruned_request(33, (logical,), [mask], nb)
    pruned = check_conditions([rm], idx, off, nb)
    for odt in ("fp32", "fp16"):
        e = QuantizedEmbeddingBagMI355(rows, dim, bitwidth=b, device=DEV, output_dtype=TDT[odt], weight=torch.from_numpy(q), index_remapping=torch.from_numpy(rm))
        assert e.pruned and e.logical_rows == [logical] and e.num_embeddings == rows
        for it in ("i32", "i64"):
            for w in (None, psw):
                got = bits_of(e(dev(idx, IDT[it]), dev(off[:-1], IDT[it]), None if w is None else dev(w)))
                assert same(got, P.forward([q], [dim], (b,), [rm], idx, off, nb, w)[0], odt), (b, odt, it)
        # a 2-D input: every row one bag of L lookups
        idx2 = idx[:40].reshape(8, 5)
        off2 = np.arange(0, 41, 5, dtype=np.int64)
        assert (rm[idx2] < 0).any() and (rm[idx2] >= 0).any()
        got = bits_of(e(dev(idx2), per_sample_weights=dev(psw[:40].reshape(8, 5))))
        assert same(got, P.forward([q], [dim], (b,), [rm], idx[:40], off2, 8, psw[:40])[0], odt)
        # an empty input: every bag is empty
        got = e(dev(np.zeros(0, dtype=np.int64)), dev(np.zeros(3, dtype=np.int64)))
        assert got.shape == (3, dim) and not bits_of(got).any()
        s = QuantizedEmbeddingMI355(rows, dim, bitwidth=b, device=DEV, output_dtype=TDT[odt], weight=torch.from_numpy(q), index_remapping=torch.from_numpy(rm))
        want = P.gather([q], dim, (b,), [rm], idx, np.zeros(1, dtype=np.int64), 1)[0]
        for it in ("i32", "i64"):
            got = bits_of(s(dev(idx, IDT[it])))
            assert same(got, want, odt) and not got[pruned].any(), (b, odt, it)
        got = s(dev(idx[:40].reshape(2, 4, 5)))
        assert got.shape == (2, 4, 5, dim) and same(bits_of(got).reshape(40, dim), want[:40], odt)
        assert s(dev(np.zeros((0, 3), dtype=np.int64))).shape == (0, 3, dim)
    # a table all of whose rows are pruned: nothing is stored, every row is zeros
    z = QuantizedEmbeddingMI355(0, dim, bitwidth=b, device=DEV, index_remapping=torch.full((5,), -1, dtype=torch.int32))
    assert not z(dev(np.arange(5))).any() and z(dev(np.arange(5))).shape == (5, dim)


def test_from_float_keep_quantises_the_kept_rows():
    from param_amd import QuantizedBatchedEmbeddingBagMI355 as QBM
    from param_amd import QuantizedEmbeddingBagMI355

    dim, bits = 64, [4, 8, 4]
    masks = keeps(41, LOGICAL, (0, 2))
    xs = float_tables(42, LOGICAL, (dim,) * 3)
    m = QBM.from_float([torch.from_numpy(x).to(DEV) for x in xs], bitwidth=bits, keep=[None if k is None else torch.from_numpy(k) for k in masks])
    assert m.pruned and m.logical_rows == list(LOGICAL) and m.rows == [int(masks[0].sum()), 40, int(masks[2].sum())] and m.weights.is_cuda
    qt, remaps = [], []
    for t, (x, k) in enumerate(zip(xs, masks)):
        qt.append(rowquant.quantize_rows(x if k is None else x[k], bits[t]))
        remaps.append(None if k is None else remap_of(k))
        assert np.array_equal(m.table(t).cpu().numpy(), qt[t])
        assert (m.index_remapping(t) is None) if k is None else np.array_equal(m.index_remapping(t).cpu().numpy(), remaps[t])
    idx, off, psw = pruned_request(43, LOGICAL, masks, B)
    check_conditions(remaps, idx, off, B)
    assert_same(split_bd(m(dev(idx), dev(off), dev(psw)), (dim,) * 3), P.forward(qt, (dim,) * 3, bits, remaps, idx, off, B, psw), "from_float")
    # the state_dict round trip into a module built from other remaps of the same lengths
    twin = QBM(m.rows, m.dims, bits, device=DEV, index_remapping=[None if r is None else torch.full((r.size,), -1, dtype=torch.int32) for r in remaps])
    assert not twin(dev(idx), dev(off)).any()                         # everything pruned: zeros
    twin.load_state_dict(m.state_dict())
    assert torch.equal(twin(dev(idx), dev(off), dev(psw)), m(dev(idx), dev(off), dev(psw)))
    bag = torch.nn.EmbeddingBag.from_pretrained(torch.from_numpy(xs[0]), mode="sum")
    e = QuantizedEmbeddingBagMI355.from_float(bag, bitwidth=8, keep=torch.from_numpy(masks[0]))
    assert e.pruned and np.array_equal(e.table(0).cpu().numpy(), rowquant.quantize_rows(xs[0][masks[0]], 8))
