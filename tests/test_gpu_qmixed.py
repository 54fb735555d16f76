"""ROW-QUANTISED TABLES of PER-TABLE FORMAT on the GPU: ``pm_embbag_fwd_qrows_mixed`` and ``pm_embedding_gather_qrows_mixed`` through
``QuantizedBatchedEmbeddingBagMI355(rows, dims, [bits per table])`` and as raw C calls, compared as BITS against tests/qmixed_rules.py
-- tests/qrows_rules.py / tests/qgather_rules.py applied table by table with that table's format.  Formats are interleaved both ways,
(8, 4, 8) and (4, 8, 4).  Modelled on tests/test_gpu_qrows.py and tests/test_gpu_qgather.py, whose helpers build the tables and
requests.  One reference per request, shared by the index types, layouts, output types and plan variants that must give the same bits."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import rowquant
from param_amd import _lib, quant
from tests import far_rows as F
from tests import out16_rules as O
from tests import qgather_rules as Q
from tests import qmixed_rules as M
from tests import qrows_cases as C
from tests import qrows_rules as R
from tests.test_gpu_qgather import PM_DT, TDT, bits_of, check_sentinel_rows, same, unroll_knob
from tests.test_gpu_qgather import request as seq_request
from tests.test_gpu_qrows import (DEV, GRID_B, GRID_LENS, GRID_ROWS, IDT, QB, assert_same, check_sentinel_out, dev, float_tables, module, request,
                                  split_bd, tuning)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FORMATS = [(8, 4, 8), (4, 8, 4)]
FMT = pytest.mark.parametrize("bits", FORMATS, ids=["848", "484"])
GRID_DIMS = {"bd": (8, 24, 128), "tbd": (24, 24, 24)}


def mqtables(seed, rows, dims, bits, scale=1.0):
    return [rowquant.quantize_rows(x, b) for x, b in zip(float_tables(seed, rows, dims, scale), bits)]


def alternating(T, first):
    return tuple((first, 12 - first)[t % 2] for t in range(T))


# ---- the main grid and its plan variants -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def grid_case(bits, layout):
    dims = GRID_DIMS[layout]
    qt = mqtables(11, GRID_ROWS, dims, bits)
    idx, off, psw = request(5, GRID_ROWS, GRID_LENS)
    want = {w: M.forward(qt, dims, bits, idx, off, GRID_B, psw if w else None) for w in (False, True)}
    return dims, qt, idx, off, psw, want


def raw_call(m, idx, off, psw, B, odt=torch.float32, gap=4, pad=12, bag_begin=0, bag_count=None):
    """``pm_embbag_fwd_qrows_mixed`` on a ``bd`` request whose output has ``gap`` unused columns between tables and ``pad`` behind the
    last: returns (out [B, stride] whose untouched bytes are 0xA5, the tables' first columns)"""
    ts = m._tables()
    op = _lib.pm_embbag_batch()
    ctypes.memmove(ctypes.byref(op), ctypes.byref(ts.request(idx, off, B, psw, bag_begin, bag_count, forward=True)), ctypes.sizeof(op))
    col0 = [c + gap * t for t, c in enumerate(ts.col0)]
    stride = col0[-1] + ts.dims[-1] + pad
    offs = torch.tensor(col0, dtype=torch.int64, device=DEV)
    op.out_offsets, op.out_stride = offs.data_ptr(), stride
    out = torch.full((B, stride * odt.itemsize), 0xA5, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().pm_embbag_fwd_qrows_mixed(ctypes.byref(op), ts.d_bits.data_ptr(), {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[odt],
                                                     out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.view(odt), col0


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("it", ["i32", "i64"])
@FMT
def test_main_grid(bits, it, weighted):
    for layout in ("bd", "tbd"):
        dims, qt, idx, off, psw, want = grid_case(bits, layout)
        m = module(GRID_ROWS, dims, list(bits), qt, layout=layout)
        assert m.bitwidth is None and m.bitwidths == list(bits)
        d_idx, d_off, d_w = dev(idx, IDT[it]), dev(off, IDT[it]), (dev(psw) if weighted else None)
        out = m(d_idx, d_off, d_w)
        assert not out.requires_grad and out.dtype == torch.float32
        if layout == "bd":
            assert out.shape == (GRID_B, sum(dims))
            assert_same(split_bd(out, dims), want[weighted], f"{bits} {it} bd")
            # the same request into an output with gaps between the tables' columns and behind the last: nothing else is written
            raw, col0 = raw_call(m, d_idx, d_off, d_w, GRID_B)
            check_sentinel_out(raw, col0, dims, want[weighted])
            # out=: the call's own tensor comes back, fully written
            buf = torch.full((GRID_B, sum(dims)), float("nan"), device=DEV)
            assert m.lookup(d_idx, d_off, d_w, out=buf) is buf
            assert_same(split_bd(buf, dims), want[weighted], f"{bits} {it} bd out=")
        else:
            assert out.shape == (3, GRID_B, 24)
            assert_same(list(out.cpu().numpy()), want[weighted], f"{bits} {it} tbd")


@FMT
def test_plan_variants(bits):
    """the main grid's request through every plan the knobs can ask for: the query reports it, the bits do not move"""
    dims, qt, idx, off, psw, want = grid_case(bits, "bd")
    m = module(GRID_ROWS, dims, list(bits), qt)
    d_idx, d_off, d_w = dev(idx), dev(off), dev(psw)
    NG = 256 // 16                                                # eight columns per lane: D = 128 is 16 lanes per bag, whatever the format
    seen = set()
    for unroll, want_u in ((0, 4), (1, 2), (2, 2), (3, 2), (4, 4), (8, 4)):
        for bpb in (0, NG, 64):
            for stage in (-1, 0):
                with tuning(unroll, bpb, stage):
                    for weighted in (False, True):
                        w = d_w if weighted else None
                        p = m.plan(d_idx, d_off, w)
                        tile = bpb or NG                      # (a request this small shrinks the automatic tile to one bag per lane group)
                        assert p["unroll"] == want_u and p["bags_per_block"] == tile and p["tiles_per_table"] == -(-GRID_B // tile)
                        assert p["stage_out"] == (128 if stage != 0 and tile * 128 * 4 <= 16384 else 0)      # 64 rows of 128 floats: no burst
                        seen.add((p["unroll"], p["bags_per_block"], p["stage_out"], weighted))
                        assert_same(split_bd(m(d_idx, d_off, w), dims), want[weighted], f"unroll {unroll} bpb {bpb} stage {stage}")
    assert {x[0] for x in seen} == {2, 4} and {x[1] for x in seen} == {NG, 64} and {x[2] for x in seen} == {0, 128}


# ---- the unstaged path -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [(8, 4), (4, 8)], ids=["84", "48"])
def test_unstaged_path_and_forced_tile(bits):
    rows, dims = (1000, 900), (128, 128)
    qt = mqtables(3, rows, dims, bits)
    m = module(rows, dims, list(bits), qt)
    idx, off, psw = request(7, rows, (1500,) * 8)                   # four bags of 1500 lookups per table
    want_u = M.forward(qt, dims, bits, idx, off, 4)
    want_w = M.forward(qt, dims, bits, idx, off, 4, psw)
    for it in ("i32", "i64"):
        d_idx, d_off = dev(idx, IDT[it]), dev(off, IDT[it])
        for u in (2, 4):
            with tuning(unroll=u):
                p = m.plan(d_idx, d_off, batch=4)
                assert p["tiles_per_table"] == 1 and p["idx_cap"] == 4096 < 6000 and p["unroll"] == u      # 6000 lookups per tile: not staged
                assert_same(split_bd(m.lookup(d_idx, d_off, batch=4), dims), want_u, f"unstaged {it} u{u}")
                assert m.plan(d_idx, d_off, dev(psw), batch=4)["idx_cap"] < 6000
                assert_same(split_bd(m.lookup(d_idx, d_off, dev(psw), batch=4), dims), want_w, f"unstaged weighted {it} u{u}")
    # 2 bags x 3 lookups per table, tile forced to 64 bags: the staged path with a partial (last and only) tile
    idx, off, psw = request(8, rows, (3, 3, 3, 3))
    want = M.forward(qt, dims, bits, idx, off, 2, psw)
    with tuning(bags_per_block=64):
        p = m.plan(dev(idx), dev(off), dev(psw), batch=2)
        assert p["bags_per_block"] == 64 and p["tiles_per_table"] == 1 and p["idx_cap"] >= 6
        assert_same(split_bd(m.lookup(dev(idx), dev(off), dev(psw), batch=2), dims), want, "forced tile")


# ---- batch slices ----------------------------------------------------------------------------------------------------------------------

@FMT
def test_batch_slices(bits):
    rows, dims, B = (50, 9, 20), (24, 128, 8), 10
    qt = mqtables(4, rows, dims, bits)
    m = module(rows, dims, list(bits), qt)
    rng = np.random.default_rng(1)
    idx, off, psw = request(9, rows, rng.integers(0, 12, 3 * B))
    d_idx, d_off, d_w = dev(idx), dev(off), dev(psw)
    for begin, count in ((0, 4), (3, 4), (6, 4), (5, 0), (0, 10)):
        want = M.forward(qt, dims, bits, idx, off, B, psw, begin, count)
        raw, col0 = raw_call(m, d_idx, d_off, d_w, B, bag_begin=begin, bag_count=count)
        check_sentinel_out(raw, col0, dims, want, rows_written=range(begin, begin + count))
        buf = torch.full((B, sum(dims)), -7.0, device=DEV)
        m.lookup(d_idx, d_off, d_w, out=buf, bag_begin=begin, bag_count=count)
        keep = np.ones(B, dtype=bool)
        keep[begin:begin + count] = False
        assert (buf.cpu().numpy()[keep] == -7.0).all()
        assert_same([b[begin:begin + count] for b in split_bd(buf, dims)], want, f"slice {begin}+{count}")


# ---- many tables -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", [8, 4])
def test_many_tables(first):
    T, B, L = 1100, 2, 3
    rows, dims, bits = (5,) * T, (8,) * T, alternating(T, first)
    qt = mqtables(6, rows, dims, bits)
    m = module(rows, dims, list(bits), qt, layout="tbd")
    idx, off, _ = request(10, rows, (L,) * (T * B))
    out = m(dev(idx), dev(off))
    assert out.shape == (T, B, 8)
    assert_same(list(out.cpu().numpy()), M.forward(qt, dims, bits, idx, off, B), "T = 1100")


# ---- the widest rows -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [(8, 4), (4, 8)], ids=["84", "48"])
def test_widest_rows(bits):
    rows, dims = (40, 30), (1024, 1024)
    qt = mqtables(12, rows, dims, bits)
    idx, off, psw = request(13, rows, (0, 7, 1, 30, 0, 2) * 2)
    want = M.forward(qt, dims, bits, idx, off, 6, psw)
    m = module(rows, dims, list(bits), qt)
    assert m.plan(dev(idx), dev(off), batch=6)["stage_out"] == 1024
    assert_same(split_bd(m.lookup(dev(idx), dev(off), dev(psw), batch=6), dims), want, "D = 1024")
    with tuning(stage_out=0):
        assert m.plan(dev(idx), dev(off), batch=6)["stage_out"] == 0
        assert_same(split_bd(m.lookup(dev(idx), dev(off), dev(psw), batch=6), dims), want, "D = 1024, no burst")
    m16 = module(rows, dims, list(bits), qt, output_dtype="bf16")
    got = m16.lookup(dev(idx), dev(off), dev(psw), batch=6).view(torch.int16).cpu().numpy().view(np.uint16)
    for t in range(2):
        assert O.same_bits(got[:, t * 1024:(t + 1) * 1024], O.round16(want[t], "bf16"), "bf16")
    with pytest.raises(ValueError, match="4096"):                   # the limit (launch_plan.h: kQrowsMaxDim)
        QB([1, 1], [4104, 8], list(bits))


# ---- 16-bit output ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", O.DTYPES)
@FMT
def test_out16_is_one_rounding(bits, dtype):
    rows, dims, B = (30, 11, 17), (24, 128, 8), 4
    xs = float_tables(14, rows, dims, scale=500.0)
    for x in xs:
        x[1] = 3000.0
    qt = [rowquant.quantize_rows(x, b) for x, b in zip(xs, bits)]
    idx, off, psw = request(15, rows, (0, 5, 40, 3) * 3)
    for t in range(3):
        idx[off[t * B + 2]:off[t * B + 3]] = 1                      # the bags of 40 sum 40 x 3000: beyond 65504, fp16 overflows to Inf
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float16
    m = module(rows, dims, list(bits), qt, output_dtype=tdt)
    overflowed = False
    for w in (None, psw):
        want32 = M.forward(qt, dims, bits, idx, off, B, w)
        want = [O.round16(x, dtype) for x in want32]
        assert all(np.array_equal(a, b) for a, b in zip(want, M.forward16(qt, dims, bits, idx, off, B, dtype, w)))
        out = m(dev(idx), dev(off), None if w is None else dev(w))
        assert out.dtype == tdt and out.shape == (B, sum(dims))
        got = out.view(torch.int16).cpu().numpy().view(np.uint16)
        edges = np.concatenate([[0], np.cumsum(dims)])
        for t in range(3):
            assert O.same_bits(got[:, edges[t]:edges[t + 1]], want[t], dtype), (bits, dtype, t)
        overflowed |= any(np.isinf(O.widen(x, dtype)).any() for x in want) and all(np.isfinite(x).all() for x in want32)
        raw, col0 = raw_call(m, dev(idx), dev(off), None if w is None else dev(w), B, odt=tdt)
        check_sentinel_out(raw, col0, dims, want)
    assert overflowed == (dtype == "fp16")                          # finite fp32 sums beyond 65504 leave as fp16 Inf; bf16 holds them


# ---- special tails ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", [8, 4])
def test_special_tails(first):
    """the fixtures' rows (read only): one 8-bit and one 4-bit table in one launch -- NaN and Inf reach the output, pooled and
    un-pooled, and no -0.0 comes from a finite row"""
    fx = np.load(os.path.join(HERE, "golden", "qrows_cases.npz"))
    gx = np.load(os.path.join(HERE, "golden", "qgather_cases.npz"))
    bits = (first, 12 - first)
    qt = [fx[f"special_q_{b}"] for b in bits]
    si, so = C.special_request()
    n, B = si.size, len(so)
    idx, off = np.concatenate([si, si]), np.concatenate([so, so + n])
    m = module((4, 4), (8, 8), list(bits), qt)
    want = M.forward(qt, (8, 8), bits, idx, off, B)
    for t in range(2):
        assert R.same_f32(fx[f"special_out_{bits[t]}"], want[t])
    got = split_bd(m.lookup(dev(idx), dev(off), batch=B), (8, 8))
    assert_same(got, want, "special tails")
    assert all(np.isnan(g).any() and np.isinf(g).any() for g in got)
    seq = m.lookup_sequence(dev(idx), dev(off), batch=B).cpu().numpy()
    assert R.same_f32(seq, M.gather(qt, 8, bits, idx, off, B)[0]) and np.isnan(seq[:n]).any() and np.isinf(seq[n:]).any()
    # signed zeros: the rows of the un-pooled fixture, every row once per table
    zt = [gx[f"zeros_q_{b}"] for b in bits]
    zi, zo = np.concatenate([np.arange(5), np.arange(5)[::-1]]), np.arange(10)
    want = M.gather(zt, 8, bits, zi, zo, 5)[0]
    assert R.same_f32(np.concatenate([gx[f"zeros_out_{bits[0]}"], gx[f"zeros_out_{bits[1]}"][::-1]]), want) and Q.negative_zeros(want) == 0
    for odt in ("fp32", "bf16", "fp16"):
        mz = module((5, 5), (8, 8), list(bits), zt, output_dtype=TDT[odt])
        got = bits_of(mz.lookup_sequence(dev(zi), dev(zo), batch=5))
        assert same(got, want, odt) and Q.negative_zeros(got if odt == "fp32" else O.widen(got, odt)) == 0, odt
        pooled = bits_of(mz.lookup(dev(zi), dev(zo), batch=5))      # bags of one: the same rows, [5, 16] = table-major halves
        assert np.array_equal(np.concatenate([pooled[:, :8], pooled[:, 8:]]), got), odt


# ---- bounds check ----------------------------------------------------------------------------------------------------------------------

@FMT
def test_bounds_check_mode(bits):
    rows, dims, B = (50, 9, 20), (24, 24, 24), 4
    qt = mqtables(17, rows, dims, bits)
    m = module(rows, dims, list(bits), qt, bounds_check_mode="warning")
    idx, off, psw = request(18, rows, (3, 0, 5, 2, 4, 1, 0, 6, 2, 2, 0, 1))
    bad_idx, bad_off = idx.copy(), off.copy()
    bad_idx[4] = 50                                                 # one past table 0's last row
    bad_off[6] = bad_off[5] - 2                                     # an offset that goes backwards
    d_idx, d_off = dev(bad_idx), dev(bad_off)
    out = m.lookup(d_idx, d_off, dev(psw), batch=B)
    rep = m.bounds_report()
    assert rep["bad_indices"] == 1 and rep["first_bad_index"] == 4 and rep["bad_offsets"] == 1
    fixed_idx, fixed_off = d_idx.cpu().numpy(), d_off.cpu().numpy()      # repaired in place
    assert fixed_idx[4] == 0 and fixed_off[6] == fixed_off[5] and (np.diff(fixed_off) >= 0).all() and fixed_off[-1] == idx.size
    assert_same(split_bd(out, dims), M.forward(qt, dims, bits, fixed_idx, fixed_off, B, psw), "repaired request")
    # the un-pooled call runs behind the same sanitiser; sanitize_ on its own repairs in place
    d_idx2 = dev(bad_idx)
    seq = m.lookup_sequence(d_idx2, dev(off), batch=B)
    assert m.bounds_report()["bad_indices"] == 1 and d_idx2.cpu().numpy()[4] == 0
    assert R.same_f32(seq.cpu().numpy(), M.gather(qt, 24, bits, d_idx2.cpu().numpy(), off, B)[0])
    d_idx3 = dev(bad_idx)
    m.sanitize_(d_idx3, dev(off), batch=B)
    assert d_idx3.cpu().numpy()[4] == 0
    fatal = module(rows, dims, list(bits), qt, bounds_check_mode="fatal")
    with pytest.raises(IndexError):
        fatal.lookup(dev(bad_idx), dev(off), batch=B)
    with pytest.raises(IndexError):
        fatal.lookup_sequence(dev(bad_idx), dev(off), batch=B)


# ---- equivalence with the single-format modules ----------------------------------------------------------------------------------------

@FMT
def test_equals_two_single_format_modules_over_the_same_bytes(bits):
    rows, dims, B = (300, 40, 77), (128, 128, 128), 8
    qt = mqtables(19, rows, dims, bits)
    idx, off, psw = request(20, rows, (0, 1, 20, 3, 100, 7, 0, 2) * 3)
    m = module(rows, dims, list(bits), qt)
    for odt in ("fp32", "bf16", "fp16"):
        mo = module(rows, dims, list(bits), qt, output_dtype=TDT[odt])
        for w in (None, psw):
            mixed = bits_of(mo.lookup(dev(idx), dev(off), None if w is None else dev(w)))
            seq = bits_of(mo.lookup_sequence(dev(idx), dev(off)))
            for b in (8, 4):
                ts = [t for t in range(3) if bits[t] == b]
                # the tables of format b alone: their bytes, their part of the request (offsets rebased table by table)
                parts = [(idx[off[t * B]:off[(t + 1) * B]], off[t * B:(t + 1) * B] - off[t * B], None if w is None else w[off[t * B]:off[(t + 1) * B]])
                         for t in ts]
                sizes = np.cumsum([0] + [p[0].size for p in parts])
                s_idx = np.concatenate([p[0] for p in parts])
                s_off = np.concatenate([p[1] + sizes[k] for k, p in enumerate(parts)] + [[s_idx.size]])
                s_w = None if w is None else dev(np.concatenate([p[2] for p in parts]))
                single = module([rows[t] for t in ts], [dims[t] for t in ts], b, [qt[t] for t in ts], output_dtype=TDT[odt])
                assert single.bitwidth == b
                got = bits_of(single.lookup(dev(s_idx), dev(s_off), s_w))
                for k, t in enumerate(ts):
                    assert np.array_equal(got[:, k * 128:(k + 1) * 128], mixed[:, t * 128:(t + 1) * 128]), (bits, odt, b, t)
                if w is None:
                    got = bits_of(single.lookup_sequence(dev(s_idx), dev(s_off)))
                    for k, t in enumerate(ts):
                        assert np.array_equal(got[sizes[k]:sizes[k + 1]], seq[off[t * B]:off[(t + 1) * B]]), (bits, odt, b, t)
    assert m.plan(dev(idx), dev(off))["unroll"] == 4


@pytest.mark.parametrize("b", [8, 4])
def test_an_all_equal_sequence_is_the_int(b):
    rows, dims, B = (300, 40), (128, 24), 8
    qt = mqtables(21, rows, dims, (b, b))
    idx, off, psw = request(22, rows, (0, 1, 20, 3, 100, 7, 0, 2) * 2)
    seq, one = module(rows, dims, [b, b], qt), module(rows, dims, b, qt)
    assert seq.bitwidth == one.bitwidth == b and seq._tables().d_bits is None
    assert seq.plan(dev(idx), dev(off), dev(psw)) == one.plan(dev(idx), dev(off), dev(psw))
    assert torch.equal(seq.weights, one.weights)
    assert np.array_equal(bits_of(seq(dev(idx), dev(off), dev(psw))), bits_of(one(dev(idx), dev(off), dev(psw))))
    assert_same(split_bd(seq(dev(idx), dev(off), dev(psw)), dims), R.forward(qt, dims, b, idx, off, B, psw), "all-equal sequence")
    # ... and the plan of a mixed module over the same dims is its own query's: eight columns per lane
    mixed = module(rows, dims, [b, 12 - b], mqtables(21, rows, dims, (b, 12 - b)))
    assert mixed.plan(dev(idx), dev(off))["bags_per_block"] % 16 == 0


def test_quantize_from_and_from_float_per_table():
    from param_amd import QuantizedBatchedEmbeddingBagMI355 as QBM

    rows, dims, bits = (40, 9, 21), (64, 32, 64), [4, 8, 4]
    xs = [torch.from_numpy(x).to(DEV) for x in float_tables(23, rows, dims)]
    m = QBM.from_float(xs, bitwidth=bits, layout="bd")
    assert m.bitwidths == bits and m.bitwidth is None and m.weights.is_cuda
    for t in range(3):
        assert np.array_equal(m.table(t).cpu().numpy(), rowquant.quantize_rows(xs[t].cpu().numpy(), bits[t]))
        assert torch.equal(m.dequantized_table(t), quant.dequantize_rows(m.table(t), dims[t], bits[t]))      # table t's own format
    twin = QB(list(rows), list(dims), bits)
    idx, off, _ = request(24, rows, (2, 0, 5) * 3)
    assert not twin(dev(idx), dev(off)).any()                       # zero bytes dequantise to zeros in either format
    twin.load_state_dict(m.state_dict())
    assert torch.equal(twin.weights, m.weights)
    qt = [m.table(t).cpu().numpy() for t in range(3)]
    assert_same(split_bd(twin(dev(idx), dev(off)), dims), M.forward(qt, dims, bits, idx, off, 3), "state_dict round trip")


# ---- un-pooled -------------------------------------------------------------------------------------------------------------------------

SEQ_LENS = (0, 4, 3, 100, 2) + (20, 0, 0, 39, 1) + (7, 0, 90, 1, 33)      # tile 0 holds positions of all three tables; N = 300


@pytest.mark.parametrize("dim", [8, 128, 1024])
@FMT
def test_sequence_main_request(bits, dim):
    rows, B = GRID_ROWS, 5
    qt = mqtables(31, rows, (dim,) * 3, bits)
    idx, off = seq_request(6, rows, SEQ_LENS)
    want, written = M.gather(qt, dim, bits, idx, off, B)
    table, _ = Q.owners(off, 3, B, idx.size)
    assert written.all() and idx.size == 300 and set(table[:256].tolist()) == {0, 1, 2}
    for odt in ("fp32", "bf16", "fp16"):
        m = module(rows, (dim,) * 3, list(bits), qt, layout="tbd", output_dtype=TDT[odt])
        for it in ("i32", "i64"):
            d_idx, d_off = dev(idx, IDT[it]), dev(off, IDT[it])
            out = m.lookup_sequence(d_idx, d_off)
            assert out.shape == (300, dim) and out.dtype == TDT[odt] and not out.requires_grad
            assert same(bits_of(out), want, odt), (bits, dim, odt, it)
        assert same(bits_of(m.lookup_sequence(d_idx, d_off[:-1], batch=B)), want, odt)      # offsets without the trailing entry
        buf = torch.full((300, dim), float("nan"), device=DEV, dtype=TDT[odt])
        assert m.lookup_sequence(d_idx, d_off, out=buf) is buf and same(bits_of(buf), want, odt)
    p = m.sequence_plan(d_idx, d_off)
    assert p["grid"] == 2 and p["tile"] == 256 and p["vec"] == 8 and p["group_lanes"] == min(64, max(8, dim // 8)) and p["lds_borders"] == 1
    assert p["col_passes"] == (2 if dim == 1024 else 1)
    # every rows-in-flight value the knob can ask for
    seen = set()
    for knob, u in ((1, 1), (2, 2), (3, 2), (4, 4), (6, 4), (8, 8)):
        with unroll_knob(knob):
            assert m.sequence_plan(d_idx, d_off)["unroll"] == u
            assert same(bits_of(m.lookup_sequence(d_idx, d_off)), want, "fp16"), (bits, dim, knob)
            seen.add(u)
    assert seen == {1, 2, 4, 8}
    # an empty input: an empty result, nothing launched
    e = m.lookup_sequence(dev(np.zeros(0, dtype=np.int64)), dev(np.zeros(3 * B + 1, dtype=np.int64)), batch=B)
    assert e.shape == (0, dim) and e.dtype == torch.float16
    with pytest.raises(ValueError, match="out must be a contiguous"):
        m.lookup_sequence(d_idx, d_off, out=torch.empty((300, dim), dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("first", [8, 4])
def test_sequence_one_wave_serves_both_formats(first):
    """tables of 3 lookups each, alternating format, D = 8 (lane groups of 8 lanes: a wave holds 8 rows at a time, of both formats): 100
    tables -- the borders and formats from LDS, two tiles -- and 300 -- beyond the LDS borders, from global memory"""
    for T in (100, 300):
        rows, bits = (7,) * T, alternating(T, first)
        qt = mqtables(71, rows, (8,) * T, bits)
        idx, off = seq_request(72, rows, (3,) * T)
        want, written = M.gather(qt, 8, bits, idx, off, 1)
        table, _ = Q.owners(off, T, 1, idx.size)
        assert written.all() and len(set(table[:256].tolist())) >= 3 and table[:8].tolist() == [0, 0, 0, 1, 1, 1, 2, 2]
        m = module(rows, (8,) * T, list(bits), qt, layout="tbd")
        p = m.sequence_plan(dev(idx), dev(off))
        assert p["lds_borders"] == (1 if T == 100 else 0) and p["grid"] == -(-3 * T // 256) > 1 and p["group_lanes"] == 8
        assert R.same_f32(m.lookup_sequence(dev(idx), dev(off)).cpu().numpy(), want), T
        assert R.same_f32(m.lookup_sequence(dev(idx, torch.int32), dev(off, torch.int32)).cpu().numpy(), want), T


@FMT
def test_sequence_batch_slices(bits):
    rows, dim, B = (50, 9, 20), 24, 10
    qt = mqtables(61, rows, (dim,) * 3, bits)
    m = module(rows, (dim,) * 3, list(bits), qt)
    idx, off = seq_request(62, rows, np.random.default_rng(2).integers(0, 40, 3 * B))
    d_idx, d_off = dev(idx), dev(off)
    for begin, count in ((0, 4), (3, 4), (6, 4), (5, 0), (0, 10)):      # first, middle, last, empty, whole
        want, written = M.gather(qt, dim, bits, idx, off, B, begin, count)
        assert written.any() == (count > 0) and written.all() == (count == B)
        buf = torch.full((idx.size, dim), -7.0, device=DEV)
        m.lookup_sequence(d_idx, d_off, out=buf, bag_begin=begin, bag_count=count)
        got = buf.cpu().numpy()
        assert (got[~written] == -7.0).all() and R.same_f32(got[written], want[written]), (begin, count)
        fresh = m.lookup_sequence(d_idx, d_off, bag_begin=begin, bag_count=count).cpu().numpy()      # allocated here: zeros outside
        assert R.same_f32(fresh, want)


def raw_sequence_call(m, idx, off, B, odt, stride, bag_begin=0, bag_count=None, it="i64"):
    """``pm_embedding_gather_qrows_mixed`` into ``[N, stride]`` elements of ``odt`` whose untouched bytes are 0xA5"""
    ts = m._tables()
    d_idx, d_off = dev(idx, IDT[it]), dev(off, IDT[it])
    op = _lib.pm_embbag_batch()
    ctypes.memmove(ctypes.byref(op), ctypes.byref(ts.request(d_idx, d_off, B, None, bag_begin, bag_count, forward=True)), ctypes.sizeof(op))
    out = torch.full((idx.size, stride * TDT[odt].itemsize), 0xA5, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().pm_embedding_gather_qrows_mixed(ctypes.byref(op), ts.d_bits.data_ptr(), PM_DT[odt], out.data_ptr(), stride,
                                                           torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("odt", ["fp32", "bf16", "fp16"])
@FMT
def test_raw_sequence_call_mixed_dims_with_a_padded_stride(bits, odt):
    rows, dims, B = (9, 50, 30), (8, 24, 128), 4
    qt = mqtables(41, rows, dims, bits)
    m = module(rows, dims, list(bits), qt)
    idx, off = seq_request(42, rows, (0, 30, 5, 70) + (3, 0, 90, 40) + (60, 1, 0, 14))      # N = 313: all three tables inside tile 0
    stride = max(dims) + 12
    for begin, count in ((0, B), (1, 2)):
        per_table = M.gather_tables(qt, dims, bits, idx, off, B, begin, count)
        for it in ("i32", "i64"):
            check_sentinel_rows(raw_sequence_call(m, idx, off, B, odt, stride, begin, count, it), per_table, odt)
    with pytest.raises(ValueError, match="one common embedding dim"):
        m.lookup_sequence(dev(idx), dev(off))


# ---- far addresses ---------------------------------------------------------------------------------------------------------------------

def test_far_rows_of_both_formats_in_one_launch():
    """an 8-bit and a 4-bit table of D = 1024, each just past 2^32 bytes, zero but for a few rows around the 2^31 and 2^32 marks (bytes
    and elements: tests/far_rows.py), looked up pooled and un-pooled in one launch each and compared with the rule on a compacted twin"""
    import param_amd

    D, bits, B = 1024, (8, 4), len(F.STAGED_LENS)
    probes = [F.probe_rows(D, bits=b) for b in bits]
    rows = [F.table_rows(p) for p in probes]
    nbytes = sum(r * F.row_bytes(D, bits=b) for r, b in zip(rows, bits))
    assert all(r * F.row_bytes(D, bits=b) > 2 ** 32 for r, b in zip(rows, bits))
    param_amd.load_library()
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + (8 << 30):
        pytest.skip(f"needs {nbytes / 2**30:.1f} GiB + 8 GiB of free HBM, {free / 2**30:.0f} GiB available")
    rng = np.random.default_rng(77)
    twin = [rowquant.quantize_rows((rng.standard_normal((len(p), D)) * 3).astype(np.float32), b) for p, b in zip(probes, bits)]
    m = QB(rows, D, list(bits))                                     # (torch.zeros: the slab is zero)
    for t in range(2):
        d = torch.from_numpy(twin[t]).to(DEV)
        for i, r in enumerate(probes[t]):
            m.table(t)[int(r)].copy_(d[i])
    reqs = [F.request(probes[t], F.STAGED_LENS, seed=5 + t) for t in range(2)]
    n0 = reqs[0][0].size
    idx = np.concatenate([reqs[0][0], reqs[1][0]])
    cidx = np.concatenate([F.compact(probes[t], reqs[t][0]) for t in range(2)])
    off = np.concatenate([reqs[0][1][:-1], reqs[1][1] + n0])
    psw = (rng.standard_normal(idx.size) * 1.5).astype(np.float32)
    assert idx.max() * F.row_bytes(D, bits=8) > 2 ** 32 and reqs[1][0].max() * F.row_bytes(D, bits=4) > 2 ** 32
    try:
        for it in ("i32", "i64"):
            for w in (None, psw):
                got = m.lookup(dev(idx, IDT[it]), dev(off, IDT[it]), None if w is None else dev(w), batch=B)
                assert_same(split_bd(got, (D, D)), M.forward(twin, (D, D), bits, cidx, off, B, w), f"far pooled {it}")
            seq = m.lookup_sequence(dev(idx, IDT[it]), dev(off, IDT[it]), batch=B)
            want, written = M.gather(twin, D, bits, cidx, off, B)
            assert written.all() and R.same_f32(seq.cpu().numpy(), want) and seq[n0:].any() and seq[:n0].any(), it
    finally:
        del m
        torch.cuda.empty_cache()
