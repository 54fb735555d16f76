"""ROW-QUANTISED TABLES on the GPU: ``pm_embbag_fwd_qrows`` through the two modules, compared as BITS against tests/qrows_rules.py (the
numpy restatement that tests/test_qrows_host.py holds to torch's CPU operators).  One reference per request, shared by the index types,
layouts and plan variants that must all give the same bits."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import rowquant
from param_amd import _lib
from tests import out16_rules as O
from tests import qrows_cases as C
from tests import qrows_rules as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
IDT = {"i32": torch.int32, "i64": torch.int64}
MIXED = {8: (4, 20, 128), 4: (8, 24, 128)}
GRID_ROWS, GRID_B = (1, 7, 1000), 5
GRID_LENS = (0, 4, 0, 300, 2, 1, 0, 9, 3, 5, 7, 2, 0, 6, 0)      # empty first, middle and last bags, one bag of 300


def QB(*a, **kw):
    from param_amd import QuantizedBatchedEmbeddingBagMI355
    return QuantizedBatchedEmbeddingBagMI355(*a, device=DEV, **kw)


def float_tables(seed, rows, dims, scale=1.0):
    rng = np.random.default_rng(seed)
    xs = []
    for r, d in zip(rows, dims):
        x = (rng.standard_normal((r, d)) * (rng.random((r, 1)) * 4 + 0.05) * scale).astype(np.float32)
        x[0] = 0.75                                               # a row whose range is zero
        xs.append(x)
    return xs


def qtables(seed, rows, dims, bits, scale=1.0):
    return [rowquant.quantize_rows(x, bits) for x in float_tables(seed, rows, dims, scale)]


def request(seed, rows, lens, weighted=True):
    """(indices int64, offsets int64 [T*B+1], psw fp32) for bag lengths ``lens`` (table-major)"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    B = len(lens) // len(rows)
    tab = np.repeat(np.arange(len(rows)), lens.reshape(len(rows), B).sum(axis=1))
    idx = (rng.random(int(lens.sum())) * np.asarray(rows)[tab]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    psw = (rng.standard_normal(idx.size) * 1.5).astype(np.float32)
    return idx, off, psw


def module(rows, dims, bits, qt, **kw):
    m = QB(rows, dims, bits, **kw)
    host = np.zeros(m.weights.numel(), dtype=np.uint8)
    for t, q in enumerate(qt):
        host[m._starts[t]:m._starts[t] + q.size] = q.reshape(-1)
    m.weights.copy_(torch.from_numpy(host))
    return m


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def split_bd(out, dims):
    """a ``[B, sum D]`` result as the list of per-table arrays the rule returns"""
    a = out.cpu().numpy()
    edges = np.concatenate([[0], np.cumsum(dims)])
    return [a[:, edges[t]:edges[t + 1]] for t in range(len(dims))]


def assert_same(got_list, want_list, what=""):
    assert len(got_list) == len(want_list)
    for t, (g, w) in enumerate(zip(got_list, want_list)):
        assert R.same_f32(g, w), f"{what} table {t}: {int((np.asarray(g).view(np.uint32) != np.asarray(w).view(np.uint32)).sum())} elements differ"


class tuning:
    """pm_set_tuning / pm_set_forward_tuning for the block; the defaults come back"""

    def __init__(self, unroll=0, bags_per_block=0, stage_out=-1):
        self.args = (unroll, bags_per_block, stage_out)

    def __enter__(self):
        _lib.set_tuning(unroll=self.args[0], bags_per_block=self.args[1])
        _lib.set_forward_tuning(stage_out=self.args[2])

    def __exit__(self, *exc):
        _lib.set_tuning()
        _lib.set_forward_tuning()
        return False


# ---- 1 / 2: the main grid and its plan variants ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def grid_case(bits, layout):
    dims = MIXED[bits] if layout == "bd" else (24, 24, 24)
    qt = qtables(11 + bits, GRID_ROWS, dims, bits)
    idx, off, psw = request(5, GRID_ROWS, GRID_LENS)
    want = {w: R.forward(qt, dims, bits, idx, off, GRID_B, psw if w else None) for w in (False, True)}
    return dims, qt, idx, off, psw, want


def raw_call(m, idx, off, psw, B, odt=torch.float32, gap=4, pad=12, bag_begin=0, bag_count=None):
    """``pm_embbag_fwd_qrows`` on a ``bd`` request whose output has ``gap`` unused columns between tables and ``pad`` behind the last:
    returns (out [B, stride] whose untouched bytes are 0xA5, the tables' first columns)"""
    ts = m._tables()
    op = _lib.pm_embbag_batch()
    ctypes.memmove(ctypes.byref(op), ctypes.byref(ts.request(idx, off, B, psw, bag_begin, bag_count, forward=True)), ctypes.sizeof(op))
    col0 = [c + gap * t for t, c in enumerate(ts.col0)]
    stride = col0[-1] + ts.dims[-1] + pad
    offs = torch.tensor(col0, dtype=torch.int64, device=DEV)
    op.out_offsets, op.out_stride = offs.data_ptr(), stride
    out = torch.full((B, stride * odt.itemsize), 0xA5, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().pm_embbag_fwd_qrows(ctypes.byref(op), m.bitwidth, {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[odt],
                                               out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.view(odt), col0


def check_sentinel_out(out, col0, dims, want, rows_written=None):
    """the tables' columns of the written rows hold ``want``; every other byte is still 0xA5"""
    a = out.cpu().view(torch.uint8).numpy().reshape(out.shape[0], -1)
    e = out.dtype.itemsize
    touched = np.zeros(a.shape, dtype=bool)
    rows_written = range(out.shape[0]) if rows_written is None else rows_written
    for t, (c, d) in enumerate(zip(col0, dims)):
        block = np.ascontiguousarray(a[list(rows_written), c * e:(c + d) * e])
        if e == 4:
            assert R.same_f32(block.view(np.float32), want[t]), f"table {t}"
        else:
            assert np.array_equal(block.view(np.uint16), want[t]), f"table {t}"
        touched[np.ix_(list(rows_written), range(c * e, (c + d) * e))] = True
    assert (a[~touched] == 0xA5).all(), "bytes outside the tables' columns / the slice were written"


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("it", ["i32", "i64"])
@pytest.mark.parametrize("bits", [8, 4])
def test_main_grid(bits, it, weighted):
    for layout in ("bd", "tbd"):
        dims, qt, idx, off, psw, want = grid_case(bits, layout)
        m = module(GRID_ROWS, dims, bits, qt, layout=layout)
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


@pytest.mark.parametrize("bits", [8, 4])
def test_plan_variants(bits):
    """the main grid's request through every plan the knobs can ask for: the query reports it, the bits do not move"""
    dims, qt, idx, off, psw, want = grid_case(bits, "bd")
    m = module(GRID_ROWS, dims, bits, qt)
    d_idx, d_off, d_w = dev(idx), dev(off), dev(psw)
    NG = 256 // (16 if bits == 8 else 8)                          # two dwords of codes per lane: D = 128 is 16 / 8 lanes per bag
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


# ---- 3: the unstaged path -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 4])
def test_unstaged_path_and_forced_tile(bits):
    rows, dims = (1000,), (128,)
    qt = qtables(3, rows, dims, bits)
    m = module(rows, dims, bits, qt)
    idx, off, psw = request(7, rows, (1500,) * 4)
    want_u = R.forward(qt, dims, bits, idx, off, 4)
    want_w = R.forward(qt, dims, bits, idx, off, 4, psw)
    for it in ("i32", "i64"):
        d_idx, d_off = dev(idx, IDT[it]), dev(off, IDT[it])
        for u in (2, 4):
            with tuning(unroll=u):
                p = m.plan(d_idx, d_off, batch=4)
                assert p["tiles_per_table"] == 1 and p["idx_cap"] == 4096 < idx.size and p["unroll"] == u      # 6000 lookups: not staged
                assert_same(split_bd(m.lookup(d_idx, d_off, batch=4), dims), want_u, f"unstaged {it} u{u}")
                assert m.plan(d_idx, d_off, dev(psw), batch=4)["idx_cap"] < idx.size
                assert_same(split_bd(m.lookup(d_idx, d_off, dev(psw), batch=4), dims), want_w, f"unstaged weighted {it} u{u}")
    # 2 bags x 3 lookups, tile forced to 64 bags: the staged path with a partial (last and only) tile
    idx, off, psw = request(8, rows, (3, 3))
    want = R.forward(qt, dims, bits, idx, off, 2, psw)
    with tuning(bags_per_block=64):
        p = m.plan(dev(idx), dev(off), dev(psw), batch=2)
        assert p["bags_per_block"] == 64 and p["tiles_per_table"] == 1 and p["idx_cap"] >= 6
        assert_same(split_bd(m.lookup(dev(idx), dev(off), dev(psw), batch=2), dims), want, "forced tile")


# ---- 4: batch slices ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 4])
def test_batch_slices(bits):
    rows, dims, B = (50, 9), MIXED[bits][1:], 10
    qt = qtables(4, rows, dims, bits)
    m = module(rows, dims, bits, qt)
    rng = np.random.default_rng(1)
    idx, off, psw = request(9, rows, rng.integers(0, 12, 2 * B))
    d_idx, d_off, d_w = dev(idx), dev(off), dev(psw)
    for begin, count in ((0, 4), (3, 4), (6, 4), (5, 0), (0, 10)):
        want = R.forward(qt, dims, bits, idx, off, B, psw, begin, count)
        raw, col0 = raw_call(m, d_idx, d_off, d_w, B, bag_begin=begin, bag_count=count)
        check_sentinel_out(raw, col0, dims, want, rows_written=range(begin, begin + count))
        buf = torch.full((B, sum(dims)), -7.0, device=DEV)
        m.lookup(d_idx, d_off, d_w, out=buf, bag_begin=begin, bag_count=count)
        keep = np.ones(B, dtype=bool)
        keep[begin:begin + count] = False
        assert (buf.cpu().numpy()[keep] == -7.0).all()
        assert_same([b[begin:begin + count] for b in split_bd(buf, dims)], want, f"slice {begin}+{count}")


# ---- 5: many tables -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 4])
def test_many_tables(bits):
    T, B, L = 1100, 2, 3
    rows, dims = (5,) * T, (8,) * T
    qt = qtables(6, rows, dims, bits)
    m = module(rows, dims, bits, qt, layout="tbd")
    idx, off, _ = request(10, rows, (L,) * (T * B))
    out = m(dev(idx), dev(off))
    assert out.shape == (T, B, 8)
    assert_same(list(out.cpu().numpy()), R.forward(qt, dims, bits, idx, off, B), "T = 1100")


# ---- 6: the widest rows ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 4])
def test_widest_rows(bits):
    rows, dims = (40,), (1024,)
    qt = qtables(12, rows, dims, bits)
    idx, off, psw = request(13, rows, (0, 7, 1, 30, 0, 2))
    want = R.forward(qt, dims, bits, idx, off, 6, psw)
    m = module(rows, dims, bits, qt)
    assert_same(split_bd(m.lookup(dev(idx), dev(off), dev(psw), batch=6), dims), want, "D = 1024")
    with tuning(stage_out=0):
        assert m.plan(dev(idx), dev(off), batch=6)["stage_out"] == 0
        assert_same(split_bd(m.lookup(dev(idx), dev(off), dev(psw), batch=6), dims), want, "D = 1024, no burst")
    m16 = module(rows, dims, bits, qt, output_dtype="bf16")
    got = m16.lookup(dev(idx), dev(off), dev(psw), batch=6)
    assert O.same_bits(got.view(torch.int16).cpu().numpy().view(np.uint16), O.round16(want[0], "bf16"), "bf16")
    with pytest.raises(ValueError, match="4096"):                   # the limit (launch_plan.h: kQrowsMaxDim)
        QB([1], [4104], bits)


# ---- 7: 16-bit output -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", O.DTYPES)
@pytest.mark.parametrize("bits", [8, 4])
def test_out16_is_one_rounding(bits, dtype):
    rows, dims, B = (30, 11), MIXED[bits][1:], 6
    xs = float_tables(14, rows, dims, scale=500.0)
    xs[0][1] = 3000.0
    qt = [rowquant.quantize_rows(x, bits) for x in xs]
    idx, off, psw = request(15, rows, (0, 5, 1, 40, 3, 0, 2, 0, 8, 1, 6, 0))
    idx[6:46] = 1                                                   # the bag of 40 sums 40 x 3000: beyond 65504, fp16 overflows to Inf
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float16
    m = module(rows, dims, bits, qt, output_dtype=tdt)
    overflowed = False
    for w in (None, psw):
        want32 = R.forward(qt, dims, bits, idx, off, B, w)
        want = [O.round16(x, dtype) for x in want32]
        out = m(dev(idx), dev(off), None if w is None else dev(w))
        assert out.dtype == tdt and out.shape == (B, sum(dims))
        got = out.view(torch.int16).cpu().numpy().view(np.uint16)
        edges = np.concatenate([[0], np.cumsum(dims)])
        for t in range(2):
            assert O.same_bits(got[:, edges[t]:edges[t + 1]], want[t], dtype), (bits, dtype, t)
        overflowed |= any(np.isinf(O.widen(x, dtype)).any() for x in want) and all(np.isfinite(x).all() for x in want32)
        raw, col0 = raw_call(m, dev(idx), dev(off), None if w is None else dev(w), B, odt=tdt)
        check_sentinel_out(raw, col0, dims, want)
    assert overflowed == (dtype == "fp16")                          # finite fp32 sums beyond 65504 leave as fp16 Inf; bf16 holds them


# ---- 8: a bag of one is dequantize_rows -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 4])
def test_bag_of_one_equals_dequantize_rows_kernel(bits):
    rows, dims = (200,), (128,)
    x = torch.from_numpy(float_tables(16, rows, dims)[0]).to(DEV)
    m = QB(rows, dims, bits)
    m.quantize_from_(0, x)                                          # the existing kernels on both sides
    assert np.array_equal(m.table(0).cpu().numpy(), rowquant.quantize_rows(x.cpu().numpy(), bits))
    perm = torch.randperm(200, generator=torch.Generator().manual_seed(1)).to(DEV)
    out = m.lookup(perm, torch.arange(200, device=DEV), batch=200)
    assert torch.equal(out, m.dequantized_table(0)[perm])          # as values


# ---- 9 / 10: the fixture --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(HERE, "golden", "qrows_cases.npz"))


@pytest.mark.parametrize("bits", [8, 4])
def test_special_tails(fixture, bits):
    q = fixture[f"special_q_{bits}"]
    si, so = C.special_request()
    m = module((4,), (8,), bits, [q])
    want = R.forward([q], [8], bits, si, so, len(so))[0]
    assert R.same_f32(fixture[f"special_out_{bits}"], want)
    got = m.lookup(dev(si), dev(so), batch=len(so)).cpu().numpy()
    assert R.same_f32(got, want) and np.isnan(got).any() and np.isinf(got).any()


@pytest.mark.parametrize("bits", [8, 4])
def test_fixture_through_the_module(fixture, bits):
    """torch's recorded results, through the kernel (the widths the column rules admit: every D for 8 bits, D % 8 == 0 for 4 bits)"""
    idx, off, psw = fixture["indices"], fixture["offsets"], fixture["psw"]
    ran = 0
    for dim in C.DIMS:
        if dim % (4 if bits == 8 else 8):
            with pytest.raises(ValueError, match="multiple of"):
                QB([C.ROWS], [dim], bits)
            continue
        m = module((C.ROWS,), (dim,), bits, [fixture[f"q_{bits}_{dim}"]])
        for it in ("i32", "i64"):
            for weighted in (False, True):
                got = m.lookup(dev(idx, IDT[it]), dev(off, IDT[it]), dev(psw) if weighted else None, batch=len(off)).cpu().numpy()
                assert R.same_f32(got, fixture[C.key(bits, dim, it, weighted)]), (bits, dim, it, weighted)
                ran += 1
    assert ran == (20 if bits == 8 else 12)


# ---- 11: bounds check -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 4])
def test_bounds_check_warning_repairs_the_request(bits):
    rows, dims, B = (50, 9), MIXED[bits][1:], 4
    qt = qtables(17, rows, dims, bits)
    m = module(rows, dims, bits, qt, bounds_check_mode="warning")
    idx, off, psw = request(18, rows, (3, 0, 5, 2, 4, 1, 0, 6))
    bad_idx, bad_off = idx.copy(), off.copy()
    bad_idx[4] = 50                                                 # one past table 0's last row
    bad_off[6] = bad_off[5] - 2                                     # an offset that goes backwards
    d_idx, d_off = dev(bad_idx), dev(bad_off)
    out = m.lookup(d_idx, d_off, dev(psw), batch=B)
    rep = m.bounds_report()
    assert rep["bad_indices"] == 1 and rep["first_bad_index"] == 4 and rep["bad_offsets"] >= 1
    fixed_idx, fixed_off = d_idx.cpu().numpy(), d_off.cpu().numpy()      # repaired in place
    assert fixed_idx[4] == 0 and rep["bad_offsets"] == 1 and fixed_off[6] == fixed_off[5] and (np.diff(fixed_off) >= 0).all() and fixed_off[-1] == idx.size
    assert_same(split_bd(out, dims), R.forward(qt, dims, bits, fixed_idx, fixed_off, B, psw), "repaired request")
    clean = module(rows, dims, bits, qt, bounds_check_mode="fatal")
    with pytest.raises(IndexError):
        clean.lookup(dev(bad_idx), dev(off), batch=B)


# ---- 12: against the fp32 module over the dequantised tables --------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 4])
def test_against_fp32_module_over_dequantized_tables(bits):
    """NOT bit-identical, by the rule: the fp32 forward rounds every dequantised element, then adds.  Per element
    |diff| <= (2L + 2) 2^-24 sum_j |w_j| (|bias_j| + code scale_j): L terms, each rounded twice on either side."""
    from param_amd import BatchedEmbeddingBagMI355

    rows, dims, B = (300, 40), (128, 128), 8
    qt = qtables(19, rows, dims, bits)
    m = module(rows, dims, bits, qt)
    m32 = BatchedEmbeddingBagMI355(list(rows), list(dims), device=DEV, init=None, fused_update=False)
    for t in range(2):
        m32.table(t).copy_(m.dequantized_table(t))
    idx, off, psw = request(20, rows, (0, 1, 20, 3, 100, 7, 0, 2) * 2)
    start, end = off[:-1], off[1:]
    for w in (None, psw):
        d_w = None if w is None else dev(w)
        diff = np.abs(m(dev(idx), dev(off), d_w).double().cpu().numpy() - m32.lookup(dev(idx), dev(off), d_w).double().cpu().numpy())
        absw = np.ones(idx.size) if w is None else np.abs(w.astype(np.float64))
        worst = 0.0
        for t in range(2):
            codes, scale, bias = (a.astype(np.float64) for a in R.unpack(qt[t], dims[t], bits))
            for b in range(B):
                j = np.arange(start[t * B + b], end[t * B + b])
                r = idx[j]
                mag = (absw[j, None] * (np.abs(bias[r])[:, None] + codes[r] * np.abs(scale[r])[:, None])).sum(axis=0)
                bound = (2 * len(j) + 2) * 2.0**-24 * mag
                d = diff[b, t * 128:(t + 1) * 128]
                assert (d <= bound).all(), (bits, t, b, float((d - bound).max()))
                worst = max(worst, float((d / np.maximum(bound, 1e-300)).max()))
        print(f"bits {bits} weighted {w is not None}: worst |diff| / bound = {worst:.3f}")


# ---- 13: the single-table module ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 4])
def test_single_table_module(bits):
    from param_amd import EmbeddingBagMI355, QuantizedEmbeddingBagMI355

    torch.manual_seed(3)
    ref = torch.nn.EmbeddingBag(60, 64, mode="sum")
    m = QuantizedEmbeddingBagMI355.from_float(ref, bits)
    q = rowquant.quantize_rows(ref.weight.detach().numpy(), bits)
    assert m.weights.is_cuda and np.array_equal(m.table(0).cpu().numpy(), q)
    m2 = QuantizedEmbeddingBagMI355.from_float(EmbeddingBagMI355(60, 64, device=DEV, _weight=ref.weight.detach().to(DEV)), bits)
    assert torch.equal(m2.table(0), m.table(0))
    # 1-D input with offsets [B]; 2-D input as fixed-length bags, with weights of the input's shape
    idx, off, psw = request(21, (60,), (4, 0, 9, 1))
    want = R.forward([q], [64], bits, idx, off[:-1], 4, psw)[0]
    assert R.same_f32(m(dev(idx), dev(off[:-1]), dev(psw)).cpu().numpy(), want)
    idx2 = idx[:12].reshape(3, 4)
    want2 = R.forward([q], [64], bits, idx[:12], np.arange(3) * 4, 3, psw[:12])[0]
    assert R.same_f32(m(dev(idx2), None, dev(psw[:12].reshape(3, 4))).cpu().numpy(), want2)
    assert R.same_f32(m(dev(idx2, torch.int32)).cpu().numpy(), R.forward([q], [64], bits, idx[:12], np.arange(3) * 4, 3)[0])
    # the packed bytes of torch's prepack operator are the layout: weight=
    packed = torch.from_numpy(C.torch_prepack(ref.weight.detach().numpy(), bits))
    m3 = QuantizedEmbeddingBagMI355(60, 64, bits, device=DEV, weight=packed)
    live = C.torch_lookup(packed.numpy(), bits, idx, off[:-1], psw)
    assert R.same_f32(m3(dev(idx), dev(off[:-1]), dev(psw)).cpu().numpy(), live)
    # state_dict round trip
    twin = QuantizedEmbeddingBagMI355(60, 64, bits, device=DEV)
    assert not twin(dev(idx), dev(off[:-1])).any()                  # zero bytes dequantise to zeros
    twin.load_state_dict(m.state_dict())
    assert torch.equal(twin.weights, m.weights) and not list(twin.parameters())
    assert R.same_f32(twin(dev(idx), dev(off[:-1]), dev(psw)).cpu().numpy(), want)
    with pytest.raises(TypeError):
        m(dev(idx).float(), dev(off[:-1]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.from_numpy(idx), torch.from_numpy(off[:-1]))


@pytest.mark.parametrize("bits", [8, 4])
def test_from_float_of_a_batched_module(bits):
    from param_amd import BatchedEmbeddingBagMI355, QuantizedBatchedEmbeddingBagMI355

    src = BatchedEmbeddingBagMI355([40, 9], [64, 32], dtype=torch.bfloat16, device=DEV, init="normal", seed=2, layout="bd", fused_update=False)
    m = QuantizedBatchedEmbeddingBagMI355.from_float(src, bits)
    for t in range(2):
        assert np.array_equal(m.table(t).cpu().numpy(), rowquant.quantize_rows(src.table(t).float().cpu().numpy(), bits))
    m2 = QuantizedBatchedEmbeddingBagMI355.from_float([src.table(t).float() for t in range(2)], bits)
    assert torch.equal(m2.weights, m.weights) and m2.layout == "bd"
    mean = BatchedEmbeddingBagMI355([40], [64], device=DEV, pooling_mode="mean", fused_update=False)
    with pytest.raises(ValueError, match="sum pooling"):
        QuantizedBatchedEmbeddingBagMI355.from_float(mean, bits)
