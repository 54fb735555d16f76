"""UN-POOLED lookups over ROW-QUANTISED TABLES on the GPU: ``pm_embedding_gather_qrows`` through ``lookup_sequence`` of the batched module,
through ``QuantizedEmbeddingMI355`` and as the raw C call, compared as BITS against tests/qgather_rules.py (the numpy restatement that
tests/test_qgather_host.py holds to torch's CPU operators).  Tables come from ``oracle.rowquant.quantize_rows`` as in
tests/test_gpu_qrows.py, whose helpers build them.  One reference per request, shared by the index types, output types and knob values
that must all give the same bits."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import rowquant
from param_amd import _lib
from tests import out16_rules as O
from tests import qgather_cases as G
from tests import qgather_rules as Q
from tests import qrows_cases as C
from tests import qrows_rules as R
from tests.test_gpu_qrows import DEV, IDT, MIXED, QB, dev, float_tables, module, qtables

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
PM_DT = {"fp32": _lib.PM_F32, "bf16": _lib.PM_BF16, "fp16": _lib.PM_F16}


def QE(*a, **kw):
    from param_amd import QuantizedEmbeddingMI355
    return QuantizedEmbeddingMI355(*a, device=DEV, **kw)


def request(seed, rows, lens):
    """(indices int64 [N], offsets int64 [T*B+1]) for bag lengths ``lens`` (table-major)"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    B = len(lens) // len(rows)
    tab = np.repeat(np.arange(len(rows)), lens.reshape(len(rows), B).sum(axis=1))
    idx = (rng.random(int(lens.sum())) * np.asarray(rows)[tab]).astype(np.int64)
    return idx, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def bits_of(t):
    """a result tensor as the array the rules compare: fp32 as it is, 16-bit as uint16 bit patterns"""
    return t.cpu().numpy() if t.dtype == torch.float32 else t.view(torch.int16).cpu().numpy().view(np.uint16)


def same(got, want32, dtype="fp32"):
    if dtype == "fp32":
        return R.same_f32(got, want32)
    return O.same_bits(got, O.round16(want32, dtype), dtype)


class unroll_knob:
    """pm_set_tuning's unroll for the block; the default comes back"""

    def __init__(self, unroll):
        self.unroll = unroll

    def __enter__(self):
        _lib.set_tuning(unroll=self.unroll)

    def __exit__(self, *exc):
        _lib.set_tuning()
        return False


# ---- the main grid ---------------------------------------------------------------------------------------------------------------------
# Three tables of D = 24, B = 5, N = 300 (no multiple of 256: the second tile is partial), the first bag empty.  Two requests, because
# three tables cannot both leave one of them without a position and put all three into one tile:
#   "hole"  table 1 owns no position (its five bags are empty): positions go from table 0 straight to table 2
#   "mixed" tile 0 holds positions of all three tables (109 + 60 + the first 87 of table 2)
GRID_ROWS, GRID_B, GRID_D = (1, 7, 1000), 5, 24
GRID_LENS = {"hole": (0, 4, 3, 100, 2) + (0,) * 5 + (7, 0, 150, 1, 33),
             "mixed": (0, 4, 3, 100, 2) + (20, 0, 0, 39, 1) + (7, 0, 90, 1, 33)}


@functools.lru_cache(maxsize=None)
def grid_case(bits, which):
    qt = qtables(31 + bits, GRID_ROWS, (GRID_D,) * 3, bits)
    idx, off = request(6, GRID_ROWS, GRID_LENS[which])
    assert idx.size == 300 and off[1] == 0
    want, written = Q.gather(qt, GRID_D, bits, idx, off, GRID_B)
    assert written.all()
    return qt, idx, off, want


@pytest.mark.parametrize("it", ["i32", "i64"])
@pytest.mark.parametrize("bits", [8, 4])
def test_main_grid(bits, it):
    for which in GRID_LENS:
        qt, idx, off, want = grid_case(bits, which)
        table, _ = Q.owners(off, 3, GRID_B, idx.size)
        assert (set(table.tolist()) == {0, 2}) if which == "hole" else (set(table[:256].tolist()) == {0, 1, 2})
        m = module(GRID_ROWS, (GRID_D,) * 3, bits, qt, layout="tbd")
        d_idx, d_off = dev(idx, IDT[it]), dev(off, IDT[it])
        out = m.lookup_sequence(d_idx, d_off)
        assert out.shape == (300, GRID_D) and out.dtype == torch.float32 and not out.requires_grad
        assert R.same_f32(out.cpu().numpy(), want), (bits, it, which)
        assert R.same_f32(m.lookup_sequence(d_idx, d_off[:-1], batch=GRID_B).cpu().numpy(), want)      # offsets without the trailing entry
        buf = torch.full((300, GRID_D), float("nan"), device=DEV)
        assert m.lookup_sequence(d_idx, d_off, out=buf) is buf and R.same_f32(buf.cpu().numpy(), want)
        p = m.sequence_plan(d_idx, d_off)
        assert p["grid"] == 2 and p["tile"] == 256 and p["group_lanes"] == 8 and p["col_passes"] == 1 and p["lds_borders"] == 1
    with pytest.raises(ValueError, match="out must be a contiguous"):
        m.lookup_sequence(d_idx, d_off, out=torch.empty((300, GRID_D), dtype=torch.float16, device=DEV))


# ---- the raw C call: mixed dims, a padded row stride, sentinels --------------------------------------------------------------------------

def raw_call(m, idx, off, B, odt, stride, bag_begin=0, bag_count=None, it="i64"):
    """``pm_embedding_gather_qrows`` into ``[N, stride]`` elements of ``odt`` whose untouched bytes are 0xA5"""
    ts = m._tables()
    d_idx, d_off = dev(idx, IDT[it]), dev(off, IDT[it])
    op = _lib.pm_embbag_batch()
    ctypes.memmove(ctypes.byref(op), ctypes.byref(ts.request(d_idx, d_off, B, None, bag_begin, bag_count, forward=True)), ctypes.sizeof(op))
    out = torch.full((idx.size, stride * TDT[odt].itemsize), 0xA5, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().pm_embedding_gather_qrows(ctypes.byref(op), m.bitwidth, PM_DT[odt], out.data_ptr(), stride,
                                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_sentinel_rows(raw, per_table, odt):
    """the written positions hold their table's columns; every other byte -- the columns from D_t to the stride, unwritten rows -- is 0xA5"""
    e = TDT[odt].itemsize
    touched = np.zeros(raw.shape, dtype=bool)
    for t, (pos, vals) in enumerate(per_table):
        d = vals.shape[1]
        block = np.ascontiguousarray(raw[pos, :d * e])
        got = block.view(np.float32) if e == 4 else block.view(np.uint16)
        assert same(got.reshape(len(pos), d), vals, odt), f"table {t}"
        touched[pos, :d * e] = True
    assert (raw[~touched] == 0xA5).all(), "bytes outside [0, D_t) of a written row, or an unwritten row, were written"


@pytest.mark.parametrize("odt", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("bits", [8, 4])
def test_raw_call_mixed_dims_with_a_padded_stride(bits, odt):
    """rows of 12, 28, 136 (8 bits) and 8, 16, 68 bytes (4 bits): a row starts at every 8-byte phase"""
    rows, dims, B = (9, 50, 30), MIXED[bits], 4
    assert [R.row_bytes(d, bits) for d in dims] == ([12, 28, 136] if bits == 8 else [8, 16, 68])
    qt = qtables(41, rows, dims, bits)
    m = module(rows, dims, bits, qt)
    idx, off = request(42, rows, (0, 30, 5, 70) + (3, 0, 90, 40) + (60, 1, 0, 14))      # N = 313: all three tables inside tile 0
    stride = max(dims) + 12
    for begin, count in ((0, B), (1, 2)):
        per_table = Q.gather_tables(qt, dims, bits, idx, off, B, begin, count)
        for it in ("i32", "i64"):
            check_sentinel_rows(raw_call(m, idx, off, B, odt, stride, begin, count, it), per_table, odt)
    with pytest.raises(ValueError, match="one common embedding dim"):
        m.lookup_sequence(dev(idx), dev(off))


# ---- every unroll knob value -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 4])
def test_every_unroll_value_gives_the_same_bits(bits):
    """D = 128 (G = 16 / 8 lanes: one or two batches at 8 rows in flight) and D = 512 (G = 64 / 32: the ping-pong loop runs)"""
    for dim, n in ((128, 700), (512, 300)):
        rows = (60, 45)
        qt = qtables(51, rows, (dim, dim), bits)
        m = module(rows, (dim, dim), bits, qt, layout="tbd")
        idx, off = request(52, rows, (n // 2, 0, n // 4, n - n // 2 - n // 4 - 9, 0, 9))
        want, _ = Q.gather(qt, dim, bits, idx, off, 3)
        d_idx, d_off = dev(idx), dev(off)
        default = m.sequence_plan(d_idx, d_off)["unroll"]
        seen = set()
        for knob, u in ((0, default), (1, 1), (2, 2), (3, 2), (4, 4), (6, 4), (8, 8)):
            with unroll_knob(knob):
                p = m.sequence_plan(d_idx, d_off)
                assert p["unroll"] == u and p["group_lanes"] == min(64, dim // (8 if bits == 8 else 16)) and p["group_lanes"] % u == 0
                assert R.same_f32(m.lookup_sequence(d_idx, d_off).cpu().numpy(), want), (bits, dim, knob)
                seen.add(p["unroll"])
        assert seen == {1, 2, 4, 8}
        assert m.sequence_plan(d_idx, d_off)["unroll"] == default


# ---- batch slices -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 4])
def test_batch_slices(bits):
    rows, dim, B = (50, 9), 24, 10
    qt = qtables(61, rows, (dim, dim), bits)
    m = module(rows, (dim, dim), bits, qt)
    idx, off = request(62, rows, np.random.default_rng(2).integers(0, 40, 2 * B))
    d_idx, d_off = dev(idx), dev(off)
    for begin, count in ((0, 4), (3, 4), (6, 4), (5, 0), (0, 10)):      # first, middle, last, empty, whole
        want, written = Q.gather(qt, dim, bits, idx, off, B, begin, count)
        assert written.any() == (count > 0) and written.all() == (count == B)
        buf = torch.full((idx.size, dim), -7.0, device=DEV)
        m.lookup_sequence(d_idx, d_off, out=buf, bag_begin=begin, bag_count=count)
        got = buf.cpu().numpy()
        assert (got[~written] == -7.0).all() and R.same_f32(got[written], want[written]), (begin, count)
        fresh = m.lookup_sequence(d_idx, d_off, bag_begin=begin, bag_count=count).cpu().numpy()      # allocated here: zeros outside
        assert R.same_f32(fresh, want)


# ---- many tables: the borders are searched in global memory --------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 4])
def test_many_tables(bits):
    T = 1100
    rows, dims = (5,) * T, (8,) * T
    qt = qtables(71, rows, dims, bits)
    m = module(rows, dims, bits, qt, layout="tbd")
    lens = np.random.default_rng(3).integers(1, 4, T)                   # 1 .. 3 positions per table, one bag each
    for first in (int(lens[0]), 0):                                     # ... and the same with table 0 empty
        lens[0] = first
        idx, off = request(72, rows, lens)
        want, written = Q.gather(qt, 8, bits, idx, off, 1)
        assert written.all()
        p = m.sequence_plan(dev(idx), dev(off))
        assert p["lds_borders"] == 0 and p["grid"] == -(-idx.size // 256) > 1
        assert R.same_f32(m.lookup_sequence(dev(idx), dev(off)).cpu().numpy(), want), first
        assert R.same_f32(m.lookup_sequence(dev(idx, torch.int32), dev(off, torch.int32)).cpu().numpy(), want), first


# ---- the widest rows: column passes -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1024, 4096])
@pytest.mark.parametrize("bits", [8, 4])
def test_widest_rows(bits, dim):
    rows = (12,)
    qt = qtables(81, rows, (dim,), bits)
    idx, off = request(82, rows, (0, 270, 3))                           # two tiles
    want, _ = Q.gather(qt, dim, bits, idx, off, 3)
    m = module(rows, (dim,), bits, qt)
    assert m.sequence_plan(dev(idx), dev(off))["col_passes"] == dim // (512 if bits == 8 else 1024)
    assert R.same_f32(m.lookup_sequence(dev(idx), dev(off)).cpu().numpy(), want)
    m16 = module(rows, (dim,), bits, qt, output_dtype="bf16")
    got = m16.lookup_sequence(dev(idx), dev(off))
    assert got.dtype == torch.bfloat16 and same(bits_of(got), want, "bf16")
    with pytest.raises(ValueError, match="4096"):                       # the limit (launch_plan.h: kQrowsMaxDim)
        QB([1], [4104], bits)


# ---- 16-bit output is one rounding --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", O.DTYPES)
@pytest.mark.parametrize("bits", [8, 4])
def test_out16_is_one_rounding(bits, dtype):
    rows, dim = (30, 11), 24
    xs = float_tables(91, rows, (dim, dim), scale=500.0)
    # finite fp32 values beyond 65504 (from a scale and a bias that fit the 4-bit format's fp16 tail): fp16 gives Inf, bf16 holds them
    xs[0][1] = np.linspace(-1000.0, 90000.0, dim, dtype=np.float32)
    qt = [rowquant.quantize_rows(x, bits) for x in xs]
    idx, off = request(92, rows, (0, 25, 1, 40, 3, 0))
    idx[3] = 1
    want, _ = Q.gather(qt, dim, bits, idx, off, 3)
    assert np.isfinite(want).all() and (np.abs(want[3]) > 65504).any()
    m = module(rows, (dim, dim), bits, qt, output_dtype=TDT[dtype])
    out = m.lookup_sequence(dev(idx), dev(off))
    assert out.dtype == TDT[dtype] and out.shape == (idx.size, dim)
    got = bits_of(out)
    assert same(got, want, dtype)
    assert np.isinf(O.widen(got[3], dtype)).any() == (dtype == "fp16") and np.isfinite(O.widen(got, dtype)).all() == (dtype == "bf16")


# ---- against the pooled kernel and the dequantiser -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 4])
def test_against_the_pooled_kernel_and_dequantize_rows(bits):
    rows, dims = (200,), (128,)
    x = torch.from_numpy(float_tables(16, rows, dims)[0]).to(DEV)
    for odt in ("fp32", "bf16", "fp16"):
        m = QB(rows, dims, bits, output_dtype=TDT[odt])
        m.quantize_from_(0, x)
        idx = torch.randint(0, 200, (777,), generator=torch.Generator().manual_seed(1)).to(DEV)
        off = torch.zeros(1, dtype=torch.int64, device=DEV)
        seq = m.lookup_sequence(idx, off, batch=1)
        pooled = m.lookup(idx, torch.arange(777, device=DEV), batch=777)          # the same rows as bags of one
        assert seq.shape == pooled.shape == (777, 128) and np.array_equal(bits_of(seq), bits_of(pooled)), odt
        if odt == "fp32":
            assert torch.equal(seq, m.dequantized_table(0)[idx])                  # as values


# ---- special values -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 4])
def test_special_tails_and_signed_zeros(bits):
    sp = R.special_rows(8, bits)
    idx = np.array([0, 1, 2, 3, 1, 0], dtype=np.int64)
    want = Q.rows(sp, 8, bits, idx)
    got = module((4,), (8,), bits, [sp]).lookup_sequence(dev(idx), dev(np.zeros(1, dtype=np.int64)), batch=1).cpu().numpy()
    assert R.same_f32(got, want) and np.isnan(got).any() and np.isinf(got).any()
    z = Q.signed_zero_rows(8, bits)
    zi = np.array([4, 3, 2, 1, 0, 2], dtype=np.int64)
    want = Q.rows(z, 8, bits, zi)
    assert Q.negative_zeros(want) == 0
    for odt in ("fp32", "bf16", "fp16"):
        out = module((5,), (8,), bits, [z], output_dtype=TDT[odt]).lookup_sequence(dev(zi), dev(np.zeros(1, dtype=np.int64)), batch=1)
        got = bits_of(out)
        assert same(got, want, odt), odt
        assert Q.negative_zeros(got if odt == "fp32" else O.widen(got, odt)) == 0                  # no -0.0 where the rule has none


# ---- the fixture --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 4])
def test_fixture_through_both_modules(bits):
    """torch's recorded results, through the kernel"""
    fx = np.load(os.path.join(HERE, "golden", "qgather_cases.npz"))
    idx = fx["indices"]
    for dim in G.DIMS:
        q = fx[f"q_{bits}_{dim}"]
        batched = module((C.ROWS,), (dim,), bits, [q])
        single = QE(C.ROWS, dim, bits, weight=torch.from_numpy(q))
        for it in ("i32", "i64"):
            got = batched.lookup_sequence(dev(idx, IDT[it]), dev(np.zeros(1, dtype=np.int64), IDT[it]), batch=1).cpu().numpy()
            assert R.same_f32(got, fx[G.key(bits, dim)]), (bits, dim, it)
            assert R.same_f32(single(dev(idx, IDT[it]).view(4, 4)).cpu().numpy().reshape(G.N, dim), fx[G.key(bits, dim)]), (bits, dim, it)
    z = QE(5, 8, bits, weight=torch.from_numpy(fx[f"zeros_q_{bits}"]))
    assert R.same_f32(z(dev(np.arange(5))).cpu().numpy(), fx[f"zeros_out_{bits}"])
    if bits == 8:
        e = QE(C.ROWS, 24, 8, weight=torch.from_numpy(fx["embedding_q_8_24"]))
        assert R.same_f32(e(dev(idx)).cpu().numpy(), fx["embedding_out_8_24"])


# ---- bounds check -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 4])
def test_bounds_check_repairs_or_refuses_before_the_lookup(bits):
    rows, dim, B = (50, 9), 24, 4
    qt = qtables(17, rows, (dim, dim), bits)
    m = module(rows, (dim, dim), bits, qt, bounds_check_mode="warning")
    idx, off = request(18, rows, (3, 0, 5, 2, 4, 1, 0, 6))
    bad = idx.copy()
    bad[4] = 50                                                         # one past table 0's last row
    d_idx, d_off = dev(bad), dev(off)
    out = m.lookup_sequence(d_idx, d_off, batch=B)
    rep = m.bounds_report()
    assert rep["bad_indices"] == 1 and rep["first_bad_index"] == 4 and rep["bad_offsets"] == 0
    fixed = d_idx.cpu().numpy()                                         # repaired in place
    assert fixed[4] == 0 and np.array_equal(np.delete(fixed, 4), np.delete(idx, 4))
    assert R.same_f32(out.cpu().numpy(), Q.gather(qt, dim, bits, fixed, off, B)[0])
    fatal = module(rows, (dim, dim), bits, qt, bounds_check_mode="fatal")
    with pytest.raises(IndexError):                                     # refused by the sanitiser: no lookup is launched on the bad index
        fatal.lookup_sequence(dev(bad), dev(off), batch=B)
    e = QE(9, dim, bits, weight=torch.from_numpy(qt[1]), bounds_check_mode="fatal")
    with pytest.raises(IndexError):
        e(dev(np.array([[1, 9], [0, 2]])))
    assert R.same_f32(e(dev(np.array([[1, 8], [0, 2]]))).cpu().numpy().reshape(4, dim), Q.rows(qt[1], dim, bits, [1, 8, 0, 2]))


# ---- the single-table module --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 4])
def test_single_table_module(bits):
    from param_amd import EmbeddingMI355, QuantizedEmbeddingMI355

    torch.manual_seed(3)
    ref = torch.nn.Embedding(60, 64, padding_idx=5)
    m = QuantizedEmbeddingMI355.from_float(ref, bits)
    q = rowquant.quantize_rows(ref.weight.detach().numpy(), bits)
    assert m.weights.is_cuda and np.array_equal(m.table(0).cpu().numpy(), q) and not list(m.parameters())
    m2 = QuantizedEmbeddingMI355.from_float(EmbeddingMI355(60, 64, device=DEV, _weight=ref.weight.detach().to(DEV)), bits, output_dtype="fp16")
    assert torch.equal(m2.table(0), m.table(0)) and m2.output_dtype == torch.float16
    assert m.dequantized_table(0).shape == (60, 64)
    rng = np.random.default_rng(4)
    for shape in ((), (5,), (3, 4), (2, 0, 3)):
        idx = np.asarray(rng.integers(0, 60, shape))
        want = Q.rows(q, 64, bits, idx.reshape(-1))
        for it in ("i32", "i64"):
            out = m(torch.from_numpy(idx).to(IDT[it]).to(DEV))          # (from_numpy keeps a 0-d array 0-d)
            assert out.shape == (*shape, 64) and out.dtype == torch.float32 and not out.requires_grad
            assert R.same_f32(out.cpu().numpy().reshape(-1, 64), want)
        out16 = m2(torch.from_numpy(idx).to(DEV))
        assert out16.shape == (*shape, 64) and same(bits_of(out16).reshape(-1, 64), want, "fp16")
    # the packed bytes of torch's prepack operator are the layout: weight= against the live operator over bags of one
    packed = C.torch_prepack(ref.weight.detach().numpy(), bits)
    m3 = QE(60, 64, bits, weight=torch.from_numpy(packed))
    idx = rng.integers(0, 60, 33)
    assert R.same_f32(m3(dev(idx)).cpu().numpy(), G.torch_rows(packed, bits, idx))
    # state_dict round trip; zero bytes dequantise to zeros
    twin = QE(60, 64, bits)
    assert not twin(dev(idx)).any()
    twin.load_state_dict(m.state_dict())
    assert torch.equal(twin.weights, m.weights) and R.same_f32(twin(dev(idx)).cpu().numpy(), Q.rows(q, 64, bits, idx))
    # the sanitiser on its own repairs in place
    bad = dev(np.array([3, 60, 7]))
    m.sanitize_(bad)
    assert bad.cpu().tolist() == [3, 0, 7] and m.bounds_report()["bad_indices"] == 1
    with pytest.raises(TypeError):
        m(dev(idx).float())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.from_numpy(idx))
