"""MIXED-FORMAT TABLES on the GPU: ``pm_embbag_fwd_anyfmt`` and ``pm_embedding_gather_anyfmt`` through
``MixedBatchedEmbeddingBagMI355`` and as raw C calls.  Every comparison is on BITS (a NaN compares as a NaN where the format's own rule
says so), against (i) tests/anyfmt_rules.py -- the existing restatements applied table by table -- and (ii) the single-format modules
over the SAME BYTES: ``BatchedEmbeddingBagMI355`` (one per float dtype), ``QuantizedBatchedEmbeddingBagMI355`` and
``Float8BatchedEmbeddingBagMI355`` (one per FP8 format), each given its tables' part of the request, their outputs placed by hand.
One reference per request, shared by the index types, layouts and output types that must give the same bits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from param_amd import _lib
from tests import anyfmt_cases as AC
from tests import anyfmt_rules as A
from tests import bounds_rules as BR
from tests import far_rows as F
from tests import special_values as SV

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDT = {"i32": torch.int32, "i64": torch.int64}
KINDS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16, "fp8_e4m3": torch.float8_e4m3fn, "fp8_e5m2": torch.float8_e5m2}
PM_DT = {"f32": _lib.PM_F32, "bf16": _lib.PM_BF16, "f16": _lib.PM_F16}


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def bits_of(t):
    """a result tensor as the bits the rules compare: uint32 / uint16"""
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def fill(m, tabs):
    host = np.zeros(m.weights.numel(), dtype=np.uint8)
    for t, tab in enumerate(tabs):
        host[m._starts[t]:m._starts[t] + tab.data.size] = tab.data.reshape(-1)
    m.weights.copy_(torch.from_numpy(host))
    return m


def mixed(tabs, kind="f32", layout="bd", **kw):
    from param_amd import MixedBatchedEmbeddingBagMI355
    m = MixedBatchedEmbeddingBagMI355([t.data.shape[0] for t in tabs], [t.dim for t in tabs], [t.fmt for t in tabs], device=DEV, layout=layout,
                                      output_dtype=KINDS[kind], **kw)
    m.table_exponents.copy_(torch.tensor([t.exp for t in tabs], dtype=torch.int32))
    return fill(m, tabs)


def single(tabs, ts, kind, scale="table"):
    """the single-format module over the tables ``ts`` (of one family and, but for quantised rows, one format) and their bytes"""
    from param_amd import BatchedEmbeddingBagMI355, Float8BatchedEmbeddingBagMI355, QuantizedBatchedEmbeddingBagMI355
    sub = [tabs[t] for t in ts]
    rows, dims, fmt = [s.data.shape[0] for s in sub], [s.dim for s in sub], sub[0].fmt
    if fmt in ("int8", "int4"):
        return fill(QuantizedBatchedEmbeddingBagMI355(rows, dims, [8 if s.fmt == "int8" else 4 for s in sub], device=DEV, output_dtype=KINDS[kind]), sub)
    if fmt.startswith("fp8"):
        m = Float8BatchedEmbeddingBagMI355(rows, dims, TORCH[fmt], device=DEV, output_dtype=KINDS[kind], scale=scale)
        for k, s in enumerate(sub):
            m.copy_from_(k, torch.from_numpy(s.data), **({} if scale is None else {"exponents": s.exp}))
        return m
    m = BatchedEmbeddingBagMI355(rows, dims, dtype=TORCH[fmt], device=DEV, init=None, output_dtype=KINDS[kind])
    for k, s in enumerate(sub):
        m.table(k).copy_(torch.from_numpy(s.data).view(TORCH[fmt]).view(rows[k], dims[k]))
    return m


def families(tabs):
    """the table indices of every single-format module: one per float dtype and FP8 format, one for all quantised tables"""
    groups = {}
    for t, tab in enumerate(tabs):
        groups.setdefault("q" if tab.fmt in ("int8", "int4") else tab.fmt, []).append(t)
    return list(groups.values())


def sub_request(idx, off, B, w, ts):
    """the part of a request that belongs to the tables ``ts``, offsets rebased: (indices, offsets [len(ts) * B + 1], weights, where each
    table's positions start)"""
    parts = [(idx[off[t * B]:off[(t + 1) * B]], off[t * B:(t + 1) * B] - off[t * B], None if w is None else w[off[t * B]:off[(t + 1) * B]]) for t in ts]
    sizes = np.cumsum([0] + [p[0].size for p in parts])
    s_idx = np.concatenate([p[0] for p in parts])
    s_off = np.concatenate([p[1] + sizes[k] for k, p in enumerate(parts)] + [[s_idx.size]])
    return s_idx, s_off, None if w is None else np.concatenate([p[2] for p in parts]), sizes


def assert_tables(got, want, kind, what, strict=False):
    """``got``: bits ``[B, sum D]`` (bd) ; ``want``: per-table bits"""
    edges = np.concatenate([[0], np.cumsum([w.shape[1] for w in want])])
    for t, w in enumerate(want):
        g = got[:, edges[t]:edges[t + 1]]
        ok = np.array_equal(g, w) if strict else A.same(g, w, kind)
        assert ok, f"{what}: table {t}: {int((g != w).sum())} of {w.size} elements differ"


def check_against_singles(tabs, idx, off, B, w, kind, got, seq=None, strict=True, scale="table"):
    """(ii): every single-format module over the same bytes gives the mixed launch's columns (and un-pooled rows), bit for bit"""
    edges = np.concatenate([[0], np.cumsum([t.dim for t in tabs])])
    for ts in families(tabs):
        s_idx, s_off, s_w, sizes = sub_request(idx, off, B, w, ts)
        m = single(tabs, ts, kind, scale)
        one = bits_of(m.lookup(dev(s_idx), dev(s_off), None if s_w is None else dev(s_w), batch=B))
        c = 0
        for k, t in enumerate(ts):
            a, b = one[:, c:c + tabs[t].dim], got[:, edges[t]:edges[t + 1]]
            assert np.array_equal(a, b) if strict else A.same(b, a, kind), (tabs[t].fmt, t, kind, w is not None)
            c += tabs[t].dim
        if seq is not None:
            rows = bits_of(m.lookup_sequence(dev(s_idx), dev(s_off), batch=B))
            for k, t in enumerate(ts):
                a, b = rows[sizes[k]:sizes[k + 1]], seq[off[t * B]:off[(t + 1) * B]]
                assert np.array_equal(a, b) if strict else A.same(b, a, kind), (tabs[t].fmt, t, kind, "un-pooled")


# ---- 1. all seven formats in one request ------------------------------------------------------------------------------------------------

ORDERS = {"seven": AC.SEVEN, "fourteen": AC.FOURTEEN, "reversed": AC.SEVEN[::-1]}


@functools.lru_cache(maxsize=None)
def seven_case(order, B):
    fmts = ORDERS[order]
    T = len(fmts)
    rows = AC.rows_for(T, 10 + B)
    tabs = AC.tables(fmts, rows, [64] * T, 11 + B, exps=[(-2, 3, 0)[t % 3] for t in range(T)])
    idx, off, psw = AC.request(12 + B, rows, B)
    want = {w: A.forward(tabs, idx, off, B, psw if w else None) for w in (False, True)}
    return tabs, idx, off, psw, want


@pytest.mark.parametrize("B", [5, 33])
@pytest.mark.parametrize("order", list(ORDERS))
def test_all_seven_formats_in_one_request(order, B):
    tabs, idx, off, psw, want = seven_case(order, B)
    T = len(tabs)
    assert (np.diff(off) == 0).any() and np.diff(off).max() <= 9 and {t.fmt for t in tabs} == set(AC.SEVEN)
    for kind in KINDS:
        for layout in ("bd", "tbd"):
            m = mixed(tabs, kind, layout)
            for it in IDT:
                d_idx, d_off = dev(idx, IDT[it]), dev(off, IDT[it])
                for weighted in (False, True):
                    out = m(d_idx, d_off, dev(psw) if weighted else None)
                    assert not out.requires_grad and out.dtype == KINDS[kind]
                    got = bits_of(out)
                    if layout == "tbd":
                        assert out.shape == (T, B, 64)
                        got = np.concatenate(list(got), axis=1)
                    else:
                        assert out.shape == (B, 64 * T)
                    assert_tables(got, [A.to_kind(x, kind) for x in want[weighted]], kind, f"{order} B{B} {kind} {layout} {it} w{weighted}")
                    if layout == "bd" and it == "i64":
                        check_against_singles(tabs, idx, off, B, psw if weighted else None, kind, got)
    # the plan does not depend on the formats: any permutation of them plans the same launch
    perm = [tabs[i] for i in np.random.default_rng(1).permutation(T)]
    assert mixed(perm).plan(dev(idx), dev(off), batch=B) == mixed(tabs).plan(dev(idx), dev(off), batch=B)


# ---- 2. multi-tile launches -------------------------------------------------------------------------------------------------------------

def test_consecutive_tiles_differ_in_format_and_a_table_spans_several():
    B, rows = 70, AC.rows_for(7, 20)
    tabs = AC.tables(AC.SEVEN, rows, [64] * 7, 21, exps=[1] * 7)
    idx, off, psw = AC.request(22, rows, B)
    m = mixed(tabs)
    p = m.plan(dev(idx), dev(off))
    assert p["bags_per_block"] == 32 and p["tiles_per_table"] == 3 and p["unroll"] == 0      # 21 tiles; tiles 2 | 3, 5 | 6, .. differ in format
    for w in (None, psw):
        got = bits_of(m(dev(idx), dev(off), None if w is None else dev(w)))
        assert_tables(got, A.forward_bits(tabs, idx, off, B, "f32", w), "f32", f"B = 70, weighted {w is not None}")
        check_against_singles(tabs, idx, off, B, w, "f32", got)


# ---- 3. mixed dims, column passes -------------------------------------------------------------------------------------------------------

def test_mixed_dims_and_two_column_passes():
    dims = [16, 128, 8, 64, 32, 16, 256]
    fmts = ["fp8_e4m3", "bf16", "int4", "fp16", "fp8_e5m2", "int8", "fp32"]
    rows, B = AC.rows_for(7, 30), 6
    tabs = AC.tables(fmts, rows, dims, 31, exps=[-1, 0, 0, 0, 2, 0, 0])
    idx, off, psw = AC.request(32, rows, B)
    for kind in KINDS:
        m = mixed(tabs, kind)
        for w in (None, psw):
            out = m(dev(idx, torch.int32), dev(off, torch.int32), None if w is None else dev(w))
            assert out.shape == (B, sum(dims))
            assert_tables(bits_of(out), A.forward_bits(tabs, idx, off, B, kind, w), kind, f"mixed dims {kind}")
            check_against_singles(tabs, idx, off, B, w, kind, bits_of(out))
    with pytest.raises(ValueError, match="one common embedding dim"):
        m.lookup_sequence(dev(idx), dev(off))
    # D = 1024 next to D = 16: lane groups of 64 lanes, two column passes over the wide table
    tabs = AC.tables(["int4", "fp32"], [40, 40], [1024, 16], 33)
    idx, off, psw = AC.request(34, [40, 40], 6)
    for kind in ("f32", "bf16"):
        m = mixed(tabs, kind)
        assert m.plan(dev(idx), dev(off))["stage_out"] == 1024
        got = bits_of(m(dev(idx), dev(off), dev(psw)))
        assert_tables(got, A.forward_bits(tabs, idx, off, 6, kind, psw), kind, f"two column passes {kind}")
        check_against_singles(tabs, idx, off, 6, psw, kind, got)
    tabs = AC.tables(["fp32", "int4"], [40, 40], [1024, 1024], 35)      # ... and un-pooled: two passes of 64 lanes x 8 columns
    seq = bits_of(mixed(tabs).lookup_sequence(dev(idx), dev(off)))
    want, written, _ = A.sequence(tabs, idx, off, 6, "f32")
    assert written.all() and A.same(seq, want, "f32")


# ---- 4. the unstaged path ---------------------------------------------------------------------------------------------------------------

def test_unstaged_path():
    """one bag longer than the index tile: the tile's indices (and weights) come from the request"""
    rows, B = [30] * 7, 2
    tabs = AC.tables(AC.SEVEN, rows, [16] * 7, 41, exps=[-4] * 7)
    rng = np.random.default_rng(42)
    lens = np.array([4300, 3] * 7)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rng.integers(0, 30, int(lens.sum())).astype(np.int64)
    psw = (rng.standard_normal(idx.size) * 0.5).astype(np.float32)
    m = mixed(tabs)
    want = {False: A.forward_bits(tabs, idx, off, B, "f32"), True: A.forward_bits(tabs, idx, off, B, "f32", psw)}
    for it in IDT:
        d_idx, d_off = dev(idx, IDT[it]), dev(off, IDT[it])
        p = m.plan(d_idx, d_off, batch=B)
        assert p["tiles_per_table"] == 1 and p["idx_cap"] == 4096 < 4303          # 4303 lookups per tile: not staged
        for weighted in (False, True):
            got = bits_of(m.lookup(d_idx, d_off, dev(psw) if weighted else None, batch=B))
            assert_tables(got, want[weighted], "f32", f"unstaged {it} weighted {weighted}")
    check_against_singles(tabs, idx, off, B, psw, "f32", got)


# ---- 5. FP8 table exponents -------------------------------------------------------------------------------------------------------------

def test_fp8_table_exponents_next_to_fp32_and_int4():
    exps = [0, -64, -64, 0, -3, -3, 0, 0, 5, 5, 64, 64]
    fmts = ["fp32", "fp8_e4m3", "fp8_e5m2", "int4", "fp8_e4m3", "fp8_e5m2", "fp8_e4m3", "fp8_e5m2", "fp8_e4m3", "fp8_e5m2", "fp8_e4m3", "fp8_e5m2"]
    T, B = len(fmts), 5
    rows = AC.rows_for(T, 50)
    tabs = AC.tables(fmts, rows, [32] * T, 51, exps=exps)
    assert sorted({t.exp for t in tabs if t.fmt.startswith("fp8")}) == [-64, -3, 0, 5, 64]
    idx, off, psw = AC.request(52, rows, B)
    for kind in KINDS:
        m = mixed(tabs, kind)
        assert m.table_exponents.tolist() == exps
        seq = bits_of(m.lookup_sequence(dev(idx), dev(off)))
        want, written, copied = A.sequence(tabs, idx, off, B, kind)
        assert written.all() and A.same(seq, want, kind, copied)
        for w in (None, psw):
            got = bits_of(m(dev(idx), dev(off), None if w is None else dev(w)))
            assert_tables(got, A.forward_bits(tabs, idx, off, B, kind, w), kind, f"exponents {kind}")
            check_against_singles(tabs, idx, off, B, w, kind, got, seq if w is None else None)
    # the tables whose exponent is 0 are the unscaled module's tables: the same bits from pm_embbag_fwd_f8 / pm_embedding_gather_f8
    zero = [t for t, tab in enumerate(tabs) if tab.fmt.startswith("fp8") and tab.exp == 0]
    assert [tabs[t].fmt for t in zero] == ["fp8_e4m3", "fp8_e5m2"]
    m = mixed(tabs)
    got, seq = bits_of(m(dev(idx), dev(off), dev(psw))), bits_of(m.lookup_sequence(dev(idx), dev(off)))
    for t in zero:
        s_idx, s_off, s_w, _ = sub_request(idx, off, B, psw, [t])
        plain = single(tabs, [t], "f32", scale=None)
        assert np.array_equal(bits_of(plain.lookup(dev(s_idx), dev(s_off), dev(s_w), batch=B)), got[:, 32 * t:32 * (t + 1)])
        assert np.array_equal(bits_of(plain.lookup_sequence(dev(s_idx), dev(s_off), batch=B)), seq[off[t * B]:off[(t + 1) * B]])


# ---- 6. special values ------------------------------------------------------------------------------------------------------------------

def test_special_values_stay_in_their_tables():
    """NaN, +-Inf, -0.0 and subnormals in the fp32 / 16-bit tables, every FP8 code (NaN and Inf codes included) in the FP8 tables; the
    quantised neighbours' columns are what they are without them; un-pooled same-dtype rows leave as stored bits"""
    D, R, B = 16, 64, 8
    rng = np.random.default_rng(61)
    codes = np.arange(256, dtype=np.uint8).reshape(16, 16)
    f8 = np.concatenate([codes, codes[::-1], AC.table_bytes("fp8_e4m3", R - 32, D, rng)])
    q8, q4 = AC.table_bytes("int8", R, D, rng), AC.table_bytes("int4", R, D, rng)
    tabs = [A.make_table("fp32", SV.special_table(R, D, rng, "f32")[0], D), A.make_table("int8", q8, D),
            A.make_table("bf16", SV.special_table(R, D, rng, "bf16")[0], D), A.make_table("int4", q4, D),
            A.make_table("fp16", SV.special_table(R, D, rng, "f16")[0], D), A.make_table("fp8_e4m3", f8, D, 2),
            A.make_table("fp8_e5m2", f8, D, -1)]
    idx, off, _ = AC.request(62, [R] * 7, B, weights=False)
    for t in range(7):                                                # every table's first lookups walk the constant special rows
        lo, hi = int(off[t * B]), int(off[(t + 1) * B])
        assert hi - lo >= 20
        idx[lo:lo + 20] = np.arange(20)
    n_special = 0
    for kind in KINDS:
        m = mixed(tabs, kind)
        got = bits_of(m(dev(idx), dev(off)))
        want = A.forward_bits(tabs, idx, off, B, kind)
        assert_tables(got, want, kind, f"specials pooled {kind}")
        n_special += sum(int(A.is_nan(w, kind).sum()) for w in want)
        for t in (1, 3):                                              # the quantised neighbours: finite, and bit for bit
            assert np.array_equal(got[:, D * t:D * (t + 1)], want[t]) and not A.is_nan(want[t], kind).any()
        seq = bits_of(m.lookup_sequence(dev(idx), dev(off)))
        swant, written, copied = A.sequence(tabs, idx, off, B, kind)
        assert written.all() and copied.any() and A.same(seq, swant, kind, copied)
        for t, tab in enumerate(tabs):                                # same dtype in and out: the stored bits, NaNs and -0.0 included
            if A._KIND.get(tab.fmt) == kind:
                lo, hi = int(off[t * B]), int(off[(t + 1) * B])
                stored = A.float_bits(tab)[idx[lo:hi]]
                assert np.array_equal(seq[lo:hi], stored) and A.is_nan(stored, kind).any() and (stored == (1 << (8 * stored.itemsize - 1))).any()
        check_against_singles(tabs, idx, off, B, None, kind, got, seq, strict=False)
    assert n_special > 0


# ---- 7. out=, batch slices, bounds_check_mode -------------------------------------------------------------------------------------------

def test_out_batch_slice_and_bounds_check():
    rows, B = AC.rows_for(7, 70), 10
    tabs = AC.tables(AC.SEVEN, rows, [64] * 7, 71, exps=[3] * 7)
    idx, off, psw = AC.request(72, rows, B)
    m = mixed(tabs)
    for begin, count in ((0, 4), (3, 4), (6, 4), (5, 0), (0, 10)):
        want = A.forward_bits(tabs, idx, off, B, "f32", psw, begin, count)
        buf = torch.full((B, 64 * 7), -7.0, device=DEV)
        assert m.lookup(dev(idx), dev(off), dev(psw), out=buf, bag_begin=begin, bag_count=count) is buf
        keep = np.ones(B, dtype=bool)
        keep[begin:begin + count] = False
        assert (buf.cpu().numpy()[keep] == -7.0).all()
        assert_tables(bits_of(buf)[begin:begin + count], want, "f32", f"slice {begin}+{count}")
        swant, written, copied = A.sequence(tabs, idx, off, B, "f32", begin, count)
        sbuf = torch.full((idx.size, 64), -7.0, device=DEV)
        m.lookup_sequence(dev(idx), dev(off), out=sbuf, bag_begin=begin, bag_count=count)
        assert (sbuf.cpu().numpy()[~written] == -7.0).all() and A.same(bits_of(sbuf)[written], swant[written], "f32", copied[written])
    with pytest.raises(ValueError, match="out must be a contiguous"):
        m.lookup(dev(idx), dev(off), out=torch.empty((B, 64 * 7), dtype=torch.float16, device=DEV))
    # bounds_check_mode="ignore" repairs a bad index and a bad offset to what tests/bounds_rules.py says, then looks the repaired request up
    bad_idx, bad_off = idx.copy(), off.copy()
    bad_idx[4] = rows[0]                                              # one past table 0's last row
    bad_off[16] = bad_off[15] - 2                                     # an offset that goes backwards
    fix_idx, fix_off, report = BR.repair(bad_idx, bad_off, rows, 7, B)
    assert report[0] >= 1 and report[1] >= 1
    mi = mixed(tabs, bounds_check_mode="ignore")
    d_idx, d_off = dev(bad_idx), dev(bad_off)
    out = mi.lookup(d_idx, d_off, dev(psw), batch=B)
    assert np.array_equal(d_idx.cpu().numpy(), fix_idx) and np.array_equal(d_off.cpu().numpy(), fix_off)
    assert_tables(bits_of(out), A.forward_bits(tabs, fix_idx, fix_off, B, "f32", psw), "f32", "repaired request")
    d_idx2 = dev(bad_idx)
    seq = mi.lookup_sequence(d_idx2, dev(off), batch=B)
    assert d_idx2.cpu().numpy()[4] == 0 and A.same(bits_of(seq), A.sequence(tabs, d_idx2.cpu().numpy(), off, B, "f32")[0], "f32")
    d_idx3 = dev(bad_idx)
    m.sanitize_(d_idx3, dev(off), batch=B)
    assert d_idx3.cpu().numpy()[4] == 0


# ---- 8. un-pooled -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [3, 40])
def test_sequence_lookup(B):
    """B = 3: one tile of 256 positions holds all seven formats; B = 40: several tiles"""
    rows = AC.rows_for(7, 80 + B)
    tabs = AC.tables(AC.SEVEN, rows, [64] * 7, 81 + B, exps=[-5, 4] * 4)
    idx, off, _ = AC.request(82 + B, rows, B, max_len=10)
    owner = np.searchsorted(off[::B][:7], np.arange(idx.size), side="right") - 1
    assert (idx.size < 256 and set(owner.tolist()) == set(range(7))) if B == 3 else idx.size > 3 * 256
    for kind in KINDS:
        want, written, copied = A.sequence(tabs, idx, off, B, kind)
        assert written.all() and copied.any()
        for layout in ("bd", "tbd"):
            m = mixed(tabs, kind, layout)
            for it in IDT:
                out = m.lookup_sequence(dev(idx, IDT[it]), dev(off, IDT[it]))
                assert out.shape == (idx.size, 64) and out.dtype == KINDS[kind] and not out.requires_grad
                seq = bits_of(out)
                assert A.same(seq, want, kind, copied), (B, kind, layout, it)
        for t, tab in enumerate(tabs):                                # bf16 -> bf16 and fp16 -> fp16 (and fp32 -> fp32) are bit copies
            if A._KIND.get(tab.fmt) == kind:
                lo, hi = int(off[t * B]), int(off[(t + 1) * B])
                assert np.array_equal(seq[lo:hi], A.float_bits(tab)[idx[lo:hi]])
        check_against_singles(tabs, idx, off, B, None, kind, bits_of(mixed(tabs, kind)(dev(idx), dev(off))), seq)
    p = m.sequence_plan(dev(idx), dev(off))
    assert p["tile"] == 256 and p["vec"] == 8 and p["group_lanes"] == 8 and p["grid"] == -(-idx.size // 256) and p["unroll"] == 4
    buf = torch.full((idx.size, 64), float("nan"), device=DEV, dtype=KINDS[kind])
    assert m.lookup_sequence(dev(idx), dev(off), out=buf) is buf and A.same(bits_of(buf), want, kind, copied)
    e = m.lookup_sequence(dev(np.zeros(0, dtype=np.int64)), dev(np.zeros(7 * B + 1, dtype=np.int64)), batch=B)
    assert e.shape == (0, 64)


# ---- 9. far addresses -------------------------------------------------------------------------------------------------------------------

def test_far_rows_of_an_fp32_table():
    """an fp32-format table whose rows pass byte offsets 2^31 and 2^32, between a 4-bit and an FP8 table: looked-up rows on both sides
    of either mark, pooled and un-pooled, compared with the rule on a compacted twin (tests/far_rows.py)"""
    import param_amd
    from param_amd import MixedBatchedEmbeddingBagMI355

    D, B = 64, len(F.STAGED_LENS)
    marks = [c for what, _, _, c in F.threshold_rows(D, es=4) if what == "bytes"]
    probes = np.array(sorted({0, 1, 2} | {c + d for c in marks for d in (-1, 0, 1)}), dtype=np.int64)
    rows = [40, F.table_rows(probes), 40]
    assert rows[1] * D * 4 > 2 ** 32 and (probes * D * 4 >= 2 ** 31).any() and (probes * D * 4 < 2 ** 31).any()
    param_amd.load_library()
    free, _ = torch.cuda.mem_get_info()
    if free < rows[1] * D * 4 + (8 << 30):
        pytest.skip(f"needs {rows[1] * D * 4 / 2**30:.1f} GiB + 8 GiB of free HBM, {free / 2**30:.0f} GiB available")
    small = AC.tables(["int4", "fp32", "fp8_e5m2"], [40, len(probes), 40], [D] * 3, 91, exps=[0, 0, 7])      # table 1: the twin
    m = MixedBatchedEmbeddingBagMI355(rows, D, ["int4", "fp32", "fp8_e5m2"], device=DEV)
    try:
        m.table(0).copy_(torch.from_numpy(small[0].data))
        m.copy_from_(2, torch.from_numpy(small[2].data), exponent=7)
        twin = torch.from_numpy(small[1].data).view(torch.float32).view(len(probes), D).to(DEV)
        for i, r in enumerate(probes):
            m.table(1)[int(r)].copy_(twin[i])
        far_idx, far_off = F.request(probes, F.STAGED_LENS, seed=5)
        i0, o0, _ = AC.request(92, [40], B, weights=False)
        i2, o2, _ = AC.request(93, [40], B, weights=False)
        idx = np.concatenate([i0, far_idx, i2])
        cidx = np.concatenate([i0, F.compact(probes, far_idx), i2])
        off = np.concatenate([o0[:-1], far_off[:-1] + i0.size, o2 + i0.size + far_idx.size])
        psw = (np.random.default_rng(94).standard_normal(idx.size) * 1.5).astype(np.float32)
        for it in IDT:
            for w in (None, psw):
                got = bits_of(m.lookup(dev(idx, IDT[it]), dev(off, IDT[it]), None if w is None else dev(w), batch=B))
                assert_tables(got, A.forward_bits(small, cidx, off, B, "f32", w), "f32", f"far pooled {it}")
            seq = bits_of(m.lookup_sequence(dev(idx, IDT[it]), dev(off, IDT[it]), batch=B))
            want, written, copied = A.sequence(small, cidx, off, B, "f32")
            assert written.all() and A.same(seq, want, "f32", copied) and seq[i0.size:i0.size + far_idx.size].any(), it
    finally:
        del m
        torch.cuda.empty_cache()


# ---- 10. an unknown format code ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("code", [7, 99, -1])
def test_unknown_format_code_gives_zero_rows(code):
    """straight to the C calls: the table whose code is none of the seven gives +0.0 rows, every other table its own -- a defined result"""
    rows, B = AC.rows_for(7, 100), 9
    tabs = AC.tables(AC.SEVEN, rows, [64] * 7, 101)
    idx, off, psw = AC.request(102, rows, B)
    L = _lib.load()
    for bad in (0, 3, 6):
        for kind in ("f32", "f16"):
            m = mixed(tabs, kind)
            ts = m._tables()
            fmts = ts.d_bits.clone()
            fmts[bad] = code
            d_idx, d_off, d_w = dev(idx), dev(off), dev(psw)
            op = _lib.pm_embbag_batch()
            ctypes.memmove(ctypes.byref(op), ctypes.byref(ts.request(d_idx, d_off, B, d_w, 0, None, forward=True)), ctypes.sizeof(op))
            out = torch.full((B, 64 * 7), float("nan"), dtype=KINDS[kind], device=DEV)
            _lib.check(L.pm_embbag_fwd_anyfmt(ctypes.byref(op), fmts.data_ptr(), m.table_exponents.data_ptr(), PM_DT[kind], out.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream))
            want = A.forward_bits(tabs, idx, off, B, kind, psw)
            want[bad] = np.zeros_like(want[bad])
            assert_tables(bits_of(out), want, kind, f"unknown code {code} at table {bad}", strict=True)
            ctypes.memmove(ctypes.byref(op), ctypes.byref(ts.request(d_idx, d_off, B, None, 0, None, forward=True)), ctypes.sizeof(op))
            seq = torch.full((idx.size, 64), float("nan"), dtype=KINDS[kind], device=DEV)
            _lib.check(L.pm_embedding_gather_anyfmt(ctypes.byref(op), fmts.data_ptr(), None, PM_DT[kind], seq.data_ptr(), 64,
                                                    torch.cuda.current_stream().cuda_stream))
            swant, written, _ = A.sequence(tabs, idx, off, B, kind)
            swant[int(off[bad * B]):int(off[(bad + 1) * B])] = 0
            assert written.all() and np.array_equal(bits_of(seq), swant)
