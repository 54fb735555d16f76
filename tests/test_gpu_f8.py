"""FP8 tables on the GPU (include/param_amd.h, "FP8 TABLES"): ``Float8BatchedEmbeddingBagMI355`` and the two T = 1 modules against
tests/f8_rules.py, on bits (``qrows_rules.same_f32`` for fp32 output; for bf16 / fp16 ``f8_rules.same16``, which is
``out16_rules.same_bits`` but for the sign of a NaN, which the rule leaves open).

1. every code in every byte lane (decides that the hardware conversion is ``dec``);  2. every group width and column passes;
3. staged and unstaged tiles, with and without padding;  4. request forms;  5. far addresses;  6. rows in flight 2 / 4 / 8;
7. the T = 1 modules against torch's CPU functions over the widened table.

The requests here are a few bags a table: a tile behind tile 0 appears only as 32 bags of one lookup (1) and as the 3-bag second tile
of D >= 1024 (2), and the un-pooled lookups are one workgroup, but for the T = 300 case.  What a launch of many tiles adds -- full
tiles behind tile 0 and a partial last one under every block order, compaction over several waves and rounds, 1024-bag tiles, a
direct tile among compacted ones, every (lane group, rows in flight) pair of both kernels, PARAM_AMD_FWD_STAGE=0 -- is pinned by the
``f8`` / ``f8_gather`` cases of the plan sweep (tests/plan_sweep.py, tests/test_gpu_plan_sweep.py), under the plan each case names."""
import numpy as np
import pytest
import torch

from param_amd import _lib
from tests import f8_rules as R
from tests import far_rows as FR
from tests import out16_rules as O
from tests.f8_rules import finite_codes
from tests.qrows_rules import same_f32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
ODTS = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
GIB = 1 << 30


def _bits(t):
    t = t.detach().contiguous()
    if t.element_size() == 2:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(got, want32, odt):
    """a device output against the fp32 rule's array: on bits; a 16-bit output against the one rounding of it"""
    g = _bits(got)
    w = np.ascontiguousarray(want32, dtype=np.float32).view(np.uint32) if odt == "fp32" else O.round16(want32, odt)
    if odt == "fp32":
        ok = same_f32(g.view(np.float32), want32)
    else:
        # where the rule has no NaN this is out16_rules.same_bits; where it has one, the output is a NaN -- its sign is not part of the
        # rule (include/param_amd.h, FP8 TABLES), which same_bits would look at
        ok = R.same16(g, w, odt)
    if not ok and g.shape == w.shape:
        bad = np.argwhere(g != w)[:8]
        print("first differing elements (index, got, want):", [(tuple(int(i) for i in ix), hex(int(g[tuple(ix)])), hex(int(w[tuple(ix)]))) for ix in bad])
    return ok


def module(fmt, tables, **kw):
    import param_amd

    m = param_amd.Float8BatchedEmbeddingBagMI355([t.shape[0] for t in tables], [t.shape[1] for t in tables], DTYPES[fmt], device=DEV, **kw)
    for t, tab in enumerate(tables):
        m.copy_from_(t, _dev(tab))
    return m


def with_output(m, odt):
    from param_amd.embedding_bag import _output_dtype

    m.output_dtype = _output_dtype(odt if odt != "fp32" else None)
    m._out16 = None if m.output_dtype == torch.float32 else m.output_dtype
    return m


def ragged(rng, rows, B, lens_max=9, dtype=np.int64, lens=None):
    """a closed TBE request over len(rows) tables: bags of 0 .. lens_max lookups (or ``lens`` for every table)"""
    T = len(rows)
    L = np.concatenate([np.asarray(lens) if lens is not None else rng.integers(0, lens_max + 1, B) for _ in range(T)]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(L)])
    idx = np.concatenate([rng.integers(0, rows[t], int(L[t * B:(t + 1) * B].sum())) for t in range(T)]).astype(np.int64)
    return idx.astype(dtype), off.astype(dtype)


def concat_bd(outs):
    return np.concatenate(outs, axis=1)


# ---- 1. every code in every byte lane --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", R.FORMATS)
def test_every_code_in_every_byte_lane(fmt):
    tab = ((np.arange(256)[:, None] + np.arange(32)[None, :]) & 255).astype(np.uint8)
    want = R.dec(tab, fmt)
    m = module(fmt, [tab])
    idx = _dev(np.arange(256, dtype=np.int64))
    off1 = _dev(np.arange(257, dtype=np.int64))
    rows32 = None
    for odt in ODTS:
        with_output(m, odt)
        rows = m.lookup_sequence(idx, _dev(np.zeros(1, dtype=np.int64)), batch=1)
        assert rows.dtype == ODTS[odt] and same(rows, want, odt), (fmt, odt, "un-pooled")
        if odt == "fp32":
            rows32 = _bits(rows).view(np.float32)
            zero = tab == 0x80
            assert (rows32.view(np.uint32)[zero] == 0x80000000).all() and (rows32.view(np.uint32)[tab == 0] == 0).all(), "-0.0 is kept"
        else:
            assert same_f32(O.widen(_bits(rows), odt), rows32), "the 16-bit outputs widened are the fp32 output"
        bags = m.lookup(idx, off1, batch=256)
        with np.errstate(invalid="ignore"):
            assert same(bags, np.float32(0.0) + want, odt), (fmt, odt, "bags of one")
    assert not np.signbit(_bits(with_output(m, "fp32").lookup(idx, off1, batch=256)).view(np.float32)[tab == 0x80]).any(), "+0.0 + -0.0 is +0.0"


# ---- 2. every group width and column passes --------------------------------------------------------------------------------------------

WIDTHS = {16: (8, 1, 8, 1), 128: (8, 1, 32, 1), 256: (16, 1, 64, 1), 512: (32, 1, 64, 2), 1024: (64, 1, 64, 4), 1040: (64, 2, 64, 5),
          2048: (64, 2, 64, 8)}      # D -> pooled G, pooled passes, gather G, gather passes


@pytest.mark.parametrize("D", sorted(WIDTHS))
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_every_group_width_and_column_passes(fmt, D):
    rng = np.random.default_rng(D + len(fmt))
    tab = finite_codes(rng, fmt, (40, D))
    B = 7
    idx, off = ragged(rng, [40], B, lens=[0, 9, 1, 4, 7, 2, 5])
    psw = rng.standard_normal(idx.size).astype(np.float32)
    G, passes, Gg, gpasses = WIDTHS[D]
    want = {"plain": R.forward([tab], fmt, idx, off, B)[0], "weighted": R.forward([tab], fmt, idx, off, B, psw=psw)[0],
            "mean": R.forward([tab], fmt, idx, off, B, mean=True)[0]}
    want_rows, _ = R.sequence([tab], fmt, idx, off, B)
    d_idx, d_off, d_psw = _dev(idx), _dev(off), _dev(psw)
    mods = {"plain": module(fmt, [tab]), "mean": module(fmt, [tab], pooling_mode="mean")}
    mods["weighted"] = mods["plain"]
    try:
        for burst in (1, 0):
            _lib.set_forward_tuning(stage_out=burst)
            for mode, m in mods.items():
                w = d_psw if mode == "weighted" else None
                for odt in ODTS:
                    with_output(m, odt)
                    plan = m.plan(d_idx, d_off, w, batch=B)
                    assert plan["bags_per_block"] >= 256 // G and plan["unroll"] == 2 and plan["ordered"] == 0 and plan["flat_bags"] == 0
                    fits = plan["bags_per_block"] * D * (4 if odt == "fp32" else 2) <= 16384      # (fp32 rows of D > 1024: 4 bags do not fit)
                    assert plan["stage_out"] == (D if burst and fits else 0) and (fits or D > 1024), (plan, burst)
                    assert -(-D // (G * 16)) == passes
                    assert same(m.lookup(d_idx, d_off, w, batch=B), want[mode], odt), (fmt, D, mode, odt, burst)
        _lib.set_forward_tuning()
        m = mods["plain"]
        for odt in ODTS:
            with_output(m, odt)
            g = m.sequence_plan(d_idx, d_off, batch=B)
            assert (g["vec"], g["group_lanes"], g["col_passes"], g["unroll"], g["grid"]) == (4, Gg, gpasses, 8, 1), g
            assert same(m.lookup_sequence(d_idx, d_off, batch=B), want_rows, odt), (fmt, D, odt, "un-pooled")
    finally:
        _lib.set_forward_tuning()


# ---- 3. staged and unstaged tiles, 6. rows in flight -----------------------------------------------------------------------------------

def _tile_request(fmt, lens, seed):
    """one table of 50 rows x 48 columns; bag 1 (the long one) begins and ends with padded lookups, bag 3 is all padding when padded"""
    rng = np.random.default_rng(seed)
    tab = finite_codes(rng, fmt, (50, 48))
    idx, off = ragged(rng, [50], len(lens), lens=lens)
    pad = 7
    idx[idx == pad] = 8                                   # padded lookups only where they are placed:
    s1, e1, s3, e3 = int(off[1]), int(off[2]), int(off[3]), int(off[4])
    idx[s1], idx[e1 - 1], idx[s1 + 1] = pad, pad, pad     # first, second and last of the long bag
    idx[s3:e3] = pad                                      # an all-padding bag
    return tab, idx, off, pad


@pytest.mark.parametrize("lens", (FR.STAGED_LENS, FR.UNSTAGED_LENS), ids=("staged", "unstaged"))
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_staged_and_unstaged_tiles_and_rows_in_flight(fmt, lens):
    tab, idx, off, pad = _tile_request(fmt, lens, 11 + len(lens))
    B = len(lens)
    psw = np.random.default_rng(5).standard_normal(idx.size).astype(np.float32)
    d_idx, d_off, d_psw = _dev(idx), _dev(off), _dev(psw)
    staged = sum(lens) <= 4096
    try:
        for pads in (None, [pad]):
            mods = {"plain": module(fmt, [tab], padding_idx=pads and pads[0]), "mean": module(fmt, [tab], padding_idx=pads and pads[0], pooling_mode="mean")}
            mods["weighted"] = mods["plain"]
            for mode, m in mods.items():
                w = psw if mode == "weighted" else None
                want = R.forward([tab], fmt, idx, off, B, pads, w, mode == "mean")[0]
                if pads:
                    assert not want[3].any()
                first = None
                for unroll in (2, 4, 8):                  # 6: the same bits at every depth
                    _lib.set_tuning(unroll=unroll)
                    plan = m.plan(d_idx, d_off, d_psw if w is not None else None, batch=B)
                    assert plan["unroll"] == unroll and (plan["idx_cap"] >= sum(lens)) == staged, plan
                    got = m.lookup(d_idx, d_off, d_psw if w is not None else None, batch=B)
                    assert same(got, want, "fp32"), (fmt, mode, pads, unroll)
                    first = _bits(got) if first is None else first
                    assert np.array_equal(_bits(got), first), "rows in flight change no bit"
                _lib.set_tuning()
                with_output(m, "fp16")
                assert same(m.lookup(d_idx, d_off, d_psw if w is not None else None, batch=B), want, "fp16")
                with_output(m, "fp32")
    finally:
        _lib.set_tuning()


# ---- 4. request forms ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", R.FORMATS)
def test_request_forms(fmt):
    rng = np.random.default_rng(3)
    # T = 3 mixed dims with "bd", int32 and int64, a weighted request
    dims, rows, B = [16, 144, 64], [30, 20, 25], 5
    tabs = [finite_codes(rng, fmt, (r, d)) for r, d in zip(rows, dims)]
    m = module(fmt, tabs)
    for dtype in (np.int64, np.int32):
        idx, off = ragged(rng, rows, B, dtype=dtype)
        psw = rng.standard_normal(idx.size).astype(np.float32)
        got = m.lookup(_dev(idx), _dev(off), _dev(psw))
        assert got.shape == (B, sum(dims)) and same(got, concat_bd(R.forward(tabs, fmt, idx, off, B, psw=psw)), "fp32"), dtype
    with pytest.raises(ValueError, match="one common embedding dim"):
        m.lookup_sequence(_dev(idx), _dev(off))
    # "tbd" with one dim; a batch slice into a caller's out whose other rows keep their bits, pooled and un-pooled
    tabs = [finite_codes(rng, fmt, (r, 32)) for r in rows]
    for odt in ("fp32", "bf16"):
        m = with_output(module(fmt, tabs, layout="tbd", pooling_mode="mean", padding_idx=[None, 3, None]), odt)
        idx, off = ragged(rng, rows, B)
        d_idx, d_off = _dev(idx), _dev(off)
        want = np.stack(R.forward(tabs, fmt, idx, off, B, [None, 3, None], mean=True))
        assert same(m.lookup(d_idx, d_off), want, odt)
        out = torch.full((3, B, 32), 7.0, dtype=ODTS[odt], device=DEV)
        m.lookup(d_idx, d_off, out=out, bag_begin=1, bag_count=3)
        want_slice = np.full((3, B, 32), 7.0, dtype=np.float32)
        want_slice[:, 1:4] = want[:, 1:4]
        assert same(out, want_slice, odt), "bags outside the slice keep their bits"
        rows_want, written = R.sequence(tabs, fmt, idx, off, B, bag_begin=1, bag_count=3)
        out = torch.full((idx.size, 32), 7.0, dtype=ODTS[odt], device=DEV)
        m.lookup_sequence(d_idx, d_off, out=out, bag_begin=1, bag_count=3)
        rows_want[~written] = 7.0
        assert 0 < written.sum() < idx.size and same(out, rows_want, odt)
        fresh = m.lookup_sequence(d_idx, d_off, bag_begin=1, bag_count=3)
        rows_want[~written] = 0.0
        assert same(fresh, rows_want, odt)
    # T = 300 tables with B = 1: the gather searches the borders in global memory
    T = 300
    tabs = [finite_codes(rng, fmt, (4, 16)) for _ in range(T)]
    m = module(fmt, tabs, layout="tbd")
    idx, off = ragged(rng, [4] * T, 1, lens_max=3)
    d_idx, d_off = _dev(idx), _dev(off)
    assert m.sequence_plan(d_idx, d_off, batch=1)["lds_borders"] == 0
    assert same(m.lookup_sequence(d_idx, d_off, batch=1), R.sequence(tabs, fmt, idx, off, 1)[0], "fp32")
    assert same(m.lookup(d_idx, d_off, batch=1), np.stack(R.forward(tabs, fmt, idx, off, 1)), "fp32")
    # bounds_check_mode="ignore" repairs one bad index (to row 0)
    tab = finite_codes(rng, fmt, (10, 16))
    m = module(fmt, [tab], bounds_check_mode="ignore")
    idx, off = ragged(rng, [10], 4, lens=[2, 3, 0, 1])
    bad = idx.copy()
    bad[3] = 10
    idx[3] = 0
    d_bad = _dev(bad)
    assert same(m.lookup(d_bad, _dev(off), batch=4), R.forward([tab], fmt, idx, off, 4)[0], "fp32")
    assert np.array_equal(d_bad.cpu().numpy(), idx), "the request was repaired in place"
    d_bad = _dev(bad)
    assert same(m.lookup_sequence(d_bad, _dev(off), batch=4), R.sequence([tab], fmt, idx, off, 4)[0], "fp32")


# ---- 5. far addresses ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def far():
    """one D = 128 e4m3 table whose rows pass byte offsets 2^31 and 2^32 (2^25 + 2 rows, 4 GiB), and its compacted twin: only the probe
    rows and their neighbours are written"""
    import param_amd

    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    D = 128
    probes = FR.probe_rows(D, es=1)
    assert probes[-1] * D >= 2 ** 32 and any(p * D >= 2 ** 31 > (p - 1) * D for p in probes)
    n = FR.table_rows(probes)
    free, _ = torch.cuda.mem_get_info()
    if free < n * D + 8 * GIB:
        pytest.skip(f"far FP8 table: needs {n * D / GIB:.1f} GiB + 8 GiB of free HBM, {free / GIB:.0f} GiB available")
    rng = np.random.default_rng(77)
    sent = FR.sentinel_rows(probes)
    content = finite_codes(rng, "e4m3", (len(probes) + len(sent), D))
    m = param_amd.Float8BatchedEmbeddingBagMI355([n], [D], "e4m3", device=DEV)
    tab = m.table(0).view(torch.uint8)
    for i, r in enumerate(list(probes) + list(sent)):      # one view per row: the host adds r * 128 to the base pointer in 64 bits
        tab[int(r)].copy_(_dev(content[i]))
    yield m, probes, content[:len(probes)]
    del m, tab
    torch.cuda.empty_cache()


@pytest.mark.parametrize("which", ("staged", "unstaged", "un-pooled"))
def test_far_addresses(far, which):
    m, probes, twin = far
    lens = FR.UNSTAGED_LENS if which == "unstaged" else FR.STAGED_LENS
    idx, off = FR.request(probes, lens, seed=9)
    B = len(lens)
    cidx = FR.compact(probes, idx)
    d_idx, d_off = _dev(idx), _dev(off)
    if which == "un-pooled":
        want, _ = R.sequence([twin], "e4m3", cidx, off, B)
        assert same(m.lookup_sequence(d_idx, d_off, batch=B), want, "fp32")
        return
    psw = np.random.default_rng(1).standard_normal(idx.size).astype(np.float32)
    assert (m.plan(d_idx, d_off, batch=B)["idx_cap"] >= sum(lens)) == (which == "staged")
    assert same(m.lookup(d_idx, d_off, batch=B), R.forward([twin], "e4m3", cidx, off, B)[0], "fp32")
    assert same(m.lookup(d_idx, d_off, _dev(psw), batch=B), R.forward([twin], "e4m3", cidx, off, B, psw=psw)[0], "fp32")


# ---- 7. the T = 1 modules --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", R.FORMATS)
def test_single_table_modules_against_torch_cpu(fmt):
    import torch.nn.functional as F
    from param_amd import Float8EmbeddingBagMI355, Float8EmbeddingMI355

    dt = DTYPES[fmt]
    torch.manual_seed(4)
    src = torch.randn(37, 48) * 4
    src[5, :4] = torch.tensor([-0.0, 1e-3, float("inf"), 300.0])      # (e4m3: the cast saturates Inf to NaN; torch's business)
    W8 = src.to(dt)                                                   # cast on the CPU
    W32 = W8.to(torch.float32)
    idx = torch.randint(0, 37, (6, 5))
    idx[2, 0] = 5
    psw = torch.randn(6, 5)
    for mode in ("sum", "mean"):
        for pad in (None, 9):
            bag = Float8EmbeddingBagMI355(37, 48, dt, mode=mode, padding_idx=pad, device=DEV, weight=W8)
            want = F.embedding_bag(idx, W32, mode=mode, padding_idx=pad)
            assert same_f32(bag(idx.to(DEV)).cpu().numpy(), want.numpy()), (fmt, mode, pad, "2-D")
            flat, off = idx.reshape(-1), torch.arange(6) * 5
            assert same_f32(bag(flat.to(DEV), off.to(DEV)).cpu().numpy(), want.numpy()), (fmt, mode, pad, "1-D")
            if mode == "sum" and pad is None:      # (torch's padded weighted path rounds twice per lookup: tests/test_f8_host.py bounds it)
                rows = torch.isfinite(W32).all(1)[idx].all(1)             # (a weight times Inf / NaN is left to the rule's own tests)
                wantw = F.embedding_bag(idx, W32, mode="sum", per_sample_weights=psw)
                got = bag(idx.to(DEV), per_sample_weights=psw.to(DEV)).cpu()
                assert same_f32(got[rows].numpy(), wantw[rows].numpy()), (fmt, pad, "weighted")
    cpu_bag = torch.nn.EmbeddingBag.from_pretrained(src, mode="mean", padding_idx=9)
    fb = Float8EmbeddingBagMI355.from_float(cpu_bag, dt, device=DEV)      # (a CPU source: the cast runs on the CPU)
    assert fb.weights.is_cuda and same_f32(fb(idx.to(DEV)).cpu().numpy(), F.embedding_bag(idx, W32, mode="mean", padding_idx=9).numpy())
    for odt, tdt in (("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16)):
        emb = Float8EmbeddingMI355.from_float(torch.nn.Embedding.from_pretrained(src), dt, device=DEV, output_dtype=None if odt == "fp32" else odt)
        got = emb(idx.to(DEV))
        assert got.shape == (6, 5, 48) and got.dtype == tdt and not got.requires_grad
        want = F.embedding(idx, W32).reshape(30, 48)
        if odt == "fp32":
            assert same_f32(got.reshape(30, 48).cpu().numpy(), want.numpy()), (fmt, odt)
        else:       # against torch's own cast (which does not keep a NaN's sign: f8_rules.same16)
            assert R.same16(_bits(got.reshape(30, 48)), _bits(want.to(tdt)), odt), (fmt, odt)
    assert emb(torch.zeros((2, 0), dtype=torch.int64, device=DEV)).shape == (2, 0, 48)
