"""Scaled FP8 tables on the GPU (include/param_amd.h, "SCALED FP8 TABLES"): the quantiser and the scaled lookups of the three ``Float8*``
modules against tests/f8s_rules.py, on bits (codes and exponents byte for byte, NaN codes by class; fp32 output with
``qrows_rules.same_f32``, 16-bit output with ``f8_rules.same16``).

1. conversions: the decode at all 129 exponents for all 256 codes, the encode for every code, tie and neighbour;  2. quantiser shapes;
3. the pooled lookup: widths, staged / unstaged tiles at 2 / 4 / 8 rows in flight, a compaction over several rounds, request forms;
4. the un-pooled lookup;  5. far addresses;  6. end to end: a 10 M-row uniform init that the plain cast turns into zeros."""
import numpy as np
import pytest
import torch

from param_amd import _lib
from tests import f8_rules as R
from tests import f8s_rules as S
from tests import far_rows as FR
from tests.f8_rules import finite_codes
from tests.test_gpu_f8 import DTYPES, ODTS, WIDTHS, _bits, _dev, concat_bd, ragged, same, with_output

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GIB = 1 << 30
KINDS = ("row", "table")
SRC = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def module(fmt, tables, exps, kind, **kw):
    """a scaled module holding ``tables`` (uint8 codes) with ``exps`` = [(E_t | None, e_rows | None)] through copy_from_"""
    import param_amd

    m = param_amd.Float8BatchedEmbeddingBagMI355([t.shape[0] for t in tables], [t.shape[1] for t in tables], DTYPES[fmt], device=DEV, scale=kind, **kw)
    for t, (tab, (E, er)) in enumerate(zip(tables, exps)):
        m.copy_from_(t, _dev(tab), exponents=E if kind == "table" else _dev(np.asarray(er, dtype=np.int64)))
    return m


def make_exps(rng, rows, kind, lo=-30, hi=10):
    """exponents of one table: row mode -- one per row in [lo, hi], no two neighbours equal; table mode -- one value"""
    if kind == "table":
        return (int(rng.integers(lo, hi + 1)), None)
    span = hi - lo + 1
    return (None, ((np.arange(rows) * 7 + int(rng.integers(0, span))) % span + lo).astype(np.int64))


# ---- 1. conversions ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", R.FORMATS)
def test_decode_every_code_at_every_exponent(fmt):
    """row mode: 129 rows of all 256 codes, row i rotated by i (every code meets every byte lane) at exponent i - 64, un-pooled and as
    bags of one; table mode: one-row tables at six exponents in one launch.  v = dec(code) * 2^s, exactly."""
    tab = ((np.arange(256)[None, :] + np.arange(129)[:, None]) & 255).astype(np.uint8)
    exps = [(None, np.arange(-64, 65))]
    want = S.dequant(tab, fmt, *exps[0])
    m = module(fmt, [tab], exps, "row")
    idx, off0, off1 = _dev(np.arange(129, dtype=np.int64)), _dev(np.zeros(1, dtype=np.int64)), _dev(np.arange(129, dtype=np.int64))
    for odt in ODTS:
        with_output(m, odt)
        assert same(m.lookup_sequence(idx, off0, batch=1), want, odt), (fmt, odt, "un-pooled")
        with np.errstate(invalid="ignore"):
            assert same(m.lookup(idx, off1, batch=129), np.float32(0.0) + want, odt), (fmt, odt, "bags of one")
    got = _bits(with_output(m, "fp32").lookup_sequence(idx, off0, batch=1))
    assert (got[tab == 0x80] == 0x80000000).all() and (got[tab == 0] == 0).all(), "-0.0 is kept at every exponent"
    assert same(m.dequantized_table(0), want, "fp32"), "dequantized_table is the rule"
    es = (-64, -20, -1, 0, 1, 64)
    tabs = [np.roll(np.arange(256, dtype=np.uint8), 3 * i)[None, :] for i in range(len(es))]
    texps = [(e, None) for e in es]
    m = module(fmt, tabs, texps, "table", layout="tbd")
    idx, off = _dev(np.zeros(len(es), dtype=np.int64)), _dev(np.arange(len(es), dtype=np.int64))
    want = np.stack(S.widened(tabs, fmt, texps))
    assert same(m.lookup_sequence(idx, off, batch=1), want[:, 0], "fp32")
    with np.errstate(invalid="ignore"):
        assert same(m.lookup(idx, off, batch=1), np.float32(0.0) + want, "fp32")


def _encode_rows(fmt):
    """fp32 rows [*, 16]: column 0 anchors the row's exponent at j (fmax * 2^j), the other fifteen hold every code's value, every midpoint
    between neighbouring codes and the fp32 neighbours of both, times 2^j; then the special rows"""
    vals = R.dec(np.arange(256, dtype=np.uint8), fmt)
    fin = np.sort(vals[np.isfinite(vals)].astype(np.float64))
    pts = np.concatenate([fin, (fin[1:] + fin[:-1]) / 2]).astype(np.float32)
    pts = np.concatenate([pts, np.nextafter(pts, np.float32(np.inf)), np.nextafter(pts, np.float32(-np.inf)),
                          np.float32([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-40, np.nan, np.inf, -np.inf])])
    pts = pts[~(np.abs(pts) > S.FMAX[fmt]) | ~np.isfinite(pts)]                  # (finite values stay within the anchor)
    pts = np.concatenate([pts, np.zeros(-pts.size % 15, dtype=np.float32)]).reshape(-1, 15)
    rows = []
    for j in (-30, 0, 9):
        block = np.concatenate([np.full((pts.shape[0], 1), S.FMAX[fmt], dtype=np.float32), pts], axis=1)
        rows.append(np.ldexp(block, j).astype(np.float32))
    special = np.zeros((6, 16), dtype=np.float32)
    special[0] = np.linspace(-3, 3, 16)
    special[0, 5] = 3.5                                                        # amax's mantissa is exactly 1.75 ...
    special[1] = special[0]
    special[1, 5] = np.nextafter(np.float32(3.5), np.float32(4))               # ... and the next fp32 above it
    special[2, 3] = -0.0                                                       # a row of zeros
    special[3] = np.nan                                                        # a row of NaN
    special[4] = np.tile(np.float32([np.inf, -np.inf, np.nan, 1.0]), 4)
    special[5] = np.linspace(-1, 1, 16) * 2.0 ** 100                           # beyond the exponent clamp
    return np.concatenate(rows + [special])


@pytest.mark.parametrize("src", SRC)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_encode_every_code_tie_and_neighbour(fmt, src):
    """decides that the quantiser's encode is torch's cast: exponents and codes against the rule, from fp32, bf16 and fp16 sources"""
    import param_amd

    x = torch.from_numpy(_encode_rows(fmt)).to(SRC[src])            # (a 16-bit source is rounded here; the rule reads it widened)
    if src == "fp32":
        e = S.row_exponents(x.numpy(), fmt)
        assert e[-6] + 1 == e[-5] and e[-4] == -64 and e[-3] == -64 and e[-1] == 64 and set(e[:-6].tolist()) == {-30, 0, 9}
    for kind in KINDS:
        xs = x if kind == "row" else x[:-1]                         # (the table's exponent without the row beyond the clamp: 9, not 64)
        x32 = xs.to(torch.float32).numpy()
        e = S.row_exponents(x32, fmt)
        n = x32.shape[0]
        m = param_amd.Float8BatchedEmbeddingBagMI355([n], [16], DTYPES[fmt], device=DEV, scale=kind)
        m.quantize_from_(0, xs.to(DEV))
        s = e.astype(np.int64) if kind == "row" else np.full(n, int(e.max()))
        want = S.quantize(x32, fmt, s)
        got = m.table(0).view(torch.uint8).cpu().numpy()
        if kind == "row":
            assert np.array_equal(m.row_exponents_of(0).cpu().numpy(), e), (fmt, src)
        else:
            assert int(m.table_exponents[0]) == int(e.max()), "the table's exponent is the largest row exponent"
        bad = np.argwhere((got != want) & ~R.is_nan_code(want, fmt))[:8]
        assert S.same_codes(got, want, fmt), (fmt, src, kind, [(x32[tuple(i)], hex(got[tuple(i)]), hex(want[tuple(i)])) for i in bad])
        fin = np.isfinite(x32) & (s < 64)[:, None]
        assert np.isfinite(R.dec(got, fmt)[fin]).all(), "a finite element never overflows"


# ---- 2. quantiser shapes -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", R.FORMATS)
def test_quantiser_shapes_and_strided_sources(fmt):
    import param_amd

    rng = np.random.default_rng(12)
    for D in (16, 48, 128, 1040, 2048):
        for n in (1, 7, 300):
            for src, strided in (("fp32", False), ("bf16", True), ("fp16", False)):
                wide = (rng.standard_normal((n, D + 32)) * np.exp2(rng.integers(-40, 12, (n, 1)))).astype(np.float32)
                wide[rng.integers(0, n), rng.integers(16, 16 + D)] = np.nan
                xw = torch.from_numpy(wide).to(SRC[src]).to(DEV)
                x = xw[:, 16:16 + D] if strided else xw[:, 16:16 + D].contiguous()
                assert x.is_contiguous() != strided or n == 1
                x32 = x.to(torch.float32).cpu().numpy()
                e = S.row_exponents(x32, fmt)
                for kind in KINDS:
                    m = param_amd.Float8BatchedEmbeddingBagMI355([n], [D], DTYPES[fmt], device=DEV, scale=kind)
                    m.quantize_from_(0, x)
                    if kind == "row":
                        assert np.array_equal(m.row_exponents_of(0).cpu().numpy(), e), (fmt, D, n, src)
                        want = S.quantize(x32, fmt, e.astype(np.int64))
                    else:
                        assert int(m.table_exponents[0]) == int(e.max()), (fmt, D, n, src)
                        want = S.quantize(x32, fmt, int(e.max()))
                    assert S.same_codes(m.table(0).view(torch.uint8).cpu().numpy(), want, fmt), (fmt, D, n, src, kind)


# ---- 3. the pooled lookup ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", sorted(WIDTHS))
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_every_group_width_and_column_passes(fmt, D):
    rng = np.random.default_rng(D + len(fmt))
    tab = finite_codes(rng, fmt, (40, D))
    B = 7
    idx, off = ragged(rng, [40], B, lens=[0, 9, 1, 4, 7, 2, 5])
    psw = rng.standard_normal(idx.size).astype(np.float32)
    d_idx, d_off, d_psw = _dev(idx), _dev(off), _dev(psw)
    G, passes, Gg, gpasses = WIDTHS[D]
    try:
        for kind in KINDS:
            exps = [make_exps(rng, 40, kind)]
            want = {"plain": S.forward([tab], fmt, exps, idx, off, B)[0], "weighted": S.forward([tab], fmt, exps, idx, off, B, psw=psw)[0],
                    "mean": S.forward([tab], fmt, exps, idx, off, B, mean=True)[0]}
            want_rows, _ = S.sequence([tab], fmt, exps, idx, off, B)
            mods = {"plain": module(fmt, [tab], exps, kind), "mean": module(fmt, [tab], exps, kind, pooling_mode="mean")}
            mods["weighted"] = mods["plain"]
            for burst in (1, 0):
                _lib.set_forward_tuning(stage_out=burst)
                for mode, m in mods.items():
                    w = d_psw if mode == "weighted" else None
                    for odt in ODTS:
                        with_output(m, odt)
                        plan = m.plan(d_idx, d_off, w, batch=B)
                        assert plan["bags_per_block"] >= 256 // G and plan["unroll"] == 2 and (plan["stage_out"] in (0, D)) and (burst or not plan["stage_out"])
                        assert same(m.lookup(d_idx, d_off, w, batch=B), want[mode], odt), (fmt, D, kind, mode, odt, burst)
            _lib.set_forward_tuning()
            m = mods["plain"]
            for odt in ODTS:
                with_output(m, odt)
                g = m.sequence_plan(d_idx, d_off, batch=B)
                assert (g["vec"], g["group_lanes"], g["col_passes"]) == (4, Gg, gpasses), g
                assert same(m.lookup_sequence(d_idx, d_off, batch=B), want_rows, odt), (fmt, D, kind, odt, "un-pooled")
    finally:
        _lib.set_forward_tuning()


def _tile_request(fmt, lens, seed):
    """one table of 50 rows x 48 columns; bag 1 (the long one) begins and ends with padded lookups, bag 3 is all padding when padded"""
    rng = np.random.default_rng(seed)
    tab = finite_codes(rng, fmt, (50, 48))
    idx, off = ragged(rng, [50], len(lens), lens=lens)
    pad = 7
    idx[idx == pad] = 8
    s1, e1, s3, e3 = int(off[1]), int(off[2]), int(off[3]), int(off[4])
    idx[s1], idx[e1 - 1], idx[s1 + 1] = pad, pad, pad
    idx[s3:e3] = pad
    return rng, tab, idx, off, pad


@pytest.mark.parametrize("lens", (FR.STAGED_LENS, FR.UNSTAGED_LENS), ids=("staged", "unstaged"))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_staged_and_unstaged_tiles_and_rows_in_flight(fmt, kind, lens):
    rng, tab, idx, off, pad = _tile_request(fmt, lens, 11 + len(lens))
    exps = [make_exps(rng, 50, kind)]
    B = len(lens)
    psw = np.random.default_rng(5).standard_normal(idx.size).astype(np.float32)
    d_idx, d_off, d_psw = _dev(idx), _dev(off), _dev(psw)
    staged = sum(lens) <= 4096
    try:
        for pads in (None, [pad]):
            mods = {"plain": module(fmt, [tab], exps, kind, padding_idx=pads and pads[0]),
                    "mean": module(fmt, [tab], exps, kind, padding_idx=pads and pads[0], pooling_mode="mean")}
            mods["weighted"] = mods["plain"]
            for mode, m in mods.items():
                w = psw if mode == "weighted" else None
                want = S.forward([tab], fmt, exps, idx, off, B, pads, w, mode == "mean")[0]
                if pads:
                    assert not want[3].any()
                first = None
                for unroll in (2, 4, 8):
                    _lib.set_tuning(unroll=unroll)
                    plan = m.plan(d_idx, d_off, d_psw if w is not None else None, batch=B)
                    assert plan["unroll"] == unroll and (plan["idx_cap"] >= sum(lens)) == staged, plan
                    got = m.lookup(d_idx, d_off, d_psw if w is not None else None, batch=B)
                    assert same(got, want, "fp32"), (fmt, kind, mode, pads, unroll)
                    first = _bits(got) if first is None else first
                    assert np.array_equal(_bits(got), first), "rows in flight change no bit"
                _lib.set_tuning()
                with_output(m, "fp16")
                assert same(m.lookup(d_idx, d_off, d_psw if w is not None else None, batch=B), want, "fp16")
                with_output(m, "fp32")
    finally:
        _lib.set_tuning()


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_compaction_over_several_rounds_keeps_every_exponent_in_its_place(fmt):
    """one staged tile of 1500 lookups (six 256-entry rounds, four waves each) in five bags, every third lookup and two runs padded:
    a kept lookup's exponent has to travel to the same compacted position as its index.  Rows' exponents differ inside every bag."""
    rng = np.random.default_rng(21)
    rows, D, pad = 90, 32, 13
    tab = finite_codes(rng, fmt, (rows, D))
    exps = [(None, (np.arange(rows) * 7) % 41 - 30)]                      # [-30, 10], neighbours differ
    lens = [400, 0, 700, 1, 399]
    idx, off = ragged(rng, [rows], len(lens), lens=lens)
    idx[idx == pad] = pad + 1
    idx[::3] = pad
    idx[500:640] = pad
    idx[1490:] = pad
    psw = rng.standard_normal(idx.size).astype(np.float32)
    for dtype in (np.int64, np.int32):
        d_idx, d_off, d_psw = _dev(idx.astype(dtype)), _dev(off.astype(dtype)), _dev(psw)
        for mode in ("sum", "mean"):
            m = module(fmt, [tab], exps, "row", padding_idx=pad, pooling_mode=mode)
            assert m.plan(d_idx, d_off, batch=len(lens))["idx_cap"] >= idx.size, "the tile is staged"
            want = S.forward([tab], fmt, exps, idx, off, len(lens), [pad], mean=mode == "mean")[0]
            assert same(m.lookup(d_idx, d_off, batch=len(lens)), want, "fp32"), (fmt, mode, dtype)
            if mode == "sum":
                wantw = S.forward([tab], fmt, exps, idx, off, len(lens), [pad], psw)[0]
                assert same(m.lookup(d_idx, d_off, d_psw, batch=len(lens)), wantw, "fp32"), (fmt, "weighted", dtype)
    # the same rows under a wrong exponent change bits: the check has teeth
    right, wrong = (S.forward([tab], fmt, [(None, e)], idx, off, len(lens), [pad])[0] for e in (exps[0][1], np.roll(exps[0][1], 1)))
    assert not np.array_equal(right.view(np.uint32), wrong.view(np.uint32))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_request_forms(fmt, kind):
    rng = np.random.default_rng(3)
    # T = 3 mixed dims with "bd" and three different exponents / exponent sets, int32 and int64, a weighted request
    dims, rows, B = [16, 144, 64], [30, 20, 25], 5
    tabs = [finite_codes(rng, fmt, (r, d)) for r, d in zip(rows, dims)]
    exps = [(-17, None), (0, None), (9, None)] if kind == "table" else [make_exps(rng, r, kind) for r in rows]
    m = module(fmt, tabs, exps, kind)
    for dtype in (np.int64, np.int32):
        idx, off = ragged(rng, rows, B, dtype=dtype)
        psw = rng.standard_normal(idx.size).astype(np.float32)
        got = m.lookup(_dev(idx), _dev(off), _dev(psw))
        assert got.shape == (B, sum(dims)) and same(got, concat_bd(S.forward(tabs, fmt, exps, idx, off, B, psw=psw)), "fp32"), dtype
    with pytest.raises(ValueError, match="one common embedding dim"):
        m.lookup_sequence(_dev(idx), _dev(off))
    # "tbd": a batch slice into a caller's out whose other rows keep their bits, pooled and un-pooled, with 16-bit output
    tabs = [finite_codes(rng, fmt, (r, 32)) for r in rows]
    for odt in ("fp32", "bf16"):
        m = with_output(module(fmt, tabs, exps, kind, layout="tbd", pooling_mode="mean", padding_idx=[None, 3, None]), odt)
        idx, off = ragged(rng, rows, B)
        d_idx, d_off = _dev(idx), _dev(off)
        want = np.stack(S.forward(tabs, fmt, exps, idx, off, B, [None, 3, None], mean=True))
        assert same(m.lookup(d_idx, d_off), want, odt)
        out = torch.full((3, B, 32), 7.0, dtype=ODTS[odt], device=DEV)
        m.lookup(d_idx, d_off, out=out, bag_begin=1, bag_count=3)
        want_slice = np.full((3, B, 32), 7.0, dtype=np.float32)
        want_slice[:, 1:4] = want[:, 1:4]
        assert same(out, want_slice, odt), "bags outside the slice keep their bits"
        rows_want, written = S.sequence(tabs, fmt, exps, idx, off, B, bag_begin=1, bag_count=3)
        out = torch.full((idx.size, 32), 7.0, dtype=ODTS[odt], device=DEV)
        m.lookup_sequence(d_idx, d_off, out=out, bag_begin=1, bag_count=3)
        rows_want[~written] = 7.0
        assert 0 < written.sum() < idx.size and same(out, rows_want, odt)
    # a state_dict carries codes and exponents to another module
    twin = with_output(module(fmt, [np.zeros_like(t) for t in tabs], [(0, None) if kind == "table" else (None, np.zeros(r)) for r in rows], kind,
                              layout="tbd", pooling_mode="mean", padding_idx=[None, 3, None]), "bf16")
    twin.load_state_dict(m.state_dict())
    assert same(twin.lookup(d_idx, d_off), want, "bf16")


# ---- 4. the un-pooled lookup ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_single_table_modules_against_torch_cpu(fmt, kind):
    """Float8EmbeddingMI355 / Float8EmbeddingBagMI355 with a scale, built by from_float on the device: the lookups equal torch's CPU
    functions over the module's own dequantised table"""
    import torch.nn.functional as F
    from param_amd import Float8EmbeddingBagMI355, Float8EmbeddingMI355
    from tests.qrows_rules import same_f32

    torch.manual_seed(4)
    src = torch.randn(37, 48) * torch.exp2(torch.randint(-25, 5, (37, 1)).float())
    idx = torch.randint(0, 37, (6, 5))
    for odt, tdt in (("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16)):
        emb = Float8EmbeddingMI355.from_float(torch.nn.Embedding.from_pretrained(src), DTYPES[fmt], scale=kind, device=DEV,
                                              output_dtype=None if odt == "fp32" else odt)
        W = emb.dequantized_table(0).cpu()
        x32 = src.numpy()
        e = S.row_exponents(x32, fmt)
        s = e.astype(np.int64) if kind == "row" else int(e.max())
        codes = S.quantize(x32, fmt, s)
        assert S.same_codes(emb.table(0).view(torch.uint8).cpu().numpy(), codes, fmt)
        assert same_f32(W.numpy(), S.dequant(codes, fmt, *((None, s) if kind == "row" else (s, None))))
        got = emb(idx.to(DEV))
        assert got.shape == (6, 5, 48) and got.dtype == tdt
        want = F.embedding(idx, W).reshape(30, 48)
        if odt == "fp32":
            assert same_f32(got.reshape(30, 48).cpu().numpy(), want.numpy())
        else:
            assert R.same16(_bits(got.reshape(30, 48)), _bits(want.to(tdt)), odt)
    rel = float((W - src).abs().sum() / src.abs().sum())
    assert rel < (0.04 if fmt == "e4m3" else 0.08) or kind == "table", rel
    for mode in ("sum", "mean"):
        bag = Float8EmbeddingBagMI355.from_float(torch.nn.EmbeddingBag.from_pretrained(src, mode=mode, padding_idx=9), DTYPES[fmt], scale=kind, device=DEV)
        W = bag.dequantized_table(0).cpu()
        assert same_f32(bag(idx.to(DEV)).cpu().numpy(), F.embedding_bag(idx, W, mode=mode, padding_idx=9).numpy()), (fmt, kind, mode)


# ---- 5. far addresses ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def far():
    """one D = 128 e4m3 table with row exponents whose rows pass byte offsets 2^31 and 2^32 (2^25 + 2 rows, 4 GiB), and its compacted
    twin: only the probe rows, their neighbours and their exponents are written (the neighbours' exponents differ from the probes')"""
    import param_amd

    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    D = 128
    probes = FR.probe_rows(D, es=1)
    n = FR.table_rows(probes)
    free, _ = torch.cuda.mem_get_info()
    if free < n * D + 8 * GIB:
        pytest.skip(f"far FP8 table: needs {n * D / GIB:.1f} GiB + 8 GiB of free HBM, {free / GIB:.0f} GiB available")
    rng = np.random.default_rng(78)
    sent = FR.sentinel_rows(probes)
    content = finite_codes(rng, "e4m3", (len(probes) + len(sent), D))
    e = np.concatenate([(np.arange(len(probes)) * 5) % 41 - 30, np.full(len(sent), 33)]).astype(np.int64)
    m = param_amd.Float8BatchedEmbeddingBagMI355([n], [D], "e4m3", device=DEV, scale="row")
    tab, rexp = m.table(0).view(torch.uint8), m.row_exponents_of(0)
    for i, r in enumerate(list(probes) + list(sent)):
        tab[int(r)].copy_(_dev(content[i]))
        rexp[int(r)] = int(e[i])
    yield m, probes, content[:len(probes)], e[:len(probes)]
    del m, tab, rexp
    torch.cuda.empty_cache()


@pytest.mark.parametrize("which", ("staged", "unstaged", "un-pooled"))
def test_far_addresses(far, which):
    m, probes, twin, e = far
    exps = [(None, e)]
    lens = FR.UNSTAGED_LENS if which == "unstaged" else FR.STAGED_LENS
    idx, off = FR.request(probes, lens, seed=9)
    B = len(lens)
    cidx = FR.compact(probes, idx)
    d_idx, d_off = _dev(idx), _dev(off)
    if which == "un-pooled":
        want, _ = S.sequence([twin], "e4m3", exps, cidx, off, B)
        assert same(m.lookup_sequence(d_idx, d_off, batch=B), want, "fp32")
        return
    psw = np.random.default_rng(1).standard_normal(idx.size).astype(np.float32)
    assert (m.plan(d_idx, d_off, batch=B)["idx_cap"] >= sum(lens)) == (which == "staged")
    assert same(m.lookup(d_idx, d_off, batch=B), S.forward([twin], "e4m3", exps, cidx, off, B)[0], "fp32")
    assert same(m.lookup(d_idx, d_off, _dev(psw), batch=B), S.forward([twin], "e4m3", exps, cidx, off, B, psw=psw)[0], "fp32")


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_ten_million_row_uniform_init_survives(kind):
    """``from_float(BatchedEmbeddingBagMI355 with the uniform_dlrm init of 10 M rows, scale=...)``: torch's plain e4m3fn cast of that table
    is all zeros; the scaled table is not, and the lookup is the rule over the module's own stored bytes"""
    import param_amd

    n, D, B, L = 10_000_000, 16, 64, 20
    src = param_amd.BatchedEmbeddingBagMI355([n], D, device=DEV, init="uniform_dlrm", seed=3, fused_update=False)
    W = src.table(0)
    assert float(W.abs().max()) <= 1.0 / np.sqrt(n) and float(W.abs().max()) > 0.9 / np.sqrt(n)
    assert not bool(W.to(torch.float8_e4m3fn).view(torch.uint8).bitwise_and(0x7f).any()), "the plain cast of this table is all zeros"
    m = param_amd.Float8BatchedEmbeddingBagMI355.from_float(src, "e4m3", scale=kind)
    assert m.scale == kind and m.pooling_mode == "sum" and m.weights.is_cuda
    codes_dev = m.table(0).view(torch.uint8)
    assert float(codes_dev.bitwise_and(0x7f).ne(0).float().mean()) > 0.95, "the scaled table is not all zeros"
    rng = np.random.default_rng(8)
    uniq = np.unique(np.concatenate([rng.integers(0, n, B * L - 3), [0, 1, n - 1]]))
    idx = rng.choice(uniq, B * L).astype(np.int64)
    off = (np.arange(B) * L).astype(np.int64)
    d_uniq = _dev(uniq)
    twin = codes_dev[d_uniq].cpu().numpy()
    x32 = W[d_uniq].cpu().numpy()
    if kind == "row":
        e = m.row_exponents_of(0)[d_uniq].cpu().numpy().astype(np.int64)
        exps = [(None, e)]
        assert np.array_equal(e, S.row_exponents(x32, "e4m3")) and S.same_codes(twin, S.quantize(x32, "e4m3", e), "e4m3")
    else:
        E = int(m.table_exponents[0])
        exps = [(E, None)]
        assert E == int(m_exp_max(W)) and S.same_codes(twin, S.quantize(x32, "e4m3", E), "e4m3")
    cidx = np.searchsorted(uniq, idx)
    want = S.forward([twin], "e4m3", exps, cidx, off, B)[0]
    got = m.lookup(_dev(idx), _dev(off), batch=B)
    assert same(got, want, "fp32") and np.abs(want).max() > 0
    rel = np.abs(S.dequant(twin, "e4m3", *exps[0]) - x32).sum() / np.abs(x32).sum()
    assert rel < 0.04, rel


def m_exp_max(W):
    """the table exponent the rule gives for a device table: the row exponent of the table's largest magnitude"""
    return S.row_exponents(W.abs().max().reshape(1, 1).cpu().numpy(), "e4m3")[0]
