"""MXFP4 tables on the GPU (include/param_amd.h, "MXFP4 TABLES"): ``MX4BatchedEmbeddingBagMI355`` against tests/mx4_rules.py, on bits
(NaN by class; the code bytes of a NaN block are not compared).  No tolerance anywhere: the rule is exact.

1. every code at the edge scales (decides the decode);  2. the quantiser (decides the encode);  3. the pooled lookup;  4. the un-pooled
lookup;  5. a table past 4 GiB;  6. end to end."""
import numpy as np
import pytest
import torch

from param_amd import _lib
from tests import far_rows as FR
from tests import mx4_rules as M
from tests.qrows_rules import fmaf
from tests.test_gpu_f8 import ODTS, _bits, _dev, ragged, same, with_output

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GIB = 1 << 30
WIDTHS = (32, 128, 160, 512, 1024, 2048)      # every lane-group width, one that is no power of two, the two-pass width


def module(tables, dims, **kw):
    import param_amd

    m = param_amd.MX4BatchedEmbeddingBagMI355([t.shape[0] for t in tables], dims, device=DEV, **kw)
    for t, (tab, d) in enumerate(zip(tables, dims)):
        m.copy_from_(t, _dev(tab[:, :d // 2]), _dev(tab[:, d // 2:d // 2 + d // 32]))
    return m


def random_table(rng, rows, dim, nan_row=0):
    """codes of every kind under scale bytes near 127 (sums stay finite); block 0 of ``nan_row`` is a NaN block"""
    tab = np.zeros((rows, M.row_bytes(dim)), dtype=np.uint8)
    tab[:, :dim // 2] = rng.integers(0, 256, (rows, dim // 2))
    tab[:, dim // 2:dim // 2 + dim // 32] = rng.integers(120, 135, (rows, dim // 32))
    tab[nan_row, dim // 2] = 255
    return tab


def pool(W, idx, off, B, t, psw=None, mean=False):
    """the rule over table t's B bags (``off``: closed offsets): sequential fp32 additions -- the exact fmaf when weighted -- in index
    order from +0.0; mean: one division by the bag's length, none for an empty bag"""
    out = np.zeros((B, W.shape[1]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for b in range(B):
            s, e = int(off[t * B + b]), int(off[t * B + b + 1])
            acc = np.zeros(W.shape[1], dtype=np.float32)
            for j in range(s, e):
                acc = fmaf(psw[j], W[idx[j]], acc) if psw is not None else acc + W[idx[j]]
            out[b] = acc / np.float32(e - s) if mean and e > s else acc
    return out


# ---- 1. every code at the edge scales ---------------------------------------------------------------------------------------------------

def test_every_code_at_the_edge_scales():
    scales = np.array([2, 3, 126, 127, 128, 251, 252, 255], dtype=np.uint8)
    # row (s, i): column c holds code (c + i) % 16 -- every code meets every nibble position of a lane's 8 bytes -- under scale s
    code = (np.arange(32)[None, :] + np.arange(16)[:, None]) % 16
    packed = (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    tab = np.zeros((128, 24), dtype=np.uint8)
    tab[:, :16] = np.tile(packed, (8, 1))
    tab[:, 16] = np.repeat(scales, 16)
    want = M.dequant(tab, 32)
    assert np.isnan(want[112:]).all() and np.isfinite(want[:112]).all() and np.abs(want[:112]).max() == 6 * 2.0 ** 125
    m = module([tab], [32])
    idx, off1 = _dev(np.arange(128, dtype=np.int64)), _dev(np.arange(129, dtype=np.int64))
    for odt in ODTS:
        with_output(m, odt)
        rows = m.lookup_sequence(idx, _dev(np.zeros(1, dtype=np.int64)), batch=1)
        assert rows.dtype == ODTS[odt] and same(rows, want, odt), (odt, "un-pooled")
        if odt == "fp32":
            neg0 = np.tile(code == 8, (7, 1))
            assert (_bits(rows)[:112][neg0] == 0x80000000).all(), "-0.0 is kept at every scale"
        assert same(m.lookup(idx, off1, batch=128), np.float32(0) + want, odt), (odt, "bags of one")


# ---- 2. the quantiser -------------------------------------------------------------------------------------------------------------------

def quantiser_blocks():
    """blocks of 32 fp32 columns: column 0 anchors the block exponent at 2^j, the others are e2m1 values, midpoints, the fp32 neighbours of
    both, values in (6, 8) and tiny values, each times the anchor's scale; then the special blocks"""
    v = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, .25, .75, 1.25, 1.75, 2.5, 3.5, 5, 6.5, 7, 7.99, 1e-3, 2.0 ** -20], dtype=np.float32)
    v = np.concatenate([v, np.nextafter(v, np.float32(100)), np.nextafter(v, np.float32(-100))])
    v = np.concatenate([v, -v])
    blocks = []
    with np.errstate(all="ignore"):
        for j in (-149, -140, -127, -126, -125, -124, -123, -122, -60, -1, 0, 1, 60, 126, 127):      # subnormal anchors, the clamp, the range
            scale = np.float32(2.0 ** (max(j + 125, 2) - 127))
            for k in range(0, v.size, 31):
                b = np.zeros(32, dtype=np.float32)
                b[0] = np.float32(2.0 ** j)
                b[1:1 + v[k:k + 31].size] = v[k:k + 31] * scale
                blocks.append(b)
    z = np.zeros(32, dtype=np.float32)
    neg = z.copy(); neg[[3, 4]] = -0.0
    fmax = z.copy(); fmax[7] = np.finfo(np.float32).max; fmax[8] = -1e38
    p2 = z.copy(); p2[5] = 8.0; p2[6] = 3.0
    pred = p2.copy(); pred[5] = np.nextafter(np.float32(8), np.float32(0))
    nan = np.linspace(-3, 3, 32, dtype=np.float32); nan[9] = np.nan
    inf = np.linspace(-3, 3, 32, dtype=np.float32); inf[31] = np.inf
    return np.stack(blocks + [z, neg, fmax, p2, pred, nan, inf])


@pytest.mark.parametrize("src_dtype", ("fp32", "bf16", "fp16"))
@pytest.mark.parametrize("dim", (32, 96, 2048))
def test_quantiser(dim, src_dtype):
    import param_amd

    blocks = quantiser_blocks()
    per_row = dim // 32
    pad = (-len(blocks)) % per_row
    x = np.concatenate([blocks, np.zeros((pad, 32), dtype=np.float32)]).reshape(-1, dim)
    with np.errstate(all="ignore"):
        src = torch.from_numpy(x).to(ODTS[src_dtype])      # (16-bit sources: other values, some of them Inf -- the rule takes what it is given)
    want = M.quantize(src.to(torch.float32).numpy())
    nan_codes = np.repeat(want[:, dim // 2:dim // 2 + per_row] == 255, 16, axis=1)
    assert nan_codes.any() and (want[:, dim // 2:dim // 2 + per_row] == 2).any(), "NaN blocks and the lower clamp are there"
    m = param_amd.MX4BatchedEmbeddingBagMI355([x.shape[0]], [dim], device=DEV)
    wide = torch.zeros((x.shape[0], dim + 64), dtype=ODTS[src_dtype], device=DEV)
    wide[:, 32:32 + dim] = src.to(DEV)
    for name, s in (("contiguous", src.to(DEV)), ("strided", wide[:, 32:32 + dim])):
        m.table(0).fill_(0xAA)                              # pad bytes must be written
        m.quantize_from_(0, s)
        got = m.table(0).cpu().numpy()
        got[:, :dim // 2][nan_codes] = 0
        bad = np.argwhere(got != want)[:6]
        assert np.array_equal(got, want), (name, [(int(r), int(c), int(got[r, c]), int(want[r, c])) for r, c in bad])


# ---- 3. the pooled lookup ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", WIDTHS)
def test_pooled(dim):
    rng = np.random.default_rng(dim)
    dims, rows, B = [dim, 32, dim], [37, 29, 41], 6
    tabs = [random_table(rng, r, d, nan_row=3) for r, d in zip(rows, dims)]
    W = [M.dequant(tab, d) for tab, d in zip(tabs, dims)]
    m = module(tabs, dims)
    col0 = np.concatenate([[0], np.cumsum(dims)])
    try:
        for U in (2, 4):
            _lib.set_tuning(unroll=U)
            idt = np.int64 if U == 2 else np.int32
            idx, off = ragged(rng, rows, B, dtype=idt, lens=[0, 1, U - 1, U, U + 1, 7])
            cap = m.plan(_dev(idx), _dev(off), batch=B)
            assert cap["unroll"] == U and cap["idx_cap"] >= idx.size, "the short request is staged"
            # the long request: table 0's last bag alone is longer than the index tile, so its tile reads the request
            lidx, loff = ragged(rng, rows, B, dtype=idt, lens=[0, 1, U - 1, U, U + 1, 7])
            long_bag = rng.integers(0, rows[0], cap["idx_cap"] + 5).astype(idt)
            lidx = np.concatenate([lidx[:loff[B]], long_bag, lidx[loff[B]:]])
            loff = loff.copy()
            loff[B:] += long_bag.size
            for name, (ix, of) in (("staged", (idx, off)), ("unstaged", (lidx, loff))):
                psw = rng.standard_normal(ix.size).astype(np.float32)
                d_ix, d_of = _dev(ix), _dev(of)
                for mode, odt in (("plain", "fp32"), ("weighted", "fp32"), ("mean", "fp32"), ("plain", "bf16"), ("weighted", "fp16")):
                    if name == "unstaged" and (odt != "fp32" or (mode == "mean" and U == 4)):
                        continue
                    m.pooling_mode, m._mean = ("mean", True) if mode == "mean" else ("sum", False)
                    with_output(m, odt)
                    w = psw if mode == "weighted" else None
                    want = np.concatenate([pool(W[t], ix, of, B, t, w, mode == "mean") for t in range(3)], axis=1)
                    got = m.lookup(d_ix, d_of, None if w is None else _dev(w), batch=B)
                    assert same(got, want, odt), (dim, U, name, mode, odt)
                    hit = np.array([[3 in ix[of[t * B + b]:of[t * B + b + 1]] for t in range(3)] for b in range(B)])
                    nan_cols = np.isnan(want)
                    assert all(nan_cols[b, col0[t]:col0[t] + 32].all() == hit[b, t] and not nan_cols[b, col0[t] + 32:col0[t + 1]].any()
                               for b in range(B) for t in range(3)), "NaN reaches the bags that look the NaN block up, and only its columns"
            # a batch slice into a caller's out: the other rows keep their bits
            m.pooling_mode, m._mean = "sum", False
            with_output(m, "fp32")
            out = torch.full((B, sum(dims)), -7.25, device=DEV)
            m.lookup(_dev(idx), _dev(off), out=out, bag_begin=1, bag_count=3, batch=B)
            want = np.concatenate([pool(W[t], idx, off, B, t) for t in range(3)], axis=1)
            want[[0, 4, 5]] = -7.25
            assert same(out, want, "fp32"), (dim, U, "slice")
    finally:
        _lib.set_tuning()
    # [T, B, D] addressing: one common dim
    tb = [random_table(rng, 19, dim) for _ in range(3)]
    m3 = module(tb, [dim] * 3, layout="tbd", output_dtype=torch.bfloat16)
    idx, off = ragged(rng, [19] * 3, B, dtype=np.int32)
    want = np.stack([pool(M.dequant(tb[t], dim), idx, off, B, t) for t in range(3)])
    assert same(m3.lookup(_dev(idx), _dev(off), batch=B), want, "bf16"), (dim, "tbd")


# ---- 4. the un-pooled lookup ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", WIDTHS)
def test_unpooled(dim):
    rng = np.random.default_rng(1000 + dim)
    rows, B = [23, 31, 17], 4
    tabs = [random_table(rng, r, dim, nan_row=1) for r in rows]
    m = module(tabs, [dim] * 3)
    idx, off = ragged(rng, rows, B, lens=[40, 0, 61, 9])      # 110 positions a table: the 256-position tiles straddle the table borders
    table_of = np.repeat(np.arange(3), 110)
    W = [M.dequant(tab, dim) for tab in tabs]
    want = np.stack([W[t][idx[j]] for j, t in enumerate(table_of)])
    for odt in ODTS:
        with_output(m, odt)
        assert same(m.lookup_sequence(_dev(idx), _dev(off), batch=B), want, odt), (dim, odt)
    # a batch slice (bags 2 and 3 of every table) into a caller's out
    with_output(m, "fp32")
    out = torch.full((idx.size, dim), 3.5, device=DEV)
    m.lookup_sequence(_dev(idx), _dev(off), batch=B, out=out, bag_begin=2, bag_count=2)
    inside = (np.arange(330) % 110) >= 40
    assert same(out, np.where(inside[:, None], want, np.float32(3.5)), "fp32"), (dim, "slice")


# ---- 5. 64-bit addressing ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def far():
    """one D = 128 table (72-byte rows) just past 4 GiB, and its compacted twin: only the probe rows and their neighbours are written"""
    import param_amd

    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    D = 128
    probes = FR.probe_rows(M.row_bytes(D), es=1)      # (far_rows counts a float row's bytes as D * es: a 72-byte row)
    n = FR.table_rows(probes)
    free, _ = torch.cuda.mem_get_info()
    if free < n * M.row_bytes(D) + 8 * GIB:
        pytest.skip(f"far MXFP4 table: needs {n * M.row_bytes(D) / GIB:.1f} GiB + 8 GiB of free HBM, {free / GIB:.0f} GiB available")
    rng = np.random.default_rng(5)
    sent = FR.sentinel_rows(probes)
    content = random_table(rng, len(probes) + len(sent), D, nan_row=len(probes))
    m = param_amd.MX4BatchedEmbeddingBagMI355([n], [D], device=DEV)
    tab = m.table(0)
    for i, r in enumerate(list(probes) + list(sent)):
        tab[int(r)].copy_(_dev(content[i]))
    yield m, probes, content[:len(probes)]
    del m, tab
    torch.cuda.empty_cache()


@pytest.mark.parametrize("which", ("staged", "unstaged", "un-pooled"))
def test_far_addresses(far, which):
    m, probes, twin = far
    assert probes[-1] * 72 > 4 * GIB
    lens = FR.UNSTAGED_LENS if which == "unstaged" else FR.STAGED_LENS
    idx, off = FR.request(probes, lens, seed=9)
    B, W = len(lens), M.dequant(twin, 128)
    cidx = FR.compact(probes, idx)
    if which == "un-pooled":
        assert same(m.lookup_sequence(_dev(idx), _dev(off), batch=B), W[cidx], "fp32")
        return
    assert (m.plan(_dev(idx), _dev(off), batch=B)["idx_cap"] >= sum(lens)) == (which == "staged")
    assert same(m.lookup(_dev(idx), _dev(off), batch=B), pool(W, cidx, off, B, 0), "fp32")


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------

def test_from_float_then_lookup_and_state_dict():
    import param_amd

    rng = np.random.default_rng(6)
    n, D, B, L = 4096, 128, 32, 20
    x = rng.uniform(-1 / np.sqrt(1e7), 1 / np.sqrt(1e7), (n, D)).astype(np.float32)      # the uniform init of a 10 M-row table
    m = param_amd.MX4BatchedEmbeddingBagMI355.from_float([_dev(x)])
    tab = M.quantize(x)
    assert np.array_equal(m.table(0).cpu().numpy(), tab)
    W = M.dequant(tab, D)
    assert same(m.dequantized_table(0), W, "fp32")
    idx = rng.integers(0, n, B * L).astype(np.int64)
    off = (np.arange(B) * L).astype(np.int64)
    got = m.lookup(_dev(idx), _dev(off), batch=B)
    assert same(got, pool(W, idx, np.concatenate([off, [B * L]]), B, 0), "fp32")
    m2 = param_amd.MX4BatchedEmbeddingBagMI355([n], [D], device=DEV)
    m2.load_state_dict(m.state_dict())
    assert torch.equal(m2.weights, m.weights) and torch.equal(m2.lookup(_dev(idx), _dev(off), batch=B), got)
