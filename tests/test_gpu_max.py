"""Max pooling on the GPU (``pytest -m gpu``): everything is compared on bits against the numpy restatement of the rule
(tests/max_rules.py), which tests/test_max_host.py holds to torch's CPU module.

Forward (``pm_embbag_fwd_max``): values and ``max_indices`` over the widths, table dtypes, index dtypes and layouts, with the special
values (NaN first / later, signed zeros, ties, negative rows, -Inf) and bag lengths 0, 1, 2, 3 and 5 in the request; the unstaged path
(a bag of 5000 lookups), staging that compacts padding over several rounds, batch slices, 16-bit output, the sanitiser in front.
Backward: the expansion kernel (``pm_embbag_max_grad``) against the rule's ``g_seq`` at every lane-group width (D = 8 .. 512: 8, 16, 32
and 64 lanes a bag, one and two rounds a lane), both index types and a bag of 5000 positions; ``dense_grad`` / ``scatter_add_`` against the
sequence calls fed the numpy-expanded gradient and against the rule, at D = 8 and at every other width; ``MaxEmbeddingBagMI355``
autograd against torch's recorded gradient; 1100 tables.  The forward's other plans (tiles of several bags per lane group, 1024-bag
tiles, the bursts against row stores, the XCD mappings ...) are run by tests/test_gpu_plan_sweep.py, its far addresses by
tests/test_gpu_far_addresses.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import max_cases as C
from tests import max_rules as M
from tests import out16_rules as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
LENS = (0, 1, 2, 3, 5)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    import param_amd

    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    param_amd.load_library()


def _bits(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().contiguous()
        return t.view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype=dtype)


def _split(out, dims, layout):
    o = out.detach().cpu().numpy() if isinstance(out, torch.Tensor) else out
    if layout == "tbd":
        return [o[t] for t in range(len(dims))]
    col = np.concatenate([[0], np.cumsum(dims)])
    return [o[:, col[t]:col[t + 1]] for t in range(len(dims))]


def _join(parts, layout):
    return np.stack(parts) if layout == "tbd" else np.concatenate(parts, axis=1)


def _special_rows(rng, rows, D):
    """fp32 weights (multiples of 1/8: exact in bf16 and fp16) whose first eight rows are the special ones"""
    w = (rng.integers(-80, 81, size=(rows, D)) / 8.0).astype(np.float32)
    w[0, 0] = np.nan
    w[1], w[2] = -0.0, 0.0
    w[3] = -np.inf
    w[5] = w[4]
    w[6], w[7] = -np.abs(w[6]) - 0.125, -np.abs(w[7]) - 0.125
    return w


def _model(rows, D, dname="f32", pads=None, layout="bd", mode="max", weights=None, seed=0, **kw):
    """a module whose tables hold ``_special_rows`` (or ``weights``) -> (module, the tables widened to fp32 as numpy)"""
    import param_amd

    kw.setdefault("fused_update", False)
    pads = None if pads is None or all(k is None for k in pads) else list(pads)
    cls = param_amd.MaxBatchedEmbeddingBagMI355 if mode == "max" else param_amd.BatchedEmbeddingBagMI355
    m = cls(list(rows), D, dtype=TDT[dname], device=DEV, init=None, layout=layout, padding_idx=pads, pooling_mode=mode, **kw)
    rng = np.random.default_rng(seed)
    tabs = []
    for t, r in enumerate(rows):
        w = _special_rows(rng, r, D) if weights is None else weights[t]
        m.table(t).copy_(_dev(w).to(TDT[dname]))
        tabs.append(m.table(t).float().cpu().numpy())
    return m, tabs


def _request(rng, rows, B, pads, extra_pad=0.25):
    """table-major indices / offsets: every table starts with the special bags, then bags whose lengths cycle through 0, 1, 2, 3, 5;
    about ``extra_pad`` of a padded table's random lookups are its padding index"""
    idx, off = [], []
    for t, r in enumerate(rows):
        p = pads[t]
        q = 8 if p is None else p
        bags = [[0, 8, 9], [8, 0, 9], [1, 2], [2, 1], [4, 5], [q, 6, 7], [q, q], [3], []]
        while len(bags) < B:
            n = LENS[len(bags) % len(LENS)]
            bag = rng.integers(0, r, size=n)
            if p is not None:
                bag = np.where(rng.random(n) < extra_pad, p, bag)
            bags.append(list(map(int, bag)))
        for bag in bags[:B]:
            off.append(len(idx))
            idx += bag
    return np.array(idx, dtype=np.int64), np.array(off, dtype=np.int64)


def _assert_conditions(tabs, idx_h, off_h, B, pads):
    """what the request is there for, asserted on the request (table 0)"""
    w, p = tabs[0], pads[0]
    end = list(off_h[1:]) + [idx_h.size]
    bags = [list(idx_h[off_h[b]:end[b]]) for b in range(B)]
    assert {len(b) for b in bags} >= set(LENS)
    assert np.isnan(w[bags[0][0], 0]) and np.isnan(w[bags[1][1], 0]) and not np.isnan(w[bags[1][0], 0])
    assert np.signbit(w[bags[2][0]]).all() and (w[bags[2][0]] == 0).all() and not np.signbit(w[bags[2][1]]).any() and bags[3] == bags[2][::-1]
    assert bags[4][0] != bags[4][1] and np.array_equal(w[bags[4][0]], w[bags[4][1]])
    assert (w[bags[5][1:]] < 0).all() and np.isneginf(w[bags[7][0]]).all() and bags[8] == []
    if p is not None:
        assert bags[5][0] == p and all(r == p for r in bags[6])


def _check_forward(rows, D, dname, pads, idt, layout, B=23, seed=0):
    rng = np.random.default_rng(seed)
    T = len(rows)
    m, tabs = _model(rows, D, dname, pads, layout, seed=seed)
    idx_h, off_h = _request(rng, rows, B, pads)
    _assert_conditions(tabs, idx_h, off_h, B, pads)
    want_v, want_a = M.forward(tabs, idx_h, off_h, B, pads)
    idx, off = _dev(idx_h, idt), _dev(off_h, idt)
    plain = m.lookup(idx, off, batch=B)
    out, arg = m.lookup(idx, off, batch=B, return_max_indices=True)
    assert arg.dtype == torch.int32 and arg.shape == out.shape
    assert np.array_equal(_bits(plain), _bits(out)), "with and without max_indices"
    dims = [D] * T
    for t, (gv, ga) in enumerate(zip(_split(out, dims, layout), _split(arg, dims, layout))):
        assert np.array_equal(_bits(gv), _bits(want_v[t])), ("values", t)
        assert np.array_equal(ga, want_a[t]), ("max_indices", t)
        assert (ga[8] == -1).all() and (pads[t] is None or (ga[6] == -1).all())
    return m, tabs, idx_h, off_h, idx, off, want_v, want_a


@pytest.mark.parametrize("dname,D", [("f32", 4), ("f32", 8), ("f32", 128), ("f32", 132), ("bf16", 8), ("bf16", 128), ("f16", 8), ("f16", 128)])
def test_forward_values_and_max_indices(dname, D):
    _check_forward((50, 17, 300), D, dname, (11, None, 299), torch.int64, "bd", seed=D)


@pytest.mark.parametrize("layout", ["bd", "tbd"])
@pytest.mark.parametrize("idt", [torch.int32, torch.int64])
def test_index_dtypes_and_layouts(idt, layout):
    _check_forward((50, 17, 300), 8, "f32", (11, None, 299), idt, layout, seed=3)
    _check_forward((50, 17), 16, "bf16", (None, None), idt, layout, seed=4)


@pytest.mark.parametrize("dname", ["f32", "bf16"])
@pytest.mark.parametrize("padded", [False, True])
def test_a_bag_beyond_the_index_tile_takes_the_unstaged_path(dname, padded):
    rng = np.random.default_rng(5)
    rows, D, B = (300,), 8, 3
    pads = (7,) if padded else (None,)
    m, tabs = _model(rows, D, dname, pads, seed=5)
    long_bag = rng.integers(0, 300, size=5000)
    if padded:
        long_bag[rng.random(5000) < 0.3] = 7
        long_bag[0] = 7                                    # padding first ...
    long_bag[1 if padded else 0] = 0                       # ... and the NaN row as the first kept lookup
    idx_h = np.concatenate([[8, 9], long_bag, [10]]).astype(np.int64)
    off_h = np.array([0, 2, 5002], dtype=np.int64)
    assert 5000 > 4096                                     # idx_cap <= 4096: the tile is not staged
    want_v, want_a = M.forward(tabs, idx_h, off_h, B, pads)
    assert np.isnan(want_v[0][1, 0]) and want_a[0][1, 0] == 0
    out, arg = m.lookup(_dev(idx_h), _dev(off_h), batch=B, return_max_indices=True)
    assert np.array_equal(_bits(out), _bits(want_v[0])) and np.array_equal(arg.cpu().numpy(), want_a[0])
    assert np.array_equal(_bits(m.lookup(_dev(idx_h), _dev(off_h), batch=B)), _bits(want_v[0]))


def test_staging_compacts_padding_over_several_rounds_and_tiles():
    import param_amd
    from param_amd import _lib

    rng = np.random.default_rng(6)
    rows, D, B, L = (400, 90), 8, 100, 20
    pads = (5, 0)
    m, tabs = _model(rows, D, "f32", pads, seed=6)
    idx_h = np.concatenate([rng.integers(0, r, size=B * L) for r in rows]).astype(np.int64)
    idx_h[:B * L][rng.random(B * L) < 0.4] = 5
    idx_h[B * L:][rng.random(B * L) < 0.4] = 0
    off_h = (np.arange(2 * B) * L).astype(np.int64)
    idx, off = _dev(idx_h), _dev(off_h)
    plan = (ctypes.c_int32 * 12)()
    op = m._tables().request(idx, off, B, None, 0, None, forward=True)
    assert param_amd.load_library().pm_embbag_plan(ctypes.byref(op), _lib.PM_PLAN_PADDED, plan) == _lib.PM_OK
    p = dict(zip(_lib.PLAN_FIELDS, plan))
    assert p["tiles_per_table"] > 1 and 2 * 256 < p["bags_per_block"] * L <= p["idx_cap"], p      # staged, several rounds, several tiles
    want_v, want_a = M.forward(tabs, idx_h, off_h, B, pads)
    out, arg = m.lookup(idx, off, batch=B, return_max_indices=True)
    for t, (gv, ga) in enumerate(zip(_split(out, [D, D], "bd"), _split(arg, [D, D], "bd"))):
        assert np.array_equal(_bits(gv), _bits(want_v[t])) and np.array_equal(ga, want_a[t]), t


def test_a_batch_slice_writes_its_own_rows_only():
    rows, D, B = (50, 17, 300), 8, 23
    pads = (11, None, 299)
    m, tabs, idx_h, off_h, idx, off, want_v, want_a = _check_forward(rows, D, "f32", pads, torch.int64, "bd", B=B, seed=7)
    b0, nb = 5, 11
    out = torch.full((B, 3 * D), 12345.0, device=DEV)
    arg = torch.full((B, 3 * D), -77, dtype=torch.int32, device=DEV)
    o2, a2 = m.lookup(idx, off, batch=B, out=out, bag_begin=b0, bag_count=nb, max_indices=arg)
    assert o2 is out and a2 is arg
    wv, wa = np.full((B, 3 * D), 12345.0, dtype=np.float32), np.full((B, 3 * D), -77, dtype=np.int32)
    wv[b0:b0 + nb] = _join(want_v, "bd")[b0:b0 + nb]
    wa[b0:b0 + nb] = _join(want_a, "bd")[b0:b0 + nb]
    assert np.array_equal(_bits(out), _bits(wv)) and np.array_equal(arg.cpu().numpy(), wa)


def test_forward_of_a_fused_update_module_is_the_lookup_and_refuses_backward():
    rng = np.random.default_rng(13)
    rows, D, B = (50, 300), 8, 23
    pads = (11, None)
    m, tabs = _model(rows, D, "f32", pads, fused_update=True)
    idx_h, off_h = _request(rng, rows, B, pads)
    idx, off = _dev(idx_h), _dev(off_h)
    want = _bits(m.lookup(idx, off, batch=B))
    out, arg = m(idx, off, return_max_indices=True)
    assert out.requires_grad and not arg.requires_grad and np.array_equal(_bits(out), want)
    before = _bits(m.weights.data.clone())
    with pytest.raises(ValueError, match="fused .backward\\(\\) does not take pooling_mode=\"max\""):
        out.sum().backward()
    assert np.array_equal(_bits(m.weights.data), before)
    with torch.no_grad():
        plain = m(idx, off)
    assert not plain.requires_grad and np.array_equal(_bits(plain), want)


@pytest.mark.parametrize("odt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("dname", ["f32", "bf16"])
def test_output_dtype_is_the_fp32_result_rounded_once(dname, odt):
    rng = np.random.default_rng(8)
    rows, D, B = (50, 300), 8, 23
    pads = (11, None)
    w = [_special_rows(rng, r, D) * np.float32(1.0009765625) if dname == "f32" else _special_rows(rng, r, D) for r in rows]      # fp32: values that do round
    m, tabs = _model(rows, D, dname, pads, weights=w, output_dtype=odt)
    idx_h, off_h = _request(rng, rows, B, pads)
    want_v, want_a = M.forward(tabs, idx_h, off_h, B, pads)
    out, arg = m.lookup(_dev(idx_h), _dev(off_h), batch=B, return_max_indices=True)
    assert out.dtype == odt
    oname = "bf16" if odt == torch.bfloat16 else "fp16"
    want16 = _join(M.round_out(want_v, oname), "bd")
    if dname == "f32":                                     # (the rounding is not a no-op on these values)
        fin = np.isfinite(want_v[1])
        assert (O.widen(want16[:, D:], oname)[fin] != want_v[1][fin]).any()
    assert np.isnan(want_v[0][0, 0]) and O.is_nan16(want16[0, 0], oname)
    assert O.same_bits(_bits(out).view(np.uint16), want16, oname) and np.array_equal(arg.cpu().numpy(), _join(want_a, "bd"))


def test_bounds_check_ignore_repairs_the_request_first():
    rng = np.random.default_rng(9)
    rows, D, B = (50, 300), 8, 23
    pads = (0, None)                                       # a bad index repaired to 0 is padding in table 0
    m, tabs = _model(rows, D, "f32", pads, bounds_check_mode="ignore")
    idx_h, off_h = _request(rng, rows, B, pads)
    bad = rng.choice(idx_h.size, size=9, replace=False)
    broken = idx_h.copy()
    broken[bad] = rng.choice([-3, 10 ** 6], size=9)
    idx, off = _dev(broken), _dev(off_h)
    out, arg = m.lookup(idx, off, batch=B, return_max_indices=True)
    repaired = idx.cpu().numpy()
    assert (broken != repaired).sum() == 9 and (repaired[bad] == 0).all()
    want_v, want_a = M.forward(tabs, repaired, off_h, B, pads)
    assert np.array_equal(_bits(out), _bits(_join(want_v, "bd"))) and np.array_equal(arg.cpu().numpy(), _join(want_a, "bd"))


def _expansion_cases():
    """(gdt, layout, D, idt) and ids.  ``launch_max_grad`` gives a bag G = group_lanes(D, 4) lanes, 4 columns a lane and round:
    D = 8, 64, 128, 132 and 512 are G = 8, 16, 32, 64 and 64 with two rounds (256 / G = 32 .. 4 bags per workgroup).  The first six
    are the cases this test always had, under the ids it always had; then every width with fp32 and with a 16-bit gradient, both index
    types at D = 8 and at D = 512."""
    f32, bf16, f16, i32, i64 = torch.float32, torch.bfloat16, torch.float16, torch.int32, torch.int64
    cases = [(g, lay, 8, i64) for lay in ("bd", "tbd") for g in (f32, bf16, f16)]
    ids = [f"{lay}-gdt{k}" for lay in ("bd", "tbd") for k in range(3)]
    more = [(f32, "bd", 8, i32), (bf16, "tbd", 8, i32), (f32, "bd", 64, i64), (bf16, "tbd", 64, i32), (f32, "tbd", 128, i32), (f16, "bd", 128, i64),
            (f32, "bd", 132, i64), (bf16, "tbd", 132, i32), (f32, "bd", 512, i64), (f32, "tbd", 512, i32), (f16, "bd", 512, i32), (bf16, "tbd", 512, i64)]
    name = {f32: "f32", bf16: "bf16", f16: "f16", i32: "i32", i64: "i64"}
    assert {(D, g == f32) for g, _, D, _ in cases + more} == {(D, f) for D in (8, 64, 128, 132, 512) for f in (False, True)}
    assert {(D, i) for _, _, D, i in cases + more} >= {(D, i) for D in (8, 512) for i in (i32, i64)}
    return cases + more, ids + [f"{lay}-{name[g]}-D{D}-{name[i]}" for g, lay, D, i in more]


@pytest.mark.parametrize("gdt,layout,D,idt", _expansion_cases()[0], ids=_expansion_cases()[1])
def test_the_expansion_kernel_is_the_rules_g_seq(gdt, layout, D, idt):
    from param_amd import embedding_bag as EB
    from tests.plan_sweep import group_lanes

    rng = np.random.default_rng(10)
    rows, B = (50, 17, 300), 23
    pads = (11, None, 299)
    assert (group_lanes(D, 4), D > 256) == {8: (8, False), 64: (16, False), 128: (32, False), 132: (64, False), 512: (64, True)}[D]
    out16 = None if gdt == torch.float32 else gdt
    m, tabs = _model(rows, D, "f32", pads, layout, output_dtype=out16)
    idx_h, off_h = _request(rng, rows, B, pads)
    _, want_a = M.forward(tabs, idx_h, off_h, B, pads)
    g = torch.randn(m._tables().out_desc(B)[2], device=DEV).to(gdt)
    g[0].fill_(-0.0)
    grads = _split(g.float(), [D] * 3, layout)
    arg = _dev(_join(want_a, layout))
    idx, off = _dev(idx_h, idt), _dev(off_h, idt)
    # a bag that holds its arg-max row at two positions (table 1, bag 6: [8, 8]), inside both slices, with a gradient that is not zero
    t2, b2 = 1, 6
    j1 = int(off_h[t2 * B + b2])
    assert off_h[t2 * B + b2 + 1] == j1 + 2 and idx_h[j1] == idx_h[j1 + 1] and (want_a[t2][b2] == idx_h[j1]).all() and (grads[t2][b2] != 0).all()
    for b0, nb in ((0, B), (5, 11)):
        want, written = M.expand(idx_h, off_h, B, grads, want_a, b0, nb)
        got = EB._max_expand(m._tables(), g, arg, idx, off, B, b0, nb, out16).cpu().numpy()
        assert got.shape == (idx_h.size, D) and written.any() and np.array_equal(_bits(got[written]), _bits(want[written])), (b0, nb)
        assert b0 <= b2 < b0 + nb and np.array_equal(_bits(got[j1]), _bits(grads[t2][b2])) and (_bits(got[j1 + 1]) == 0).all(), (b0, nb)


@pytest.mark.parametrize("D", [8, 132])
@pytest.mark.parametrize("padded", [False, True])
def test_the_expansion_of_a_bag_of_thousands_of_positions(padded, D):
    """one lane group walks 5000 positions (the request of ``test_a_bag_beyond_the_index_tile_takes_the_unstaged_path``); the gradient
    with the saved ``max_indices`` and with the recomputed ones"""
    from param_amd import embedding_bag as EB

    rng = np.random.default_rng(15)
    rows, B = (300,), 3
    pads = (7,) if padded else (None,)
    m, tabs = _model(rows, D, "f32", pads, seed=15)
    long_bag = rng.integers(0, 300, size=5000)
    if padded:
        long_bag[rng.random(5000) < 0.3] = 7
        long_bag[0] = 7
    idx_h = np.concatenate([[8, 9], long_bag, [10]]).astype(np.int64)
    off_h = np.array([0, 2, 5002], dtype=np.int64)
    idx, off = _dev(idx_h), _dev(off_h)
    want_v, want_a = M.forward(tabs, idx_h, off_h, B, pads)
    out, arg = m.lookup(idx, off, batch=B, return_max_indices=True)
    assert np.array_equal(arg.cpu().numpy(), want_a[0])
    g = torch.randn(B, D, device=DEV)
    want, written = M.expand(idx_h, off_h, B, [g.cpu().numpy()], want_a)
    assert written.all() and len(np.unique(want_a[0][1])) > 1 and (np.bincount(long_bag)[want_a[0][1]] > 1).any()      # rows met again later
    got = EB._max_expand(m._tables(), g, arg, idx, off, B)
    assert np.array_equal(_bits(got), _bits(want))
    assert (_bits(got[2:5002]) != 0).any(axis=1).sum() == len(np.unique(want_a[0][1]))      # one position per winning row, +0.0 elsewhere
    saved = m.dense_grad(g, idx, off, batch=B, max_indices=arg)
    again = m.dense_grad(g, idx, off, batch=B, max_indices=None)
    assert np.array_equal(_bits(saved[0]), _bits(again[0])) and saved[0].any()
    if padded:
        assert not saved[0][7].any()


@pytest.mark.parametrize("dname,D", [("f32", 64), ("f32", 132), ("f32", 512), ("bf16", 256)])
def test_dense_grad_is_the_rule_at_every_width(dname, D):
    """``dense_grad`` and ``scatter_add_`` end to end where the expansion runs 16, 32 and 64 lanes a bag and two rounds a lane"""
    rng = np.random.default_rng(14)
    rows, B = (50, 17, 300), 330
    pads = (11, None, 299)
    m, tabs = _model(rows, D, dname, pads, seed=14)
    s, _ = _model(rows, D, dname, pads, mode="sum", seed=14)
    same = lambda: all(np.array_equal(_bits(m.table(t)), _bits(s.table(t))) for t in range(3))      # noqa: E731
    assert same()
    idx_h, off_h = _hot_request(rng, rows, B, pads, 0)
    for t in range(3):
        assert np.bincount(idx_h[off_h[t * B]:off_h[(t + 1) * B] if t < 2 else idx_h.size]).max() <= 256      # (the sorted apply's exact-run limit)
    idx, off = _dev(idx_h), _dev(off_h)
    out, arg = m.lookup(idx, off, batch=B, return_max_indices=True)
    want_v, want_a = M.forward(tabs, idx_h, off_h, B, pads)
    assert np.array_equal(arg.cpu().numpy(), _join(want_a, "bd"))
    g = torch.randn(B, 3 * D, device=DEV)
    grads = _split(g, [D] * 3, "bd")
    want = M.dense_grad(rows, [D] * 3, grads, want_a)
    for mi in (arg, None):
        got = m.dense_grad(g, idx, off, batch=B, max_indices=mi)
        for t in range(3):
            assert got[t].dtype == torch.float32 and np.array_equal(_bits(got[t]), _bits(want[t])), (t, mi is None)
    assert all(w.any() for w in want)
    g_seq, written = M.expand(idx_h, off_h, B, grads, want_a)
    assert written.all()
    m.scatter_add_(g, idx, off, alpha=-0.5, batch=B, max_indices=arg)
    s.sequence_scatter_add_(_dev(g_seq), idx, off, alpha=-0.5, batch=B)
    assert same() and not np.array_equal(_bits(m.table(2).float()), _bits(tabs[2]))
    for t, p in enumerate(pads):
        if p is not None:
            assert np.array_equal(_bits(m.table(t)[p].float()), _bits(tabs[t][p]))


def _hot_request(rng, rows, B, pads, hot):
    """``_request`` with row 9 of table 0 in ``hot`` more bags (appended to bags of the cycle)"""
    idx_h, off_h = _request(rng, rows, B, pads)
    end = list(off_h[1:]) + [idx_h.size]
    bags = [list(idx_h[off_h[g]:end[g]]) for g in range(len(off_h))]
    for b in range(9, 9 + hot):
        bags[b] = bags[b] + [9]
    off = np.cumsum([0] + [len(b) for b in bags[:-1]]).astype(np.int64)
    return np.array([r for b in bags for r in b], dtype=np.int64), off


@pytest.mark.parametrize("hot", [0, 300])
def test_dense_grad_and_scatter_add_are_the_sequence_calls_on_the_expanded_gradient(hot):
    rng = np.random.default_rng(11)
    rows, D, B = (50, 17, 300), 8, 330
    pads = (11, None, 299)
    m, tabs = _model(rows, D, "f32", pads, seed=11)
    s, _ = _model(rows, D, "f32", pads, mode="sum", seed=11)
    same = lambda: all(np.array_equal(_bits(m.table(t)), _bits(s.table(t))) for t in range(3))      # noqa: E731
    assert same()
    idx_h, off_h = _hot_request(rng, rows, B, pads, hot)
    counts = np.bincount(idx_h[:off_h[B]], minlength=rows[0])
    assert (counts[9] > 256) == (hot > 0) and (hot > 0 or np.bincount(idx_h).max() <= 256)
    idx, off = _dev(idx_h), _dev(off_h)
    out, arg = m.lookup(idx, off, batch=B, return_max_indices=True)
    want_v, want_a = M.forward(tabs, idx_h, off_h, B, pads)
    assert np.array_equal(arg.cpu().numpy(), _join(want_a, "bd"))
    g = torch.randn(B, 3 * D, device=DEV)
    grads = _split(g, [D] * 3, "bd")
    g_seq, written = M.expand(idx_h, off_h, B, grads, want_a)
    assert written.all()
    # dense_grad: with the saved max_indices, with None (recomputed), and the sequence call on the numpy-expanded gradient
    ref = s.sequence_dense_grad(_dev(g_seq), idx, off, batch=B)
    for mi in (arg, None):
        got = m.dense_grad(g, idx, off, batch=B, max_indices=mi)
        for t in range(3):
            assert np.array_equal(_bits(got[t]), _bits(ref[t])), (t, mi is None)
    if not hot:      # every row has at most 256 lookups: the rule's sequential sum, bit for bit
        for t, w in enumerate(M.dense_grad(rows, [D] * 3, grads, want_a)):
            assert np.array_equal(_bits(got[t]), _bits(w)), t
    # scatter_add_ in place, padding rows untouched
    m.scatter_add_(g, idx, off, alpha=-0.5, batch=B, max_indices=arg)
    s.sequence_scatter_add_(_dev(g_seq), idx, off, alpha=-0.5, batch=B)
    assert same() and not np.array_equal(_bits(m.table(2)), _bits(tabs[2]))
    for t, p in enumerate(pads):
        if p is not None:
            assert np.array_equal(_bits(m.table(t)[p]), _bits(tabs[t][p]))


@pytest.mark.parametrize("form", ["1d", "2d"])
@pytest.mark.parametrize("dname", ["f32", "bf16"])
@pytest.mark.parametrize("pname", ["pad", "nopad"])
def test_single_table_autograd_is_torchs_recorded_gradient(pname, dname, form):
    import param_amd

    pad = C.pad() if pname == "pad" else None
    t_out, t_arg, t_dw = C.torch_result(form, pname, dname)
    idx_h, off_h, B, i2 = C.request(form)
    m = param_amd.MaxEmbeddingBagMI355(C.ROWS, C.DIM, dtype=TDT[dname], _weight=C.table(dname).to(DEV), padding_idx=pad)
    out = m(_dev(idx_h), _dev(off_h)) if i2 is None else m(_dev(i2))
    assert out.dtype == torch.float32 and np.array_equal(_bits(out), _bits(t_out))
    out.backward(_dev(C.grad(form, dname)))
    assert m.weight.grad.dtype == TDT[dname] and np.array_equal(_bits(m.weight.grad.float()), _bits(t_dw))
    with torch.no_grad():
        assert np.array_equal(_bits(m(_dev(idx_h), _dev(off_h))), _bits(t_out))
    # max_indices: torch's wherever the bag has a kept lookup and the column no tie between different rows
    bm, tabs = _model((C.ROWS,), C.DIM, dname, (pad,), weights=[C.table32(dname)])
    _, arg = bm.lookup(_dev(idx_h), _dev(off_h), batch=B, return_max_indices=True)
    want_v, want_a = M.forward(tabs, idx_h, off_h, B, [pad])
    arg = arg.cpu().numpy()
    assert np.array_equal(arg, want_a[0])
    kept = arg >= 0
    assert kept.any() and np.array_equal(arg[kept], t_arg[kept])


def test_1100_tables_forward_and_the_gradient_through_the_table_range_split():
    rng = np.random.default_rng(12)
    T, D, B = 1100, 8, 4
    rows = [20] * T
    pads = [None] * T
    w = [(rng.integers(-80, 81, size=(20, D)) / 8.0).astype(np.float32) for _ in range(T)]
    m, tabs = _model(rows, D, "f32", pads, weights=w)
    lens = rng.integers(0, 4, size=T * B)
    off_h = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    idx_h = rng.integers(0, 20, size=int(lens.sum())).astype(np.int64)
    idx, off = _dev(idx_h), _dev(off_h)
    want_v, want_a = M.forward(tabs, idx_h, off_h, B, pads)
    out, arg = m.lookup(idx, off, batch=B, return_max_indices=True)
    assert np.array_equal(_bits(out), _bits(_join(want_v, "bd"))) and np.array_equal(arg.cpu().numpy(), _join(want_a, "bd"))
    g = torch.randn(B, T * D, device=DEV)
    got = m.dense_grad(g, idx, off, batch=B, max_indices=arg)
    want = M.dense_grad(rows, [D] * T, _split(g, [D] * T, "bd"), want_a)
    assert np.array_equal(_bits(torch.stack(got)), _bits(np.stack(want)))
