"""The un-pooled lookup on the GPU (``pytest -m gpu``): ``pm_embedding_gather`` through ctypes, ``EmbeddingMI355`` and
``BatchedEmbeddingBagMI355.lookup_sequence``, every case held to the numpy rule (tests/embedding_rules.py) bit for bit -- shapes at
which a tile of 256 positions straddles table borders, a table owns no lookup, the column loop runs (fp32 D = 260) and the borders are
searched in global memory (T = 1100); every (table dtype, output dtype) pair; special values; autograd against the rule with a row hot
enough to leave the sorted apply's exact run; and that modules which exist today never reach the new entry point."""
import ctypes

import numpy as np
import pytest
import torch

from tests import embedding_rules as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
ROWS = (50, 7, 1000)
PAIRS = [(a, b) for a in E.KINDS for b in E.KINDS]
SENT = {"f32": 0x7b7b7b7b, "bf16": 0x7b7b, "f16": 0x7b7b}
EXACT_RUN = 256      # kExactRun of the sorted apply: a row looked up more often is summed as ordered chunk partials


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    import param_amd

    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    param_amd.load_library()


def _dev_bits(bits, kind):
    """a device tensor of ``kind`` holding exactly these bits"""
    b = np.ascontiguousarray(bits, dtype=E.BITS[kind])
    t = torch.from_numpy(b.view(np.int32 if kind == "f32" else np.int16).copy()).to(DEV)
    return t.view(TDT[kind])


def _bits(t):
    t = t.detach().contiguous()
    if t.element_size() == 2:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _tables(rng, rows, dims, kind):
    """per-table bits of ``kind``: ordinary values"""
    return [E.to_bits(rng.standard_normal((r, d)).astype(np.float32), kind) for r, d in zip(rows, dims)]


def _request(rng, rows, N, B, dtype=np.int64):
    """N lookups over the three tables: the first third to table 0, NONE to table 1, the rest to table 2 (a single lookup goes to
    table 2: tables 0 and 1 own none), ragged bags inside a table, some empty -> (indices, offsets [T * B])"""
    counts = [N // 3, 0, N - N // 3]
    idx, off, at = [], [], 0
    for r, c in zip(rows, counts):
        cuts = np.sort(rng.integers(0, c + 1, B - 1)) if c else np.zeros(B - 1, dtype=np.int64)
        off += [at] + [at + int(x) for x in cuts]
        idx.append(rng.integers(0, r, c))
        at += c
    return np.concatenate(idx).astype(dtype), np.asarray(off, dtype=dtype)


def _call(tabs_dev, kin, kout, idx, off, B, out, stride, bag_begin=0, bag_count=None):
    """pm_embedding_gather through ctypes on device tensors; returns the library's code"""
    from param_amd import _lib

    T = len(tabs_dev)
    dims = [int(t.shape[1]) for t in tabs_dev]
    keep = (torch.tensor([t.data_ptr() for t in tabs_dev], dtype=torch.int64, device=DEV),
            torch.tensor([int(t.shape[0]) for t in tabs_dev], dtype=torch.int64, device=DEV),
            torch.tensor(dims, dtype=torch.int32, device=DEV), torch.zeros(T, dtype=torch.int64, device=DEV))
    op = _lib.pm_embbag_batch()
    op.num_tables, op.weight_dtype, op.index_dtype = T, {"f32": 0, "bf16": 1, "f16": 2}[kin], 11 if idx.dtype == torch.int64 else 10
    op.max_dim, op.min_dim = max(dims), min(dims)
    op.batch, op.num_indices, op.bag_begin, op.bag_count = B, idx.numel(), bag_begin, B - bag_begin if bag_count is None else bag_count
    op.tables, op.rows, op.dims, op.out_offsets = (k.data_ptr() for k in keep)
    op.out_stride = 4
    op.indices, op.offsets = idx.data_ptr(), off.data_ptr()
    rc = _lib.load().pm_embedding_gather(ctypes.byref(op), {"f32": 0, "bf16": 1, "f16": 2}[kout], out.data_ptr(), stride,
                                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _check(tabs, kin, kout, idx_h, off_h, B, pad_cols=4, bag_begin=0, bag_count=None):
    """the call on a sentinel canvas of ``max_dim + pad_cols`` columns equals the rule on that canvas, bit for bit"""
    stride = max(t.shape[1] for t in tabs) + pad_cols
    canvas = np.full((idx_h.size, stride), SENT[kout], dtype=E.BITS[kout])
    out = _dev_bits(canvas, kout)
    tdev = [_dev_bits(t, kin) for t in tabs]
    idx, off = torch.from_numpy(idx_h).to(DEV), torch.from_numpy(off_h).to(DEV)
    assert _call(tdev, kin, kout, idx, off, B, out, stride, bag_begin, bag_count) == 0
    want = E.forward(tabs, kin, kout, idx_h, off_h, B, canvas, bag_begin, bag_count)
    got = _bits(out)
    assert E.same(got, want, kin, kout), (kin, kout, idx_h.size, [t.shape for t in tabs], np.argwhere(got != want)[:3])
    return want


# ---- 1. through ctypes ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kin,kout", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_gather_equals_the_rule(kin, kout):
    """rows (50, 7, 1000), table 1 owns no lookup, a tile straddles the border between tables 0 and 2; N = 1 / 255 / 257 / ~3000;
    int32 and int64; out_row_stride > D with the gap columns keeping the sentinel"""
    rng = np.random.default_rng(40 + 3 * E.KINDS.index(kin) + E.KINDS.index(kout))
    for D in ((4, 8, 64, 128, 260) if kin == "f32" else (8, 64, 512)):
        tabs = _tables(rng, ROWS, [D] * 3, kin)
        for k, N in enumerate((1, 255, 257, 3001)):
            idx_h, off_h = _request(rng, ROWS, N, 5, np.int32 if (k + D // 4) % 2 else np.int64)
            want = _check(tabs, kin, kout, idx_h, off_h, 5)
            assert (want[:, D:] == SENT[kout]).all() and not (want[:, :D] == SENT[kout]).all(axis=1).any()


@pytest.mark.parametrize("kin,kout", [("f32", "f32"), ("bf16", "bf16"), ("f16", "f32"), ("f32", "bf16")])
def test_gather_bag_slice_keeps_the_rows_outside(kin, kout):
    rng = np.random.default_rng(50)
    tabs = _tables(rng, ROWS, [64] * 3, kin)
    idx_h, off_h = _request(rng, ROWS, 700, 6)
    for b0, nb in ((1, 3), (0, 2), (5, 1), (2, 0)):
        want = _check(tabs, kin, kout, idx_h, off_h, 6, 0, b0, nb)
        tab, inside = E.in_slice(off_h, 3, 6, idx_h.size, b0, nb)
        assert (want[~inside] == SENT[kout]).all() and (nb == 0 or inside.any()) and not inside.all()


@pytest.mark.parametrize("kin,kout", [("f32", "f32"), ("bf16", "f32"), ("f16", "f16"), ("f32", "f16")])
def test_gather_mixed_dims(kin, kout):
    """dims (8, 64, 128): row j has dims[t] columns written, the rest of the output row keeps the sentinel"""
    rng = np.random.default_rng(51)
    dims = (8, 64, 128)
    tabs = _tables(rng, ROWS, dims, kin)
    rows = (50, 7, 1000)
    counts = [200, 57, 300]
    idx_h = np.concatenate([rng.integers(0, r, c) for r, c in zip(rows, counts)]).astype(np.int64)
    off_h = np.array([0, 120, 200, 230, 257, 400], dtype=np.int64)               # T = 3, B = 2
    want = _check(tabs, kin, kout, idx_h, off_h, 2, 0)
    tab = E.P.table_of(off_h, 3, 2, idx_h.size)
    for t, d in enumerate(dims):
        assert (want[tab == t][:, d:] == SENT[kout]).all()


def _special_bits(kind):
    if kind == "f32":
        f = np.array([-0.0, np.inf, -np.inf, 65504.0, 65520.0, 1.0e5, -7.0e4, 3.4e38, -3.4e38, 1.00390625, 6.0e-8, -2.0e-8, 1e-40], np.float32)
        return np.concatenate([f.view(np.uint32), np.array([0x00000001, 0x807fffff, 0x7fc00001, 0x7f800001, 0xffc12345, 0x7fffffff], np.uint32)])
    if kind == "bf16":
        return np.array([0x8000, 0x7f80, 0xff80, 0x0001, 0x807f, 0x0080, 0x4780, 0xc7ff, 0x7f7f, 0xff7f, 0x3f81, 0x3301, 0x7fc1, 0x7f81, 0xffff],
                        np.uint16)
    return np.array([0x8000, 0x7c00, 0xfc00, 0x0001, 0x83ff, 0x0400, 0x7bff, 0xfbff, 0x3c01, 0x7e01, 0x7c01, 0xfe00, 0xffff], np.uint16)


@pytest.mark.parametrize("kin,kout", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_special_values(kin, kout):
    """-0.0, +-Inf, subnormals, values that overflow fp16 / bf16 and NaNs with distinct payloads: a same-dtype output keeps every bit
    (payloads included); a converted output follows tests/out16_rules.py"""
    rng = np.random.default_rng(52)
    sp = _special_bits(kin)
    D = 16
    tab = E.to_bits(rng.standard_normal((2 * len(sp) + 3, D)).astype(np.float32), kin)
    tab[:len(sp)] = sp[:, None]
    tab[len(sp):2 * len(sp)] = np.stack([np.roll(np.resize(sp, D), k) for k in range(len(sp))])
    idx_h = np.concatenate([np.arange(tab.shape[0]), rng.integers(0, tab.shape[0], 300)]).astype(np.int64)
    want = _check([tab], kin, kout, idx_h, np.zeros(1, np.int64), 1)
    if kin == kout:
        assert np.array_equal(want[:tab.shape[0], :D], tab)                       # the rule itself is the identity here
        assert E.is_nan(want, kout).any() and len(set(want[E.is_nan(want, kout)].tolist())) >= 3


# ---- 2. EmbeddingMI355 -----------------------------------------------------------------------------------------------------------------

def _module(rows, D, kind="f32", seed=0, **kw):
    from param_amd import EmbeddingMI355

    w = np.random.default_rng(seed).standard_normal((rows, D)).astype(np.float32)
    return EmbeddingMI355.from_pretrained(_dev_bits(E.to_bits(w, kind), kind), freeze=False, **kw)


@pytest.mark.parametrize("kind,out", [("f32", None), ("bf16", None), ("bf16", "bf16"), ("f16", "fp16"), ("f32", "fp16"), ("f16", "bf16")])
def test_module_forward_shapes_and_dtypes(kind, out):
    m = _module(37, 24 if kind != "f32" else 12, kind, seed=1, output_dtype=out)
    kout = {None: "f32", "bf16": "bf16", "fp16": "f16"}[out]
    D = m.embedding_dim
    wb = _bits(m.weight)
    rng = np.random.default_rng(2)
    for shape, idt in (((29,), torch.int64), ((5, 7), torch.int32), ((2, 3, 4), torch.int64), ((0,), torch.int64), ((3, 0), torch.int32)):
        idx = torch.from_numpy(rng.integers(0, 37, shape)).to(DEV, dtype=idt)
        with torch.no_grad():
            got = m(idx)
        assert tuple(got.shape) == (*shape, D) and got.dtype == TDT[kout] and got.is_contiguous()
        want = E.conv(wb[idx.cpu().numpy().reshape(-1)], kind, kout).reshape(*shape, D)
        assert E.same(_bits(got).reshape(*shape, D), want, kind, kout)
    assert m(idx[:0]).requires_grad                                               # the empty lookup stays in the graph


def _hot_request(rng, rows, shape, hot_row, hot_n):
    idx = rng.integers(0, rows, int(np.prod(shape)))
    idx[rng.permutation(idx.size)[:hot_n]] = hot_row
    return idx.reshape(shape).astype(np.int64)


def _check_grad_rows(got32, idx_h, g32, rows, pad, hot_row):
    """every row but the hot one bit for bit against the rule; the hot row (past the exact run: ordered chunk partials) within 1e-5 of
    sum |contribution| of an fp64 sum -- the bar tests/test_gpu_parity.py holds hot rows to"""
    want = E.dense_grad(rows, idx_h, g32, pad)
    cold = np.arange(rows) != hot_row
    assert np.array_equal(got32[cold].view(np.uint32), want[cold].view(np.uint32))
    sel = idx_h.reshape(-1) == hot_row
    assert sel.sum() > EXACT_RUN
    g = g32.reshape(sel.size, -1).astype(np.float64)[sel]
    assert (np.abs(got32[hot_row].astype(np.float64) - g.sum(axis=0)) <= 1e-5 * np.abs(g).sum(axis=0) + 1e-30).all()


def test_module_dense_autograd_equals_the_rule():
    rows, D, pad, hot = 60, 8, 9, 5
    rng = np.random.default_rng(3)
    m = _module(rows, D, seed=3, padding_idx=pad)
    idx_h = _hot_request(rng, rows, (35, 24), hot, 300)
    assert (idx_h == pad).any()
    g_h = rng.standard_normal((35, 24, D)).astype(np.float32)
    idx, g = torch.from_numpy(idx_h).to(DEV), torch.from_numpy(g_h).to(DEV)
    m(idx).backward(g)
    got = m.weight.grad.cpu().numpy()
    assert m.weight.grad.dtype == torch.float32 and not got[pad].any()
    _check_grad_rows(got, idx_h, g_h, rows, pad, hot)
    # a second backward accumulates into .grad (torch's own add)
    g2_h = rng.standard_normal((35, 24, D)).astype(np.float32)
    m(idx).backward(torch.from_numpy(g2_h).to(DEV))
    cold = np.arange(rows) != hot
    want = E.dense_grad(rows, idx_h, g_h, pad) + E.dense_grad(rows, idx_h, g2_h, pad)
    assert np.array_equal(m.weight.grad.cpu().numpy()[cold].view(np.uint32), want[cold].view(np.uint32))


def test_module_sparse_autograd_equals_the_rule():
    rows, D, pad, hot = 60, 8, 9, 5
    rng = np.random.default_rng(4)
    m = _module(rows, D, seed=4, padding_idx=pad, sparse=True)
    idx_h = _hot_request(rng, rows, (700,), hot, 300)
    g_h = rng.standard_normal((700, D)).astype(np.float32)
    m(torch.from_numpy(idx_h).to(DEV)).backward(torch.from_numpy(g_h).to(DEV))
    g = m.weight.grad
    assert g.is_sparse and g.is_coalesced() and tuple(g.shape) == (rows, D)
    r, v = E.sparse_grad(rows, idx_h, g_h, pad)
    assert np.array_equal(g._indices()[0].cpu().numpy(), r) and pad not in r
    dense = np.zeros((rows, D), np.float32)
    dense[r] = g._values().cpu().numpy()
    _check_grad_rows(dense, idx_h, g_h, rows, pad, hot)


def test_module_padding_row_comes_back_unchanged_and_gets_no_gradient():
    rows, D, pad = 20, 8, 6
    m = _module(rows, D, seed=5, padding_idx=pad)
    with torch.no_grad():
        m.weight[pad] = float("nan")
    idx = torch.tensor([[pad, 1, pad], [2, 3, pad]], device=DEV)
    out = m(idx)
    assert torch.isnan(out[idx == pad]).all() and not torch.isnan(out[idx != pad]).any()
    out.backward(torch.ones_like(out))
    gr = m.weight.grad.cpu().numpy()
    assert not gr[pad].any() and (gr[[1, 2, 3]] == 1.0).all()
    from param_amd import EmbeddingMI355
    assert not EmbeddingMI355(rows, D, padding_idx=pad, device=DEV).weight[pad].any()      # module-made weights: zero-filled


@pytest.mark.parametrize("kind,out", [("bf16", "bf16"), ("f32", "fp16")])
def test_module_16_bit_output_and_gradient(kind, out):
    """a gradient in the module's 16-bit output dtype is widened exactly, then summed as its fp32 values"""
    rows, D = 30, 16
    kout = {"bf16": "bf16", "fp16": "f16"}[out]
    rng = np.random.default_rng(6)
    m = _module(rows, D, kind, seed=6, output_dtype=out)
    idx_h = rng.integers(0, rows, (9, 11)).astype(np.int64)
    g16 = E.to_bits(rng.standard_normal((9, 11, D)).astype(np.float32), kout)
    y = m(torch.from_numpy(idx_h).to(DEV))
    assert y.dtype == TDT[kout]
    y.backward(_dev_bits(g16, kout))
    want = E.dense_grad(rows, idx_h, E.to_f32(g16, kout))
    assert m.weight.grad.dtype == TDT[kind]
    assert np.array_equal(_bits(m.weight.grad), E.to_bits(want, kind))


def test_module_bounds_check_modes():
    rows, D = 20, 8
    m = _module(rows, D, seed=7, bounds_check_mode="warning")
    idx = torch.tensor([3, rows + 5, 4, -1], device=DEV)
    with torch.no_grad():
        out = m(idx)
    assert idx.tolist() == [3, 0, 4, 0] and torch.equal(out, m.weight[idx])        # repaired in place to row 0
    rep = m.bounds_report()
    assert rep["bad_indices"] == 2 and rep["first_bad_index"] == 1 and rep["bad_offsets"] == 0
    f = _module(rows, D, seed=7, bounds_check_mode="fatal")
    bad = torch.tensor([[3, rows]], device=DEV)
    with pytest.raises(IndexError, match="1 out-of-range indices"):
        f(bad)
    assert bad.tolist() == [[3, rows]]
    n = _module(rows, D, seed=7)
    bad2 = torch.tensor([1, rows + 1], device=DEV)
    n.sanitize_(bad2)
    assert bad2.tolist() == [1, 0]


# ---- 3. lookup_sequence ------------------------------------------------------------------------------------------------------------

def _batched(rows, D, dtype=torch.float32, **kw):
    import param_amd

    return param_amd.BatchedEmbeddingBagMI355(list(rows), D, dtype=dtype, device=DEV, init="normal", seed=11, fused_update=False, **kw)


@pytest.mark.parametrize("kind,out", [("f32", None), ("bf16", "bf16"), ("f16", None), ("f32", "bf16")])
def test_lookup_sequence_equals_per_table_gathers(kind, out):
    kout = {None: "f32", "bf16": "bf16"}[out]
    rng = np.random.default_rng(8)
    m = _batched(ROWS, 64, TDT[kind], output_dtype=out, padding_idx=[0, None, 3])      # (padding does not affect the un-pooled forward)
    idx_h, off_h = _request(rng, ROWS, 900, 7)
    idx, off = torch.from_numpy(idx_h).to(DEV), torch.from_numpy(off_h).to(DEV)
    tabs = [_bits(m.table(t)) for t in range(3)]
    got = m.lookup_sequence(idx, off, batch=7)
    assert tuple(got.shape) == (900, 64) and got.dtype == TDT[kout]
    zero = np.zeros((900, 64), dtype=E.BITS[kout])
    assert E.same(_bits(got), E.forward(tabs, kind, kout, idx_h, off_h, 7, zero), kind, kout)
    # out= and a batch slice: rows outside keep what out held; a tensor the method allocates holds zeros there
    canvas = np.full((900, 64), SENT[kout], dtype=E.BITS[kout])
    out_t = _dev_bits(canvas, kout)
    assert m.lookup_sequence(idx, off, batch=7, out=out_t, bag_begin=2, bag_count=3) is out_t
    assert E.same(_bits(out_t), E.forward(tabs, kind, kout, idx_h, off_h, 7, canvas, 2, 3), kind, kout)
    fresh = m.lookup_sequence(idx, off, batch=7, bag_begin=2, bag_count=3)
    assert E.same(_bits(fresh), E.forward(tabs, kind, kout, idx_h, off_h, 7, zero, 2, 3), kind, kout)


def test_lookup_sequence_1100_tables():
    """more tables than the LDS copy of the borders holds: every position searches them in global memory"""
    T, B, D = 1100, 2, 8
    rng = np.random.default_rng(9)
    rows = [16] * T
    m = _batched(rows, D)
    lens = rng.integers(0, 4, T * B)
    lens[B * 7:B * 9] = 0                                                          # two tables without lookups
    off_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx_h = rng.integers(0, 16, int(off_h[-1])).astype(np.int64)
    got = m.lookup_sequence(torch.from_numpy(idx_h).to(DEV), torch.from_numpy(off_h).to(DEV), batch=B)
    tab = np.repeat(np.arange(T), np.add.reduceat(lens, np.arange(0, T * B, B)))
    want = torch.stack([m.table(t) for t in range(T)]).cpu().numpy()[tab, idx_h]
    assert np.array_equal(_bits(got), want.view(np.uint32))


def test_gather_equals_the_bag_of_one_lookup():
    """on tables without -0.0 the fp32 gather is the existing pooled ``lookup`` of the request "every lookup is a bag", bit for bit"""
    T, n, D = 3, 211, 128
    rng = np.random.default_rng(10)
    m = _batched(ROWS, D)
    assert not (torch.signbit(m.weights.data) & (m.weights.data == 0)).any()
    idx = torch.from_numpy(np.concatenate([rng.integers(0, r, n) for r in ROWS])).to(DEV)
    off = torch.arange(T * n + 1, device=DEV)
    pooled = m.lookup(idx, off, batch=n)                                           # [n, T * D]
    seq = m.lookup_sequence(idx, off, batch=n)                                     # [T * n, D]
    assert torch.equal(seq.view(T, n, D).permute(1, 0, 2).reshape(n, T * D).view(torch.int32), pooled.view(torch.int32))


# ---- 4. nothing that exists reaches the new entry point ---------------------------------------------------------------------------

def test_existing_modules_never_call_the_gather(monkeypatch):
    import param_amd
    from param_amd import _lib

    real = _lib.load()
    seen = []

    class Raising:
        def __getattr__(self, name):
            if name == "pm_embedding_gather":
                raise AssertionError("pm_embedding_gather reached from a pooled module")
            return getattr(real, name)

    monkeypatch.setattr(_lib, "load", lambda: Raising())
    rng = np.random.default_rng(12)
    idx_h, off_h = _request(rng, ROWS, 300, 4)
    idx, off = torch.from_numpy(idx_h).to(DEV), torch.from_numpy(np.append(off_h, 300)).to(DEV)
    for mode in ("sum", "mean"):
        b = _batched(ROWS, 16, pooling_mode=mode)
        b.lookup(idx, off, batch=4)
        b(idx, off)
        e = param_amd.EmbeddingBagMI355(50, 16, mode=mode, device=DEV)
        e(idx[:100], off[:4]).sum().backward()

    class Counting:
        def __getattr__(self, name):
            if name == "pm_embedding_gather":
                seen.append(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "load", lambda: Counting())
    _batched(ROWS, 16).lookup_sequence(idx, off, batch=4)
    param_amd.EmbeddingMI355(50, 16, device=DEV)(idx[:100])
    assert len(seen) == 2
