"""The coalesced sparse gradient (ABI v8) on a real MI355X: ``BatchedEmbeddingBagMI355.sparse_grad`` and
``EmbeddingBagMI355(sparse=True)``.

Bars:
  * against the non-fused sorted backward (``_sort_indices`` + ``_bwd(presorted=True)``, alpha = 1, into zeroed fp32 tables) read at
    the returned rows: bit for bit, for any run length (the same apply, relabelled to a compact destination);
  * against the sequential C oracle and the dense gradient: bit for bit for rows looked up at most 256 times, else within 1e-5 of
    the sum of |contributions| (fp64);
  * against torch's CPU ``EmbeddingBag(sparse=True)`` + ``coalesce()``: the same rows, values to fp32 summation tolerance.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EXACT_RUN = 256  # kExactRun in param_amd/csrc/bwd_sorted_apply.h


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    import param_amd

    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    param_amd.load_library()  # raises loudly if libparam_amd.so is missing: no fallback
    yield


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _hits(idx, rows):
    return np.bincount(np.asarray(idx, dtype=np.int64), minlength=rows)


# ----------------------------------------------------------------------------- 1. goldens through EmbeddingBagMI355(sparse=True)
@pytest.mark.parametrize("wdtype", [torch.float32, torch.bfloat16, torch.float16])
def test_sparse_module_goldens(cases, coracle, wdtype):
    from param_amd import EmbeddingBagMI355

    data, meta = cases
    for name in [n for n, m in meta.items() if "tables" not in m]:
        W, idx, off, g = data[f"{name}.W"], data[f"{name}.idx"], data[f"{name}.off"], data[f"{name}.grad"]
        psw = data[f"{name}.psw"] if f"{name}.psw" in data.files else None
        R, D = W.shape
        if wdtype != torch.float32 and D % 8:
            continue
        ms = EmbeddingBagMI355(R, D, sparse=True, _weight=_t(W, wdtype))
        md = EmbeddingBagMI355(R, D, _weight=_t(W, wdtype))
        for m in (ms, md):
            out = m(_t(idx), _t(off), None if psw is None else _t(psw))
            out.backward(_t(g))
        sg = ms.weight.grad
        assert sg.layout == torch.sparse_coo and sg.is_coalesced(), name
        assert sg.dtype == wdtype and tuple(sg.shape) == (R, D)
        rows = sg.indices()[0].cpu().numpy()
        assert np.array_equal(rows, np.unique(idx)), name
        assert rows.size < 2 or (np.diff(rows) > 0).all()
        dense = sg.to_dense()
        assert md.weight.grad.layout == torch.strided
        # the oracle's sequential fp32 sum, cast once to the weight dtype like the module's gradient
        ref32 = coracle.bwd_f32(np.zeros((R, D), np.float32), idx, off, g, psw)
        ref = torch.from_numpy(ref32).to(wdtype)
        hits = _hits(idx, R)
        short = torch.from_numpy(hits <= EXACT_RUN)
        got = dense.cpu()
        assert torch.equal(got[short], md.weight.grad.cpu()[short]), name
        assert torch.equal(got[short], ref[short]), name
        w = np.ones(len(idx)) if psw is None else psw.astype(np.float64)
        exp = np.zeros((R, D)); mag = np.zeros((R, D))
        bag = np.searchsorted(off, np.arange(len(idx)), side="right") - 1
        contrib = w[:, None] * g[bag].astype(np.float64)
        np.add.at(exp, idx, contrib); np.add.at(mag, idx, np.abs(contrib))
        if (~short).any():
            long_ = ~short.numpy()
            vals32 = ms.weight.grad.to_dense().float().cpu().numpy() if wdtype == torch.float32 else None
            if vals32 is not None:
                assert (np.abs(vals32[long_] - exp[long_]) <= 1e-5 * mag[long_] + 1e-30).all(), name
        # torch's CPU EmbeddingBag(sparse=True), coalesced: same rows, values to fp32 summation tolerance
        if wdtype == torch.float32:
            eb = torch.nn.EmbeddingBag(R, D, mode="sum", sparse=True, _weight=torch.from_numpy(W.copy()))
            eb(torch.from_numpy(idx), torch.from_numpy(off), None if psw is None else torch.from_numpy(psw)).backward(torch.from_numpy(g))
            tg = eb.weight.grad.coalesce()
            assert torch.equal(tg.indices()[0], sg.indices()[0].cpu()), name
            # (two fp32 sums of the same terms in different orders: |difference| <= hits * 2^-23 * sum |terms| per element)
            tol = (hits[rows] + 1)[:, None] * 2.0 ** -23 * mag[rows] + 1e-30
            assert (np.abs(sg.values().cpu().numpy().astype(np.float64) - tg.values().numpy()) <= tol).all(), name


# ----------------------------------------------------------------------------- 2. the batched matrix
def _request(rows, B, pooling, seed, empty_table=None, ragged=False):
    """TBE request (offsets [T*B+1], int64) on the host: fixed / per-table pooling, or ragged bags with empty ones"""
    rng = np.random.default_rng(seed)
    T = len(rows)
    lens = []
    for t in range(T):
        L = pooling if isinstance(pooling, int) else pooling[t]
        ln = rng.integers(0, 2 * L + 1, size=B) if ragged else np.full(B, L)
        if ragged:
            ln[rng.integers(0, B, size=max(1, B // 8))] = 0
        if t == empty_table:
            ln[:] = 0
        lens.append(ln)
    lens = np.concatenate(lens)
    off = np.zeros(T * B + 1, np.int64)
    off[1:] = np.cumsum(lens)
    idx = np.concatenate([rng.integers(0, rows[t], size=int(lens[t * B:(t + 1) * B].sum())) for t in range(T)]).astype(np.int64)
    return idx, off


def _table_grad(grad, t, ts, B):
    """[B, D_t] gradient rows of table t for the module's layout"""
    if ts.layout == "bd":
        return grad[:, ts.col0[t]:ts.col0[t] + ts.dims[t]]
    if ts.layout == "tbd":
        return grad[t]
    return grad[:, t].reshape(B, ts.dims[t])


def _nonfused_reference(m, grad, idx, off, psw, B, bag_begin, bag_count):
    """the sorted backward's own non-fused pair into a zeroed fp32 copy of the module's tables"""
    from param_amd import BatchedEmbeddingBagMI355, embedding_bag as eb

    ref = BatchedEmbeddingBagMI355(m.rows, m.dims, dtype=torch.float32, device=DEV, layout=m.layout, init=None,
                                   fused_update=False, block_bags=m.block_bags)
    ref.weights.data.zero_()
    ts = ref._tables()
    eb._sort_indices(ts, idx, off, B, psw, bag_begin, bag_count, phases=1)
    eb._bwd(ts, grad, idx, off, B, ts.d_ptrs, torch.float32, 1.0, psw, bag_begin, bag_count, presorted=True)
    return ref


CASES = {
    # name: (rows, dims, dtype, layout, index dtype, pooling, ragged, weighted, slice, empty table)
    "fp32_bd_fixed": ([3000, 500, 7000, 64], 64, torch.float32, "bd", torch.int64, 20, False, False, None, None),
    "bf16_bd_mixed": ([4000, 300, 2000, 9000], [16, 32, 64, 128], torch.bfloat16, "bd", torch.int64, [1, 3, 20, 7], False, False,
                      None, None),
    "f16_tbd_i32": ([2000, 800, 100], 32, torch.float16, "tbd", torch.int32, 12, False, False, None, None),
    "fp32_blocked": ([1500, 700, 90, 4000], 64, torch.float32, "blocked", torch.int64, 10, False, False, None, None),
    "fp32_mixed_ragged_weighted": ([600, 5000, 40, 3000, 800], [16, 128, 32, 64, 16], torch.float32, "bd", torch.int32, 6, True, True,
                                   None, 2),
    "bf16_slice_weighted": ([2500, 900, 60], 128, torch.bfloat16, "bd", torch.int64, [4, 9, 30], False, True, (37, 150), None),
    "fp32_tbd_ragged_empty": ([1000, 1000, 1000], 16, torch.float32, "tbd", torch.int64, 5, True, False, None, 1),
    "criteo_like": ([100000, 3, 40, 7, 20000, 1000, 12, 5000], [128, 16, 16, 16, 64, 32, 16, 64], torch.float32, "bd", torch.int64,
                    [1, 1, 2, 1, 30, 5, 1, 10], False, False, None, None),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_batched_sparse_grad_matrix(case, coracle):
    from param_amd import BatchedEmbeddingBagMI355

    rows, dims, wdtype, layout, idt, pooling, ragged, weighted, sl, empty = CASES[case]
    T = len(rows)
    B = 256
    dims_l = [dims] * T if isinstance(dims, int) else dims
    m = BatchedEmbeddingBagMI355(rows, dims, dtype=wdtype, device=DEV, layout=layout, init="normal", seed=3, fused_update=False,
                                 block_bags=64 if layout == "blocked" else None)
    idx_h, off_h = _request(rows, B, pooling, seed=sorted(CASES).index(case), empty_table=empty, ragged=ragged)
    idx, off = _t(idx_h).to(idt), _t(off_h).to(idt)
    psw_h = np.random.default_rng(5).standard_normal(len(idx_h)).astype(np.float32) if weighted else None
    psw = None if psw_h is None else _t(psw_h)
    shape = m._tables().out_desc(B)[2]
    grad = torch.randn(shape, device=DEV, generator=torch.Generator(DEV).manual_seed(11))
    b0, bc = (0, None) if sl is None else sl
    got = m.sparse_grad(grad, idx, off, psw, batch=B, bag_begin=b0, bag_count=bc)
    again = m.sparse_grad(grad, idx, off, psw, batch=B, bag_begin=b0, bag_count=bc)
    assert len(got) == T
    ref = _nonfused_reference(m, grad, idx, off, psw, B, b0, bc)
    dense = m.dense_grad(grad, idx, off, psw, batch=B) if sl is None else None
    ts = m._tables()
    g_h = grad.cpu().numpy()
    b1 = B if bc is None else b0 + bc
    for t in range(T):
        r, v = got[t]
        assert r.dtype == torch.int64 and v.dtype == torch.float32 and tuple(v.shape) == (r.numel(), dims_l[t])
        assert torch.equal(r, again[t][0]) and torch.equal(v, again[t][1]), (case, t)      # deterministic
        s, e = off_h[t * B + b0], off_h[t * B + b1]
        it = idx_h[s:e]
        assert np.array_equal(r.cpu().numpy(), np.unique(it)), (case, t)
        if t == empty:
            assert r.numel() == 0 and v.numel() == 0
        # bit for bit against the non-fused sorted pair, read at the rows
        assert torch.equal(v, ref.table(t)[r]), (case, t)
        # rows looked up at most 256 times: bit for bit against the dense gradient and the sequential oracle
        short = torch.from_numpy(_hits(it, rows[t])[r.cpu().numpy()] <= EXACT_RUN).to(DEV)
        if dense is not None:
            assert torch.equal(v[short], dense[t][r][short]), (case, t)
        gt = np.ascontiguousarray(_table_grad(g_h, t, ts, B))[b0:b1]
        orc = coracle.bwd_f32(np.zeros((rows[t], dims_l[t]), np.float32), it, off_h[t * B + b0:t * B + b1] - s, gt,
                              None if psw_h is None else psw_h[s:e])
        assert torch.equal(v[short], _t(orc)[r][short]), (case, t)


def test_batched_sparse_grad_splits_requests_of_more_than_1024_tables(coracle):
    from param_amd import BatchedEmbeddingBagMI355

    T, B = 1100, 16
    rows = [int(x) for x in np.random.default_rng(1).integers(20, 200, size=T)]
    dims = [[16, 32, 64, 128][t % 4] for t in range(T)]
    m = BatchedEmbeddingBagMI355(rows, dims, device=DEV, init="normal", fused_update=False)
    idx_h, off_h = _request(rows, B, 3, seed=7, empty_table=1050, ragged=True)
    idx, off = _t(idx_h), _t(off_h)
    grad = torch.randn(B, sum(dims), device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    got = m.sparse_grad(grad, idx, off, batch=B)
    again = m.sparse_grad(grad, idx, off, batch=B)
    assert len(got) == T
    g_h = grad.cpu().numpy()
    col = np.concatenate([[0], np.cumsum(dims)])
    for t in range(T):
        r, v = got[t]
        assert torch.equal(r, again[t][0]) and torch.equal(v, again[t][1])
        s, e = off_h[t * B], off_h[(t + 1) * B]
        it = idx_h[s:e]
        assert np.array_equal(r.cpu().numpy(), np.unique(it)), t
        orc = coracle.bwd_f32(np.zeros((rows[t], dims[t]), np.float32), it, off_h[t * B:(t + 1) * B] - s,
                              np.ascontiguousarray(g_h[:, col[t]:col[t + 1]]))
        assert torch.equal(v, _t(orc)[r]), t                 # every row here is looked up far fewer than 256 times


# ----------------------------------------------------------------------------- 3. long runs (Zipf heads)
@pytest.mark.parametrize("alpha", [1.05, 1.2])
def test_long_runs_bit_exact_with_the_sorted_apply(alpha):
    from param_amd import BatchedEmbeddingBagMI355
    from param_amd.indices import tbe_request

    rows, B, L, D = [200000, 50000], 8192, 20, 64
    m = BatchedEmbeddingBagMI355(rows, D, device=DEV, init=None, fused_update=False)
    idx, off = tbe_request(rows, B, L, alpha=alpha, device=DEV, seed=4)
    grad = torch.randn(B, len(rows) * D, device=DEV, generator=torch.Generator(DEV).manual_seed(9))
    got = m.sparse_grad(grad, idx, off, batch=B)
    ref = _nonfused_reference(m, grad, idx, off, None, B, 0, None)
    idx_h, off_h, g_h = idx.cpu().numpy(), off.cpu().numpy(), grad.cpu().numpy().astype(np.float64)
    for t in range(len(rows)):
        r, v = got[t]
        assert torch.equal(v, ref.table(t)[r]), t
        it = idx_h[t * B * L:(t + 1) * B * L]
        hits = _hits(it, rows[t])
        assert hits.max() > 2000, hits.max()                 # the head row's run spans several apply tiles
        contrib = g_h[np.repeat(np.arange(B), L), t * D:(t + 1) * D]
        exp = np.zeros((rows[t], D)); mag = np.zeros((rows[t], D))
        np.add.at(exp, it, contrib); np.add.at(mag, it, np.abs(contrib))
        rr = r.cpu().numpy()
        err = np.abs(v.cpu().numpy().astype(np.float64) - exp[rr])
        assert (err <= 1e-5 * mag[rr] + 1e-30).all(), t


# ----------------------------------------------------------------------------- 4. torch's sparse optimizers
@pytest.mark.parametrize("opt", ["SparseAdam", "SGD"])
def test_sparse_optimizers_match_torch_cpu(opt):
    from param_amd import EmbeddingBagMI355

    R, D, B, L = 5000, 64, 128, 10
    rng = np.random.default_rng(0)
    W = rng.standard_normal((R, D)).astype(np.float32)
    mg = EmbeddingBagMI355(R, D, sparse=True, _weight=_t(W))
    mc = torch.nn.EmbeddingBag(R, D, mode="sum", sparse=True, _weight=torch.from_numpy(W.copy()))
    make = (lambda p: torch.optim.SparseAdam(p, lr=0.01)) if opt == "SparseAdam" else (lambda p: torch.optim.SGD(p, lr=0.1))
    og, oc = make(mg.parameters()), make(mc.parameters())
    for step in range(3):
        idx = rng.integers(0, R // 10, size=B * L)            # plenty of duplicates
        off = np.arange(B, dtype=np.int64) * L
        g = rng.standard_normal((B, D)).astype(np.float32)
        for m, o, to in ((mg, og, _t), (mc, oc, torch.from_numpy)):
            o.zero_grad()
            m(to(idx), to(off)).backward(to(g))
            o.step()
    torch.testing.assert_close(mg.weight.detach().cpu(), mc.weight.detach(), rtol=1e-6, atol=1e-6)


# ----------------------------------------------------------------------------- 5. real size: no dense gradient
def test_real_size_table_without_a_dense_gradient():
    from param_amd import EmbeddingBagMI355

    R, D, B, L = 10_000_000, 128, 8192, 20
    m = EmbeddingBagMI355(R, D, sparse=True, device=DEV)
    gen = torch.Generator(DEV).manual_seed(3)
    idx = torch.randint(0, R, (B * L,), device=DEV, generator=gen)
    off = torch.arange(B, device=DEV) * L
    grad = torch.randn(B, D, device=DEV, generator=gen)
    out = m(idx, off)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out.backward(grad)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    sg = m.weight.grad
    assert sg.is_sparse and sg.is_coalesced()
    U = sg.indices().shape[1]
    ws = m._tables()._ws.numel()
    bound = U * D * 4 + U * 8 + ws + (2 << 20)              # values + row ids + workspace (+ the pointer arrays, allocator rounding)
    assert growth <= bound, (growth, bound)
    assert growth < R * D * 4 // 20, growth
    assert np.array_equal(sg.indices()[0].cpu().numpy(), np.unique(idx.cpu().numpy()))
    # spot check: 10 000 of the rows against an fp64 reference built on the device for those rows only
    rows, vals = sg.indices()[0], sg.values()
    pick = torch.randperm(U, device=DEV, generator=gen)[:10000].sort().values
    chosen = rows[pick]
    pos = torch.searchsorted(chosen, idx)
    hit = (pos < chosen.numel()) & (chosen[pos.clamp(max=chosen.numel() - 1)] == idx)
    j = hit.nonzero().squeeze(1)
    contrib = grad[j // L].double()
    exp = torch.zeros(chosen.numel(), D, dtype=torch.float64, device=DEV).index_add_(0, pos[j], contrib)
    mag = torch.zeros(chosen.numel(), D, dtype=torch.float64, device=DEV).index_add_(0, pos[j], contrib.abs())
    err = (vals[pick].double() - exp).abs()
    assert bool((err <= 1e-5 * mag + 1e-30).all())
