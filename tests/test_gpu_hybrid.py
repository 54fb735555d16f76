"""Hybrid backward (round 4) and the key sort's failure channel -- GPU parity tests (``pytest -m gpu``), through the C ABI.

Hybrid: tables whose step touches (nearly) every row once skip the sort -- rows looked up once are applied bag-major
(``bwd_unique_kernel``), only lookups flagged by the four hashed "looked up twice" bitmaps go through the sorted apply.  The bar
is the sorted backward's: bit-exact against the sequential oracle for every row looked up at most 256 times.
Reference semantics: fbgemm TBE backward / aten::_embedding_bag_dense_backward at
train/comms/pt/pytorch_dist_backend.py:854-857, split_table_batched_embeddings_ops.py:318-324.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    import param_amd

    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    param_amd.load_library()
    # (round 6: the library offers the hybrid path to requests of >= 1024 bag-major workgroups only; these tests drive its kernels with
    # small requests, so the bound is lifted here -- test_small_requests_are_not_offered_the_hybrid_path pins the product rule)
    param_amd.set_hybrid_min_tiles(0)
    yield
    param_amd.set_hybrid_min_tiles()
    param_amd.set_hybrid_tuning()
    param_amd.set_hybrid_rest()
    param_amd.set_sort_tuning()


def _model(rows, D, dtype=torch.float32, layout="bd", seed=0):
    import param_amd

    return param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=dtype, device=DEV, init="normal", layout=layout, seed=seed, fused_update=False)


def _request(rows, B, pools, alpha, seed, index_dtype=torch.int64):
    from param_amd.indices import tbe_request

    return tbe_request(rows, B, pools, alpha=alpha, device=DEV, seed=seed, index_dtype=index_dtype)


def _oracle_tables(coracle, tabs, idx, off, B, grad, D, alpha, layout="bd"):
    out = []
    idx_h, off_h, g_h = idx.cpu().numpy().astype(np.int64), off.cpu().numpy().astype(np.int64), grad.cpu().numpy()
    for t, W in enumerate(tabs):
        s = off_h[t * B]
        e = off_h[(t + 1) * B] if (t + 1) * B < len(off_h) else len(idx_h)
        loc = off_h[t * B:(t + 1) * B] - s
        g = np.ascontiguousarray(g_h[:, t * D:(t + 1) * D]) if layout == "bd" else np.ascontiguousarray(g_h[t])
        out.append(coracle.bwd_f32(W.copy(), idx_h[s:e], loc, g, alpha=alpha))
    return out


@pytest.mark.parametrize("layout,idt", [("bd", torch.int64), ("tbd", torch.int32)])
def test_hybrid_uniform_tables_bit_exact_vs_oracle(coracle, layout, idt):
    """8 uniform-index tables (20 480 lookups into 400 000 rows each: ~2.5 % repeats): every table goes hybrid, every row equals
    the sequential oracle bit for bit; the same request with the hybrid path off gives the same bits."""
    import param_amd

    rows, D, B, L = [400_000] * 8, 128, 1024, 20
    idx, off = _request(rows, B, L, 0.0, 3, idt)
    gshape = (B, len(rows) * D) if layout == "bd" else (len(rows), B, D)
    grad = torch.randn(gshape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    results = {}
    for en in (1, 0):
        param_amd.set_hybrid_tuning(en)
        m = _model(rows, D, layout=layout, seed=7)
        tabs = [m.table(t).cpu().numpy() for t in range(len(rows))]
        m.scatter_add_(grad, idx, off, alpha=-0.05, batch=B)
        st = m.sort_status(idx, off, batch=B)
        torch.cuda.synchronize()
        assert st["lookback_fallbacks"] == 0
        if en:
            assert st["hybrid_tables"] == len(rows) and st["hybrid_launched"] == 1, st
            # only the flagged lookups left the bag-major kernel -- and (round 6) a few hundred per table are finished inside LDS
            assert 0 < st["pairs_sorted"] + st["lds_pairs"] < 0.1 * idx.numel(), st
            assert st["lds_tables"] == len(rows) and st["pairs_sorted"] == 0, st
        else:
            assert st["hybrid_tables"] == 0 and st["pairs_sorted"] == idx.numel(), st
        results[en] = [m.table(t).cpu().numpy() for t in range(len(rows))]
        if en:
            exp = _oracle_tables(coracle, tabs, idx, off, B, grad, D, -0.05, layout)
            for t in range(len(rows)):
                assert np.array_equal(results[en][t], exp[t]), t
    for t in range(len(rows)):
        assert np.array_equal(results[1][t], results[0][t]), t


def test_hybrid_forced_on_skewed_and_mixed_tables(coracle):
    """enable = 2 sends every structurally eligible table down the hybrid path whatever its indices look like: Zipf tables (most
    lookups flagged, hot rows in long runs), a table too small to qualify, one with too many lookups per row.  Rows looked up at
    most 256 times must equal the oracle bit for bit; the default classification (enable = 1) must give the same bits."""
    import param_amd

    rows = [300_000, 300_000, 5_000, 60_000, 300_000, 300_000]
    pools = [20, 20, 20, 20, 9, 20]
    alphas = [1.05, 0.0, 0.0, 0.0, 1.05, 0.0]
    D, B = 64, 1024
    from param_amd.indices import tbe_request

    parts = [tbe_request([r], B, [p], alpha=a, device=DEV, seed=11 + i)[0] for i, (r, p, a) in enumerate(zip(rows, pools, alphas))]
    idx = torch.cat(parts)
    lens = torch.cat([torch.full((B,), p, dtype=torch.int64, device=DEV) for p in pools])
    off = torch.zeros(len(rows) * B + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(lens, 0, out=off[1:])
    grad = torch.randn((B, len(rows) * D), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    got = {}
    for en in (2, 1):
        param_amd.set_hybrid_tuning(en)
        m = _model(rows, D, seed=9)
        tabs = [m.table(t).cpu().numpy() for t in range(len(rows))]
        m.scatter_add_(grad, idx, off, alpha=0.25, batch=B)
        st = m.sort_status(idx, off, batch=B)
        got[en] = [m.table(t).cpu().numpy() for t in range(len(rows))]
        if en == 2:
            assert st["hybrid_tables"] == 4, st          # tables 0, 1, 4 (9216 lookups >= 8192), 5; not 2 (tiny) nor 3 (20480 * 8 > 60000)
            exp = _oracle_tables(coracle, tabs, idx, off, B, grad, D, 0.25)
            idx_h, off_h = idx.cpu().numpy(), off.cpu().numpy()
            for t in range(len(rows)):
                cnt = np.bincount(idx_h[off_h[t * B]:off_h[(t + 1) * B]], minlength=rows[t])
                cold = cnt <= 256
                assert np.array_equal(got[en][t][cold], exp[t][cold]), t
                hot = ~cold
                if hot.any():
                    np.testing.assert_allclose(got[en][t][hot], exp[t][hot], rtol=2e-4, atol=2e-4)
        else:
            # the two uniform tables that qualify on their own (1 and 5) hold 37 % of the request's lookups: below one half the
            # request stays on the sorted path (HybTable::cand, common.h)
            assert st["hybrid_tables"] == 0, st
    idx_h, off_h = idx.cpu().numpy(), off.cpu().numpy()
    for t in range(len(rows)):
        # rows looked up more than 256 times are summed as ordered chunk partials, and which lookups share a chunk depends on what
        # else is in the sorted arrays: same value up to fp32 association (the documented contract), same bits everywhere else
        cold = np.bincount(idx_h[off_h[t * B]:off_h[(t + 1) * B]], minlength=rows[t]) <= 256
        assert np.array_equal(got[2][t][cold], got[1][t][cold]), t
        np.testing.assert_allclose(got[2][t][~cold], got[1][t][~cold], rtol=2e-4, atol=2e-4)


def test_hybrid_bf16_tables_and_batch_slices(coracle):
    """bf16 tables (widened, one rounding per row) and a request applied as two batch slices, hybrid on vs off: same bits"""
    import param_amd

    rows, D, B, L = [250_000] * 4, 128, 2048, 10
    idx, off = _request(rows, B, L, 0.0, 5)
    grad = torch.randn((B, len(rows) * D), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    res = {}
    for en in (1, 0):
        param_amd.set_hybrid_tuning(en)
        m = _model(rows, D, dtype=torch.bfloat16, seed=4)
        m.scatter_add_(grad, idx, off, alpha=-0.5, batch=B, bag_begin=0, bag_count=1500)
        if en:
            assert m.sort_status(idx, off, batch=B, bag_begin=0, bag_count=1500)["hybrid_tables"] == 4
        m.scatter_add_(grad, idx, off, alpha=-0.5, batch=B, bag_begin=1500, bag_count=B - 1500)
        res[en] = m.weights.data.view(torch.int16).cpu().numpy().copy()
    assert np.array_equal(res[1], res[0])
    # and against the oracle's bf16 routine for table 0, whole batch in one call
    param_amd.set_hybrid_tuning(1)
    m = _model(rows, D, dtype=torch.bfloat16, seed=4)
    W0 = m.table(0).view(torch.int16).cpu().numpy().view(np.uint16).copy()
    m.scatter_add_(grad, idx, off, alpha=-0.5, batch=B)
    idx_h, off_h = idx.cpu().numpy(), off.cpu().numpy()
    exp = coracle.bwd_bf16(W0, idx_h[:off_h[B]], off_h[:B], np.ascontiguousarray(grad.cpu().numpy()[:, :D]), alpha=-0.5)
    assert np.array_equal(m.table(0).view(torch.int16).cpu().numpy().view(np.uint16), exp)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_hybrid_rowwise_adagrad_same_bits_as_sorted_path(coracle, dtype):
    """fused row-wise Adagrad (weight decay L2, the reference's TBE optimizer settings) through the hybrid path == through the
    sorted path, tables and optimizer state, bit for bit; fp32 also against the oracle"""
    import param_amd

    rows, D, B, L = [200_000] * 3, 128, 1024, 12
    idx, off = _request(rows, B, L, 0.0, 8)
    grad = torch.randn((B, len(rows) * D), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    res = {}
    for en in (1, 0):
        param_amd.set_hybrid_tuning(en)
        m = _model(rows, D, dtype=dtype, seed=6)
        m.optimizer, m.learning_rate, m.eps, m.weight_decay, m.weight_decay_mode = "rowwise_adagrad", 0.05, 1e-8, 0.01, "l2"
        W0 = m.table(0).float().cpu().numpy().copy()
        for _ in range(2):
            m.adagrad_step_(grad, idx, off, batch=B)
        if en:
            assert m.sort_status(idx, off, batch=B)["hybrid_tables"] == 3
        res[en] = (m.weights.data.float().cpu().numpy().copy(), m.momentum.cpu().numpy().copy())
    assert np.array_equal(res[1][0], res[0][0]) and np.array_equal(res[1][1], res[0][1])
    if dtype == torch.float32:
        idx_h, off_h = idx.cpu().numpy(), off.cpu().numpy()
        g0 = np.ascontiguousarray(grad.cpu().numpy()[:, :D])
        W, mom = W0.copy(), np.zeros(rows[0], dtype=np.float32)
        for _ in range(2):
            W, mom = coracle.bwd_rowwise_adagrad(W, mom, idx_h[:off_h[B]], off_h[:B], g0, lr=0.05, eps=1e-8, weight_decay=0.01,
                                                 weight_decay_mode=1)
        got = res[1][0].reshape(-1)[:rows[0] * D].reshape(rows[0], D)
        np.testing.assert_allclose(got, W, rtol=2e-5, atol=1e-6)


# The launch ladders of the bag-major kernel (bwd_unique_kernel) and of the LDS left-over kernel (hyb_rest_kernel) pick one instance
# per (destination dtype, lane-group width G, optimizer OPT: 0 plain update, 1 row-wise Adagrad, 2 element-wise Adagrad).  Reached by
# other tests (G = D / 4 for fp32 tables, D / 8 for 16-bit ones, at least 8):
#   OPT 0  fp32 G 8 / 16 / 32 / 64: test_gpu_rest.py (D 32 / 64 / 128 / 256); bf16 G 16: test_hybrid_bf16_tables_and_batch_slices
#   OPT 1  fp32 G 32, bf16 G 16: test_hybrid_rowwise_adagrad_same_bits_as_sorted_path, test_gpu_rest.py
#   OPT 2  fp32 G 32, bf16 G 8 (both kernels), fp32 G 8 (bag-major only): test_gpu_elem_adagrad.py
# (the random requests below and in test_gpu_fuzz.py add whatever their seeds draw).  The cases here are every other pair.
_LADDER = ([(torch.bfloat16, g, 0) for g in (8, 32, 64)] +
           [(torch.float32, g, 1) for g in (8, 16, 64)] + [(torch.bfloat16, g, 1) for g in (8, 32, 64)] +
           [(torch.float32, g, 2) for g in (8, 16, 64)] + [(torch.bfloat16, g, 2) for g in (16, 32, 64)])


@pytest.mark.parametrize("dtype,G,opt", _LADDER, ids=[f"{'f32' if d == torch.float32 else 'bf16'}-G{g}-opt{o}" for d, g, o in _LADDER])
def test_every_lane_group_width_and_optimizer_of_the_hybrid_kernels(coracle, dtype, G, opt):
    """The smallest hybrid-eligible request at the row width that selects lane groups of G: two tables, 8192 lookups each (batch 1024 x
    pooling 8) into 4 x as many rows, a few rows looked up several times on top of what uniform indices repeat, so that both the
    bag-major kernel and the LDS left-over kernel have work.  Tables and optimizer state after two steps equal the same steps with
    the hybrid path off, bit for bit; the plain update also equals the sequential oracle, bit for bit."""
    import param_amd

    B, L = 1024, 8
    rows = [4 * B * L] * 2
    D = G * (4 if dtype == torch.float32 else 8)
    idx, off = _request(rows, B, L, 0.0, 31)
    idx = idx.clone()
    for t in range(2):
        idx[t * B * L + 3:t * B * L + 40 * L:L] = 17                 # one row in 40 bags ...
        idx[t * B * L + 5:t * B * L + 5 + 3] = 4242 + t               # ... and one three times in one bag
    grad = torch.randn((B, len(rows) * D), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    kw = {} if opt == 0 else dict(optimizer="rowwise_adagrad" if opt == 1 else "adagrad", learning_rate=0.05, eps=1e-8)
    res = {}
    for hyb in (2, 0):
        param_amd.set_hybrid_tuning(hyb)
        m = param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=dtype, device=DEV, init="normal", seed=3, fused_update=False, **kw)
        W0 = m.table(0).clone()
        for _ in range(2):
            if opt == 0:
                m.scatter_add_(grad, idx, off, alpha=-0.05, batch=B)
            else:
                m.adagrad_step_(grad, idx, off, batch=B)
        st = m.sort_status(idx, off, batch=B)
        if hyb:
            assert st["hybrid_launched"] and st["hybrid_tables"] == 2, st      # (launched: the mode it ran in, 2 = forced)
            assert st["lds_tables"] == 2 and st["lds_pairs"] > 0 and st["pairs_sorted"] == 0, st
        else:
            assert st["hybrid_tables"] == 0 and st["pairs_sorted"] == idx.numel(), st
        res[hyb] = (m.weights.data.clone(), m.momentum.clone() if opt else None)
        del m
    param_amd.set_hybrid_tuning()
    assert torch.equal(res[2][0].view(torch.uint8), res[0][0].view(torch.uint8))
    if opt:
        assert torch.equal(res[2][1], res[0][1]) and bool(res[2][1].any())
    else:                                                              # (bf16 tables: the only plain-update cases of the list)
        idx_h, off_h = idx.cpu().numpy(), off.cpu().numpy()
        g0 = np.ascontiguousarray(grad.cpu().numpy()[:, :D])
        exp = W0.view(torch.int16).cpu().numpy().view(np.uint16).copy()
        for _ in range(2):
            exp = coracle.bwd_bf16(exp, idx_h[:off_h[B]], off_h[:B], g0, alpha=-0.05)
        got = res[2][0].reshape(-1)[:rows[0] * D].reshape(rows[0], D)
        assert np.array_equal(got.view(torch.int16).cpu().numpy().view(np.uint16), exp)


def test_the_path_taken_depends_on_the_request_alone():
    """Which tables go hybrid is decided on the device from the request itself -- nothing is cached or carried over: uniform and
    Zipf requests alternating on ONE workspace take the same paths (and leave the same bits) as each of them on a fresh one."""
    import param_amd

    rows, D, B, L = [400_000] * 8, 32, 1024, 20
    uni = _request(rows, B, L, 0.0, 1)
    zipf = _request(rows, B, L, 1.05, 2)
    grad = torch.randn((B, len(rows) * D), device=DEV)
    param_amd.set_hybrid_tuning(1)
    m = _model(rows, D, seed=1)
    seq = [("u", uni), ("z", zipf), ("z", zipf), ("u", uni), ("u", uni)]
    seen = []
    for tag, (i, o) in seq:
        m.scatter_add_(grad, i, o, alpha=-0.01, batch=B)
        st = m.sort_status(i, o, batch=B)
        seen.append((tag, st["hybrid_launched"], st["hybrid_tables"]))
    assert seen == [("u", 1, 8), ("z", 1, 0), ("z", 1, 0), ("u", 1, 8), ("u", 1, 8)], seen
    ref = _model(rows, D, seed=1)
    for tag, (i, o) in seq:
        fresh = _model(rows, D, seed=1)                      # a fresh module = a fresh workspace
        fresh.weights.data.copy_(ref.weights.data)
        fresh.scatter_add_(grad, i, o, alpha=-0.01, batch=B)
        ref.weights.data.copy_(fresh.weights.data)
    assert torch.equal(m.weights.data, ref.weights.data)


def test_lookback_walks_that_count_for_their_predecessors_give_the_same_sort():
    """The sort's progress guarantee: a look-back walk that has waited too long for a predecessor's published digit counts counts
    that tile's digits itself.  lookback_spin_cap = 1 takes that path wherever a predecessor is a moment late (rare on an idle
    device), 0xFFFFFFFF takes it for EVERY predecessor of every tile of passes 1 and 2 (nothing published is believed).  The
    sorted pairs must be numpy's stable order and the table must equal the default run's either way."""
    import param_amd
    from param_amd.embedding_bag import _sort_indices, sorted_pairs

    rows, D, B, L = [2_000_000], 16, 65536, 16          # one segment of 256 radix tiles
    idx, off = _request(rows, B, L, 1.05, 13)
    grad = torch.randn((B, D), device=DEV)
    param_amd.set_hybrid_tuning(0)
    good = _model(rows, D, seed=2)
    good.scatter_add_(grad, idx, off, alpha=1.0, batch=B)
    assert good.sort_status(idx, off, batch=B)["lookback_fallbacks"] == 0
    keys = idx.cpu().numpy()
    order = np.argsort(keys, kind="stable")
    for cap in (0xFFFFFFFF, 1, 1):
        param_amd.set_hybrid_tuning(0, cap)
        m = _model(rows, D, seed=2)
        ts = m._tables()
        _sort_indices(ts, idx, off, B)
        k, v, _ = sorted_pairs(ts, idx, off, B)
        assert np.array_equal(k.cpu().numpy(), keys[order]) and np.array_equal(v.cpu().numpy(), order // L)
        m.scatter_add_(grad, idx, off, alpha=1.0, batch=B)
        fb = m.sort_status(idx, off, batch=B)["lookback_fallbacks"]
        if cap == 0xFFFFFFFF:
            assert fb == 2 * (255 * 256 // 2), fb           # passes 1 and 2: tile j counts for its j predecessors
        assert torch.equal(m.weights.data, good.weights.data)
    param_amd.set_hybrid_tuning(0, 0)


def test_lookback_sort_on_a_cu_masked_stream_beside_a_saturating_forward():
    """The look-back sort on a 32-CU-masked stream while a full-size forward saturates the default stream, 200 times: the sorted
    pairs equal numpy's stable order (a walk that waits too long counts for its predecessor, so the sort's progress does not
    depend on how the dispatcher interleaves its workgroups with the forward's; how often that happened is reported)."""
    import param_amd
    from bench import masked_stream
    from param_amd.embedding_bag import _sort_indices, sorted_pairs

    param_amd.set_hybrid_tuning(0)
    big_rows, D, B, L = [4_000_000] * 8, 128, 8192, 20
    big = _model(big_rows, D, seed=3)
    bi, bo = _request(big_rows, B, L, 0.0, 21)
    out = torch.empty((B, len(big_rows) * D), device=DEV)
    rows = [1_000_000] * 4
    sm = _model(rows, 16, seed=4)
    si, so = _request(rows, 16384, 10, 1.05, 22)              # 4 segments of 40 tiles
    ts = sm._tables()
    ms = masked_stream(32, torch.device(DEV))
    keys_h = si.cpu().numpy()
    n1 = 16384 * 10
    expect = []
    for t in range(len(rows)):
        seg = keys_h[t * n1:(t + 1) * n1]
        order = np.argsort(seg, kind="stable")
        expect.append(((t << 20) | seg[order], order // 10))
    for it in range(200):
        for _ in range(3):
            big.lookup(bi, bo, out=out, batch=B)
        ms.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(ms):
            _sort_indices(ts, si, so, 16384)
        for _ in range(3):
            big.lookup(bi, bo, out=out, batch=B)
        torch.cuda.current_stream().wait_stream(ms)
        if it % 20 == 0 or it == 199:
            st = sm.sort_status(si, so, batch=16384)
            k, v, tsh = sorted_pairs(ts, si, so, 16384)
            assert tsh == 20
            k, v = k.cpu().numpy(), v.cpu().numpy()
            for t in range(len(rows)):
                assert np.array_equal(k[t * n1:(t + 1) * n1], expect[t][0]) and np.array_equal(v[t * n1:(t + 1) * n1], expect[t][1]), (it, t)


import os  # noqa: E402

_HYB_SEEDS = int(os.environ.get("PARAM_AMD_HYBRID_FUZZ_SEEDS", "10"))      # soak runs raise it


@pytest.mark.parametrize("seed", range(_HYB_SEEDS))
def test_random_mid_size_requests_hybrid_vs_sorted_and_oracle(seed, coracle):
    """Random requests LARGE enough for tables to qualify (the small-request fuzz of test_gpu_fuzz.py never reaches 8192 lookups
    per table): 1 .. 10 tables of mixed sizes, per-table pooling factors, some tables ragged, Zipf or uniform per table, dims,
    fp32 / bf16 tables, int32 / int64 indices, both layouts, batch slices, plain update or fused Adagrad; classified (enable 1) and
    forced (enable 2).  Bar: the hybrid result equals the hybrid-off result bit for bit on every row looked up at most 256 times
    (everywhere else to fp32 association), and table 0 equals the oracle (fp32, plain update)."""
    import param_amd
    from param_amd.indices import tbe_request

    rng = np.random.default_rng(7000 + seed)
    T = int(rng.integers(1, 11))
    B = int(rng.choice([512, 1024, 2048, 4096]))
    wdt = torch.bfloat16 if rng.random() < 0.35 else torch.float32
    D = int(rng.choice([32, 64, 128, 256]))
    rows = [int(rng.choice([3, 1000, 60_000, 300_000, 1_000_000, 2_500_000])) for _ in range(T)]
    pools = [int(rng.choice([1, 4, 9, 20, 40])) for _ in range(T)]
    alphas = [1.05 if rng.random() < 0.35 else 0.0 for _ in range(T)]
    idt = torch.int32 if rng.random() < 0.4 else torch.int64
    layout = "tbd" if rng.random() < 0.4 else "bd"
    adagrad = rng.random() < 0.3
    parts, lens = [], []
    for t in range(T):
        i_t, _ = tbe_request([rows[t]], B, [pools[t]], alpha=alphas[t], device=DEV, seed=int(rng.integers(1 << 30)))
        ln = torch.full((B,), pools[t], dtype=torch.int64, device=DEV)
        if rng.random() < 0.25 and pools[t] > 1:              # a ragged table: same lookups, uneven bags
            cut = torch.randint(0, pools[t], (B // 2,), device=DEV)
            ln[0:B // 2 * 2:2] -= cut
            ln[1:B // 2 * 2:2] += cut
        parts.append(i_t)
        lens.append(ln)
    idx = torch.cat(parts).to(idt)
    off = torch.zeros(T * B + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(torch.cat(lens), 0, out=off[1:])
    off = off.to(idt)
    gshape = (B, T * D) if layout == "bd" else (T, B, D)
    grad = torch.randn(gshape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    b0 = int(rng.integers(0, B // 4)) if rng.random() < 0.3 else 0
    bc = B - b0 - (int(rng.integers(0, B // 4)) if b0 else 0)
    res, hyb_tables = {}, {}
    for en in (0, 1, 2):
        param_amd.set_hybrid_tuning(en)
        m = _model(rows, D, dtype=wdt, layout=layout, seed=seed)
        W0 = m.table(0).float().cpu().numpy().copy() if en == 0 else None
        if adagrad:
            m.optimizer, m.learning_rate, m.eps = "rowwise_adagrad", 0.05, 1e-8
            if b0 == 0 and bc == B:
                m.adagrad_step_(grad, idx, off, batch=B)
            else:                                              # the fused optimizer takes whole batches: plain update for slices
                m.scatter_add_(grad, idx, off, alpha=-0.05, batch=B, bag_begin=b0, bag_count=bc)
        else:
            m.scatter_add_(grad, idx, off, alpha=-0.05, batch=B, bag_begin=b0, bag_count=bc)
        st = m.sort_status(idx, off, batch=B, bag_begin=b0, bag_count=bc)
        hyb_tables[en] = st["hybrid_tables"]
        res[en] = [m.table(t).float().cpu().numpy().copy() for t in range(T)]
        if en == 0:
            w0_after = res[0][0]
            w0_before = W0
    assert hyb_tables[0] == 0
    idx_h, off_h = idx.cpu().numpy().astype(np.int64), off.cpu().numpy().astype(np.int64)
    for t in range(T):
        s = off_h[t * B + b0]
        e = off_h[t * B + b0 + bc]
        cold = np.bincount(idx_h[s:e], minlength=rows[t]) <= 256
        for en in (1, 2):
            assert np.array_equal(res[en][t][cold], res[0][t][cold]), (seed, en, t, hyb_tables)
            # hotter rows: ordered chunk partials whose boundaries follow what else is in the sorted arrays -- fp32 association,
            # and for bf16 tables one rounding of the result on top (an ulp of bf16 is 2^-8 relative)
            tol = 3e-4 if wdt == torch.float32 else 1.6e-2
            np.testing.assert_allclose(res[en][t][~cold], res[0][t][~cold], rtol=tol, atol=tol)
    if wdt == torch.float32 and not adagrad:
        s, e = off_h[b0], off_h[b0 + bc]
        g0 = grad.cpu().numpy()
        g0 = np.ascontiguousarray(g0[b0:b0 + bc, :D]) if layout == "bd" else np.ascontiguousarray(g0[0, b0:b0 + bc])
        exp = coracle.bwd_f32(w0_before.copy(), idx_h[s:e], off_h[b0:b0 + bc] - s, g0, alpha=-0.05)
        cold = np.bincount(idx_h[s:e], minlength=rows[0]) <= 256
        assert np.array_equal(w0_after[cold], exp[cold]), seed
    param_amd.set_hybrid_tuning()


def test_sort_aside_consumes_the_request_and_only_fused_calls_defer(coracle):
    """Round 5: the hybrid backward defers part of the sort into the apply, which reads the request's indices AGAIN.
    That is safe only when the library sequences sort and apply itself (pm_embbag_bwd_fused*).  A sort issued on its own must
    consume the request completely -- the caller may refill the index buffer before the apply:
      * sort aside, overwrite the indices with another request's, apply presorted -> the tables of the ORIGINAL request, bit for bit;
      * pm_embbag_sorted_pairs after the bare sort (hybrid at its default) shows every pair, in numpy's stable order;
      * the fused call on the same request goes hybrid (status) and gives the same tables."""
    import param_amd
    from param_amd.embedding_bag import _sort_indices, sorted_pairs

    param_amd.set_hybrid_tuning()                       # default: on
    rows, D, B, L = [300_000] * 8, 128, 1024, 16
    idx, off = _request(rows, B, L, 0.0, 5)
    other, _ = _request(rows, B, L, 0.0, 6)
    grad = torch.randn(B, len(rows) * D, device=DEV)
    ref = _model(rows, D, seed=4)
    tabs = [ref.table(t).cpu().numpy() for t in range(len(rows))]
    exp = _oracle_tables(coracle, tabs, idx, off, B, grad, D, -0.5)

    fused = _model(rows, D, seed=4)
    fused.scatter_add_(grad, idx, off, alpha=-0.5, batch=B)
    st = fused.sort_status(idx, off, batch=B)
    assert st["hybrid_launched"] == 1 and st["hybrid_tables"] == len(rows), st
    for t in range(len(rows)):
        assert np.array_equal(fused.table(t).cpu().numpy(), exp[t]), t

    aside = _model(rows, D, seed=4)
    ts = aside._tables()
    work = idx.clone()
    _sort_indices(ts, work, off, B)
    k, v, tsh = sorted_pairs(ts, work, off, B)          # a bare sort is complete: no PM_ERR_INVALID, all pairs there
    n1 = B * L
    kh, ih = k.cpu().numpy(), idx.cpu().numpy()
    for t in range(len(rows)):
        seg = ih[t * n1:(t + 1) * n1]
        order = np.argsort(seg, kind="stable")
        assert np.array_equal(kh[t * n1:(t + 1) * n1], (t << tsh) | seg[order]), t
    st = aside.sort_status(work, off, batch=B)
    assert st["hybrid_launched"] == 0 and st["pairs_sorted"] == idx.numel(), st
    work.copy_(other)                                   # the caller reuses its index buffer ...
    torch.cuda.synchronize()
    aside.scatter_add_(grad, work, off, alpha=-0.5, batch=B, presorted=True)      # ... and the apply still applies what was sorted
    for t in range(len(rows)):
        assert np.array_equal(aside.table(t).cpu().numpy(), exp[t]), t


@pytest.mark.parametrize("lookups_per_table,rows", [(327_680, 3_000_000), (655_360, 6_000_000), (1_310_720, 10_000_000)])
def test_hybrid_scales_its_dup_maps_with_the_tables_lookups(lookups_per_table, rows):
    """Round 5: a rank of an N-GPU table-wise sharded step serves the GLOBAL batch for its tables -- 327 K / 655 K / 1.3 M lookups per
    table at N = 2 / 4 / 8 -- and round 4's 2^18-lookup limit made the hybrid path an N = 1 optimisation.  The dup map now grows with
    the table's lookups (8 / 16 / 32 slices of 16 384 words): such tables go hybrid, and the fused call leaves the tables of the fully
    sorted path bit for bit (rows looked up <= 256 times: every row here)."""
    import param_amd

    T, D, L = 2, 32, 20
    B = lookups_per_table // L
    idx, off = _request([rows] * T, B, L, 0.0, 11)
    grad = torch.randn(B, T * D, device=DEV)
    out = {}
    for en in (1, 0):
        param_amd.set_hybrid_tuning(en)
        m = _model([rows] * T, D, seed=8)
        m.scatter_add_(grad, idx, off, alpha=-0.125, batch=B)
        st = m.sort_status(idx, off, batch=B)
        if en:
            assert st["hybrid_launched"] == 1 and st["hybrid_tables"] == T, st
            assert st["pairs_sorted"] < 0.3 * idx.numel(), st            # true repeats (5-12 % of the lookups) + ~1.5 % false positives
            assert st["lds_tables"] == 0 and st["lds_pairs"] == 0, st     # tens of thousands per table: too many for the LDS sort
        else:
            assert st["hybrid_tables"] == 0 and st["pairs_sorted"] == idx.numel(), st
        out[en] = m.weights.data.clone()
        del m
    param_amd.set_hybrid_tuning()
    assert torch.equal(out[1], out[0])


@pytest.mark.parametrize("idt", [torch.int64, torch.int32])
def test_rows_dealt_out_to_slice_queues_overflow_and_batch_slices(idt):
    """Round 5, hyb_part_kernel: from 8 map slices per table on (> 2^18 lookups) the candidate tables' rows are dealt out to one queue
    per (table, slice) and the mark workgroups read their queue only.  A queue holds twice a slice's mean share: here half of table
    0's lookups are ONE row (forced eligibility), its slice overflows and is scanned the old way; table 1 is uniform.  Every row
    but the hot one keeps the fully sorted path's bits; the hot row (a run of 164 K lookups: chunk partials, whose boundaries
    follow what else is in the sorted arrays) stays within 1e-5.  Then the same through a batch slice."""
    import param_amd

    T, D, L, R = 2, 32, 20, 3_000_000
    B = 16384                                                          # 327 680 lookups per table: 8 slices
    idx, off = _request([R] * T, B, L, 0.0, 21, index_dtype=idt)
    idx = idx.clone()
    idx[:B * L:2] = 7                                                  # every other lookup of table 0
    grad = torch.randn(B, T * D, device=DEV)
    for kw in ({}, {"bag_begin": 1024, "bag_count": B - 2048}):
        out = {}
        for en in (2, 0):
            param_amd.set_hybrid_tuning(en)
            m = _model([R] * T, D, seed=8)
            m.scatter_add_(grad, idx, off, alpha=-0.125, batch=B, **kw)
            st = m.sort_status(idx, off, batch=B, **kw)
            assert st["hybrid_tables"] == (T if en else 0), (st, kw)
            out[en] = [m.table(t).clone() for t in range(T)]
            del m
        assert torch.equal(out[2][1], out[0][1]), kw
        keep = torch.ones(R, dtype=torch.bool, device=DEV)
        keep[7] = False
        assert torch.equal(out[2][0][keep], out[0][0][keep]), kw
        n_hot = (B * L // 2) if not kw else ((B - 2048) * L // 2)
        tol = 1e-5 * (0.125 * n_hot * 4.0 + 4.0)                       # |g| < 4 practically: sum of |contribution| bound
        assert (out[2][0][7] - out[0][0][7]).abs().max() <= tol, kw
    param_amd.set_hybrid_tuning()



def test_small_requests_are_not_offered_the_hybrid_path(coracle):
    """Round 6: the bag-major kernel tiles 128 bags, so a request of few tables is a handful of workgroups pooling in turn while the
    chip idles (one 10 M-row table, batch 8192: 254 us against the sorted path's 96; profiles/r06_few_tables_hybrid.jsonl).  The
    library offers the hybrid path from 1024 such workgroups on -- a rule on the request's sizes: 8 tables x batch 4096 = 256 of them
    sort everything by default, go hybrid with the bound lifted (pm_set_hybrid_min_tiles(0)) or lowered below the request, and give
    the oracle's tables, bit for bit, every time."""
    import param_amd

    rows, D, B, L = [400_000] * 8, 64, 4096, 4
    idx, off = _request(rows, B, L, 0.0, 11)
    grad = torch.randn(B, len(rows) * D, device=DEV)
    ref = _model(rows, D, seed=9)
    tabs = [ref.table(t).cpu().numpy() for t in range(len(rows))]
    exp = _oracle_tables(coracle, tabs, idx, off, B, grad, D, -0.25)
    try:
        for tiles, hybrid in ((-1, False), (0, True), (256, True), (257, False)):
            param_amd.set_hybrid_min_tiles(tiles)
            m = _model(rows, D, seed=9)
            m.scatter_add_(grad, idx, off, alpha=-0.25, batch=B)
            st = m.sort_status(idx, off, batch=B)
            assert (st["hybrid_launched"] == 1 and st["hybrid_tables"] == len(rows)) == hybrid, (tiles, st)
            if not hybrid:
                assert st["hybrid_launched"] == 0 and st["pairs_sorted"] == idx.numel(), (tiles, st)
            for t in range(len(rows)):
                assert np.array_equal(m.table(t).cpu().numpy(), exp[t]), (tiles, t)
    finally:
        param_amd.set_hybrid_min_tiles(0)               # (the module's setting)
