"""padding_idx and 2-D input on the GPU (``pytest -m gpu``), against the numpy restatement of the rule (tests/padding_rules.py).

Forward (``pm_embbag_fwd_padded``): every case bit-identical to the rule AND to the product forward on the request with the padded
lookups removed on the host; NaN stored in the padding rows reaches no output.  Backward: the guard (``pm_pad_rows_guard``) around
the unchanged sorted / hybrid bag-major / LDS left-over routes -- every row but the padding rows equals, bit for bit, what a second
module without ``padding_idx`` makes of the same request; the padding rows and their optimizer state keep their bits.  The sparse
gradient leaves the row out, the ``per_sample_weights`` gradient is +0.0 there, and a module without ``padding_idx`` reaches none
of the new entry points."""
import numpy as np
import pytest
import torch

from tests import padding_rules as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS, PADS, B0 = (50, 7, 1000), (3, None, 999), 37
NEW = ("pm_embbag_fwd_padded", "pm_embbag_pad_mask", "pm_pad_rows_guard_bytes", "pm_pad_rows_guard")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    import param_amd

    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    param_amd.load_library()
    param_amd.set_hybrid_min_tiles(0)      # the route tests drive the hybrid kernels with small requests
    yield
    param_amd.set_hybrid_min_tiles()
    param_amd.set_hybrid_tuning()
    param_amd.set_hybrid_rest()


def _bits(t):
    """the bits of a tensor / array of 4- or 2-byte elements as integers (numpy)"""
    if isinstance(t, torch.Tensor):
        t = t.detach().contiguous()
        return t.view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


def _model(rows, dims, pads=None, dtype=torch.float32, layout="bd", seed=0, **kw):
    import param_amd

    kw.setdefault("fused_update", False)
    return param_amd.BatchedEmbeddingBagMI355(list(rows), dims, dtype=dtype, device=DEV, init="normal", layout=layout, seed=seed,
                                              padding_idx=pads, **kw)


def _pair(rows, dims, pads, **kw):
    """a module with padding and one without, holding the same weights (the padding rows too: random, not zero)"""
    ref = _model(rows, dims, None, **kw)
    m = _model(rows, dims, pads, **kw)
    m.weights.data.copy_(ref.weights.data)
    return m, ref


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype=dtype)


def _split(out, dims, layout):
    """the module's output as a list of per-table [bags, D_t] arrays"""
    o = out.cpu().numpy()
    if layout == "tbd":
        return [o[t] for t in range(len(dims))]
    col = np.concatenate([[0], np.cumsum(dims)])
    return [o[:, col[t]:col[t + 1]] for t in range(len(dims))]


def _check_forward(rows, dims, pads, dtype, idt, weighted, fixed, layout, seed, max_len=9, B=B0, slice_=(5, 20)):
    rng = np.random.default_rng(seed)
    T = len(rows)
    dims_l = [dims] * T if isinstance(dims, int) else list(dims)
    m, ref = _pair(rows, dims_l, list(pads), dtype=dtype, layout=layout, seed=seed)
    idx_h, off_h = R.padded_request(rng, rows, B, pads, share=0.4, max_len=max_len, fixed=fixed)
    psw_h = rng.standard_normal(idx_h.size).astype(np.float32) if weighted else None
    idx, off, psw = _dev(idx_h, idt), _dev(off_h, idt), _dev(psw_h)
    tabs = [m.table(t).float().cpu().numpy() for t in range(T)]
    want = R.forward(tabs, idx_h, off_h, B, pads, psw_h)
    # 1. the rule, bit for bit
    out = m.lookup(idx, off, psw, batch=B)
    for t, (g, w) in enumerate(zip(_split(out, dims_l, layout), want)):
        assert np.array_equal(_bits(g), _bits(w)), ("rule", t)
    # 2. the product forward on the request with the padded lookups removed on the host
    fi, fo, fw = R.filtered_request(idx_h, off_h, T, B, pads, psw_h)
    if fi.size:
        prod = ref.lookup(_dev(fi, idt), _dev(fo, idt), _dev(fw), batch=B)
        assert np.array_equal(_bits(out), _bits(prod)), "product forward on the filtered request"
    # a bag slice writes its own rows only
    if slice_ is not None:
        b0, nb = slice_
        canvas = torch.full_like(out, 7.0)
        m.lookup(idx, off, psw, out=canvas, bag_begin=b0, bag_count=nb, batch=B)
        for t, (g, w) in enumerate(zip(_split(canvas, dims_l, layout), want)):
            assert np.array_equal(_bits(g[b0:b0 + nb]), _bits(w[b0:b0 + nb])), ("slice", t)
            assert (g[:b0] == 7.0).all() and (g[b0 + nb:] == 7.0).all()
    # NaN in the padding rows: finite and unchanged
    for t, k in enumerate(pads):
        if k is not None:
            m.table(t)[k] = float("nan")
    again = m.lookup(idx, off, psw, batch=B)
    assert torch.isfinite(again).all() and np.array_equal(_bits(again), _bits(out))


_DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.mark.parametrize("fixed", [None, 7], ids=["ragged", "fixed7"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("dtype", _DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("dims", [8, 16, 128, 256, (16, 128, 64)], ids=["d8", "d16", "d128", "d256", "mixed"])
def test_forward_equals_the_rule_and_the_filtered_product_forward(dims, dtype, weighted, fixed):
    """T = 3, rows (50, 7, 1000), pads (3, None, 999), B = 37: ragged bags of 0 .. 9 lookups and fixed L = 7; index dtype and layout
    alternate over the cases so that int32 / int64 and bd / tbd each meet every dtype, width and pooling kind"""
    case = _DTYPES.index(dtype) + 2 * int(weighted) + (fixed is not None) + (0 if isinstance(dims, tuple) else dims // 8)
    idt = torch.int32 if case % 2 else torch.int64
    layout = "tbd" if not isinstance(dims, tuple) and (case // 2) % 2 else "bd"
    _check_forward(ROWS, dims, PADS, dtype, idt, weighted, fixed, layout, seed=1000 + case)


@pytest.mark.parametrize("idt", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("layout", ["bd", "tbd"])
def test_forward_every_index_dtype_and_layout_at_one_shape(idt, layout):
    _check_forward(ROWS, 128, PADS, torch.float32, idt, True, None, layout, seed=77)
    _check_forward(ROWS, 64, PADS, torch.bfloat16, idt, False, 7, layout, seed=78)


def test_forward_more_than_one_tile_and_staged_ragged_tiles():
    """B = 300 bags per table: several tiles per table (the last one short), compacted in LDS"""
    _check_forward(ROWS, 128, PADS, torch.float32, torch.int64, True, None, "bd", seed=5, B=300, slice_=(33, 250))
    _check_forward(ROWS, 32, (0, 6, None), torch.float16, torch.int32, False, 20, "tbd", seed=6, B=300, slice_=(1, 299))


def test_forward_tiles_compacted_over_several_rounds():
    """tiles of more than 256 lookups: the compaction carries its running count from one round of 256 entries to the next
    (D = 32 fp16: 32 bags per tile, 1280 lookups = 5 rounds; D = 128 fp32: 8 bags, 320 lookups; ragged bags of up to 60)"""
    _check_forward(ROWS, 32, (0, 6, None), torch.float16, torch.int32, True, 40, "bd", seed=7, B=100, slice_=(3, 90))
    _check_forward(ROWS, 128, PADS, torch.float32, torch.int64, False, 40, "tbd", seed=8, B=100, slice_=None)
    _check_forward(ROWS, 32, PADS, torch.bfloat16, torch.int64, False, None, "bd", seed=9, max_len=60, B=100, slice_=(50, 50))


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_forward_bag_longer_than_the_lds_index_tile(weighted):
    """one table, one bag of 5000 lookups (the LDS index tile holds 4096) between two short ones: half of it padding, in a pattern
    that straddles the two-lookup batches and the tail"""
    rng = np.random.default_rng(31)
    rows, D, pad = 1000, 128, 17
    m, ref = _pair([rows], D, [pad], seed=4)
    long_ = rng.integers(0, rows, 5001)
    long_[long_ == pad] = 18
    long_[rng.random(5001) < 0.5] = pad
    long_[:6] = [pad, 5, pad, pad, 6, 7]              # batches (pad, keep), (pad, pad), (keep, keep)
    long_[-3:] = [8, pad, pad]                         # ... and a padded tail
    idx_h = np.concatenate([[1, pad, 2], long_, [pad, 3, 4, pad]]).astype(np.int64)
    off_h = np.array([0, 3, 3 + 5001, idx_h.size], dtype=np.int64)
    psw_h = rng.standard_normal(idx_h.size).astype(np.float32) if weighted else None
    out = m.lookup(_dev(idx_h), _dev(off_h), _dev(psw_h), batch=3)
    want = R.forward([m.table(0).cpu().numpy()], idx_h, off_h, 3, [pad], psw_h)[0]
    assert np.array_equal(_bits(out), _bits(want))
    fi, fo, fw = R.filtered_request(idx_h, off_h, 1, 3, [pad], psw_h)
    assert np.array_equal(_bits(out), _bits(ref.lookup(_dev(fi), _dev(fo), _dev(fw), batch=3)))
    m.table(0)[pad] = float("nan")
    assert np.array_equal(_bits(m.lookup(_dev(idx_h), _dev(off_h), _dev(psw_h), batch=3)), _bits(out))


def test_forward_request_of_padding_only_is_all_plus_zero():
    rows, pads, B, L = (9, 12), (0, 5), 19, 4
    m = _model(rows, 16, list(pads))
    idx = torch.cat([torch.full((B * L,), k, dtype=torch.int64, device=DEV) for k in pads])
    off = torch.arange(2 * B + 1, dtype=torch.int64, device=DEV) * L
    for t, k in enumerate(pads):
        m.table(t)[k] = float("inf")
    out = torch.full((B, 32), 7.0, device=DEV)
    m.lookup(idx, off, out=out)
    assert (_bits(out) == 0).all()
    psw = torch.randn(idx.numel(), device=DEV)
    assert (_bits(m.lookup(idx, off, psw)) == 0).all()


def test_modules_zero_fill_the_padding_rows_they_create():
    import param_amd

    for init in ("normal", "uniform_dlrm"):
        m = param_amd.BatchedEmbeddingBagMI355(list(ROWS), [16, 128, 64], device=DEV, init=init, padding_idx=list(PADS))
        for t, k in enumerate(PADS):
            w = m.table(t)
            assert (w != 0).any(dim=1).sum().item() == ROWS[t] - (k is not None)
            assert k is None or (_bits(w[k]) == 0).all()
    keep = torch.ones(10, 8, device=DEV)
    assert (param_amd.EmbeddingBagMI355(10, 8, device=DEV, _weight=keep, padding_idx=2).weight == 1).all()


# ---- 2-D input -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pad", [None, 5, -1])
def test_two_d_input_equals_the_one_d_call(pad):
    import param_amd

    n, D, B, L = 40, 32, 64, 7
    g = torch.Generator(device=DEV).manual_seed(3)
    m = param_amd.EmbeddingBagMI355(n, D, device=DEV, padding_idx=pad)
    inp = torch.randint(0, n, (B, L), device=DEV, generator=g)
    if pad is not None:
        assert (_bits(m.weight[m.padding_idx]) == 0).all()                  # module-made weights: the row starts as zeros
        inp[torch.rand(B, L, device=DEV, generator=g) < 0.4] = m.padding_idx
        with torch.no_grad():
            m.weight[m.padding_idx] = float("nan")
    off = torch.arange(B, device=DEV) * L
    psw = torch.randn(B, L, device=DEV, generator=g)
    with torch.no_grad():
        assert np.array_equal(_bits(m(inp)), _bits(m(inp.reshape(-1), off)))
        assert np.array_equal(_bits(m(inp, per_sample_weights=psw)), _bits(m(inp.reshape(-1), off, psw.reshape(-1))))
        assert torch.isfinite(m(inp)).all()
        assert m(inp.to(torch.int32)).shape == (B, D) and len(m._off2d) == 2 and m(inp) is not None and len(m._off2d) == 2
    with pytest.raises(ValueError, match="^if input is 2D, then offsets has to be None"):
        m(inp, off)
    # autograd: the per_sample_weights gradient comes back in the input's shape and equals the 1-D call's
    if pad is not None:
        with torch.no_grad():
            m.weight[m.padding_idx] = 0.5
    gout = torch.randn(B, D, device=DEV, generator=g)
    w2 = psw.clone().requires_grad_(True)
    m(inp, per_sample_weights=w2).backward(gout)
    dW2, m.weight.grad = m.weight.grad.clone(), None
    w1 = psw.reshape(-1).clone().requires_grad_(True)
    m(inp.reshape(-1), off, w1).backward(gout)
    assert w2.grad.shape == (B, L) and np.array_equal(_bits(w2.grad.reshape(-1)), _bits(w1.grad))
    assert np.array_equal(_bits(dW2), _bits(m.weight.grad))
    if pad is not None:
        assert (_bits(dW2[m.padding_idx]) == 0).all() and (_bits(w2.grad[inp == m.padding_idx]) == 0).all()
        assert (dW2 != 0).any()


# ---- backward: the guard around every route --------------------------------------------------------------------------------------

BW_ROWS, BW_PADS, BW_B, BW_L, BW_D = (100_000, 70_000, 100_000), (3, None, 99_999), 1024, 8, 32
ROUTES = {"sorted": (0, 1), "bag_major": (2, 0), "lds_rest": (2, 1)}          # pm_set_hybrid_tuning(enable), pm_set_hybrid_rest(mode)


def _bw_request(seed=9, weighted=False):
    rng = np.random.default_rng(seed)
    idx_h, off_h = R.padded_request(rng, BW_ROWS, BW_B, BW_PADS, share=0.3, fixed=BW_L)
    psw_h = rng.standard_normal(idx_h.size).astype(np.float32) if weighted else None
    grad = torch.randn(BW_B, len(BW_ROWS) * BW_D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    return idx_h, off_h, psw_h, _dev(idx_h), _dev(off_h), _dev(psw_h), grad


def _assert_guarded(m, ref, before_w, before_s, pads):
    """every row but the padding rows: the reference module's bits; the padding rows (and their state): their earlier bits"""
    for t, k in enumerate(pads):
        got, want = _bits(m.table(t)), _bits(ref.table(t))
        keep = np.ones(got.shape[0], dtype=bool)
        if k is not None:
            keep[k] = False
            assert np.array_equal(got[k], before_w[t][k]), ("padding row moved", t)
            assert not np.array_equal(want[k], before_w[t][k]), ("the unguarded step does move it", t)
        assert np.array_equal(got[keep], want[keep]), ("other rows", t)
        if before_s is not None:
            gs, ws = _bits(m.momentum_table(t)), _bits(ref.momentum_table(t))
            if k is not None:
                assert np.array_equal(gs[k], before_s[t][k]), ("padding row's state moved", t)
                assert not np.array_equal(ws[k], before_s[t][k]), t
            assert np.array_equal(gs[keep], ws[keep]), ("other rows' state", t)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("opt", ["sgd", "rowwise_adagrad", "adagrad_l2", "adagrad_bf16_sr"])
def test_fused_step_leaves_padding_rows_and_state_alone_on_every_route(route, opt):
    import param_amd

    hyb, rest = ROUTES[route]
    param_amd.set_hybrid_tuning(hyb)
    param_amd.set_hybrid_rest(rest)
    kw = {"sgd": dict(optimizer="sgd"), "rowwise_adagrad": dict(optimizer="rowwise_adagrad", weight_decay=0.01, weight_decay_mode="decouple"),
          "adagrad_l2": dict(optimizer="adagrad", weight_decay=0.01, weight_decay_mode="l2"),
          "adagrad_bf16_sr": dict(optimizer="adagrad", dtype=torch.bfloat16, stochastic_rounding=True)}[opt]
    _, _, _, idx, off, _, grad = _bw_request()
    m, ref = _pair(BW_ROWS, BW_D, list(BW_PADS), learning_rate=0.05, seed=2, **kw)
    before_s = None
    if opt != "sgd":
        ref.momentum_table(0), m.momentum_table(0)
        ref.momentum.uniform_(0.1, 1.0)
        m.momentum.copy_(ref.momentum)
        before_s = [_bits(m.momentum_table(t)).copy() for t in range(3)]
    before_w = [_bits(m.table(t)).copy() for t in range(3)]
    for mod in (m, ref):
        mod.optimizer_step_(grad, idx, off, batch=BW_B)
    st = ref.sort_status(idx, off, batch=BW_B)
    if route == "sorted":
        assert st["hybrid_tables"] == 0 and st["pairs_sorted"] == idx.numel(), st
    else:
        assert st["hybrid_tables"] == 3 and st["lds_tables"] == (3 if route == "lds_rest" else 0), st
    _assert_guarded(m, ref, before_w, before_s, BW_PADS)


def test_weighted_autograd_step_of_the_batched_module():
    """fused_update through ``.backward()``: the tables as above, and the per_sample_weights gradient +0.0 at the padded lookups,
    the unpadded module's bits elsewhere"""
    import param_amd

    param_amd.set_hybrid_tuning()
    param_amd.set_hybrid_rest()
    idx_h, off_h, psw_h, idx, off, psw, grad = _bw_request(seed=12, weighted=True)
    m, ref = _pair(BW_ROWS, BW_D, list(BW_PADS), learning_rate=0.05, seed=3, fused_update=True, optimizer="rowwise_adagrad")
    before_w = [_bits(m.table(t)).copy() for t in range(3)]
    ref.momentum_table(0), m.momentum_table(0)
    before_s = [_bits(m.momentum_table(t)).copy() for t in range(3)]
    grads = []
    for mod in (m, ref):
        w = psw.clone().requires_grad_(True)
        mod(idx, off, w).backward(grad)
        grads.append(w.grad)
    skip = R.padded_mask(idx_h, off_h, 3, BW_B, BW_PADS)
    got, want = _bits(grads[0]), _bits(grads[1])
    assert skip.any() and (got[skip] == 0).all() and np.array_equal(got[~skip], want[~skip]) and (want[skip] != 0).any()
    for t, k in enumerate(BW_PADS):                        # (fresh state is zero: the unguarded step is told apart by the tables)
        if k is not None:
            assert np.array_equal(_bits(m.momentum_table(t))[k], before_s[t][k])
    _assert_guarded(m, ref, before_w, None, BW_PADS)


def test_dense_grad_keeps_the_pattern_in_padding_rows():
    import param_amd

    param_amd.set_hybrid_tuning()
    param_amd.set_hybrid_rest()
    rng = np.random.default_rng(21)
    dims = [16, 128, 64]
    m, ref = _pair(ROWS, dims, list(PADS), seed=5)
    idx_h, off_h = R.padded_request(rng, ROWS, B0, PADS)
    psw_h = rng.standard_normal(idx_h.size).astype(np.float32)
    idx, off, psw = _dev(idx_h), _dev(off_h), _dev(psw_h)
    grad = torch.randn(B0, sum(dims), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    pattern = [torch.full((r, d), 3.25, device=DEV) for r, d in zip(ROWS, dims)]
    got = m.dense_grad(grad, idx, off, psw, batch=B0, out=[p.clone() for p in pattern])
    want = ref.dense_grad(grad, idx, off, psw, batch=B0, out=[p.clone() for p in pattern])
    fresh = m.dense_grad(grad, idx, off, psw, batch=B0)
    col = np.concatenate([[0], np.cumsum(dims)])
    rule = R.dense_grad(ROWS, dims, idx_h, off_h, B0, PADS, [grad.cpu().numpy()[:, col[t]:col[t + 1]] for t in range(3)], psw_h)
    for t, k in enumerate(PADS):
        keep = np.ones(ROWS[t], dtype=bool)
        if k is not None:
            keep[k] = False
            assert (got[t][k] == 3.25).all() and (want[t][k] != 3.25).any() and (_bits(fresh[t][k]) == 0).all()
        assert np.array_equal(_bits(got[t])[keep], _bits(want[t])[keep])
        np.testing.assert_allclose(fresh[t].cpu().numpy(), rule[t], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_sparse_gradient_leaves_the_padding_row_out(weighted):
    import param_amd

    rng = np.random.default_rng(41)
    n, D, B, pad = 60, 32, 50, 7
    idx_h, off_h = R.padded_request(rng, [n], B, [pad], closed=False)
    idx, off = _dev(idx_h), _dev(off_h)
    psw = torch.randn(idx.numel(), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)) if weighted else None
    gout = torch.randn(B, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    m = param_amd.EmbeddingBagMI355(n, D, device=DEV, sparse=True, padding_idx=pad)
    ref = param_amd.EmbeddingBagMI355(n, D, device=DEV, sparse=True, _weight=m.weight.detach().clone())
    with torch.no_grad():
        m.weight[pad] = 0.75
        ref.weight[pad] = 0.75
    for mod in (m, ref):
        mod(idx, off, psw).backward(gout)
    g, gr = m.weight.grad, ref.weight.grad
    assert g.is_sparse and g.is_coalesced()
    rows = g._indices()[0].cpu().numpy()
    assert rows.tolist() == R.sparse_rows(idx_h, off_h, 1, B, [pad])[0].tolist() and pad not in rows.tolist()
    rr = gr._indices()[0].cpu().numpy()
    assert pad in rr.tolist()
    assert np.array_equal(_bits(g._values()), _bits(gr._values())[rr != pad])
    before = m.weight.detach().clone()
    torch.optim.SGD([m.weight], lr=0.1).step()
    assert np.array_equal(_bits(m.weight[pad]), _bits(before[pad])) and not torch.equal(m.weight[rows[0]], before[rows[0]])
    # the batched module's sparse_grad, per-table pads
    bm, bref = _pair(ROWS, 16, list(PADS), seed=8)
    bi_h, bo_h = R.padded_request(rng, ROWS, B0, PADS)
    bg = torch.randn(B0, 48, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    got, want = bm.sparse_grad(bg, _dev(bi_h), _dev(bo_h), batch=B0), bref.sparse_grad(bg, _dev(bi_h), _dev(bo_h), batch=B0)
    for t, ((r, v), (r0, v0), rule) in enumerate(zip(got, want, R.sparse_rows(bi_h, bo_h, 3, B0, PADS))):
        assert r.cpu().numpy().tolist() == rule.tolist(), t
        keep = (r0 != (-1 if PADS[t] is None else PADS[t])).cpu().numpy()
        assert np.array_equal(_bits(v), _bits(v0)[keep]), t


def test_guard_around_the_table_chunks_of_1100_tables():
    T, n, D, B, L = 1100, 16, 8, 4, 3
    rows = [n] * T
    pads = [1 if t % 3 else None for t in range(T)]
    rng = np.random.default_rng(51)
    idx_h, off_h = R.padded_request(rng, rows, B, pads, fixed=L)
    idx, off = _dev(idx_h), _dev(off_h)
    grad = torch.randn(B, T * D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    m, ref = _pair(rows, D, pads, learning_rate=0.1, seed=6)
    before = m.weights.data.clone()
    for mod in (m, ref):
        mod.optimizer_step_(grad, idx, off, batch=B)
    got = _bits(m.weights.data).reshape(T, n, D)
    want, was = _bits(ref.weights.data).reshape(T, n, D), _bits(before).reshape(T, n, D)
    padded = np.array([k is not None for k in pads])
    assert np.array_equal(got[padded, 1], was[padded, 1]) and not np.array_equal(want[padded, 1], was[padded, 1])
    assert np.array_equal(got[~padded], want[~padded])
    assert np.array_equal(np.delete(got, 1, axis=1), np.delete(want, 1, axis=1))
    assert (R.padded_mask(idx_h, off_h, T, B, pads).reshape(T, -1).sum(axis=1)[[1, 1025, 1099]] > 0).all()      # both chunks see padding


# ---- per_sample_weights gradient ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,idt", [(torch.float32, torch.int64), (torch.bfloat16, torch.int32)])
def test_psw_gradient_is_plus_zero_at_padded_lookups(dtype, idt):
    import param_amd

    rng = np.random.default_rng(61)
    dims = [16, 128, 64]
    m, ref = _pair(ROWS, dims, list(PADS), dtype=dtype, seed=7)
    idx_h, off_h = R.padded_request(rng, ROWS, B0, PADS)
    idx, off = _dev(idx_h, idt), _dev(off_h, idt)
    grad = torch.randn(B0, sum(dims), device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))
    raw = ref.per_sample_weights_grad(grad, idx, off, batch=B0)
    got = m.per_sample_weights_grad(grad, idx, off, batch=B0)
    assert np.array_equal(_bits(got), _bits(R.psw_grad_mask(raw.cpu().numpy(), idx_h, off_h, 3, B0, PADS)))
    skip = R.padded_mask(idx_h, off_h, 3, B0, PADS)
    assert skip.any() and (_bits(got)[skip] == 0).all() and (_bits(raw)[skip] != 0).any()
    # a bag slice into the caller's buffer: entries outside the slice are not touched, padded or not
    canvas = torch.full((idx.numel(),), 7.0, device=DEV)
    m.per_sample_weights_grad(grad, idx, off, batch=B0, out=canvas, bag_begin=5, bag_count=20)
    want = torch.full((idx.numel(),), 7.0, device=DEV)
    ref.per_sample_weights_grad(grad, idx, off, batch=B0, out=want, bag_begin=5, bag_count=20)
    assert np.array_equal(_bits(canvas), _bits(R.psw_grad_mask(want.cpu().numpy(), idx_h, off_h, 3, B0, PADS, 5, 20)))
    # autograd of the single-table module (dense gradient)
    if dtype == torch.float32:
        k, n = 4, 30
        sm = param_amd.EmbeddingBagMI355(n, 32, device=DEV, padding_idx=k)
        sref = param_amd.EmbeddingBagMI355(n, 32, device=DEV, _weight=sm.weight.detach().clone())
        with torch.no_grad():
            sm.weight[k] = 1.5
            sref.weight[k] = 1.5
        si_h, so_h = R.padded_request(rng, [n], B0, [k], closed=False)
        gout = torch.randn(B0, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
        res = []
        for mod in (sm, sref):
            w = torch.ones(si_h.size, device=DEV).requires_grad_(True)
            mod(_dev(si_h), _dev(so_h), w).backward(gout)
            res.append((w.grad, mod.weight.grad))
        sk = R.padded_mask(si_h, so_h, 1, B0, [k])
        assert (_bits(res[0][0])[sk] == 0).all() and np.array_equal(_bits(res[0][0])[~sk], _bits(res[1][0])[~sk])
        assert (_bits(res[0][1][k]) == 0).all() and (res[1][1][k] != 0).any()
        assert np.array_equal(np.delete(_bits(res[0][1]), k, axis=0), np.delete(_bits(res[1][1]), k, axis=0))


# ---- the default path ---------------------------------------------------------------------------------------------------------

def test_modules_without_padding_idx_reach_none_of_the_new_entry_points(monkeypatch):
    import param_amd
    from param_amd import _lib

    real = _lib.load()
    calls = []

    class Counting:
        def __getattr__(self, name):
            if name in NEW:
                calls.append(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "load", lambda: Counting())
    rng = np.random.default_rng(71)
    idx_h, off_h = R.padded_request(rng, ROWS, B0, PADS)
    idx, off = _dev(idx_h), _dev(off_h)
    psw = torch.randn(idx.numel(), device=DEV).requires_grad_(True)
    grad = torch.randn(B0, 48, device=DEV)
    for opt in ("sgd", "rowwise_adagrad", "adagrad"):
        m = _model(ROWS, 16, None, optimizer=opt, fused_update=True)
        m(idx, off, psw).backward(grad)
        m.lookup(idx, off)
        m.dense_grad(grad, idx, off)
        m.sparse_grad(grad, idx, off)
        m.per_sample_weights_grad(grad, idx, off)
    s = param_amd.EmbeddingBagMI355(50, 16, device=DEV)
    s(idx[:off_h[B0]], off[:B0], psw[:off_h[B0]]).backward(grad[:, :16])
    s(torch.randint(0, 50, (8, 5), device=DEV)).sum().backward()
    torch.cuda.synchronize()
    assert calls == []
    # ... and a module with one does
    p = _model(ROWS, 16, list(PADS), fused_update=True)
    p(idx, off, psw).backward(grad)
    assert {"pm_embbag_fwd_padded", "pm_pad_rows_guard", "pm_embbag_pad_mask"} <= set(calls)
