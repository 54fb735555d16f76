"""Mean pooling on the GPU (``pytest -m gpu``), against the numpy restatement of the rule (tests/mean_rules.py).

Forward (``pm_embbag_fwd_mean``): every case bit-identical to the rule, and a padded request also to the mean forward of the request
with the padded lookups removed on the host.  Backward: ``pm_embbag_mean_grad`` equals ``scale_grad`` bit for bit, and a mean module's
``optimizer_step_(g)`` / ``scatter_add_`` / ``dense_grad`` / ``sparse_grad`` leave exactly what a sum module makes of the gradient scaled
on the host -- on the sorted, the hybrid bag-major and the LDS left-over route, for every optimizer.  ``EmbeddingBagMI355(mode="mean")``
autograd, dense and sparse, equals the rule bit for bit.  A sum-mode module reaches neither new entry point."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mean_rules as M
from tests import padding_rules as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS, PADS, B0 = (50, 7, 1000), (3, None, 999), 37
NONE3 = (None, None, None)
NEW = ("pm_embbag_fwd_mean", "pm_embbag_mean_grad")


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


def _model(rows, dims, pads=None, mode="mean", dtype=torch.float32, layout="bd", seed=0, **kw):
    import param_amd

    kw.setdefault("fused_update", False)
    pads = None if pads is None or all(k is None for k in pads) else list(pads)
    return param_amd.BatchedEmbeddingBagMI355(list(rows), dims, dtype=dtype, device=DEV, init="normal", layout=layout, seed=seed,
                                              padding_idx=pads, pooling_mode=mode, **kw)


def _pair(rows, dims, pads, **kw):
    """a mean module and a sum module with the same padding rows, holding the same weights (the padding rows too: random, not zero)"""
    ref = _model(rows, dims, None, "sum", **kw)
    m = _model(rows, dims, pads, "mean", **kw)
    s = _model(rows, dims, pads, "sum", **kw)
    for mod in (m, s):
        mod.weights.data.copy_(ref.weights.data)
    return m, s


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype=dtype)


def _split(out, dims, layout):
    """a tensor in the module's output layout as a list of per-table [bags, D_t] arrays"""
    o = out.detach().cpu().numpy()
    if layout == "tbd":
        return [o[t] for t in range(len(dims))]
    col = np.concatenate([[0], np.cumsum(dims)])
    return [o[:, col[t]:col[t + 1]] for t in range(len(dims))]


def _join(parts, layout):
    """the inverse of _split, on the device"""
    return _dev(np.stack(parts) if layout == "tbd" else np.concatenate(parts, axis=1))


def _scaled(grad, dims, layout, idx_h, off_h, B, pads):
    """``scale_grad`` of a gradient tensor in the module's layout, computed on the host"""
    return _join(M.scale_grad(_split(grad, dims, layout), idx_h, off_h, B, pads), layout)


def _check_forward(rows, dims, pads, dtype, idt, fixed, layout, seed, max_len=9, B=B0, slice_=(5, 20)):
    rng = np.random.default_rng(seed)
    T = len(rows)
    dims_l = [dims] * T if isinstance(dims, int) else list(dims)
    m, _ = _pair(rows, dims_l, pads, dtype=dtype, layout=layout, seed=seed)
    idx_h, off_h = R.padded_request(rng, rows, B, pads, share=0.4, max_len=max_len, fixed=fixed)
    if fixed is None:
        assert (np.diff(off_h) == 0).any() and (np.diff(off_h) == 1).any()      # empty and one-lookup bags
    idx, off = _dev(idx_h, idt), _dev(off_h, idt)
    tabs = [m.table(t).float().cpu().numpy() for t in range(T)]
    want = M.forward(tabs, idx_h, off_h, B, pads)
    # 1. the rule, bit for bit
    out = m.lookup(idx, off, batch=B)
    for t, (g, w) in enumerate(zip(_split(out, dims_l, layout), want)):
        assert np.array_equal(_bits(g), _bits(w)), ("rule", t)
    # 2. a padded request: the mean forward (no pad array) of the request with the padded lookups removed on the host
    if any(k is not None for k in pads):
        plain = _model(rows, dims_l, None, "mean", dtype=dtype, layout=layout, seed=seed)
        plain.weights.data.copy_(m.weights.data)
        fi, fo, _ = R.filtered_request(idx_h, off_h, T, B, pads)
        assert np.array_equal(_bits(out), _bits(plain.lookup(_dev(fi, idt), _dev(fo, idt), batch=B))), "filtered request"
    # a bag slice writes its own rows only
    if slice_ is not None:
        b0, nb = slice_
        canvas = torch.full_like(out, 7.0)
        m.lookup(idx, off, out=canvas, bag_begin=b0, bag_count=nb, batch=B)
        for t, (g, w) in enumerate(zip(_split(canvas, dims_l, layout), want)):
            assert np.array_equal(_bits(g[b0:b0 + nb]), _bits(w[b0:b0 + nb])), ("slice", t)
            assert (g[:b0] == 7.0).all() and (g[b0 + nb:] == 7.0).all()
    # NaN in the padding rows: finite and unchanged
    if any(k is not None for k in pads):
        for t, k in enumerate(pads):
            if k is not None:
                m.table(t)[k] = float("nan")
        again = m.lookup(idx, off, batch=B)
        assert torch.isfinite(again).all() and np.array_equal(_bits(again), _bits(out))


_DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.mark.parametrize("padded", [False, True], ids=["nopad", "padded"])
@pytest.mark.parametrize("fixed", [None, 7], ids=["ragged", "fixed7"])
@pytest.mark.parametrize("dtype", _DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("dims", [8, 16, 128, 256, (16, 128, 64)], ids=["d8", "d16", "d128", "d256", "mixed"])
def test_forward_equals_the_rule(dims, dtype, fixed, padded):
    """T = 3, rows (50, 7, 1000), B = 37 with the slice (5, 20): ragged bags of 0 .. 9 lookups and fixed L = 7, with pads
    (3, None, 999) and without; index dtype and layout alternate over the cases so that int32 / int64 and bd / tbd each meet every
    dtype, width and pooling kind"""
    case = _DTYPES.index(dtype) + 2 * int(padded) + (fixed is not None) + (0 if isinstance(dims, tuple) else dims // 8)
    idt = torch.int32 if case % 2 else torch.int64
    layout = "tbd" if not isinstance(dims, tuple) and (case // 2) % 2 else "bd"
    _check_forward(ROWS, dims, PADS if padded else NONE3, dtype, idt, fixed, layout, seed=2000 + case)


@pytest.mark.parametrize("idt", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("layout", ["bd", "tbd"])
def test_forward_every_index_dtype_and_layout_at_one_shape(idt, layout):
    _check_forward(ROWS, 128, PADS, torch.float32, idt, None, layout, seed=77)
    _check_forward(ROWS, 64, NONE3, torch.bfloat16, idt, 7, layout, seed=78)


def test_forward_more_than_one_tile_and_tiles_compacted_over_several_rounds():
    """B = 300: several tiles per table, the last one short.  Tiles of more than 256 lookups: the compaction carries its running
    count over rounds of 256 entries (D = 32 fp16: 32 bags per tile, 1280 lookups = 5 rounds; ragged bags of up to 60)"""
    _check_forward(ROWS, 128, PADS, torch.float32, torch.int64, None, "bd", seed=5, B=300, slice_=(33, 250))
    _check_forward(ROWS, 32, (0, 6, None), torch.float16, torch.int32, 40, "bd", seed=7, B=100, slice_=(3, 90))
    _check_forward(ROWS, 32, NONE3, torch.bfloat16, torch.int64, None, "tbd", seed=9, max_len=60, B=100, slice_=(50, 50))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("padded", [False, True], ids=["nopad", "padded"])
def test_forward_bag_longer_than_the_lds_index_tile(padded, dtype):
    """the 7-row table, one bag of 5000 lookups (the LDS index tile holds at most 4096) between two short ones: the kept lookups are
    counted along the walk; padded, half of it is padding in a pattern that straddles the two-lookup batches and the tail"""
    rng = np.random.default_rng(31)
    rows, D, pad = 7, 128, (3 if padded else None)
    m = _model([rows], D, [pad], "mean", dtype=dtype, seed=4)
    long_ = rng.integers(0, rows, 5000)
    if padded:
        long_[long_ == pad] = 4
        long_[rng.random(5000) < 0.5] = pad
        long_[:6] = [pad, 5, pad, pad, 6, 0]
        long_[-3:] = [1, pad, pad]
    edge = 3 if padded else 2
    idx_h = np.concatenate([[1, edge, 2], long_, [edge, 5, 4, edge]]).astype(np.int64)
    off_h = np.array([0, 3, 3 + 5000, idx_h.size], dtype=np.int64)
    out = m.lookup(_dev(idx_h), _dev(off_h), batch=3)
    want = M.forward([m.table(0).float().cpu().numpy()], idx_h, off_h, 3, [pad])[0]
    n = M.count(idx_h, off_h, 1, 3, [pad])
    assert n[1] == (5000 if not padded else int((long_ != pad).sum())) and 2000 < n[1] <= 5000
    assert np.array_equal(_bits(out), _bits(want))
    if padded:
        fi, fo, _ = R.filtered_request(idx_h, off_h, 1, 3, [pad])
        plain = _model([rows], D, None, "mean", dtype=dtype, seed=4)
        assert np.array_equal(_bits(out), _bits(plain.lookup(_dev(fi), _dev(fo), batch=3)))
        m.table(0)[pad] = float("nan")
        assert np.array_equal(_bits(m.lookup(_dev(idx_h), _dev(off_h), batch=3)), _bits(out))


def test_forward_request_of_padding_only_is_all_plus_zero():
    rows, pads, B, L = (9, 12), (0, 5), 19, 4
    m = _model(rows, 16, pads, "mean")
    idx = torch.cat([torch.full((B * L,), k, dtype=torch.int64, device=DEV) for k in pads])
    off = torch.arange(2 * B + 1, dtype=torch.int64, device=DEV) * L
    for t, k in enumerate(pads):
        m.table(t)[k] = float("inf")
    out = torch.full((B, 32), 7.0, device=DEV)
    m.lookup(idx, off, out=out)
    assert (_bits(out) == 0).all()


@pytest.mark.parametrize("pad", [None, 5, -1])
def test_two_d_input_equals_the_one_d_call(pad):
    import param_amd

    n, D, B, L = 40, 32, 64, 7
    g = torch.Generator(device=DEV).manual_seed(3)
    m = param_amd.EmbeddingBagMI355(n, D, mode="mean", device=DEV, padding_idx=pad)
    inp = torch.randint(0, n, (B, L), device=DEV, generator=g)
    if pad is not None:
        inp[torch.rand(B, L, device=DEV, generator=g) < 0.4] = m.padding_idx
        with torch.no_grad():
            m.weight[m.padding_idx] = float("nan")
    off = torch.arange(B, device=DEV) * L
    with torch.no_grad():
        out = m(inp)
        assert np.array_equal(_bits(out), _bits(m(inp.reshape(-1), off))) and torch.isfinite(out).all()
        assert np.array_equal(_bits(m(inp.to(torch.int32))), _bits(out))
    want = M.forward([m.weight.detach().cpu().numpy()], inp.reshape(-1).cpu().numpy(), off.cpu().numpy(), B, [m.padding_idx])[0]
    assert np.array_equal(_bits(out), _bits(want))
    with pytest.raises(NotImplementedError, match="per_sample_weights is only supported for mode='sum'"):
        m(inp, per_sample_weights=torch.ones(B, L, device=DEV))


# ---- the scaling kernel on its own ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,dims,idt", [("bd", (16, 128, 64), torch.int64), ("tbd", 8, torch.int32), ("bd", 512, torch.int64)],
                         ids=["bd-mixed", "tbd-d8", "bd-d512"])
@pytest.mark.parametrize("padded", [False, True], ids=["nopad", "padded"])
def test_mean_grad_equals_scale_grad_and_a_slice_leaves_the_rest_alone(layout, dims, idt, padded):
    from param_amd import _lib
    from param_amd.embedding_bag import _mean_scale, _stream_ptr

    rng = np.random.default_rng(11)
    pads = PADS if padded else NONE3
    dims_l = [dims] * 3 if isinstance(dims, int) else list(dims)
    m = _model(ROWS, dims_l, pads, "mean", layout=layout)
    idx_h, off_h = R.padded_request(rng, ROWS, B0, pads, share=0.4, max_len=70)      # bags longer than a lane group
    idx, off = _dev(idx_h, idt), _dev(off_h, idt)
    shape = (3, B0, dims_l[0]) if layout == "tbd" else (B0, sum(dims_l))
    grad = torch.randn(shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    grad.view(-1)[::97] = float("inf")
    grad.view(-1)[5::101] = -0.0
    keep = grad.clone()
    ts = m._tables()
    got = _mean_scale(ts, grad, idx, off, B0, m._pad_dev())
    want = _scaled(grad, dims_l, layout, idx_h, off_h, B0, pads)
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(grad), _bits(keep))
    n = M.count(idx_h, off_h, 3, B0, pads)
    assert (n == 0).any() and (n > 64).any()
    # a slice: only its bags are written
    b0, nb = 5, 20
    canvas = torch.full(shape, 7.0, device=DEV)
    op = ts.request(idx, off, B0, None, b0, nb)
    pad_t = m._pad_dev()
    rc = _lib.load().pm_embbag_mean_grad(ctypes.byref(op), None if pad_t is None else pad_t.data_ptr(), grad.data_ptr(),
                                         canvas.data_ptr(), _stream_ptr())
    assert rc == _lib.PM_OK
    for t, (c, w) in enumerate(zip(_split(canvas, dims_l, layout), _split(want, dims_l, layout))):
        assert np.array_equal(_bits(c[b0:b0 + nb]), _bits(w[b0:b0 + nb])), t
        assert (c[:b0] == 7.0).all() and (c[b0 + nb:] == 7.0).all()


# ---- backward: the scaled gradient through every route ------------------------------------------------------------------------------

BW_ROWS, BW_PADS, BW_B, BW_L, BW_D = (100_000, 70_000, 100_000), (3, None, 99_999), 1024, 8, 32
ROUTES = {"sorted": (0, 1), "bag_major": (2, 0), "lds_rest": (2, 1)}          # pm_set_hybrid_tuning(enable), pm_set_hybrid_rest(mode)
_BW = {}


def _bw_request():
    """the route tests' request and its host-scaled gradient, computed once and left unchanged"""
    if not _BW:
        rng = np.random.default_rng(9)
        idx_h, off_h = R.padded_request(rng, BW_ROWS, BW_B, BW_PADS, share=0.3, fixed=BW_L)
        grad = torch.randn(BW_B, len(BW_ROWS) * BW_D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
        _BW["r"] = (idx_h, off_h, _dev(idx_h), _dev(off_h), grad, _scaled(grad, [BW_D] * 3, "bd", idx_h, off_h, BW_B, BW_PADS))
    return _BW["r"]


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("opt", ["sgd", "rowwise_adagrad", "adagrad_l2", "adagrad_bf16_sr"])
def test_optimizer_step_equals_the_sum_step_on_the_scaled_gradient_on_every_route(route, opt):
    import param_amd

    hyb, rest = ROUTES[route]
    param_amd.set_hybrid_tuning(hyb)
    param_amd.set_hybrid_rest(rest)
    kw = {"sgd": dict(optimizer="sgd"), "rowwise_adagrad": dict(optimizer="rowwise_adagrad", weight_decay=0.01, weight_decay_mode="decouple"),
          "adagrad_l2": dict(optimizer="adagrad", weight_decay=0.01, weight_decay_mode="l2"),
          "adagrad_bf16_sr": dict(optimizer="adagrad", dtype=torch.bfloat16, stochastic_rounding=True)}[opt]
    _, _, idx, off, grad, scaled = _bw_request()
    keep = grad.clone()
    m, s = _pair(BW_ROWS, BW_D, BW_PADS, learning_rate=0.05, seed=2, **kw)
    if opt != "sgd":
        s.momentum_table(0), m.momentum_table(0)
        s.momentum.uniform_(0.1, 1.0)
        m.momentum.copy_(s.momentum)
    before = m.weights.data.clone()
    m.optimizer_step_(grad, idx, off, batch=BW_B)
    s.optimizer_step_(scaled, idx, off, batch=BW_B)
    st = m.sort_status(idx, off, batch=BW_B)
    if route == "sorted":
        assert st["hybrid_tables"] == 0 and st["pairs_sorted"] == idx.numel(), st
    else:
        assert st["hybrid_tables"] == 3 and st["lds_tables"] == (3 if route == "lds_rest" else 0), st
    assert np.array_equal(_bits(m.weights.data), _bits(s.weights.data)) and not torch.equal(m.weights.data, before)
    if opt != "sgd":
        assert np.array_equal(_bits(m.momentum), _bits(s.momentum))
    assert np.array_equal(_bits(grad), _bits(keep))                          # the caller's gradient is never modified


def test_fused_backward_of_the_batched_module():
    """``.backward()`` through autograd with fused_update: the tables a sum module's fused backward makes of the scaled gradient"""
    import param_amd

    param_amd.set_hybrid_tuning()
    param_amd.set_hybrid_rest()
    _, _, idx, off, grad, scaled = _bw_request()
    m, s = _pair(BW_ROWS, BW_D, BW_PADS, learning_rate=0.05, seed=3, fused_update=True, optimizer="rowwise_adagrad")
    keep = grad.clone()
    m(idx, off).backward(grad)
    s(idx, off).backward(scaled)
    assert np.array_equal(_bits(m.weights.data), _bits(s.weights.data)) and np.array_equal(_bits(m.momentum), _bits(s.momentum))
    assert np.array_equal(_bits(grad), _bits(keep))


@pytest.mark.parametrize("layout", ["bd", "tbd"])
def test_scatter_add_dense_grad_sparse_grad_and_a_batch_slice(layout):
    import param_amd

    param_amd.set_hybrid_tuning()
    param_amd.set_hybrid_rest()
    rng = np.random.default_rng(21)
    dims = [16, 128, 64] if layout == "bd" else [32] * 3
    m, s = _pair(ROWS, dims, PADS, seed=5, layout=layout)
    idx_h, off_h = R.padded_request(rng, ROWS, B0, PADS)
    idx, off = _dev(idx_h), _dev(off_h)
    shape = (3, B0, 32) if layout == "tbd" else (B0, sum(dims))
    grad = torch.randn(shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    scaled = _scaled(grad, dims, layout, idx_h, off_h, B0, PADS)
    gparts = _split(grad, dims, layout)
    # dense_grad: the sum module on the scaled gradient, and the rule (a sequential fp32 scatter-add of the scaled gradient)
    got, want = m.dense_grad(grad, idx, off, batch=B0), s.dense_grad(scaled, idx, off, batch=B0)
    rule = M.dense_grad(ROWS, dims, idx_h, off_h, B0, PADS, gparts)
    for t in range(3):
        assert np.array_equal(_bits(got[t]), _bits(want[t])) and np.array_equal(_bits(got[t]), _bits(rule[t])), t
    # sparse_grad, whole batch and a slice: rows and values
    for b0, nb in ((0, None), (5, 20)):
        sg = m.sparse_grad(grad, idx, off, batch=B0, bag_begin=b0, bag_count=nb)
        sw = s.sparse_grad(scaled, idx, off, batch=B0, bag_begin=b0, bag_count=nb)
        sr = M.sparse_grad(ROWS, dims, idx_h, off_h, B0, PADS, gparts, b0, nb)
        for t, ((r, v), (r0, v0), (r1, v1)) in enumerate(zip(sg, sw, sr)):
            assert r.cpu().numpy().tolist() == r0.cpu().numpy().tolist() == r1.tolist(), t
            assert np.array_equal(_bits(v), _bits(v0)) and np.array_equal(_bits(v), _bits(v1)), t
    # scatter_add_, whole batch and a slice
    for b0, nb in ((0, None), (5, 20)):
        m.scatter_add_(grad, idx, off, alpha=-0.25, batch=B0, bag_begin=b0, bag_count=nb)
        s.scatter_add_(scaled, idx, off, alpha=-0.25, batch=B0, bag_begin=b0, bag_count=nb)
        assert np.array_equal(_bits(m.weights.data), _bits(s.weights.data))
    with pytest.raises(ValueError, match="per_sample_weights"):
        m.scatter_add_(grad, idx, off, alpha=1.0, per_sample_weights=torch.ones(idx.numel(), device=DEV), batch=B0)


def test_1100_tables_one_scaling_launch_around_the_table_chunks(monkeypatch):
    from param_amd import _lib

    T, n, D, B, L = 1100, 16, 8, 4, 3
    rows = [n] * T
    pads = [1 if t % 3 else None for t in range(T)]
    rng = np.random.default_rng(51)
    idx_h, off_h = R.padded_request(rng, rows, B, pads, fixed=L)
    idx, off = _dev(idx_h), _dev(off_h)
    grad = torch.randn(B, T * D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    m, s = _pair(rows, D, pads, learning_rate=0.1, seed=6)
    tabs = m.weights.data.cpu().numpy().reshape(T, n, D)
    out = m.lookup(idx, off, batch=B)
    want = M.forward(list(tabs), idx_h, off_h, B, pads)
    assert np.array_equal(_bits(out), _bits(np.concatenate(want, axis=1)))
    scaled = _scaled(grad, [D] * T, "bd", idx_h, off_h, B, pads)
    real, calls = _lib.load(), []

    class Counting:      # counts CALLS (the chunk loop fetches an entry point once and calls it per table range)
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name not in NEW and name != "pm_embbag_bwd_fused":
                return fn
            return lambda *a: (calls.append(name), fn(*a))[1]

    monkeypatch.setattr(_lib, "load", lambda: Counting())
    m.optimizer_step_(grad, idx, off, batch=B)
    assert calls.count("pm_embbag_mean_grad") == 1 and calls.count("pm_embbag_bwd_fused") == 2, calls
    s.optimizer_step_(scaled, idx, off, batch=B)
    assert calls.count("pm_embbag_mean_grad") == 1
    assert np.array_equal(_bits(m.weights.data), _bits(s.weights.data))
    assert (M.count(idx_h, off_h, T, B, pads).reshape(T, B)[[1, 1025, 1099]] < L).any()      # both chunks see padding


# ---- EmbeddingBagMI355(mode="mean") autograd ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("pad", [None, 7], ids=["nopad", "padded"])
@pytest.mark.parametrize("once", [False, True], ids=["repeats", "once_per_row"])
def test_single_table_autograd_equals_the_rule(sparse, pad, once):
    """``once_per_row``: no row is looked up twice, where the rule is torch's CPU gradient bit for bit (tests/test_mean_host.py)"""
    import param_amd

    rng = np.random.default_rng(41)
    n, D, B = (600, 32, 50) if once else (60, 32, 50)
    idx_h, off_h = R.padded_request(rng, [n], B, [pad], closed=False)
    if once:
        live = idx_h != (-1 if pad is None else pad)
        fresh = np.array([r for r in rng.permutation(n) if r != pad][:int(live.sum())], dtype=np.int64)
        idx_h[live] = fresh
    idx, off = _dev(idx_h), _dev(off_h)
    gout = torch.randn(B, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    keep = gout.clone()
    m = param_amd.EmbeddingBagMI355(n, D, mode="mean", device=DEV, sparse=sparse, padding_idx=pad)
    if pad is not None:
        with torch.no_grad():
            m.weight[pad] = 0.75
    W = m.weight.detach().cpu().numpy()
    out = m(idx, off)
    assert np.array_equal(_bits(out), _bits(M.forward([W], idx_h, off_h, B, [pad])[0]))
    out.backward(gout)
    assert np.array_equal(_bits(gout), _bits(keep))                          # autograd's grad_out is never modified
    g = m.weight.grad
    if sparse:
        assert g.is_sparse and g.is_coalesced()
        rows, vals = M.sparse_grad([n], [D], idx_h, off_h, B, [pad], [gout.cpu().numpy()])[0]
        assert g._indices()[0].cpu().numpy().tolist() == rows.tolist() and np.array_equal(_bits(g._values()), _bits(vals))
        assert pad is None or pad not in rows.tolist()
    else:
        dense = M.dense_grad([n], [D], idx_h, off_h, B, [pad], [gout.cpu().numpy()])[0]
        assert np.array_equal(_bits(g), _bits(dense))
        assert pad is None or (_bits(g[pad]) == 0).all()


# ---- the default path ---------------------------------------------------------------------------------------------------------------

def test_sum_mode_modules_reach_neither_new_entry_point(monkeypatch):
    import param_amd
    from param_amd import _lib

    real = _lib.load()
    calls = []

    class Raising:
        def __getattr__(self, name):
            if name in NEW:
                calls.append(name)
                raise AssertionError(f"{name} reached from a sum-mode module")
            return getattr(real, name)

    monkeypatch.setattr(_lib, "load", lambda: Raising())
    rng = np.random.default_rng(71)
    idx_h, off_h = R.padded_request(rng, ROWS, B0, PADS)
    idx, off = _dev(idx_h), _dev(off_h)
    psw = torch.randn(idx.numel(), device=DEV).requires_grad_(True)
    grad = torch.randn(B0, 48, device=DEV)
    for opt in ("sgd", "rowwise_adagrad", "adagrad"):
        for pads in (None, PADS):
            m = _model(ROWS, 16, pads, "sum", optimizer=opt, fused_update=True)
            m(idx, off, psw).backward(grad)
            m.lookup(idx, off)
            m.dense_grad(grad, idx, off)
            m.sparse_grad(grad, idx, off)
            m.per_sample_weights_grad(grad, idx, off)
    for sparse in (False, True):
        sm = param_amd.EmbeddingBagMI355(50, 16, device=DEV, sparse=sparse, padding_idx=3)
        sm(idx[:off_h[B0]], off[:B0]).backward(grad[:, :16])
        sm(torch.randint(0, 50, (8, 5), device=DEV)).sum().backward()
    torch.cuda.synchronize()
    assert calls == []
    # ... and a mean module does reach them (this fails where the feature is missing: the constructor refuses the mode)
    monkeypatch.setattr(_lib, "load", lambda: real)
    seen = []

    class Counting:
        def __getattr__(self, name):
            if name in NEW:
                seen.append(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "load", lambda: Counting())
    p = _model(ROWS, 16, PADS, "mean", fused_update=True)
    p(idx, off).backward(grad)
    param_amd.EmbeddingBagMI355(50, 16, mode="mean", device=DEV)(idx[:off_h[B0]], off[:B0]).sum().backward()
    assert set(seen) == set(NEW)
