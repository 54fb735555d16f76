"""Backward and fused optimizers for requests of MORE than 1024 tables (the sorted path's limit per call): ``scatter_add_``,
``dense_grad``, ``adagrad_step_`` and ``.backward()`` with ``fused_update=True`` split such a request into table ranges of at most
1024 tables (``param_amd.embedding_bag._table_chunks``).  T = 1100, mixed dims 16 / 32 / 64 / 128, ragged bags, a table with no
lookups on each side of the cut at table 1024, the cut itself inside a run of empty tables.

Bars: scatter-add and dense gradient bit-equal to the sequential oracle (every row here is looked up far fewer than 256 times);
Adagrad as for the single-call path (fp32: 2e-5; bf16: the interval rule of tests/lowp_rules.py), every step judged from the bits
and state the device held before it; the first 1024 tables of a 1025-table request get the bits a 1024-table request gives them.
"""
import numpy as np
import pytest
import torch

from tests.test_gpu_lowp_update import _bits, _grad_shape, _t, _table_grad, check_adagrad_step

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T_MANY = 1100
EMPTY = set(range(1018, 1031)) | {300, 1075}            # the cut at 1024 falls inside a run of empty tables; one more on each side


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    import param_amd

    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    param_amd.load_library()
    yield


def _rows_dims(T, one_dim=None, seed=1):
    rows = [int(x) for x in np.random.default_rng(seed).integers(20, 200, size=T)]
    dims = [one_dim or [16, 32, 64, 128][t % 4] for t in range(T)]
    return rows, dims


def _request(rng, rows, B, empty=EMPTY):
    T = len(rows)
    lens = rng.integers(0, 5, size=(T, B))
    lens[rng.random((T, B)) < 0.2] = 0
    for t in empty:
        if t < T:
            lens[t] = 0
    off = np.zeros(T * B + 1, np.int64)
    off[1:] = np.cumsum(lens.ravel())
    idx = np.concatenate([rng.integers(0, rows[t], size=int(lens[t].sum())) for t in range(T)]).astype(np.int64)
    return idx, off


def _module(rows, dims, dtype=torch.float32, **kw):
    from param_amd import BatchedEmbeddingBagMI355

    return BatchedEmbeddingBagMI355(rows, dims, dtype=dtype, device=DEV, init="normal", seed=5, **kw)


def _host_tables(m):
    if m.weights.dtype == torch.float32:
        return [m.table(t).cpu().numpy().copy() for t in range(len(m.rows))]
    return [_bits(m.table(t)) for t in range(len(m.rows))]


def _same_tables(ma, mb):
    """bit-equal tables (table by table: the slab's padding between tables is never written)"""
    as_int = lambda w: w.view(torch.int32 if w.dtype == torch.float32 else torch.int16)          # noqa: E731
    return all(torch.equal(as_int(ma.table(t)), as_int(mb.table(t))) for t in range(len(ma.rows)))


def _check_scatter(coracle, m, before, grad_h, idx_h, off_h, psw_h, B, alpha, b0=0, b1=None):
    b1 = B if b1 is None else b1
    after = _host_tables(m)
    changed = 0
    for t in range(len(m.rows)):
        s, e = off_h[t * B + b0], off_h[t * B + b1]
        loc = off_h[t * B + b0:t * B + b1] - s
        g = np.ascontiguousarray(_table_grad(grad_h, t, m, B)[b0:b1])
        pw = None if psw_h is None else psw_h[s:e]
        fn = coracle.bwd_f32 if m.weights.dtype == torch.float32 else coracle.bwd_bf16
        exp = fn(before[t].copy(), idx_h[s:e], loc, g, pw, alpha=alpha)
        assert np.array_equal(after[t], exp), t
        changed += int(not np.array_equal(exp, before[t]))
        if t in EMPTY:
            assert e == s and np.array_equal(after[t], before[t])
    assert changed > len(m.rows) * 0.9


@pytest.mark.parametrize("dtype,idt,weighted,B,sl", [(torch.float32, torch.int64, False, 16, None), (torch.bfloat16, torch.int32, True, 48, (5, 20)),
                                                     (torch.float32, torch.int32, True, 96, (40, 56)), (torch.bfloat16, torch.int64, False, 32, None)],
                         ids=["fp32_i64", "bf16_i32_weighted_slice", "fp32_i32_weighted_slice", "bf16_i64"])
def test_scatter_add_and_dense_grad_1100_tables(coracle, dtype, idt, weighted, B, sl):
    rng = np.random.default_rng(B)
    rows, dims = _rows_dims(T_MANY)
    m = _module(rows, dims, dtype, fused_update=False)
    idx_h, off_h = _request(rng, rows, B)
    psw_h = rng.standard_normal(len(idx_h)).astype(np.float32) if weighted else None
    grad_h = rng.standard_normal((B, sum(dims))).astype(np.float32)
    idx, off, grad, psw = _t(idx_h, idt), _t(off_h, idt), _t(grad_h), None if psw_h is None else _t(psw_h)
    dws = m.dense_grad(grad, idx, off, psw, batch=B)
    assert len(dws) == T_MANY
    for t in range(T_MANY):
        s, e = off_h[t * B], off_h[(t + 1) * B]
        exp = coracle.bwd_f32(np.zeros((rows[t], dims[t]), np.float32), idx_h[s:e], off_h[t * B:(t + 1) * B] - s,
                              np.ascontiguousarray(grad_h[:, sum(dims[:t]):sum(dims[:t + 1])]), None if psw_h is None else psw_h[s:e])
        assert np.array_equal(dws[t].cpu().numpy(), exp), t
    before = _host_tables(m)
    b0, bc = (0, None) if sl is None else sl
    m.scatter_add_(grad, idx, off, alpha=-0.125, per_sample_weights=psw, batch=B, bag_begin=b0, bag_count=bc)
    _check_scatter(coracle, m, before, grad_h, idx_h, off_h, psw_h, B, -0.125, b0, B if bc is None else b0 + bc)


@pytest.mark.parametrize("layout", ["tbd", "blocked"])
def test_scatter_add_1100_tables_other_layouts(coracle, layout):
    rng = np.random.default_rng(3)
    B = 32
    rows, dims = _rows_dims(T_MANY, one_dim=16)
    m = _module(rows, dims, fused_update=False, layout=layout, block_bags=8 if layout == "blocked" else None)
    idx_h, off_h = _request(rng, rows, B)
    grad_h = rng.standard_normal(_grad_shape(m, B)).astype(np.float32)
    before = _host_tables(m)
    m.scatter_add_(_t(grad_h), _t(idx_h), _t(off_h), alpha=0.5, batch=B)
    _check_scatter(coracle, m, before, grad_h, idx_h, off_h, None, B, 0.5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_adagrad_1100_tables_two_steps(coracle, dtype):
    rng = np.random.default_rng(4)
    B = 24
    rows, dims = _rows_dims(T_MANY)
    kw = dict(learning_rate=0.05, optimizer="rowwise_adagrad", eps=1e-6, weight_decay=0.02, weight_decay_mode="l2")
    m = _module(rows, dims, dtype, **kw)
    for step in range(2):
        idx_h, off_h = _request(rng, rows, B)
        psw_h = rng.standard_normal(len(idx_h)).astype(np.float32)
        grad_h = rng.standard_normal((B, sum(dims))).astype(np.float32)
        before = [(w, m.momentum_table(t).cpu().numpy().copy()) for t, w in enumerate(_host_tables(m))]
        m.adagrad_step_(_t(grad_h), _t(idx_h), _t(off_h), _t(psw_h), batch=B)
        if dtype != torch.float32:
            cold, hot = check_adagrad_step(coracle, m, before, grad_h, idx_h, off_h, psw_h, B, tag=step)
            assert cold > 500000 and hot == 0
            continue
        for t in range(T_MANY):
            s, e = off_h[t * B], off_h[(t + 1) * B]
            W, mom = before[t][0].copy(), before[t][1].copy()
            coracle.bwd_rowwise_adagrad(W, mom, idx_h[s:e], off_h[t * B:(t + 1) * B] - s,
                                        np.ascontiguousarray(grad_h[:, sum(dims[:t]):sum(dims[:t + 1])]), psw_h[s:e], lr=0.05, eps=1e-6,
                                        weight_decay=0.02, weight_decay_mode=1)
            touched = np.bincount(idx_h[s:e], minlength=rows[t]) > 0
            gw, gm = m.table(t).cpu().numpy(), m.momentum_table(t).cpu().numpy()
            assert np.array_equal(gw[~touched], before[t][0][~touched]) and np.array_equal(gm[~touched], before[t][1][~touched]), t
            assert np.allclose(gm, mom, rtol=2e-5, atol=1e-12), (step, t)
            assert np.allclose(gw, W, rtol=2e-5, atol=2e-6), (step, t)
            assert t in EMPTY or not np.array_equal(gw, before[t][0])


@pytest.mark.parametrize("optimizer", ["sgd", "rowwise_adagrad"])
def test_autograd_fused_update_1100_tables_equals_the_direct_call(optimizer):
    """``m(idx, off).backward(g)`` with ``fused_update=True`` trains a step at T = 1100 and is the direct call, bit for bit"""
    rng = np.random.default_rng(6)
    B = 16
    rows, dims = _rows_dims(T_MANY)
    kw = dict(learning_rate=0.03, optimizer=optimizer, fused_update=True)
    ma, mb = _module(rows, dims, **kw), _module(rows, dims, **kw)
    assert _same_tables(ma, mb)
    w0 = ma.weights.clone()
    idx_h, off_h = _request(rng, rows, B)
    idx, off = _t(idx_h), _t(off_h)
    g = _t(rng.standard_normal((B, sum(dims))).astype(np.float32))
    out = ma(idx, off)
    assert out.requires_grad
    out.backward(g)
    mb.optimizer_step_(g, idx, off)
    assert _same_tables(ma, mb)
    for t in (0, 1017, 1031, 1099):                                          # both sides of the cut
        assert not torch.equal(ma.table(t), w0[ma._starts[t]:ma._starts[t] + ma._sizes[t]].view(rows[t], dims[t])), t
    if optimizer == "rowwise_adagrad":
        assert torch.equal(ma.momentum, mb.momentum) and float(ma.momentum_table(1099).sum()) > 0 and float(ma.momentum_table(0).sum()) > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_the_split_changes_nothing_for_the_first_1024_tables(dtype):
    """T = 1024 (one call) and T = 1025 (two ranges) give their common 1024 tables the same bits: scatter-add and Adagrad"""
    rng = np.random.default_rng(8)
    B = 20
    rows, dims = _rows_dims(1025)
    kw = dict(learning_rate=0.05, optimizer="rowwise_adagrad")
    m24, m25 = _module(rows[:1024], dims[:1024], dtype, **kw), _module(rows, dims, dtype, **kw)
    idx_h, off_h = _request(rng, rows, B, empty={7})
    n24 = int(off_h[1024 * B])
    assert n24 < len(idx_h)                                                   # the 1025th table has lookups of its own
    grad_h = rng.standard_normal((B, sum(dims))).astype(np.float32)
    g24 = np.ascontiguousarray(grad_h[:, :sum(dims[:1024])])
    for m, i, o, g in ((m24, idx_h[:n24], off_h[:1024 * B + 1], g24), (m25, idx_h, off_h, grad_h)):
        m.scatter_add_(_t(g), _t(i), _t(o), alpha=-0.25, batch=B)
        m.adagrad_step_(_t(g), _t(i), _t(o), batch=B)
    for t in range(1024):
        assert torch.equal(m24.table(t).view(torch.int32 if dtype == torch.float32 else torch.int16),
                           m25.table(t).view(torch.int32 if dtype == torch.float32 else torch.int16)), t
        assert torch.equal(m24.momentum_table(t), m25.momentum_table(t)), t
    assert float(m25.momentum_table(1024).sum()) > 0


def test_presorted_is_refused_beyond_1024_tables():
    """a pre-sorted request lives in the one cached workspace, which cannot hold the sorts of several table ranges: a ValueError
    that names the limit and the way out, raised on the host before anything is launched"""
    rng = np.random.default_rng(9)
    B = 16
    rows, dims = _rows_dims(T_MANY)
    m = _module(rows, dims, optimizer="rowwise_adagrad")
    idx_h, off_h = _request(rng, rows, B)
    idx, off = _t(idx_h), _t(off_h)
    g = _t(rng.standard_normal((B, sum(dims))).astype(np.float32))
    w0 = m.weights.clone()
    for call in (lambda: m.sort_indices(idx, off, batch=B),
                 lambda: m.scatter_add_(g, idx, off, alpha=1.0, batch=B, presorted=True),
                 lambda: m.adagrad_step_(g, idx, off, batch=B, presorted=True),
                 lambda: m.optimizer_step_(g, idx, off, batch=B, presorted=True)):
        with pytest.raises(ValueError, match=r"1024 tables.*without presorted"):
            call()
    torch.cuda.synchronize()
    assert torch.equal(m.weights.view(torch.int32), w0.view(torch.int32)) and float(m.momentum.abs().sum()) == 0
