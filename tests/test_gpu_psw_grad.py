"""Gradient of per_sample_weights (``pm_embbag_psw_grad``, ``per_sample_weights_grad``, the ``psw`` slot of the three autograd
functions) -- GPU parity (``pytest -m gpu``).

Every case is compared BIT FOR BIT with the numpy restatement of the kernel's arithmetic rule (tests/psw_grad_rules.py; NaN
positions must coincide instead of NaN bits) and must lie within the derived bar of the fp64 value:
``(D + 1) 2^-24 sum |g_c w_c| + D 2^-149`` -- the gamma_D bound of an fp32 dot product in any order.  The restatement itself is
pinned to torch's CPU autograd in tests/test_psw_grad_host.py; the mixed request is compared with torch here as well.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import psw_grad_rules as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NPDT = {torch.float32: "float32", torch.bfloat16: "bfloat16", torch.float16: "float16"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    import param_amd

    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    param_amd.load_library()
    yield


def _module(rows, dims, dtype=torch.float32, layout="bd", seed=5, **kw):
    import param_amd

    kw.setdefault("fused_update", False)
    return param_amd.BatchedEmbeddingBagMI355(rows, dims, dtype=dtype, device=DEV, init="normal", seed=seed, layout=layout, **kw)


def _tables_np(m):
    return [m.table(t).float().cpu().numpy() for t in range(len(m.rows))]


def _request(rng, rows, lens_per_table, idt=torch.int64, trailing=True):
    """table-major TBE request from per-table bag-length arrays"""
    lens = np.concatenate(lens_per_table).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    idx = np.concatenate([rng.integers(0, r, int(l.sum())) for r, l in zip(rows, lens_per_table)] + [np.zeros(0, np.int64)]).astype(np.int64)
    off_t = torch.from_numpy(off if trailing else off[:-1]).to(idt).to(DEV)
    return idx, off, torch.from_numpy(idx).to(idt).to(DEV), off_t


def _bd_grads(g_bd, dims):
    """[B, sum D] -> per-table [B, D_t] numpy"""
    g, out, c = g_bd.cpu().numpy(), [], 0
    for d in dims:
        out.append(np.ascontiguousarray(g[:, c:c + d]))
        c += d
    return out


def _check(got, tables, idx, off, B, grads, V, bag_begin=0, bag_count=None, what=""):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    ref, written, exact, bar = R.restate(tables, idx, off, B, grads, V, bag_begin, bag_count)
    fin = written & np.isfinite(exact)
    ratio = np.abs(got.astype(np.float64)[fin] - exact[fin]) / bar[fin] if fin.any() else np.zeros(1)
    print(f"{what}: {int(written.sum())} lookups, max |err| / bar {ratio.max():.3g}")
    assert R.same_bits(got[written], ref[written]), what
    assert R.within_bar(got[written], exact[written], bar[written]), what
    return ref, written


def _mixed_lens(rng, B):
    ragged = rng.integers(1, 11, B)
    ragged[rng.permutation(B)[:max(1, B // 8)]] = 0                      # an eighth of the bags empty
    ragged[0] = 0
    return [ragged, np.ones(B, np.int64), np.full(B, 20, np.int64), np.zeros(B, np.int64)]


MIX_ROWS, MIX_DIMS, MIX_B = (1000, 50, 300, 7), (128, 16, 64, 4), 37


@pytest.mark.parametrize("trailing", [True, False])
@pytest.mark.parametrize("idt", [torch.int64, torch.int32])
def test_mixed_request_both_layouts_and_torch(idt, trailing):
    import torch.nn.functional as F
    from param_amd import _lib
    from param_amd.embedding_bag import _stream_ptr

    rng = np.random.default_rng(11)
    B, T = MIX_B, len(MIX_ROWS)
    m = _module(list(MIX_ROWS), list(MIX_DIMS))
    tabs = _tables_np(m)
    idx, off, idx_t, off_t = _request(rng, MIX_ROWS, _mixed_lens(rng, B), idt, trailing)
    g = torch.randn(B, sum(MIX_DIMS), device=DEV)
    grads = _bd_grads(g, MIX_DIMS)
    got = m.per_sample_weights_grad(g, idx_t, off_t, batch=B)
    assert got.dtype == torch.float32 and tuple(got.shape) == (idx.size,)
    ref, written = _check(got, tabs, idx, off, B, grads, 4, what=f"mixed [B, sum D] {idt} trailing={trailing}")
    assert written.all()
    # the same gradient values in a [T, B, Dmax] layout (out_offsets[t] = t * B * Dmax, out_stride = Dmax), through the C ABI
    Dm = max(MIX_DIMS)
    g_tbd = torch.zeros(T, B, Dm, device=DEV)
    for t, gt in enumerate(grads):
        g_tbd[t, :, :gt.shape[1]] = torch.from_numpy(gt).to(DEV)
    ts = m._tables()
    op = _lib.pm_embbag_batch.from_buffer_copy(ts.request(idx_t, off_t, B, None, 0, None))
    offs = (torch.arange(T, dtype=torch.int64, device=DEV) * (B * Dm)).contiguous()
    op.out_offsets, op.out_stride = offs.data_ptr(), Dm
    out2 = torch.full((idx.size,), 7.0, device=DEV)
    _lib.check(_lib.load().pm_embbag_psw_grad(ctypes.byref(op), g_tbd.data_ptr(), out2.data_ptr(), _stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(out2, got)
    # torch CPU autograd per table, within the bar
    _, _, exact, bar = R.restate(tabs, idx, off, B, grads, 4)
    for t in range(T):
        s, e = int(off[t * B]), int(off[(t + 1) * B])
        if e == s:
            continue
        w = torch.zeros(e - s, requires_grad=True)
        o = F.embedding_bag(torch.from_numpy(idx[s:e]), torch.from_numpy(tabs[t]), torch.from_numpy(off[t * B:(t + 1) * B] - s), mode="sum",
                            per_sample_weights=w)
        o.backward(torch.from_numpy(grads[t]))
        assert (np.abs(w.grad.numpy().astype(np.float64) - exact[s:e]) <= bar[s:e]).all(), t
        assert (np.abs(got[s:e].cpu().numpy().astype(np.float64) - w.grad.numpy()) <= 2 * bar[s:e]).all(), t


@pytest.mark.parametrize("dtype,D", [(torch.float32, 128), (torch.float32, 256), (torch.bfloat16, 8), (torch.bfloat16, 128), (torch.bfloat16, 512),
                                     (torch.float16, 8), (torch.float16, 128), (torch.float16, 512)])
def test_one_width_route_equals_mixed_dim_launch(dtype, D):
    """T = 2, B = 64, pooling 20: the bag-tile launch; with a D = V table added the request is mixed (per-table lane groups, flat
    tiles) -- the common tables' lookups keep their bits"""
    rng = np.random.default_rng(D)
    V = R.vec_of(NPDT[dtype])
    B, L, rows = 64, 20, [500, 300]
    a = _module(rows, [D, D], dtype)
    b = _module(rows + [40], [D, D, V], dtype)
    for t in range(2):
        b.table(t).copy_(a.table(t))
    tabs = _tables_np(a)
    idx, off, idx_t, off_t = _request(rng, rows, [np.full(B, L)] * 2)
    ga = torch.randn(B, 2 * D, device=DEV)
    got = a.per_sample_weights_grad(ga, idx_t, off_t, batch=B)
    _check(got, tabs, idx, off, B, _bd_grads(ga, [D, D]), V, what=f"one width {dtype} D={D}")
    idx3, off3, idx3_t, off3_t = _request(rng, rows + [40], [np.full(B, L)] * 2 + [np.full(B, 3)])
    idx3[:idx.size] = idx
    idx3_t = torch.from_numpy(idx3).to(DEV)
    gb = torch.cat([ga, torch.randn(B, V, device=DEV)], dim=1).contiguous()
    got3 = b.per_sample_weights_grad(gb, idx3_t, off3_t, batch=B)
    _check(got3, _tables_np(b), idx3, off3, B, _bd_grads(gb, [D, D, V]), V, what=f"with a D={V} table {dtype} D={D}")
    assert torch.equal(got3[:idx.size], got)


def test_long_bag_is_walked_in_pieces():
    rng = np.random.default_rng(2)
    m = _module([5000], [64])
    idx, off, idx_t, off_t = _request(rng, [5000], [np.array([9000, 0, 5])])
    g = torch.randn(3, 64, device=DEV)
    _check(m.per_sample_weights_grad(g, idx_t, off_t, batch=3), _tables_np(m), idx, off, 3, _bd_grads(g, [64]), 4, what="long bag")


def test_batch_slice_into_caller_owned_out():
    rng = np.random.default_rng(4)
    B = MIX_B
    m = _module(list(MIX_ROWS), list(MIX_DIMS))
    idx, off, idx_t, off_t = _request(rng, MIX_ROWS, _mixed_lens(rng, B))
    g = torch.randn(B, sum(MIX_DIMS), device=DEV)
    whole = m.per_sample_weights_grad(g, idx_t, off_t, batch=B)
    out = torch.full((idx.size,), -123.5, device=DEV)
    ret = m.per_sample_weights_grad(g, idx_t, off_t, batch=B, out=out, bag_begin=5, bag_count=11)
    assert ret is out
    _, written = _check(out, _tables_np(m), idx, off, B, _bd_grads(g, MIX_DIMS), 4, 5, 11, what="slice")
    w = torch.from_numpy(written).to(DEV)
    assert 0 < int(w.sum()) < idx.size
    assert torch.equal(out[w], whole[w])
    assert bool((out[~w] == -123.5).all())
    # allocated by the method: zero outside the slice
    alloc = m.per_sample_weights_grad(g, idx_t, off_t, batch=B, bag_begin=5, bag_count=11)
    assert torch.equal(alloc[w], whole[w]) and bool((alloc[~w] == 0).all())


def test_blocked_gradient_layout():
    rng = np.random.default_rng(6)
    T, B, Bl, D = 3, 16, 4, 64
    rows = [200, 90, 31]
    mb = _module(rows, D, layout="blocked", block_bags=Bl)
    md = _module(rows, D)
    idx, off, idx_t, off_t = _request(rng, rows, [rng.integers(0, 6, B) for _ in range(T)])
    g_tbd = torch.randn(T, B, D, device=DEV)
    g_blk = g_tbd.view(T, B // Bl, Bl, D).permute(1, 0, 2, 3).contiguous()          # [W, T, Bl, D]
    g_bd = g_tbd.permute(1, 0, 2).reshape(B, T * D).contiguous()
    got = mb.per_sample_weights_grad(g_blk, idx_t, off_t, batch=B)
    _check(got, _tables_np(mb), idx, off, B, [g_tbd[t].cpu().numpy() for t in range(T)], 4, what="blocked")
    assert torch.equal(got, md.per_sample_weights_grad(g_bd, idx_t, off_t, batch=B))


def test_many_tables():
    rng = np.random.default_rng(8)
    T, B, L = 1030, 2, 3
    rows = [5 + (t % 7) for t in range(T)]
    m = _module(rows, 4)
    idx, off, idx_t, off_t = _request(rng, rows, [np.full(B, L)] * T)
    g = torch.randn(B, 4 * T, device=DEV)
    _check(m.per_sample_weights_grad(g, idx_t, off_t, batch=B), _tables_np(m), idx, off, B, _bd_grads(g, [4] * T), 4, what="1030 tables")


def test_two_calls_give_the_same_bits():
    rng = np.random.default_rng(9)
    B = MIX_B
    m = _module(list(MIX_ROWS), list(MIX_DIMS))
    idx, off, idx_t, off_t = _request(rng, MIX_ROWS, _mixed_lens(rng, B))
    g = torch.randn(B, sum(MIX_DIMS), device=DEV)
    a = m.per_sample_weights_grad(g, idx_t, off_t, batch=B)
    b = m.per_sample_weights_grad(g, idx_t, off_t, batch=B)
    assert torch.equal(a, b)
    m2 = _module([20000] * 2, 128)
    idx, off, idx_t, off_t = _request(rng, [20000] * 2, [np.full(64, 20)] * 2)
    g = torch.randn(64, 256, device=DEV)
    assert torch.equal(m2.per_sample_weights_grad(g, idx_t, off_t, batch=64), m2.per_sample_weights_grad(g, idx_t, off_t, batch=64))


def test_special_values():
    """one row holds a NaN, one +Inf, one -0.0 throughout and one an fp16 subnormal"""
    rng = np.random.default_rng(10)
    rows, D, B = 40, 64, 32
    m = _module([rows], [D], torch.float16)
    clean = m.table(0).clone()
    NAN_R, INF_R, NZ_R, SUB_R = 3, 7, 11, 13
    m.table(0)[NAN_R, 5] = float("nan")
    m.table(0)[INF_R, 9] = float("inf")
    m.table(0)[NZ_R] = -0.0
    m.table(0)[SUB_R, 2] = 2.0 ** -24                                  # the smallest fp16 subnormal
    idx, off, idx_t, off_t = _request(rng, [rows], [rng.integers(2, 9, B)])
    idx[[1, 4, 6, 9]] = (NAN_R, INF_R, NZ_R, SUB_R)                     # each special row is looked up at least once
    idx_t = torch.from_numpy(idx).to(DEV)
    g = torch.randn(B, D, device=DEV)
    assert bool((g != 0).all())
    got = m.per_sample_weights_grad(g, idx_t, off_t, batch=B)
    tabs = _tables_np(m)
    assert tabs[0][SUB_R, 2] == 2.0 ** -24 and np.signbit(tabs[0][NZ_R]).all()
    ref, written = _check(got, tabs, idx, off, B, _bd_grads(g, [D]), 8, what="special values")
    h = got.cpu().numpy()
    assert np.array_equal(np.isnan(h), idx == NAN_R)                   # exactly the NaN row's lookups
    assert np.isinf(h[idx == INF_R]).all() and R.same_bits(h[idx == INF_R], ref[idx == INF_R])
    assert (h[idx == NZ_R] == 0).all() and not np.signbit(h[idx == NZ_R]).any()      # +0 + (-0) = +0
    # every other lookup is what the clean table gives
    m.table(0).copy_(clean)
    base = m.per_sample_weights_grad(g, idx_t, off_t, batch=B).cpu().numpy()
    other = ~np.isin(idx, (NAN_R, INF_R, NZ_R, SUB_R))
    assert other.any() and R.same_bits(h[other], base[other])


@pytest.mark.parametrize("sparse", [False, True])
def test_autograd_single_table_module(sparse):
    import param_amd

    rng = np.random.default_rng(12)
    n, D, B = 300, 64, 48
    m = param_amd.EmbeddingBagMI355(n, D, sparse=sparse, device=DEV)
    idx, off, idx_t, off_t = _request(rng, [n], [rng.integers(0, 8, B)], trailing=False)
    g = torch.randn(B, D, device=DEV)
    psw = torch.randn(idx.size, device=DEV, requires_grad=True)
    m(idx_t, off_t, psw).backward(g)
    assert psw.grad is not None                                        # None before this change
    W = m.weight.detach().float().cpu().numpy()
    _check(psw.grad, [W], idx, off, B, [g.cpu().numpy()], 4, what=f"autograd sparse={sparse}")
    wg = m.weight.grad.to_dense().clone() if sparse else m.weight.grad.clone()
    m.weight.grad = None
    det = psw.detach()
    m(idx_t, off_t, det).backward(g)
    wg2 = m.weight.grad.to_dense() if sparse else m.weight.grad
    assert torch.equal(wg, wg2)
    assert det.grad is None


@pytest.mark.parametrize("optimizer", ["sgd", "rowwise_adagrad"])
def test_autograd_fused_update_uses_the_weights_the_forward_read(optimizer):
    rng = np.random.default_rng(13)
    rows, dims, B = [400, 60], [64, 16], 40
    kw = dict(fused_update=True, optimizer=optimizer, learning_rate=0.1)
    m, twin = _module(rows, dims, **kw), _module(rows, dims, **kw)
    assert torch.equal(m.weights.data, twin.weights.data)
    idx, off, idx_t, off_t = _request(rng, rows, [rng.integers(0, 7, B), np.full(B, 2)])
    g = torch.randn(B, sum(dims), device=DEV)
    psw = torch.randn(idx.size, device=DEV, requires_grad=True)
    out = m(idx_t, off_t, psw)
    before = _tables_np(m)                                             # snapshot BEFORE backward()
    out.backward(g)
    assert psw.grad is not None
    _check(psw.grad, before, idx, off, B, _bd_grads(g, dims), 4, what=f"fused {optimizer}")
    det = psw.detach()
    twin(idx_t, off_t, det).backward(g)
    assert det.grad is None
    assert torch.equal(m.weights.data, twin.weights.data)
    assert any(not np.array_equal(a, b) for a, b in zip(before, _tables_np(m)))      # the step did move the tables
    if optimizer == "rowwise_adagrad":
        assert torch.equal(m.momentum, twin.momentum) and float(m.momentum.abs().sum()) > 0


def test_weights_that_do_not_require_grad_get_none():
    import param_amd

    rng = np.random.default_rng(14)
    n, D, B = 100, 16, 8
    m = param_amd.EmbeddingBagMI355(n, D, device=DEV)
    idx, off, idx_t, off_t = _request(rng, [n], [rng.integers(1, 5, B)], trailing=False)
    psw = torch.randn(idx.size, device=DEV)
    m(idx_t, off_t, psw).backward(torch.randn(B, D, device=DEV))
    assert psw.grad is None and m.weight.grad is not None
