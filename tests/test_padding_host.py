"""padding_idx and 2-D input, the parts that need no GPU: the numpy restatement of the rule (tests/padding_rules.py) against torch's
CPU ``nn.EmbeddingBag(mode="sum", padding_idx=...)`` -- unweighted forward bit for bit, weighted forward within a derived bound
(torch's padded CPU path multiplies and then adds, the rule is one fused multiply-add), gradients, COO rows, the
``per_sample_weights`` gradient, NaN in the padding row --; what the two modules accept and refuse at construction
(``device="cpu"``: nothing is launched); the four new entry points in the header, the binding and both libraries, with the ABI
version and the request struct where they were."""
import ctypes
import os

import numpy as np
import pytest
import torch

import param_amd
from param_amd import _lib
from tests import padding_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS, DIM, BAGS = 11, 8, 23


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _torch_bag(weight, pad, sparse=False):
    return torch.nn.EmbeddingBag(weight.shape[0], weight.shape[1], mode="sum", padding_idx=pad, sparse=sparse,
                                 _weight=torch.from_numpy(weight.copy()))


def _request(rng, pad, fixed=None):
    """1-D request over one table with ~40 % padding, plus the edge bags: all padding, empty, padding first and last"""
    k = pad % N_ROWS
    idx, off = R.padded_request(rng, [N_ROWS], BAGS, [k], share=0.4, max_len=6, fixed=fixed, closed=False)
    if fixed is None:
        other = (k + 1) % N_ROWS
        extra = [[k, k, k], [], [k, other, other], [other, other, k]]
        off = np.concatenate([off, idx.size + np.cumsum([0] + [len(e) for e in extra[:-1]])]).astype(np.int64)
        idx = np.concatenate([idx, np.array(sum(extra, []), dtype=np.int64)])
    return idx, off, k


@pytest.mark.parametrize("pad", [0, 3, N_ROWS - 1, -2])
def test_unweighted_forward_rule_is_torch_bit_for_bit(pad):
    rng = np.random.default_rng(100 + pad)
    W = rng.standard_normal((N_ROWS, DIM)).astype(np.float32)
    idx, off, k = _request(rng, pad)
    B = off.size
    want = _torch_bag(W, pad)(torch.from_numpy(idx), torch.from_numpy(off)).detach().numpy()
    got = R.forward([W], idx, off, B, [k])[0]
    assert np.array_equal(_bits(got), _bits(want))
    assert (_bits(got[B - 4]) == 0).all() and (_bits(got[B - 3]) == 0).all()      # the all-padding bag and the empty bag: +0.0
    assert 0.25 < R.padded_mask(idx, off, 1, B, [k]).mean() < 0.6
    # 2-D input: fixed-length bags
    idx2, off2, _ = _request(rng, pad, fixed=7)
    want2 = _torch_bag(W, pad)(torch.from_numpy(idx2.reshape(BAGS, 7))).detach().numpy()
    assert np.array_equal(_bits(R.forward([W], idx2, off2, BAGS, [k])[0]), _bits(want2))


@pytest.mark.parametrize("pad", [0, 3, N_ROWS - 1, -2])
def test_weighted_forward_rule_is_torch_within_the_derived_bound(pad):
    """torch's padded CPU path rounds the product and the sum (two roundings per kept lookup), the rule one: after K kept lookups
    the two differ by at most (2K + 2) * 2^-24 * sum |psw * row| per element"""
    rng = np.random.default_rng(200 + pad)
    W = rng.standard_normal((N_ROWS, DIM)).astype(np.float32)
    idx, off, k = _request(rng, pad)
    B = off.size
    psw = rng.standard_normal(idx.size).astype(np.float32)
    want = _torch_bag(W, pad)(torch.from_numpy(idx), torch.from_numpy(off), per_sample_weights=torch.from_numpy(psw)).detach().numpy()
    got = R.forward([W], idx, off, B, [k], psw)[0]
    skip = R.padded_mask(idx, off, 1, B, [k])
    start, end = R.bag_bounds(off, 1, B, idx.size)
    for b in range(B):
        js = [j for j in range(start[b], end[b]) if not skip[j]]
        mag = sum(np.abs(np.float64(psw[j]) * W[idx[j]].astype(np.float64)) for j in js) if js else np.zeros(DIM)
        err = np.abs(got[b].astype(np.float64) - want[b].astype(np.float64))
        assert (err <= (2 * len(js) + 2) * 2.0 ** -24 * mag).all(), (b, err.max())
    # 2-D weighted input
    idx2, off2, _ = _request(rng, pad, fixed=5)
    psw2 = rng.standard_normal(idx2.size).astype(np.float32)
    want2 = _torch_bag(W, pad)(torch.from_numpy(idx2.reshape(BAGS, 5)), per_sample_weights=torch.from_numpy(psw2.reshape(BAGS, 5))).detach().numpy()
    got2 = R.forward([W], idx2, off2, BAGS, [k], psw2)[0]
    keep2 = ~R.padded_mask(idx2, off2, 1, BAGS, [k])
    mag2 = (np.abs(psw2[:, None].astype(np.float64) * W[idx2]) * keep2[:, None]).reshape(BAGS, 5, DIM).sum(axis=1)
    k2 = keep2.reshape(BAGS, 5).sum(axis=1)[:, None]
    assert (np.abs(got2.astype(np.float64) - want2) <= (2 * k2 + 2) * 2.0 ** -24 * mag2).all()


def test_fma32_is_a_single_rounding():
    """cases where rounding the fp64 sum to nearest first and to fp32 second would give the neighbour"""
    import fractions
    # 2^30 + 2^7 + (2^6 - 2^-24): just BELOW the midpoint of two fp32 neighbours.  The fp64 sum rounds to the midpoint itself, and a
    # second rounding to nearest-even would then go up to 2^30 + 2^8; the fused result stays at 2^30 + 2^7
    w, f, acc = np.float32(64.0 * (1.0 + 2.0 ** -15)), np.float32(1.0 - 2.0 ** -15), np.float32(2.0 ** 30 + 2.0 ** 7)
    assert np.float32(float(w) * float(f) + float(acc)) == np.float32(2.0 ** 30 + 2.0 ** 8)          # (the trap is real)
    assert R.fma32(w, f, acc) == np.float32(2.0 ** 30 + 2.0 ** 7)
    rng = np.random.default_rng(5)
    a, b, c = (rng.standard_normal(4000).astype(np.float32) for _ in range(3))
    ref = np.array([np.float32(float(fractions.Fraction(float(x)) * fractions.Fraction(float(y)) + fractions.Fraction(float(z))))
                    for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert np.array_equal(_bits(R.fma32(a, b, c)), _bits(ref))


@pytest.mark.parametrize("pad", [0, 3, -2])
def test_gradients_rule_and_torch_leave_the_padding_row_out(pad):
    rng = np.random.default_rng(300 + pad)
    W = rng.standard_normal((N_ROWS, DIM)).astype(np.float32)
    idx, off, k = _request(rng, pad)
    B = off.size
    psw = rng.standard_normal(idx.size).astype(np.float32)
    g = rng.standard_normal((B, DIM)).astype(np.float32)
    # dense weight gradient: the padding row exactly zero in both
    m = _torch_bag(W, pad)
    w_t = torch.from_numpy(psw).requires_grad_(True)
    m(torch.from_numpy(idx), torch.from_numpy(off), per_sample_weights=w_t).backward(torch.from_numpy(g))
    want = m.weight.grad.numpy()
    got = R.dense_grad([N_ROWS], [DIM], idx, off, B, [k], [g], psw)[0]
    assert (_bits(want[k]) == 0).all() and (got[k] == 0).all() and not np.signbit(got[k]).any()
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)
    # per_sample_weights gradient: +0.0 (sign bit clear) at the padded positions in both
    skip = R.padded_mask(idx, off, 1, B, [k])
    dpsw = w_t.grad.numpy()
    assert skip.any() and (_bits(dpsw[skip]) == 0).all()
    start, _ = R.bag_bounds(off, 1, B, idx.size)
    bag = np.searchsorted(start, np.arange(idx.size), side="right") - 1
    raw = np.einsum("nd,nd->n", g[bag], W[idx]).astype(np.float32)
    masked = R.psw_grad_mask(raw, idx, off, 1, B, [k])
    assert (_bits(masked[skip]) == 0).all() and np.array_equal(_bits(masked[~skip]), _bits(raw[~skip]))
    np.testing.assert_allclose(masked, dpsw, rtol=1e-5, atol=1e-5)
    # a bag slice masks only its own lookups
    sl = R.psw_grad_mask(raw, idx, off, 1, B, [k], bag_begin=2, bag_count=5)
    inside = (np.arange(idx.size) >= off[2]) & (np.arange(idx.size) < off[7])
    assert np.array_equal(_bits(sl[~(skip & inside)]), _bits(raw[~(skip & inside)])) and (_bits(sl[skip & inside]) == 0).all()
    # sparse gradient: the COO rows exclude the padding row in both
    ms = _torch_bag(W, pad, sparse=True)
    ms(torch.from_numpy(idx), torch.from_numpy(off)).backward(torch.from_numpy(g))
    coo = ms.weight.grad.coalesce()
    t_rows = coo.indices()[0].numpy()
    mine = R.sparse_rows(idx, off, 1, B, [k])[0]
    assert k not in mine.tolist() and k not in t_rows.tolist()
    assert mine.tolist() == sorted(set(idx[~skip].tolist())) == t_rows.tolist()


def test_nan_in_the_padding_row_reaches_no_output():
    rng = np.random.default_rng(9)
    W = rng.standard_normal((N_ROWS, DIM)).astype(np.float32)
    idx, off, k = _request(rng, 3)
    clean = R.forward([W], idx, off, off.size, [k])[0]
    W[k] = np.nan
    psw = rng.standard_normal(idx.size).astype(np.float32)
    assert np.array_equal(_bits(R.forward([W], idx, off, off.size, [k])[0]), _bits(clean))
    assert np.isfinite(R.forward([W], idx, off, off.size, [k], psw)[0]).all()
    assert np.isfinite(_torch_bag(W, 3)(torch.from_numpy(idx), torch.from_numpy(off)).detach().numpy()).all()


def test_filtered_request_and_guard_rules():
    rng = np.random.default_rng(11)
    rows, pads, B = [9, 4, 30], [2, None, 29], 6
    W = [rng.standard_normal((r, DIM)).astype(np.float32) for r in rows]
    for closed in (False, True):
        idx, off = R.padded_request(rng, rows, B, pads, closed=closed)
        psw = rng.standard_normal(idx.size).astype(np.float32)
        fi, fo, fw = R.filtered_request(idx, off, 3, B, pads, psw)
        assert fo.size == off.size and fi.size == fw.size == int((~R.padded_mask(idx, off, 3, B, pads)).sum())
        assert not R.padded_mask(fi, fo, 3, B, pads).any()
        for a, b in zip(R.forward(W, idx, off, B, pads, psw), R.forward(W, fi, fo, B, [None] * 3, fw)):
            assert np.array_equal(_bits(a), _bits(b))
    after = [w + 1 for w in W]
    kept = R.guard(W, after, pads)
    assert np.array_equal(kept[0][2], W[0][2]) and np.array_equal(kept[2][29], W[2][29]) and np.array_equal(kept[1], after[1])
    assert np.array_equal(np.delete(kept[0], 2, axis=0), np.delete(after[0], 2, axis=0))


# ---- constructors (device="cpu": nothing is launched) ---------------------------------------------------------------------------

def test_single_table_constructor():
    m = param_amd.EmbeddingBagMI355(10, 8, device="cpu", padding_idx=3)
    assert m.padding_idx == 3 and (m.weight[3] == 0).all() and (m.weight[2] != 0).any()
    assert "padding_idx=3" in m.extra_repr() and "padding_idx=3" in repr(m)
    assert param_amd.EmbeddingBagMI355(10, 8, device="cpu", padding_idx=-2).padding_idx == 8
    assert param_amd.EmbeddingBagMI355(10, 8, device="cpu", padding_idx=-10).padding_idx == 0
    plain = param_amd.EmbeddingBagMI355(10, 8, device="cpu")
    assert plain.padding_idx is None and "padding_idx" not in plain.extra_repr() and plain._pad_dev() is None
    for bad in (10, -11):
        with pytest.raises(ValueError, match="padding_idx must be within num_embeddings"):
            param_amd.EmbeddingBagMI355(10, 8, device="cpu", padding_idx=bad)
    w = torch.ones(10, 8)
    kept = param_amd.EmbeddingBagMI355(10, 8, device="cpu", _weight=w, padding_idx=3)
    assert (kept.weight == 1).all()                                          # a caller's weights are left alone
    t = torch.nn.EmbeddingBag(10, 8, mode="sum", padding_idx=-2)
    assert t.padding_idx == 8 and (t.weight[8] == 0).all()                   # (the rule is torch's)


def test_two_d_input_with_offsets_is_refused_with_torchs_text():
    m = param_amd.EmbeddingBagMI355(10, 8, device="cpu")
    idx = torch.zeros(4, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="^if input is 2D, then offsets has to be None"):
        m(idx, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="offsets has to be a 1D Tensor"):
        m(idx.reshape(-1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(idx)                                                               # a sound 2-D request gets as far as the device check
    with pytest.raises(ValueError, match="same shape as the input"):
        m._bags_2d(idx, None, torch.zeros(12))
    flat, off, w = m._bags_2d(idx, None, torch.zeros(4, 3))
    assert flat.shape == (12,) and off.tolist() == [0, 3, 6, 9] and off.dtype == torch.int64 and w.shape == (12,)
    assert m._bags_2d(idx, None, None)[1] is off                             # built once per (B, L, dtype), reused


def test_batched_constructor():
    mk = lambda **kw: param_amd.BatchedEmbeddingBagMI355([50, 7, 1000], 8, device="cpu", init=None, **kw)      # noqa: E731
    assert mk().padding_idx is None and mk()._pad_dev() is None
    assert mk(padding_idx=3).padding_idx == [3, 3, 3]
    assert mk(padding_idx=-1).padding_idx == [49, 6, 999]
    assert mk(padding_idx=np.int64(2)).padding_idx == [2, 2, 2] and mk(padding_idx=np.array([1, 2, 3])).padding_idx == [1, 2, 3]
    with pytest.raises(TypeError):
        mk(padding_idx=True)
    m = mk(padding_idx=(3, None, -1))
    assert m.padding_idx == [3, None, 999]
    assert m._pad_dev().tolist() == [3, -1, 999] and m._pad_dev().dtype == torch.int64
    assert mk(padding_idx=[None, None, None]).padding_idx is None
    with pytest.raises(ValueError, match="padding_idx must be within num_embeddings"):
        mk(padding_idx=7)                                                    # outside the 7-row table
    with pytest.raises(ValueError, match="padding_idx must be within num_embeddings"):
        mk(padding_idx=[0, -8, 0])
    with pytest.raises(ValueError, match="padding_idx has 2 entries for 3 tables"):
        mk(padding_idx=[1, 2])
    with pytest.raises(ValueError, match="padding_idx"):
        param_amd.BatchedEmbeddingBagMI355([64, 64], 8, device="cpu", init=None, layout="blocked", block_bags=4, padding_idx=0)
    i, o = torch.zeros(6, dtype=torch.int64), torch.arange(7, dtype=torch.int64)
    with pytest.raises(ValueError, match="padding_idx"):
        m.lookup_quantized(i, o, 8)
    with pytest.raises(ValueError, match="padding_idx"):
        m.lookup(i, o, split_bags=True, batch=2)


def test_batched_module_zero_fills_its_padding_rows_on_the_host_too():
    m = param_amd.BatchedEmbeddingBagMI355([5, 6], 8, device="cpu", init=None, padding_idx=[1, None])
    with torch.no_grad():
        m.weights.fill_(2.0)
    for t, k in enumerate(m.padding_idx):                                    # what reset_parameters does behind the random fill
        if k is not None:
            m.table(t)[k].zero_()
    assert (m.table(0)[1] == 0).all() and (m.table(0)[0] == 2).all() and (m.table(1) == 2).all()


# ---- library surface ----------------------------------------------------------------------------------------------------------

NEW = ("pm_embbag_fwd_padded", "pm_embbag_pad_mask", "pm_pad_rows_guard_bytes", "pm_pad_rows_guard")


def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "param_amd.h")).read()
    for lib in (_lib.load(), _lib.load_alternates()):
        for name in NEW:
            assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS and name + "(" in header
        assert lib.pm_abi_version() == 8
    assert _lib.PM_ABI_VERSION == 8 and "#define PM_ABI_VERSION 8" in header
    assert ctypes.sizeof(_lib.pm_embbag_batch) == 144


def test_host_side_refusals_answer_before_a_hip_call():
    L = _lib.load()
    op = _lib.pm_embbag_batch()
    assert L.pm_embbag_fwd_padded(None, 8, 8, None) == _lib.PM_ERR_INVALID
    op.num_tables, op.weight_dtype, op.index_dtype, op.max_dim = 1, _lib.PM_F32, _lib.PM_I64, 8
    op.tables = op.rows = op.dims = op.out_offsets = 8                        # non-null dummies, never dereferenced on the host
    op.batch, op.bag_count, op.num_indices, op.indices, op.offsets = 4, 4, 8, 8, 8
    assert L.pm_embbag_fwd_padded(ctypes.byref(op), None, 8, None) == _lib.PM_ERR_INVALID and b"padding_idx" in L.pm_last_error()
    assert L.pm_embbag_fwd_padded(ctypes.byref(op), 8, None, None) == _lib.PM_ERR_INVALID and b"out is NULL" in L.pm_last_error()
    assert L.pm_embbag_pad_mask(ctypes.byref(op), None, 8, None) == _lib.PM_ERR_INVALID
    assert L.pm_embbag_pad_mask(ctypes.byref(op), 8, None, None) == _lib.PM_ERR_INVALID
    op.weight_dtype = 7
    assert L.pm_embbag_fwd_padded(ctypes.byref(op), 8, 8, None) == _lib.PM_ERR_INVALID and b"dtype" in L.pm_last_error()
    op.weight_dtype, op.batch, op.bag_count = _lib.PM_F32, 0, 0
    assert L.pm_embbag_fwd_padded(ctypes.byref(op), 8, None, None) == _lib.PM_OK      # no bags: nothing is launched
    # the guard: stash size = T * (row slot + state), refusals
    assert L.pm_pad_rows_guard_bytes(3, 128, _lib.PM_F32, _lib.PM_PAD_STATE_NONE) == 3 * 512
    assert L.pm_pad_rows_guard_bytes(3, 128, _lib.PM_BF16, _lib.PM_PAD_STATE_ROW) == 3 * (256 + 16)
    assert L.pm_pad_rows_guard_bytes(3, 128, _lib.PM_F16, _lib.PM_PAD_STATE_ELEM) == 3 * (256 + 512)
    assert L.pm_pad_rows_guard_bytes(3, 128, 7, 0) == _lib.PM_ERR_INVALID and L.pm_pad_rows_guard_bytes(3, 128, _lib.PM_F32, 3) == _lib.PM_ERR_INVALID
    assert L.pm_pad_rows_guard_bytes(0, 128, _lib.PM_F32, 0) == _lib.PM_ERR_INVALID
    assert L.pm_pad_rows_guard_bytes(3, 12, _lib.PM_BF16, 0) == _lib.PM_ERR_UNSUPPORTED
    g = lambda *a: L.pm_pad_rows_guard(*a)                                     # noqa: E731
    assert g(1, 8, None, 16, _lib.PM_F32, 16, None, 0, 16, 1 << 20, 0, None) == _lib.PM_ERR_INVALID       # tables NULL
    assert g(1, 8, 16, 16, _lib.PM_F32, None, None, 0, 16, 1 << 20, 0, None) == _lib.PM_ERR_INVALID       # padding_idx NULL
    assert g(1, 8, 16, 16, _lib.PM_F32, 16, None, 1, 16, 1 << 20, 0, None) == _lib.PM_ERR_INVALID         # state NULL with a state kind
    assert g(1, 8, 16, 16, _lib.PM_F32, 16, None, 0, 16, 31, 0, None) == _lib.PM_ERR_INVALID and b"32 bytes" in L.pm_last_error()
    assert g(1, 8, 16, 16, _lib.PM_F32, 16, None, 0, 16, 1 << 20, 2, None) == _lib.PM_ERR_INVALID and b"direction" in L.pm_last_error()
    assert g(1, 8, 16, 16, _lib.PM_F32, 16, None, 0, 8, 1 << 20, 0, None) == _lib.PM_ERR_INVALID and b"aligned" in L.pm_last_error()
