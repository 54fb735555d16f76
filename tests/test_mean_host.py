"""Mean pooling, the parts that need no GPU: the numpy restatement of the rule (tests/mean_rules.py) against torch's CPU
``nn.EmbeddingBag(mode="mean")`` on fp32 tables -- forward bit for bit, dense and sparse gradient bit for bit where no row is looked
up twice and within a derived bound otherwise --; the division's special values; what the two modules accept and refuse at
construction and how fbgemm's ``PoolingMode`` values are read (``device="cpu"``: nothing is launched); the two new entry points in the header, the binding and
both libraries, with the ABI version and the request struct where they were; their host-side refusals."""
import ctypes
import enum
import os

import numpy as np
import pytest
import torch

import param_amd
from param_amd import _lib
from param_amd.embedding_bag import pooling_mode_name
from tests import mean_rules as M
from tests import padding_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS, DIM, BAGS = 11, 8, 23


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _torch_bag(weight, pad, sparse=False):
    return torch.nn.EmbeddingBag(weight.shape[0], weight.shape[1], mode="mean", padding_idx=pad, sparse=sparse,
                                 _weight=torch.from_numpy(weight.copy()))


def _request(rng, pad, fixed=None, n_rows=N_ROWS):
    """1-D request over one table (with ~40 % padding when it has a padding row), plus the edge bags: all padding (or a second empty
    bag), empty, a bag of one, padding first and last -> (indices, offsets [B], padding row or None)"""
    k = None if pad is None else pad % n_rows
    idx, off = R.padded_request(rng, [n_rows], BAGS, [k], share=0.4, max_len=6, fixed=fixed, closed=False)
    if fixed is None:
        other = ((k or 0) + 1) % n_rows
        kk = [] if k is None else [k]
        extra = [kk * 3, [], [other], kk + [other, other], [other, other] + kk]
        off = np.concatenate([off, idx.size + np.cumsum([0] + [len(e) for e in extra[:-1]])]).astype(np.int64)
        idx = np.concatenate([idx, np.array(sum(extra, []), dtype=np.int64)])
    return idx, off, k


def _once_request(rng, pad, n_rows=64, bags=BAGS):
    """every row looked up at most once (the padding row any number of times): a permutation dealt over ragged bags, one of them
    empty, with padded lookups sprinkled in"""
    k = None if pad is None else pad % n_rows
    perm = [r for r in rng.permutation(n_rows).tolist() if r != k]
    cuts = np.sort(rng.integers(0, len(perm) + 1, bags - 1))
    cuts[3] = cuts[2]                                                          # an empty bag
    bags_l = [perm[a:b] for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(perm)]]))]
    if k is not None:
        bags_l = [([k] if i % 3 == 0 else []) + b + ([k, k] if i % 4 == 1 else []) for i, b in enumerate(bags_l)]
    off = np.cumsum([0] + [len(b) for b in bags_l[:-1]]).astype(np.int64)
    return np.array(sum(bags_l, []), dtype=np.int64), off, k


# ---- the rule against torch's CPU module -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("pad", [None, 0, 3, -2])
def test_forward_rule_is_torch_bit_for_bit(pad):
    rng = np.random.default_rng(100 + (pad or 50))
    W = rng.standard_normal((N_ROWS, DIM)).astype(np.float32)
    idx, off, k = _request(rng, pad)
    B = off.size
    want = _torch_bag(W, pad)(torch.from_numpy(idx), torch.from_numpy(off)).detach().numpy()
    got = M.forward([W], idx, off, B, [k])[0]
    assert np.array_equal(_bits(got), _bits(want))
    n = M.count(idx, off, 1, B, [k])
    assert n[B - 5] == 0 and n[B - 4] == 0 and n[B - 3] == 1 and n[B - 2] == 2 and n[B - 1] == 2
    assert (_bits(got[B - 5]) == 0).all() and (_bits(got[B - 4]) == 0).all()      # the all-padding bag and the empty bag: +0.0
    assert np.array_equal(_bits(got[B - 3]), _bits(W[((k or 0) + 1) % N_ROWS]))     # a bag of one: the row itself
    assert n.max() >= 3 and (pad is None or 0.25 < R.padded_mask(idx, off, 1, B, [k]).mean() < 0.6)
    # 2-D input: fixed-length bags
    idx2, off2, _ = _request(rng, pad, fixed=7)
    want2 = _torch_bag(W, pad)(torch.from_numpy(idx2.reshape(BAGS, 7))).detach().numpy()
    assert np.array_equal(_bits(M.forward([W], idx2, off2, BAGS, [k])[0]), _bits(want2))


def _torch_grads(W, pad, idx, off, g):
    res = []
    for sparse in (False, True):
        m = _torch_bag(W, pad, sparse)
        m(torch.from_numpy(idx), torch.from_numpy(off)).backward(torch.from_numpy(g))
        res.append(m.weight.grad)
    return res[0].numpy(), res[1].coalesce()


@pytest.mark.parametrize("pad", [None, 0, 3, -2])
def test_gradients_are_torch_bit_for_bit_when_no_row_is_looked_up_twice(pad):
    rng = np.random.default_rng(300 + (pad or 50))
    n_rows = 64
    W = rng.standard_normal((n_rows, DIM)).astype(np.float32)
    idx, off, k = _once_request(rng, pad, n_rows)
    B = off.size
    keep = idx[idx != (-1 if k is None else k)]
    assert np.unique(keep).size == keep.size and (np.diff(np.concatenate([off, [idx.size]])) == 0).any()
    g = rng.standard_normal((B, DIM)).astype(np.float32)
    dense_t, coo = _torch_grads(W, pad, idx, off, g)
    dense = M.dense_grad([n_rows], [DIM], idx, off, B, [k], [g])[0]
    assert np.array_equal(_bits(dense), _bits(dense_t))
    rows, vals = M.sparse_grad([n_rows], [DIM], idx, off, B, [k], [g])[0]
    assert rows.tolist() == coo.indices()[0].numpy().tolist() and np.array_equal(_bits(vals), _bits(coo.values().numpy()))
    if k is not None:
        assert (_bits(dense[k]) == 0).all() and k not in rows.tolist()
    # ... and the other candidate rules are NOT torch's: dividing the gradient, or scaling in fp64
    n = M.count(idx, off, 1, B, [k]).astype(np.float64)
    has = n > 0
    bag = np.searchsorted(off, np.arange(idx.size), side="right") - 1
    sel = idx != (-1 if k is None else k)
    for other in ((g[has] / n[has, None].astype(np.float32)), (g[has].astype(np.float64) / n[has, None]).astype(np.float32)):
        alt = np.zeros_like(g)
        alt[has] = other
        d = np.zeros_like(dense)
        d[idx[sel]] = alt[bag[sel]]
        assert not np.array_equal(_bits(d), _bits(dense_t))


@pytest.mark.parametrize("pad", [None, 3, -2])
def test_gradients_with_repeated_rows_are_torch_within_the_derived_bound(pad):
    """torch adds the same fp32 contributions ``grad * r`` in another order: two fp32 sums of the k contributions of a row differ by
    at most 2 * (k - 1) * 2^-24 * sum |contribution| per element (each is within (k - 1) * 2^-24 * sum |c| of the exact sum, to
    first order; the bound is evaluated in float64)"""
    rng = np.random.default_rng(400 + (pad or 50))
    W = rng.standard_normal((N_ROWS, DIM)).astype(np.float32)
    idx, off, k = _request(rng, pad)
    B = off.size
    g = rng.standard_normal((B, DIM)).astype(np.float32)
    dense_t, coo = _torch_grads(W, pad, idx, off, g)
    dense = M.dense_grad([N_ROWS], [DIM], idx, off, B, [k], [g])[0]
    scaled = M.scale_grad([g], idx, off, B, [k])[0].astype(np.float64)
    bag = np.searchsorted(off, np.arange(idx.size), side="right") - 1
    sel = idx != (-1 if k is None else k)
    mag = np.zeros((N_ROWS, DIM))
    np.add.at(mag, idx[sel], np.abs(scaled[bag[sel]]))
    looks = np.bincount(idx[sel], minlength=N_ROWS)
    assert looks.max() >= 3
    bound = 2.0 * np.maximum(looks - 1, 0)[:, None] * 2.0 ** -24 * mag
    assert (np.abs(dense.astype(np.float64) - dense_t.astype(np.float64)) <= bound).all()
    rows, vals = M.sparse_grad([N_ROWS], [DIM], idx, off, B, [k], [g])[0]
    assert rows.tolist() == coo.indices()[0].numpy().tolist()
    assert (np.abs(vals.astype(np.float64) - coo.values().numpy().astype(np.float64)) <= bound[rows]).all()
    if k is not None:
        assert (_bits(dense[k]) == 0).all() and (_bits(dense_t[k]) == 0).all()


def test_the_division_and_the_scaling_on_special_values():
    tiny = np.float32(2.0 ** -126)                                           # the smallest normal
    W = np.zeros((6, DIM), dtype=np.float32)
    W[0, :] = tiny
    W[0, 1] = 7.0
    W[1, 0], W[1, 1], W[1, 2], W[1, 3] = -0.0, np.inf, -np.inf, np.nan
    W[5, :] = np.nan                                                         # the padding row
    idx = np.array([0, 2, 2, 1, 2, 5, 5, 0, 5], dtype=np.int64)
    off = np.array([0, 3, 5, 7], dtype=np.int64)                             # (tiny, 0, 0) | (special, 0) | (pad, pad) | (tiny, pad)
    got = M.forward([W], idx, off, 4, [5])[0]
    want = _torch_bag(W, 5)(torch.from_numpy(idx), torch.from_numpy(off)).detach().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    third = got[0, 0]
    assert 0 < third < tiny and third == np.float32(float(tiny) / 3.0)       # a subnormal quotient, correctly rounded
    assert got[0, 1] == np.float32(7.0) / np.float32(3.0) != np.float32(7.0) * (np.float32(1.0) / np.float32(3.0))      # a division, not a reciprocal
    assert got[1, 1] == np.inf and got[1, 2] == -np.inf and np.isnan(got[1, 3])
    # -0.0 / n stays -0.0 (a pooled sum starts from +0.0 and is -0.0 only after an underflow: the division itself is asked)
    assert _bits(M.divide(np.array([[-0.0, -1e-45]], dtype=np.float32), np.array([3])))[0].tolist() == [0x80000000, 0x80000000]
    assert _bits(got[1, 0:1])[0] == 0
    assert (_bits(got[2]) == 0).all()                                        # padding only: +0.0, the NaN row reached nothing
    assert np.array_equal(_bits(got[3]), _bits(W[0]))                        # count 1 although the bag has two entries
    assert np.isfinite(got[[0, 2, 3]]).all()
    # the gradient's scaling: r first, then one multiplication; +0.0 for a bag without kept lookups, whatever the gradient holds
    g = np.array([[3.0, -0.0, np.inf, np.nan, 1e-45, 1.0, 7.0, -5.0]] * 4, dtype=np.float32)
    s = M.scale_grad([g], idx, off, 4, [5])[0]
    r3 = np.float32(1.0) / np.float32(3.0)
    assert np.array_equal(_bits(s[0]), _bits(g[0] * r3)) and s[0, 6] != np.float32(7.0) / np.float32(3.0)
    assert _bits(s[0, 1:2])[0] == 0x80000000 and s[0, 2] == np.inf and np.isnan(s[0, 3])
    assert (_bits(s[2]) == 0).all() and np.array_equal(_bits(s[3]), _bits(g[3]))


def test_count_follows_slices_and_tables():
    rng = np.random.default_rng(7)
    rows, pads, B = [9, 4, 30], [2, None, 29], 6
    idx, off = R.padded_request(rng, rows, B, pads)
    n = M.count(idx, off, 3, B, pads)
    skip = R.padded_mask(idx, off, 3, B, pads)
    assert n.tolist() == [int((~skip[off[g]:off[g + 1]]).sum()) for g in range(3 * B)]
    W = [rng.standard_normal((r, DIM)).astype(np.float32) for r in rows]
    full, part = M.forward(W, idx, off, B, pads), M.forward(W, idx, off, B, pads, bag_begin=2, bag_count=3)
    assert all(np.array_equal(_bits(f[2:5]), _bits(p)) for f, p in zip(full, part))


# ---- constructors (device="cpu": nothing is launched) ---------------------------------------------------------------------------

class _PoolingMode(enum.IntEnum):      # fbgemm_gpu's enum, by shape
    SUM = 0
    MEAN = 1
    NONE = 2


def test_single_table_constructor_and_refusals():
    m = param_amd.EmbeddingBagMI355(10, 8, mode="mean", device="cpu", padding_idx=3)
    assert m.mode == "mean" and "mode=mean" in m.extra_repr() and "mode=mean" in repr(m)
    assert "mode=sum" in param_amd.EmbeddingBagMI355(10, 8, device="cpu").extra_repr()
    with pytest.raises(NotImplementedError):
        param_amd.EmbeddingBagMI355(10, 8, mode="max", device="cpu")
    idx, off = torch.zeros(6, dtype=torch.int64), torch.arange(3, dtype=torch.int64) * 2
    text = (r"^embedding_bag: per_sample_weights was not None\. per_sample_weights is only supported for mode='sum' "
            r"\(got mode='mean'\)\. Please open a feature request on GitHub\.$")
    with pytest.raises(NotImplementedError, match=text):
        m(idx, off, torch.ones(6))
    with pytest.raises(NotImplementedError, match=text):
        m(idx.reshape(3, 2), per_sample_weights=torch.ones(3, 2))
    with pytest.raises(NotImplementedError) as torchs:
        torch.nn.EmbeddingBag(10, 8, mode="mean")(idx, off, per_sample_weights=torch.ones(6))
    import re
    assert re.match(text, str(torchs.value))                                 # (the text is torch's)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(idx, off)                                                          # a sound request gets as far as the device check


def test_batched_constructor_and_refusals():
    mk = lambda **kw: param_amd.BatchedEmbeddingBagMI355([50, 7, 1000], 8, device="cpu", init=None, **kw)      # noqa: E731
    assert mk().pooling_mode == "sum" and not mk()._mean
    for spelling in ("mean", "MEAN", "Mean", 1, _PoolingMode.MEAN):
        assert mk(pooling_mode=spelling).pooling_mode == "mean" and mk(pooling_mode=spelling)._mean
    for spelling in ("sum", "SUM", 0, _PoolingMode.SUM):
        assert mk(pooling_mode=spelling).pooling_mode == "sum"
    for bad in ("none", "NONE", 2, _PoolingMode.NONE, "max", 3, -1, None, True, 1.0):
        with pytest.raises(ValueError, match="pooling_mode"):
            mk(pooling_mode=bad)
    with pytest.raises(ValueError, match="pooling_mode"):                    # validated before anything is allocated
        param_amd.BatchedEmbeddingBagMI355([2 ** 40], 2 ** 20, device="cpu", init=None, pooling_mode=2)
    with pytest.raises(ValueError, match="blocked"):
        param_amd.BatchedEmbeddingBagMI355([64, 64], 8, device="cpu", init=None, layout="blocked", block_bags=4, pooling_mode="mean")
    m = mk(pooling_mode="mean", padding_idx=(3, None, -1))
    i, o, w = torch.zeros(6, dtype=torch.int64), torch.arange(7, dtype=torch.int64), torch.ones(6)
    g = torch.zeros(2, 24)
    with pytest.raises(ValueError, match="per_sample_weights"):
        m.lookup(i, o, w)
    with pytest.raises(ValueError, match="per_sample_weights"):
        m(i, o, w)
    with pytest.raises(ValueError, match="mean"):
        mk(pooling_mode="mean").lookup(i, o, split_bags=True, batch=2)
    with pytest.raises(ValueError, match="mean"):
        mk(pooling_mode="mean").lookup_quantized(i, o, 8)
    with pytest.raises(ValueError, match="mean"):
        m.per_sample_weights_grad(g, i, o)


def test_the_plug_ins_pooling_mapping():
    from param_amd.compute.python.split_table_batched_embeddings_ops import SplitTableBatchedEmbeddingBagsCodegenOp

    """fbgemm's ``PoolingMode`` values as the module reads them; the operator plug-in itself keeps refusing every ``pooling`` but 0
    (tests/test_host_logic.py pins that refusal): mean pooling is reached through the module's ``pooling_mode``"""
    assert [pooling_mode_name(v) for v in (0, 1, "sum", "Mean", _PoolingMode.SUM, _PoolingMode.MEAN)] == ["sum", "mean"] * 3
    for bad in (2, _PoolingMode.NONE, "none"):
        with pytest.raises(ValueError, match="pooling_mode"):
            pooling_mode_name(bad)
    op = SplitTableBatchedEmbeddingBagsCodegenOp()
    op.device = "cuda:0"
    for pooling in (1, 2):
        with pytest.raises(ValueError, match="SUM"):
            op.build(2, 10, 8, pooling, False, "fp32", "sgd")
    op.device = "cpu"
    with pytest.raises(ValueError, match="Unknown compute device"):
        op.build(2, 10, 8, 0, False, "fp32", "sgd")                          # SUM gets as far as the device check


# ---- library surface ----------------------------------------------------------------------------------------------------------

NEW = ("pm_embbag_fwd_mean", "pm_embbag_mean_grad")


def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "param_amd.h")).read()
    for lib in (_lib.load(), _lib.load_alternates()):
        for name in NEW:
            assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS and name + "(" in header
        assert lib.pm_abi_version() == 8
    assert _lib.PM_ABI_VERSION == 8 and "#define PM_ABI_VERSION 8" in header
    assert ctypes.sizeof(_lib.pm_embbag_batch) == 144
    assert "mean_pool.hip" in open(os.path.join(ROOT, "param_amd", "csrc", "Makefile")).read()


def test_host_side_refusals_answer_before_a_hip_call():
    L = _lib.load()
    assert L.pm_embbag_fwd_mean(None, None, 16, None) == _lib.PM_ERR_INVALID
    assert L.pm_embbag_mean_grad(None, None, 16, 16, None) == _lib.PM_ERR_INVALID
    op = _lib.pm_embbag_batch()
    op.num_tables, op.weight_dtype, op.index_dtype, op.max_dim = 1, _lib.PM_F32, _lib.PM_I64, 8
    op.tables = op.rows = op.dims = op.out_offsets = 16                      # non-null dummies, never dereferenced on the host
    op.batch, op.bag_count, op.num_indices, op.indices, op.offsets = 4, 4, 8, 16, 16
    ref = ctypes.byref(op)
    assert L.pm_embbag_fwd_mean(ref, None, None, None) == _lib.PM_ERR_INVALID and b"out is NULL" in L.pm_last_error()
    assert L.pm_embbag_mean_grad(ref, None, None, 16, None) == _lib.PM_ERR_INVALID and b"NULL" in L.pm_last_error()
    assert L.pm_embbag_mean_grad(ref, None, 16, None, None) == _lib.PM_ERR_INVALID and b"NULL" in L.pm_last_error()
    assert L.pm_embbag_mean_grad(ref, None, 16, 24, None) == _lib.PM_ERR_INVALID and b"aligned" in L.pm_last_error()
    op.per_sample_weights = 16
    assert L.pm_embbag_fwd_mean(ref, None, 16, None) == _lib.PM_ERR_UNSUPPORTED and b"unweighted" in L.pm_last_error()
    op.per_sample_weights = None
    op.table_group = 2                                                       # the blocked forward's request
    assert L.pm_embbag_fwd_mean(ref, None, 16, None) == _lib.PM_ERR_UNSUPPORTED and b"blocked" in L.pm_last_error()
    assert L.pm_embbag_mean_grad(ref, None, 16, 16, None) == _lib.PM_ERR_UNSUPPORTED
    op.table_group, op.grad_block_shift, op.grad_block_extra = 0, 1, 64      # the blocked gradient
    assert L.pm_embbag_fwd_mean(ref, None, 16, None) == _lib.PM_ERR_UNSUPPORTED
    assert L.pm_embbag_mean_grad(ref, None, 16, 16, None) == _lib.PM_ERR_UNSUPPORTED and b"blocked" in L.pm_last_error()
    op.grad_block_shift, op.grad_block_extra = 0, 0
    op.weight_dtype = 7
    assert L.pm_embbag_fwd_mean(ref, None, 16, None) == _lib.PM_ERR_INVALID and b"dtype" in L.pm_last_error()
    assert L.pm_embbag_mean_grad(ref, None, 16, 16, None) == _lib.PM_ERR_INVALID
    op.weight_dtype, op.batch, op.bag_count = _lib.PM_F32, 0, 0
    assert L.pm_embbag_fwd_mean(ref, None, None, None) == _lib.PM_OK          # no bags: nothing is launched
    assert L.pm_embbag_mean_grad(ref, None, None, None, None) == _lib.PM_OK
