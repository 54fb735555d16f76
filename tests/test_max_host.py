"""MAX POOLING without a GPU: the numpy restatement (tests/max_rules.py) against torch's CPU module -- live and through
tests/golden/max_cases.npz --, the special cases that file is built around, the modules' refusals and the host side of the two new C
calls."""
import ctypes
import os

import numpy as np
import pytest
import torch

import param_amd
from param_amd import _lib
from param_amd import embedding_bag as EB
from tests import max_cases as C
from tests import max_rules as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS, PADS, DNAMES = ("1d", "2d"), ("pad", "nopad"), ("f32", "bf16", "f16")


def _pad(pname):
    return C.pad() if pname == "pad" else None


def _rule(form, pname, dname):
    """(values, args, dense gradient) of the rule for one recorded case"""
    idx, off, B, _ = C.request(form)
    vals, args = M.forward([C.table32(dname)], idx, off, B, [_pad(pname)])
    dw = M.dense_grad([C.ROWS], [C.DIM], [C.grad(form, dname)], args)
    return vals[0], args[0], dw[0]


def _torch_live(form, pname, dname):
    idx, off, B, i2 = C.request(form)
    w = C.table(dname).requires_grad_(True)
    if i2 is None:
        out = torch.nn.functional.embedding_bag(torch.from_numpy(idx), w, torch.from_numpy(off), mode="max", padding_idx=_pad(pname))
    else:
        out = torch.nn.functional.embedding_bag(torch.from_numpy(i2), w, mode="max", padding_idx=_pad(pname))
    out.backward(torch.from_numpy(C.grad(form, dname)).to(w.dtype))
    return out.detach().float().numpy(), w.grad.float().numpy()


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("pname", PADS)
@pytest.mark.parametrize("form", FORMS)
def test_rule_is_torch_bit_for_bit_recorded_and_live(form, pname, dname):
    val, arg, dw = _rule(form, pname, dname)
    t_out, t_arg, t_dw = C.torch_result(form, pname, dname)
    assert np.array_equal(M.bits(val), M.bits(t_out))
    assert np.array_equal(M.bits(dw), M.bits(t_dw))
    kept = arg >= 0                                         # (torch writes 0 for a bag without kept lookups and never reads it)
    assert np.array_equal(arg[kept], t_arg[kept]) and (t_arg[~kept] == 0).all()
    live_out, live_dw = _torch_live(form, pname, dname)
    assert np.array_equal(M.bits(val), M.bits(live_out))
    assert np.array_equal(M.bits(dw), M.bits(live_dw))


def test_the_cases_hold_the_conditions_they_were_built_for():
    w, pad, bags = C.table32("f32"), C.pad(), C.bags("1d")
    idx, off, B, _ = C.request("1d")
    (v,), (a,) = M.forward([w], idx, off, B, [pad])
    kept = [[r for r in bag if r != pad] for bag in bags]
    neg0, pos0 = np.uint32(0x80000000), np.uint32(0)
    # an empty bag, an all-padding bag: +0.0 and -1
    assert bags[0] == [] and bags[1] and kept[1] == []
    for b in (0, 1):
        assert (M.bits(v[b]) == pos0).all() and (a[b] == -1).all()
    # padding as a bag's first lookup; the padding row would win every column; the rest of the bag is negative: a negative maximum
    assert bags[2][0] == pad and (w[pad] > np.nan_to_num(w, nan=0.0, neginf=0.0).max(axis=0) - 1e-3).all()
    assert all((w[r] < 0).all() for r in kept[2]) and (v[2] < 0).all() and pad not in a[2]
    # a bag of one: the row itself, bit for bit
    assert len(bags[3]) == 1 and np.array_equal(M.bits(v[3]), M.bits(w[bags[3][0]]))
    # NaN first in column 0: stays; NaN only later: never enters
    assert np.isnan(w[kept[4][0], 0]) and np.isnan(v[4, 0]) and a[4, 0] == kept[4][0]
    assert not np.isnan(w[kept[5][0], 0]) and any(np.isnan(w[r, 0]) for r in kept[5][1:]) and not np.isnan(v[5, 0])
    assert v[5, 0] == max(w[r, 0] for r in kept[5] if not np.isnan(w[r, 0]))
    # -0.0 before +0.0 stays -0.0, and the reverse stays +0.0
    assert M.bits(w[bags[6][0], 1]) == neg0 and M.bits(w[bags[6][1], 1]) == pos0 and bags[7] == bags[6][::-1]
    assert M.bits(v[6, 1]) == neg0 and a[6, 1] == bags[6][0] and M.bits(v[7, 1]) == pos0 and a[7, 1] == bags[7][0]
    # equal maxima from two different rows: the first wins
    r0, r1 = bags[8]
    assert r0 != r1 and w[r0, 2] == w[r1, 2] and a[8, 2] == r0 and w[r0, 3] < w[r1, 3] and a[8, 3] == r1
    # a bag of -Inf
    assert np.isneginf(w[bags[9]]).all() and np.isneginf(v[9]).all() and (a[9] == bags[9][0]).all()
    # a row twice in one bag: the gradient arrives once; the same row in several bags
    twice = [r for r in set(bags[10]) if bags[10].count(r) == 2]
    assert twice and sum(twice[0] in bag for bag in bags) >= 3
    g = np.ones((B, C.DIM), dtype=np.float32)
    g_seq, written = M.expand(idx, off, B, [g], [a])
    assert written.all()
    s10 = int(off[10])
    cols = a[10] == twice[0]
    assert cols.any() and (g_seq[s10 + bags[10].index(twice[0])][cols] == 1).all()
    assert (g_seq[s10 + len(bags[10]) - 1 - bags[10][::-1].index(twice[0])] == 0).all()           # its second position gets +0.0
    (dw,) = M.dense_grad([C.ROWS], [C.DIM], [g], [a])
    assert np.array_equal(dw, np.stack([(a == r).sum(axis=0) for r in range(C.ROWS)]).astype(np.float32))
    assert (M.bits(dw[pad]) == pos0).all()
    # the expansion, summed per row in position order, is the dense gradient
    acc = np.zeros_like(dw)
    for j, r in enumerate(idx):
        acc[r] = acc[r] + g_seq[j]
    assert np.array_equal(M.bits(acc), M.bits(dw))
    # the 2-D form holds padding first, padding last, a padding-only row and a NaN first / later
    i2 = C.request("2d")[3]
    assert i2[0, 0] == pad and i2[2, -1] == pad and (i2[3] == pad).all() and np.isnan(w[i2[1, 0], 0]) and np.isnan(w[i2[2, 1], 0])


def test_expansion_honours_the_batch_slice():
    idx, off, B, _ = C.request("1d")
    (_, ), (a,) = M.forward([C.table32("f32")], idx, off, B, [C.pad()])
    g = C.grad("1d", "f32")
    full, _ = M.expand(idx, off, B, [g], [a])
    part, written = M.expand(idx, off, B, [g], [a], 4, 5)
    lo, hi = int(off[4]), int(off[9])
    assert written[lo:hi].all() and not written[:lo].any() and not written[hi:].any()
    assert np.array_equal(M.bits(part[lo:hi]), M.bits(full[lo:hi])) and not part[:lo].any() and not part[hi:].any()


# ---- the modules' surface ----------------------------------------------------------------------------------------------------------

def test_single_table_constructor_and_refusals():
    m = param_amd.MaxEmbeddingBagMI355(10, 8, device="cpu", padding_idx=3)
    assert m.mode == "max" and "mode=max" in m.extra_repr() and isinstance(m, param_amd.EmbeddingBagMI355)
    assert param_amd.MaxEmbeddingBagMI355(10, 8, mode="max", device="cpu").mode == "max"
    with pytest.raises(ValueError, match=r"^max mode does not support sparse weights$"):
        param_amd.MaxEmbeddingBagMI355(10, 8, sparse=True, device="cpu")
    with pytest.raises(ValueError) as torchs:
        torch.nn.functional.embedding_bag(torch.zeros(2, dtype=torch.int64), torch.zeros(4, 8), torch.zeros(1, dtype=torch.int64),
                                          mode="max", sparse=True)
    assert str(torchs.value) == "max mode does not support sparse weights"
    for cls, mode in ((param_amd.MaxEmbeddingBagMI355, "sum"), (param_amd.MaxEmbeddingBagMI355, "mean"),
                      (param_amd.EmbeddingBagMI355, "max")):                 # the class is the mode: neither constructor takes the other's
        with pytest.raises(NotImplementedError):
            cls(10, 8, mode=mode, device="cpu")
    idx, off = torch.zeros(6, dtype=torch.int64), torch.arange(3, dtype=torch.int64) * 2
    text = (r"^embedding_bag: per_sample_weights was not None\. per_sample_weights is only supported for mode='sum' "
            r"\(got mode='max'\)\. Please open a feature request on GitHub\.$")
    with pytest.raises(NotImplementedError, match=text):
        m(idx, off, torch.ones(6))
    with pytest.raises(NotImplementedError, match=text):
        m(idx.reshape(3, 2), per_sample_weights=torch.ones(3, 2))
    with pytest.raises(NotImplementedError, match=text):                     # (the text is torch's)
        torch.nn.EmbeddingBag(10, 8, mode="max")(idx, off, per_sample_weights=torch.ones(6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(idx, off)                                                          # a sound request gets as far as the device check


def test_batched_constructor_and_refusals():
    import enum

    class PoolingMode(enum.IntEnum):      # fbgemm_gpu's enum, by shape, with a member it does not have
        SUM = 0
        MEAN = 1
        NONE = 2
        MAX = 3

    mk = lambda **kw: param_amd.MaxBatchedEmbeddingBagMI355([50, 7, 1000], 8, device="cpu", init=None, **kw)      # noqa: E731
    base = lambda **kw: param_amd.BatchedEmbeddingBagMI355([50, 7, 1000], 8, device="cpu", init=None, **kw)      # noqa: E731
    for kw in ({}, {"pooling_mode": "max"}, {"pooling_mode": "MAX"}, {"pooling_mode": "Max"}):
        m = mk(**kw)
        assert m.pooling_mode == "max" and m._max and not m._mean and isinstance(m, param_amd.BatchedEmbeddingBagMI355)
    assert not base()._max and not base(pooling_mode="mean")._max
    for bad in (3, PoolingMode.MAX, 2, PoolingMode.NONE, "none", "sum", 0, None):      # the class pools with max; the string only
        with pytest.raises(ValueError, match="pooling_mode"):
            mk(pooling_mode=bad)
    for bad in ("max", 3, PoolingMode.MAX, 2, PoolingMode.NONE):              # the sum / mean constructor keeps refusing all of these
        with pytest.raises(ValueError, match="pooling_mode"):
            base(pooling_mode=bad)
    with pytest.raises(ValueError, match="blocked"):
        param_amd.MaxBatchedEmbeddingBagMI355([64, 64], 8, device="cpu", init=None, layout="blocked", block_bags=4)
    m = mk(padding_idx=(3, None, -1))
    i, o, w = torch.zeros(6, dtype=torch.int64), torch.arange(7, dtype=torch.int64), torch.ones(6)
    g, gs = torch.zeros(2, 24), torch.zeros(6, 8)
    for call in (lambda: m.lookup(i, o, w), lambda: m(i, o, w), lambda: m.dense_grad(g, i, o, w), lambda: m.scatter_add_(g, i, o, 1.0, w)):
        with pytest.raises(ValueError, match="per_sample_weights"):
            call()
    fused = "weight decay and state updates to looked-up rows whose gradient is zero"
    for call in (lambda: m.optimizer_step_(g, i, o), lambda: m.adagrad_step_(g, i, o)):
        with pytest.raises(ValueError, match=fused):
            call()
    for call in (lambda: m.sparse_grad(g, i, o), lambda: m.per_sample_weights_grad(g, i, o), lambda: m.lookup_sequence(i, o),
                 lambda: m.forward_sequence(i, o), lambda: m.sequence_sort_indices(i, o), lambda: m.sequence_scatter_add_(gs, i, o, 1.0),
                 lambda: m.sequence_optimizer_step_(gs, i, o), lambda: m.sequence_dense_grad(gs, i, o),
                 lambda: m.lookup(i, o, split_bags=True, batch=2), lambda: mk().lookup_quantized(i, o, 8)):
        with pytest.raises(ValueError, match="max"):
            call()
    for call in (lambda: m.dense_grad(g, i, o, method="atomic"), lambda: m.scatter_add_(g, i, o, 1.0, presorted=True)):
        with pytest.raises(ValueError, match="sequence backward"):
            call()
    mixed = param_amd.MaxBatchedEmbeddingBagMI355([50, 7], [8, 16], device="cpu", init=None)
    for call in (lambda: mixed.dense_grad(g, i, o), lambda: mixed.scatter_add_(g, i, o, 1.0)):
        with pytest.raises(ValueError, match="one common embedding dim"):
            call()
    # the fused .backward(): the forward is the lookup; its backward node refuses, with the reason
    with pytest.raises(ValueError, match=fused):
        EB._FusedMaxRefusedFn.apply(torch.zeros((), requires_grad=True), torch.zeros(2, 24)).sum().backward()
    # max-only arguments on a sum module
    s = base()
    for call in (lambda: s.lookup(i, o, return_max_indices=True), lambda: s(i, o, return_max_indices=True),
                 lambda: s.dense_grad(g, i, o, max_indices=torch.zeros(2, 24, dtype=torch.int32)),
                 lambda: s.scatter_add_(g, i, o, 1.0, max_indices=torch.zeros(2, 24, dtype=torch.int32))):
        with pytest.raises(ValueError, match="MaxBatchedEmbeddingBagMI355"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.lookup(i, o)                                                       # a sound request gets as far as the device check


def test_sum_and_mean_modules_never_call_the_new_entry_points(monkeypatch):
    """every route of a sum / mean module that can run without a device, with the new bindings and host functions booby-trapped"""
    def trap(*a, **k):
        raise AssertionError("a sum / mean module reached the max-pooling code")
    L = _lib.load()
    for name in ("pm_embbag_fwd_max", "pm_embbag_max_grad"):
        monkeypatch.setattr(L, name, trap, raising=True)
    for name in ("_fwd_max", "_max_expand", "_max_bwd"):
        monkeypatch.setattr(EB, name, trap, raising=True)
    calls = []
    monkeypatch.setattr(EB, "_fwd", lambda *a, **k: calls.append("fwd") or torch.zeros(1))
    monkeypatch.setattr(EB, "_bwd", lambda *a, **k: calls.append("bwd"))
    import types
    monkeypatch.setattr(EB.BatchedEmbeddingBagMI355, "_tables", lambda self: types.SimpleNamespace(d_ptrs=None))
    monkeypatch.setattr(EB.BatchedEmbeddingBagMI355, "_dense_grad_buffers", lambda self, ts, out: ([], None))
    monkeypatch.setattr(EB, "_require_device", lambda *a, **k: None)
    i, o, g = torch.zeros(6, dtype=torch.int64), torch.arange(7, dtype=torch.int64), torch.zeros(2, 24)
    for mode in ("sum", "mean"):
        m = param_amd.BatchedEmbeddingBagMI355([50, 7, 1000], 8, device="cpu", init=None, pooling_mode=mode, fused_update=False)
        monkeypatch.setattr(m, "_pad_dev", lambda: None)
        m.lookup(i, o)
        m(i, o)
        m.dense_grad(g, i, o)
        m.scatter_add_(g, i, o, 1.0)
        e = param_amd.EmbeddingBagMI355(10, 8, mode=mode, device="cpu")
        monkeypatch.setattr(e, "_tables", lambda: None)
        monkeypatch.setattr(e, "_pad_dev", lambda: None)
        with torch.no_grad():
            e(i, o[:3])
    assert calls == ["fwd", "fwd", "bwd", "bwd", "fwd"] * 2


# ---- library surface ---------------------------------------------------------------------------------------------------------------

NEW = ("pm_embbag_fwd_max", "pm_embbag_max_grad")


def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "param_amd.h")).read()
    for lib in (_lib.load(), _lib.load_alternates()):
        for name in NEW:
            assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS and name + "(" in header
        assert lib.pm_abi_version() == 8
    assert "MAX POOLING" in header and "#define PM_ABI_VERSION 8" in header and ctypes.sizeof(_lib.pm_embbag_batch) == 144
    mk = open(os.path.join(ROOT, "param_amd", "csrc", "Makefile")).read()
    assert "embbag_fwd_max.hip" in mk and "embbag_max_grad.hip" in mk


def test_host_side_refusals_answer_before_a_hip_call():
    L = _lib.load()
    F32, BF16 = _lib.PM_F32, _lib.PM_BF16
    assert L.pm_embbag_fwd_max(None, None, F32, 16, None, None) == _lib.PM_ERR_INVALID
    assert L.pm_embbag_max_grad(None, 16, F32, 16, 16, 8, None) == _lib.PM_ERR_INVALID
    op = _lib.pm_embbag_batch()
    op.num_tables, op.weight_dtype, op.index_dtype, op.max_dim = 1, F32, _lib.PM_I64, 8
    op.tables = op.rows = op.dims = op.out_offsets = 16                      # non-null dummies, never dereferenced on the host
    op.batch, op.bag_count, op.num_indices, op.indices, op.offsets = 4, 4, 8, 16, 16
    ref = ctypes.byref(op)
    fwd = lambda dt=F32, out=16, arg=None: L.pm_embbag_fwd_max(ref, None, dt, out, arg, None)                      # noqa: E731
    grd = lambda g=16, dt=F32, arg=16, gs=16, st=8: L.pm_embbag_max_grad(ref, g, dt, arg, gs, st, None)          # noqa: E731
    # what pm_embbag_fwd refuses
    op.max_dim = 6
    assert fwd() == _lib.PM_ERR_UNSUPPORTED and b"multiple of 4" in L.pm_last_error() and grd() == _lib.PM_ERR_UNSUPPORTED
    op.max_dim = 8
    # NULL and misaligned pointers
    assert fwd(out=None) == _lib.PM_ERR_INVALID and b"out is NULL" in L.pm_last_error()
    assert fwd(out=24) == _lib.PM_ERR_INVALID and b"aligned" in L.pm_last_error()
    assert fwd(BF16, out=20) == _lib.PM_ERR_INVALID and b"aligned" in L.pm_last_error()
    assert fwd(arg=24) == _lib.PM_ERR_INVALID and b"max_indices" in L.pm_last_error()
    for kw in ({"g": None}, {"arg": None}, {"gs": None}):
        assert grd(**kw) == _lib.PM_ERR_INVALID and b"NULL" in L.pm_last_error()
    for kw in ({"g": 24}, {"arg": 24}, {"gs": 24}, {"g": 20, "dt": BF16}):
        assert grd(**kw) == _lib.PM_ERR_INVALID and b"aligned" in L.pm_last_error()
    # an unknown dtype
    assert fwd(dt=7) == _lib.PM_ERR_INVALID and b"out_dtype" in L.pm_last_error()
    assert grd(dt=7) == _lib.PM_ERR_INVALID and b"grad_dtype" in L.pm_last_error()
    # the stride of g_seq
    for st in (4, 10):
        assert grd(st=st) == _lib.PM_ERR_INVALID and b"g_seq_row_stride" in L.pm_last_error()
    # mixed dims: the gradient call only
    op.max_dim, op.min_dim = 16, 8
    assert grd(st=16) == _lib.PM_ERR_UNSUPPORTED and b"one common embedding dim" in L.pm_last_error()
    op.max_dim, op.min_dim = 8, 0
    # per_sample_weights, blocked layouts
    op.per_sample_weights = 16
    assert fwd() == _lib.PM_ERR_UNSUPPORTED and b"unweighted" in L.pm_last_error() and grd() == _lib.PM_ERR_UNSUPPORTED
    op.per_sample_weights = None
    op.table_group = 2
    assert fwd() == _lib.PM_ERR_UNSUPPORTED and b"blocked" in L.pm_last_error() and grd() == _lib.PM_ERR_UNSUPPORTED
    op.table_group, op.grad_block_shift, op.grad_block_extra = 0, 1, 64
    assert fwd() == _lib.PM_ERR_UNSUPPORTED and grd() == _lib.PM_ERR_UNSUPPORTED and b"blocked" in L.pm_last_error()
    op.grad_block_shift, op.grad_block_extra = 0, 0
    op.weight_dtype = 7
    assert fwd() == _lib.PM_ERR_INVALID and b"dtype" in L.pm_last_error() and grd() == _lib.PM_ERR_INVALID
    # the empty request: PM_OK without a launch
    op.weight_dtype, op.batch, op.bag_count = F32, 0, 0
    assert fwd(out=None) == _lib.PM_OK and grd(None, F32, None, None) == _lib.PM_OK
    op.batch, op.bag_count, op.num_indices = 4, 4, 0
    assert grd(None, F32, None, None) == _lib.PM_OK
