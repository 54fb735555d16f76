"""The batched sequence backward without a GPU: the numpy rule (tests/sequence_grad_rules.py) against torch's CPU autograd of one
``nn.Embedding`` per table; the five ``pm_embseq_*`` names in the header, in ``_lib`` and in the library, with the ABI version and the
request struct unchanged; every host-side refusal of the C ABI, before any HIP call; and what the ``sequence_*`` methods of
``BatchedEmbeddingBagMI355`` refuse before they need a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import sequence_grad_rules as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pm_embseq_sort_indices", "pm_embseq_bwd_sorted", "pm_embseq_bwd_fused", "pm_embseq_bwd_sorted_adagrad",
         "pm_embseq_bwd_fused_adagrad")


# ---- 1. the rule is torch's embedding_dense_backward, per table ---------------------------------------------------------------------

def test_rule_is_torch_cpu_autograd_of_three_embeddings_bit_for_bit():
    """T = 3, ragged bags, rows repeated up to dozens of times, table 1 with a padding row: every table's gradient equals
    ``nn.Embedding(...)(indices of its stretch).backward(gradient rows of its stretch)`` bit for bit"""
    rows, D, B, pads = [9, 40, 5], 8, 6, [None, 3, None]
    rng = np.random.default_rng(1)
    lens = rng.integers(0, 7, 3 * B)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(off[-1])
    idx = np.concatenate([rng.integers(0, rows[t], int(off[(t + 1) * B] - off[t * B])) for t in range(3)]).astype(np.int64)
    lo1, hi1 = int(off[B]), int(off[2 * B])
    idx[lo1:lo1 + 4] = 3                                                        # the padding row is looked up
    assert np.bincount(idx[:lo1], minlength=rows[0]).max() >= 3 and hi1 - lo1 >= 8
    g = rng.standard_normal((N, D)).astype(np.float32)
    got = S.dense_grad(rows, [D] * 3, idx, off[:-1], B, g, pads)
    assert S.table_slices(off[:-1], 3, B, N) == [(int(off[t * B]), int(off[(t + 1) * B])) for t in range(3)]
    for t in range(3):
        lo, hi = int(off[t * B]), int(off[(t + 1) * B])
        m = torch.nn.Embedding(rows[t], D, padding_idx=pads[t])
        m(torch.from_numpy(idx[lo:hi])).backward(torch.from_numpy(g[lo:hi]))
        assert np.array_equal(m.weight.grad.numpy().view(np.uint32), got[t].view(np.uint32)), t
    assert not got[1][3].any() and got[1].any()


def test_rule_reads_nothing_outside_the_slice():
    rows, D, B = [6, 7], 4, 5
    rng = np.random.default_rng(2)
    lens = rng.integers(1, 4, 2 * B)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)[:-1]
    N = int(lens.sum())
    idx = np.concatenate([rng.integers(0, rows[t], int(lens[t * B:(t + 1) * B].sum())) for t in range(2)])
    g = rng.standard_normal((N, D)).astype(np.float32)
    sl = S.table_slices(off, 2, B, N, 1, 3)
    assert sl == [(int(off[1]), int(off[4])), (int(off[B + 1]), int(off[B + 4]))]
    poisoned = g.copy()
    keep = np.zeros(N, dtype=bool)
    for lo, hi in sl:
        keep[lo:hi] = True
    poisoned[~keep] = np.nan
    a, b = S.dense_grad(rows, [D, D], idx, off, B, g, slice=(1, 3)), S.dense_grad(rows, [D, D], idx, off, B, poisoned, slice=(1, 3))
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b)) and not np.isnan(b[0]).any()
    assert S.table_slices(off, 2, B, N, 2, 0) == [(0, 0), (0, 0)]


# ---- 2. the names, the ABI version, the struct ---------------------------------------------------------------------------------------

def test_header_lib_and_bindings_agree_on_the_five_names():
    from param_amd import _lib

    header = open(os.path.join(ROOT, "include", "param_amd.h")).read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(const pm_embbag_batch\* op,", header, re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
    L = _lib.load()
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and fn.argtypes[0]._type_ is _lib.pm_embbag_batch
    assert [len(getattr(L, n).argtypes) for n in NAMES] == [5, 10, 10, 12, 12]
    assert re.search(r"#define\s+PM_ABI_VERSION\s+8\b", header) and _lib.PM_ABI_VERSION == 8 and L.pm_abi_version() == 8
    assert ctypes.sizeof(_lib.pm_embbag_batch) == 144


# ---- 3. every host-side refusal, before any HIP call ----------------------------------------------------------------------------------

def _valid_op(_lib, T=2, D=8, N=100, B=4, wdt=None):
    op = _lib.pm_embbag_batch()
    op.num_tables, op.weight_dtype, op.index_dtype, op.max_dim = T, _lib.PM_F32 if wdt is None else wdt, _lib.PM_I64, D
    op.tables = op.rows = op.dims = op.out_offsets = op.indices = op.offsets = 64      # non-null dummies, never dereferenced on the host
    op.batch, op.bag_count, op.num_indices, op.out_stride = B, B, N, 4
    return op


def test_argument_validation_without_gpu():
    from param_amd import _lib

    L = _lib.load()
    F32, BF16, INVALID, UNSUPPORTED = _lib.PM_F32, _lib.PM_BF16, _lib.PM_ERR_INVALID, _lib.PM_ERR_UNSUPPORTED
    op = _valid_op(_lib)
    ref, MR, WS, BIG = ctypes.byref(op), 1000, 4096, 1 << 40
    opt = _lib.pm_rowwise_adagrad(0.1, 1e-8, 0.0, _lib.PM_WD_NONE, 0, 0, 0)
    err = L.pm_last_error

    def sort(ws=WS, nbytes=BIG, mr=MR, o=ref):
        return L.pm_embseq_sort_indices(o, mr, ws, nbytes, None)

    def sgd(fn, grad=64, stride=8, dst=64, dt=F32, ws=WS, nbytes=BIG, mr=MR, o=ref):
        return fn(o, grad, stride, dst, dt, 1.0, mr, ws, nbytes, None)

    def ada(fn, grad=64, stride=8, tabs=64, dt=F32, state=64, options=opt, elem=0, ws=WS, nbytes=BIG, mr=MR, o=ref):
        return fn(o, grad, stride, tabs, dt, state, None if options is None else ctypes.byref(options), elem, mr, ws, nbytes, None)

    every = [sort, lambda **kw: sgd(L.pm_embseq_bwd_sorted, **kw), lambda **kw: sgd(L.pm_embseq_bwd_fused, **kw),
             lambda **kw: ada(L.pm_embseq_bwd_sorted_adagrad, **kw), lambda **kw: ada(L.pm_embseq_bwd_fused_adagrad, **kw)]
    with_grad = every[1:]
    applies = [every[1], every[3]]

    # everything pm_embbag_bwd_sorted refuses
    for f in every:
        assert f(o=None) == INVALID and b"op is NULL" in err()
    op.num_tables = 0
    for f in every:
        assert f() == INVALID and b"num_tables" in err()
    op.num_tables = 1025
    for f in every:
        assert f() == UNSUPPORTED and b"at most 1024 tables" in err()
    op.num_tables, op.num_indices = 2, 1 << 32
    for f in every:
        assert f() == UNSUPPORTED and b"below 2^32" in err()
    op.num_indices = 100
    for f in every:
        assert f(mr=0) == INVALID and b"max_rows" in err()
    op.index_dtype = 99
    for f in every:
        assert f() == INVALID and b"index_dtype" in err()
    op.index_dtype, op.weight_dtype = _lib.PM_I64, 7
    assert sort() == INVALID and b"dtype" in err()
    op.weight_dtype = F32
    for f in with_grad:
        assert f(dt=7) == INVALID and b"dtype" in err()
    op.max_dim = 12                                                                  # a 16-bit destination: dims multiples of 8
    for f in with_grad:
        assert f(dt=BF16, stride=12) == UNSUPPORTED and b"multiple of 8" in err()
    op.max_dim = 8
    need = L.pm_embbag_bwd_sorted_workspace(ref, MR)
    assert need > 0
    for f in (every[0], every[1], every[3]):
        assert f(ws=None) == INVALID and b"workspace too small" in err()
        assert f(nbytes=need - 1) == INVALID and b"workspace too small" in err()
    # a missing sort: nothing has been sorted on this workspace (the record is a host-side table)
    for f in applies:
        assert f() == INVALID and b"pm_embseq_sort_indices has not been called" in err()

    # unweighted, un-blocked
    op.per_sample_weights = 64
    for f in every:
        assert f() == UNSUPPORTED and b"per_sample_weights" in err()
    op.per_sample_weights = None
    for field, value in (("table_group", 2), ("grad_block_shift", 2), ("grad_block_extra", 64)):
        setattr(op, field, value)
        if field == "grad_block_extra":
            op.grad_block_shift = 2                                                  # (an extra needs a shift: the request's own rule)
        for f in every:
            assert f() == UNSUPPORTED and b"blocked" in err(), field
        op.table_group = op.grad_block_shift = op.grad_block_extra = 0

    # the gradient
    for f in with_grad:
        assert f(grad=None) == INVALID and b"grad is NULL" in err()
        assert f(grad=64 + 8) == INVALID and b"16-byte aligned" in err()
        assert f(stride=4) == INVALID and b"grad_row_stride" in err()            # < max_dim
        assert f(stride=10) == INVALID and b"grad_row_stride" in err()           # not a multiple of 4
    for f in (every[1], every[2]):
        assert f(dst=None) == INVALID and b"NULL" in err()

    # Adagrad: options, state, width, the elementwise flag
    for f in every[3:]:
        assert f(elem=2) == INVALID and b"elementwise" in err()
        assert f(elem=-1) == INVALID and b"elementwise" in err()
        assert f(options=None) == INVALID and b"options are NULL" in err()
        assert f(state=None) == INVALID and b"NULL" in err()
        assert f(tabs=None) == INVALID and b"NULL" in err()
        bad = _lib.pm_rowwise_adagrad(0.1, 1e-8, 0.0, 9, 0, 0, 0)
        assert f(options=bad) == INVALID and b"weight_decay_mode" in err()
    op.max_dim = 260
    for f in every[3:]:
        for elem in (0, 1):
            assert f(stride=260, elem=elem) == UNSUPPORTED and b"max_dim <= 256" in err()
    op.max_dim, op.weight_dtype = 520, BF16
    for f in every[3:]:
        assert f(stride=520, dt=BF16) == UNSUPPORTED and b"max_dim <= 512" in err()


def test_empty_requests_are_ok_without_a_launch():
    """num_indices == 0 or bag_count == 0: PM_OK, no workspace, no gradient, no sort needed"""
    from param_amd import _lib

    L = _lib.load()
    opt = _lib.pm_rowwise_adagrad(0.1, 1e-8, 0.0, _lib.PM_WD_NONE, 0, 0, 0)
    for n, bags in ((0, 4), (100, 0)):
        op = _valid_op(_lib, N=n)
        op.bag_count = bags
        if n == 0:
            op.indices = None
        ref = ctypes.byref(op)
        grad = None if n == 0 else 64
        assert L.pm_embseq_sort_indices(ref, 1000, None, 0, None) == _lib.PM_OK
        for fn in (L.pm_embseq_bwd_sorted, L.pm_embseq_bwd_fused):
            assert fn(ref, grad, 8, None, _lib.PM_F32, 1.0, 1000, None, 0, None) == _lib.PM_OK, (n, bags)
        for fn in (L.pm_embseq_bwd_sorted_adagrad, L.pm_embseq_bwd_fused_adagrad):
            for elem in (0, 1):
                assert fn(ref, grad, 8, None, _lib.PM_F32, None, ctypes.byref(opt), elem, 1000, None, 0, None) == _lib.PM_OK, (n, bags)


# ---- 4. the module's refusals on the CPU ---------------------------------------------------------------------------------------------

def test_sequence_method_refusals_without_a_device():
    from param_amd import BatchedEmbeddingBagMI355

    idx, off = torch.zeros(6, dtype=torch.int64), torch.arange(0, 7, 1, dtype=torch.int64)
    g = torch.zeros(6, 8)
    mk = lambda dims=8, **kw: BatchedEmbeddingBagMI355([5, 6, 7], dims, device="cpu", init=None, **kw)      # noqa: E731

    def calls(m, grad=g):
        return [lambda: m.sequence_sort_indices(idx, off), lambda: m.sequence_scatter_add_(grad, idx, off, 1.0),
                lambda: m.sequence_optimizer_step_(grad, idx, off), lambda: m.sequence_dense_grad(grad, idx, off)]

    for m, text in ((mk(layout="blocked", block_bags=2), 'layout="blocked"'), (mk(dims=[8, 16, 8]), "one common embedding dim"),
                    (mk(pooling_mode="mean"), "no un-pooled form")):
        for c in calls(m):
            with pytest.raises(ValueError, match=text):
                c()
    m = mk()
    for bad in (torch.zeros(6, 8, dtype=torch.float16), torch.zeros(5, 8), torch.zeros(6, 4), torch.zeros(6, 8, dtype=torch.float64),
                torch.zeros(48)):
        for c in calls(m, bad)[1:]:
            with pytest.raises(ValueError, match="grad must be float32 of shape"):
                c()
    h = mk(output_dtype="bf16")
    for c in calls(h, torch.zeros(6, 8, dtype=torch.float16))[1:]:
        with pytest.raises(ValueError, match="bfloat16"):
            c()
    # sound requests reach "no CPU fallback": fp32 always, and the module's own 16-bit dtype
    for mod, grad in ((m, g), (h, g), (h, g.to(torch.bfloat16))):
        for c in calls(mod, grad):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                c()
    # pooling_mode NONE stays a constructor refusal: the sequence calls are methods of a sum module
    for none in ("none", 2):
        with pytest.raises(ValueError, match="pooling_mode"):
            mk(pooling_mode=none)
    # forward_sequence without autograd glue is lookup_sequence
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_sequence(idx, off)
    with pytest.raises(ValueError, match="no un-pooled form"):
        mk(pooling_mode="mean").forward_sequence(idx, off)
