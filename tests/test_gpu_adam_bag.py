"""AdamBatchedEmbeddingBagMI355 on the GPU: w, exp_avg and exp_avg_sq of every row of every table, bit for bit against
tests/adam_bag_rules.py, over two consecutive steps (the second sees non-zero state and another bias correction)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from param_amd import AdamBatchedEmbeddingBagMI355, _lib, sparse_adam_rows_
from param_amd.optim import _step_scalars
from tests import adam_bag_rules as R
from tests import mean_rules as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS, B = (50, 7, 300), 96
HYPER = {"lr": 1.0e-2, "betas": (0.9, 0.999), "eps": 1.0e-8}
DNAME = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
_bits = lambda x: x.detach().float().cpu().numpy().view(np.uint32)      # noqa: E731


@functools.lru_cache(maxsize=None)
def _base():
    """three tables, ragged bags (empty ones included) of about 12 lookups: about 3.4 k pairs, more than three tiles; the last rows of
    every table are never looked up; one bag holds a row twice"""
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 28, len(ROWS) * B)
    lens[rng.random(lens.size) < 0.1] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate([rng.integers(0, r - 1 - r // 10, int(lens[t * B:(t + 1) * B].sum())) for t, r in enumerate(ROWS)]).astype(np.int64)
    b = int(np.argmax(lens[:B] >= 2))
    idx[off[b] + 1] = idx[off[b]]
    assert off[-1] > 3 * 1024
    return idx, off, B


@functools.lru_cache(maxsize=None)
def _hot():
    """one table: rows looked up 256 (from sorted position 0), 257 and 600 times (sorted positions 516 .. 1115: two tiles), and cold ones"""
    nb = 600
    bags = [[3] + ([0] if b < 256 else []) + ([1] if b < 257 else []) + [5 + b % 7] + ([2] if b < 3 else []) for b in range(nb)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in bags])]).astype(np.int64)
    return np.concatenate(bags).astype(np.int64), off, nb


def _grads(dims, nb, seed, layout="bd", dtype=torch.float32):
    """(per-table float32 [nb, D_t] arrays holding values of `dtype`, the device tensor in `layout`)"""
    rng = np.random.default_rng(seed)
    dev = [torch.from_numpy(rng.standard_normal((nb, d)).astype(np.float32)).to(dtype) for d in dims]
    return [g.float().numpy() for g in dev], (torch.stack(dev) if layout == "tbd" else torch.cat(dev, 1)).to(DEV).contiguous()


def _module(rows, dims, dtype=torch.float32, **kw):
    return AdamBatchedEmbeddingBagMI355(rows, dims, dtype=dtype, device=DEV, init="normal", seed=5, learning_rate=HYPER["lr"], **kw)


def _state(m):
    return [(m.table(t).float().cpu().numpy(), m.exp_avg_table(t).cpu().numpy(), m.exp_avg_sq_table(t).cpu().numpy()) for t in range(len(m.rows))]


def _same(m, want, what):
    for t, (got, exp) in enumerate(zip(_state(m), want)):
        for name, a, b in zip(("w", "exp_avg", "exp_avg_sq"), got, exp):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, t, name)


def _two_steps(rows, dims, req, dtype=torch.float32, idt=torch.int64, wd=0.0, begin=0, count=None, **kw):
    idx_h, off_h, nb = req
    m = _module(rows, dims, dtype, weight_decay=wd, **kw)
    idx, off = torch.from_numpy(idx_h).to(DEV, idt), torch.from_numpy(off_h).to(DEV, idt)
    state, hyper, pads = _state(m), dict(HYPER, weight_decay=wd), m.padding_idx
    for step in (1, 2):
        g_h, g = _grads(dims, nb, step, m.layout, m.output_dtype)
        m.optimizer_step_(g, idx, off, batch=nb, bag_begin=begin, bag_count=count)
        if m.pooling_mode == "mean":
            g_h = M.scale_grad(g_h, idx_h, off_h, nb, pads or [None] * len(rows))
        state = R.step(state, R.summed_grads(dims, idx_h, off_h, nb, g_h, begin, count, pads), step, hyper, DNAME[dtype])
        _same(m, state, step)
    assert int(m.step) == 2
    return m


@pytest.mark.parametrize("dims,dtype,idt,wd", [
    ((8, 8, 8), torch.float32, torch.int64, 0.0), ((128, 128, 128), torch.float32, torch.int64, 0.0), ((8, 128, 320), torch.float32, torch.int64, 0.0),
    ((8, 128, 320), torch.bfloat16, torch.int64, 0.0), ((8, 128, 320), torch.float16, torch.int64, 0.0),
    ((8, 128, 320), torch.float32, torch.int32, 0.0), ((8, 128, 320), torch.float32, torch.int64, 0.01)])
def test_base_request(dims, dtype, idt, wd):
    _two_steps(ROWS, dims, _base(), dtype, idt, wd)


@pytest.mark.parametrize("D", [8, 128])
def test_hot_rows(D):
    idx_h, off_h, nb = _hot()
    runs = R.lookups(idx_h, off_h, nb, 0)
    assert [len(runs[r]) for r in (0, 1, 3)] == [256, 257, 600] and sum(len(runs[r]) for r in (0, 1, 2)) == 516
    _two_steps((20,), (D,), _hot())


@pytest.mark.parametrize("kw", [dict(output_dtype="bf16"), dict(layout="tbd"), dict(pooling_mode="mean"), dict(begin=10, count=70),
                                dict(padding_idx=[3, None, 5])], ids=lambda kw: next(iter(kw)))
def test_gradient_and_layout(kw):
    if "padding_idx" in kw:
        assert all(p is None or p in R.lookups(_base()[0], _base()[1], B, t) for t, p in enumerate(kw["padding_idx"]))
    _two_steps(ROWS, (128, 128, 128), _base(), **kw)


def test_eight_byte_keys():
    """``pm_embbag_bwd_adam`` with a ``max_rows`` of 2^30: the sort plan says 8-byte keys; the bits equal the module's 4-byte-key run"""
    dims, (idx_h, off_h, nb) = (8, 8, 8), _base()
    small = _two_steps(ROWS, dims, _base())
    m, L, max_rows = _module(ROWS, dims), _lib.load(), 1 << 30
    idx, off = torch.from_numpy(idx_h).to(DEV), torch.from_numpy(off_h).to(DEV)
    ts = m._tables()
    op = _lib.pm_embbag_batch.from_buffer_copy(ts.request(idx, off, nb, None, 0, None))
    op.fixed_pooling = 0
    buf = ctypes.create_string_buffer(512)
    assert L.pm_embbag_sort_plan(ctypes.byref(op), max_rows, 1, buf, 512) == _lib.PM_OK, L.pm_last_error()
    assert dict(kv.split("=") for kv in buf.value.decode().split())["key_bytes"] == "8"
    need = L.pm_embbag_bwd_adam_workspace(ctypes.byref(op), max_rows)
    assert 0 < need < 1 << 30, need
    ws, (mp, vp) = torch.empty(need, dtype=torch.uint8, device=DEV), m._state_ptrs()
    for step in (1, 2):
        opt = _step_scalars(step, HYPER["lr"], HYPER["betas"], HYPER["eps"], 0.0, False, True)
        g = _grads(dims, nb, step)[1]
        assert L.pm_embbag_bwd_adam(ctypes.byref(op), g.data_ptr(), _lib.PM_F32, ts.d_ptrs.data_ptr(), _lib.PM_F32, mp.data_ptr(), vp.data_ptr(),
                                    None, ctypes.byref(opt), max_rows, ws.data_ptr(), need, None) == _lib.PM_OK, L.pm_last_error()
    torch.cuda.synchronize()
    _same(m, _state(small), "8-byte keys")


def _pair(req, rows=ROWS, dims=(8, 128, 320), **kw):
    """two equal modules, and the request and a gradient on the device"""
    idx_h, off_h, nb = req
    return (_module(rows, dims, **kw), _module(rows, dims, **kw), torch.from_numpy(idx_h).to(DEV), torch.from_numpy(off_h).to(DEV),
            _grads(dims, nb, 1)[1])


def test_equals_sparse_grad_then_sparse_adam_rows():
    idx_h, off_h, nb = _base()
    assert max(len(run) for t in range(3) for run in R.lookups(idx_h, off_h, nb, t).values()) <= R.EXACT_RUN      # nothing is exempt
    a, b, idx, off, g = _pair(_base(), weight_decay=0.01)
    a.optimizer_step_(g, idx, off)
    T = range(3)
    sparse_adam_rows_([b.table(t) for t in T], b.sparse_grad(g, idx, off), [b.exp_avg_table(t) for t in T], [b.exp_avg_sq_table(t) for t in T],
                      1, HYPER["lr"], HYPER["betas"], HYPER["eps"], 0.01)
    _same(a, _state(b), "composition")


def test_fused_backward_is_optimizer_step():
    a, b, idx, off, g = _pair(_base())
    a(idx, off).backward(g)
    b.optimizer_step_(g, idx, off)
    _same(a, _state(b), "autograd")
    assert int(a.step) == 1 and bool(a.exp_avg.any())


def test_sort_left_behind_feeds_a_presorted_apply():
    """the step keeps its hot-run count in its own area, not in the sorted apply's control words: the inherited
    ``scatter_add_(presorted=True)`` on the sort it leaves equals a freshly sorted one, hot rows included"""
    nb = _hot()[2]
    a, b, idx, off, g = _pair(_hot(), (20,), (8,))
    for m in (a, b):
        m.optimizer_step_(g, idx, off, batch=nb)
    a.scatter_add_(g, idx, off, -0.5, batch=nb, presorted=True)
    b.scatter_add_(g, idx, off, -0.5, batch=nb)
    _same(a, _state(b), "presorted")
