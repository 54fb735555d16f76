"""The host layer's call trace, without a GPU and without a built library: which entry points of the C ABI every module method
reaches, in which order and with which arguments, for the options the methods take (pooling mode, padding, optimizer, bounds check
mode, layouts, batch slices, more than 1024 tables).  The library is replaced by a recorder (the pattern of
tests/test_bounds_check_host.py): every entry point is written down and returns 0 -- the size queries (``*_workspace``, ``*_bytes``,
``*_scratch``) return 64, so that the scratch tensors are real memory and the sizes handed on can be seen.  Modules live on the CPU.

A call is recorded as ``[name, [argument, ...]]``: scalars as they are; a pointer as ``"NULL"``, the label of the tensor it points
into (``"indices"``, ``"offsets"``, ``"grad"``, ``"weights"``, ``"out"``, the module's ``"pad"`` / ``"state"`` arrays and the table
set's ``"d_ptrs"`` / ``"d_rows"`` / ``"d_dims"`` / ``"d_col0"``; ``"label+bytes"`` behind its start) or ``"other"``; the request
struct as ``{"op": {...}}`` (its scalar fields and, labelled the same way, its pointers), the Adagrad options as ``{"opt": {...}}``.
``["--", step]`` lines separate the steps of a case, ``["raises", type, text]`` is a refusal.

The expected traces are tests/call_trace_host.json.  ``PARAM_AMD_REWRITE_CALL_TRACES=1 pytest tests/test_call_trace_host.py`` writes
that file anew from what the code does (every test then passes by construction: read the diff)."""
import json
import os

import pytest
import torch

import param_amd
from param_amd import _lib
from param_amd import embedding_bag as eb

TRACES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "call_trace_host.json")
REWRITE = os.environ.get("PARAM_AMD_REWRITE_CALL_TRACES") == "1"

_OP_SCALARS = ("num_tables", "batch", "bag_begin", "bag_count", "num_indices", "max_dim", "min_dim", "out_stride", "fixed_pooling",
               "grad_block_shift", "grad_block_extra", "table_group")
_OP_POINTERS = ("tables", "rows", "dims", "out_offsets", "indices", "offsets", "per_sample_weights")
_SIZE_QUERIES = ("_workspace", "_bytes", "_scratch")


class _Recorder:
    """stands in for the loaded library"""

    def __init__(self):
        self.calls = []
        self.named = []      # (label, tensor | callable giving a tensor or None), looked at when a call is recorded

    def step(self, name):
        self.calls.append(["--", name])

    def _ptr(self, a):
        if not a:
            return "NULL"
        for label, t in self.named:
            t = t() if callable(t) else t
            if t is None or t.numel() == 0:
                continue
            off = a - t.data_ptr()
            if 0 <= off < t.numel() * t.element_size():
                return label if off == 0 else f"{label}+{off}"
        return "other"

    def _arg(self, a):
        obj = getattr(a, "_obj", None)
        if isinstance(obj, _lib.pm_embbag_batch):
            d = {f: getattr(obj, f) for f in _OP_SCALARS}
            d.update({f: self._ptr(getattr(obj, f)) for f in _OP_POINTERS})
            return {"op": d}
        if isinstance(obj, _lib.pm_rowwise_adagrad):
            return {"opt": {f: getattr(obj, f) for f, _ in obj._fields_}}
        if a is None:
            return "NULL"
        if isinstance(a, int) and not isinstance(a, bool):
            return self._ptr(a) if a >= 1 << 32 else a      # (host addresses lie above 4 GB; no scalar of these calls does)
        if isinstance(a, (float, bool)):
            return a
        return type(a).__name__

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append([name, [self._arg(a) for a in args]])
            return 64 if name.endswith(_SIZE_QUERIES) else 0
        return fn


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(eb, "_require_device", lambda t, what: None)
    monkeypatch.setattr(eb, "_stream_ptr", lambda: 0)
    monkeypatch.setattr(_lib, "load", lambda: r)

    def sparse_call(ts, op, grad, max_rows, dims, pads=None):
        # the sparse gradient behind its prelude sizes its outputs from device contents: stubbed, its arguments written down
        r.calls.append(["_sparse_grad_call", [r._arg(_Byref(op)), r._ptr(grad.data_ptr()), max_rows, list(dims), pads]])
        return [(torch.empty(0, dtype=torch.int64), torch.empty((0, d), dtype=torch.float32)) for d in dims]
    monkeypatch.setattr(eb, "_sparse_grad_call", sparse_call)
    return r


class _Byref:
    def __init__(self, obj):
        self._obj = obj


def _attempt(rec, name, fn):
    """one step of a case: its calls, or the refusal it ends in"""
    rec.step(name)
    try:
        return fn()
    except (ValueError, NotImplementedError, TypeError) as e:
        rec.calls.append(["raises", type(e).__name__, str(e)])
        return None


_OP_KEYS = _OP_SCALARS + _OP_POINTERS
_expected = None


def _load():
    """the file keeps every distinct request struct once (``"ops"``: the values of _OP_KEYS) and the calls refer to it by number"""
    if not os.path.exists(TRACES):
        return {}
    data = json.load(open(TRACES))
    arg = lambda a: {"op": dict(zip(_OP_KEYS, data["ops"][a["op"]]))} if isinstance(a, dict) and "op" in a else a      # noqa: E731
    return {k: [[arg(a) if not isinstance(a, list) else [arg(b) for b in a] for a in c] for c in v] for k, v in data["cases"].items()}


def _store(cases):
    ops = []

    def arg(a):
        if isinstance(a, dict) and "op" in a:
            vals = [a["op"][k] for k in _OP_KEYS]
            if vals not in ops:
                ops.append(vals)
            return {"op": ops.index(vals)}
        return a
    cases = {k: [[arg(a) if not isinstance(a, list) else [arg(b) for b in a] for a in c] for c in v] for k, v in sorted(cases.items())}
    with open(TRACES, "w") as f:
        f.write('{"ops": [\n' + ",\n".join(" " + json.dumps(o) for o in ops) + '\n],\n"cases": {\n')
        f.write(",\n".join(f" {json.dumps(k)}: [\n" + ",\n".join("  " + json.dumps(c) for c in v) + "\n ]" for k, v in cases.items()))
        f.write("\n}}\n")


def _check(name, calls):
    """compare with (or, under the flag, store as) the recorded trace of this case"""
    global _expected
    calls = json.loads(json.dumps(calls))
    if _expected is None:
        _expected = _load()
    if REWRITE:
        _expected[name] = calls
        _store(_expected)
        return
    want = _expected[name]
    for i, (g, w) in enumerate(zip(calls, want)):
        assert g == w, f"{name}: call {i} differs\n got  {g}\n want {w}"
    assert len(calls) == len(want), f"{name}: {len(calls)} calls, expected {len(want)}: {[c[0] for c in calls]}"


# ---- BatchedEmbeddingBagMI355 -------------------------------------------------------------------------------------------------

def _batched(rec, rows, dims, **kw):
    m = param_amd.BatchedEmbeddingBagMI355(rows, dims, device="cpu", init=None, **kw)
    ts = lambda name: (lambda: getattr(m._ts, name) if m._ts is not None else None)      # noqa: E731
    rec.named += [("pad", m._pad_dev), ("state", lambda: m._mom_ptrs), ("weights", m.weights.data),
                  ("d_ptrs", ts("d_ptrs")), ("d_rows", ts("d_rows")), ("d_dims", ts("d_dims")), ("d_col0", ts("d_col0"))]
    return m


def _request(rec, rows, B, L=2):
    T = len(rows)
    idx = torch.arange(T * B * L, dtype=torch.int64) % min(rows)
    off = torch.arange(T * B + 1, dtype=torch.int64) * L
    rec.named += [("indices", idx), ("offsets", off)]
    return idx, off


def _named(rec, label, t):
    rec.named.append((label, t))
    return t


ROWS3 = [5, 6, 7]
PADS3 = [0, None, -1]


@pytest.mark.parametrize("bounds", ["none", "ignore", "warning"])
@pytest.mark.parametrize("optimizer", ["sgd", "rowwise_adagrad", "adagrad"])
@pytest.mark.parametrize("padding", ["nopad", "pad"])
@pytest.mark.parametrize("pooling", ["sum", "mean"])
def test_batched_module_every_entry_point(rec, pooling, padding, optimizer, bounds):
    T, B, D = 3, 4, 8
    m = _batched(rec, ROWS3, D, pooling_mode=pooling, padding_idx=PADS3 if padding == "pad" else None, optimizer=optimizer,
                 bounds_check_mode=bounds, learning_rate=0.5)
    idx, off = _request(rec, ROWS3, B)
    grad = _named(rec, "grad", torch.ones(B, T * D))
    out = _named(rec, "out", torch.empty(B, T * D))
    psw = _named(rec, "psw", torch.ones(idx.numel(), requires_grad=True))
    dense = [torch.zeros(r, D) for r in ROWS3]
    _attempt(rec, "lookup", lambda: m.lookup(idx, off))
    _attempt(rec, "lookup slice out=", lambda: m.lookup(idx, off, out=out, bag_begin=1, bag_count=2))
    _attempt(rec, "lookup weighted", lambda: m.lookup(idx, off, psw.detach()))
    _attempt(rec, "lookup split_bags", lambda: m.lookup(idx, off, split_bags=True))
    _attempt(rec, "forward backward", lambda: m(idx, off).sum().backward())
    _attempt(rec, "forward backward weighted", lambda: m(idx, off, psw).sum().backward())
    _attempt(rec, "scatter_add_", lambda: m.scatter_add_(grad, idx, off, alpha=-0.25))
    _attempt(rec, "scatter_add_ slice weighted", lambda: m.scatter_add_(grad, idx, off, -0.25, psw.detach(), bag_begin=1, bag_count=2))
    _attempt(rec, "sort_indices", lambda: m.sort_indices(idx, off, for_adagrad=False))
    _attempt(rec, "scatter_add_ presorted", lambda: m.scatter_add_(grad, idx, off, alpha=-0.25, presorted=True))
    _attempt(rec, "adagrad_step_", lambda: m.adagrad_step_(grad, idx, off))
    _attempt(rec, "adagrad_step_ weighted", lambda: m.adagrad_step_(grad, idx, off, psw.detach()))
    _attempt(rec, "optimizer_step_", lambda: m.optimizer_step_(grad, idx, off))
    _attempt(rec, "dense_grad", lambda: m.dense_grad(grad, idx, off))
    _attempt(rec, "dense_grad out=", lambda: m.dense_grad(grad, idx, off, out=dense))
    _attempt(rec, "dense_grad weighted", lambda: m.dense_grad(grad, idx, off, psw.detach()))
    _attempt(rec, "sparse_grad", lambda: m.sparse_grad(grad, idx, off))
    _attempt(rec, "sparse_grad slice weighted", lambda: m.sparse_grad(grad, idx, off, psw.detach(), bag_begin=1, bag_count=2))
    _attempt(rec, "per_sample_weights_grad", lambda: m.per_sample_weights_grad(grad, idx, off))
    _attempt(rec, "per_sample_weights_grad slice out=",
             lambda: m.per_sample_weights_grad(grad, idx, off, out=_named(rec, "psw_out", torch.empty(idx.numel())), bag_begin=1, bag_count=2))
    _attempt(rec, "sanitize_", lambda: m.sanitize_(idx, off))
    _attempt(rec, "sanitize_ ignore", lambda: m.sanitize_(idx, off, mode="ignore"))
    _attempt(rec, "lookup_quantized", lambda: m.lookup_quantized(idx, off, 8))
    _check(f"batched-{pooling}-{padding}-{optimizer}-{bounds}", rec.calls)


@pytest.mark.parametrize("padding", ["nopad", "pad"])
@pytest.mark.parametrize("pooling", ["sum", "mean"])
def test_batched_module_mixed_dims_and_tbd_layout(rec, pooling, padding):
    B, dims = 4, [8, 16, 8]
    kw = dict(pooling_mode=pooling, padding_idx=PADS3 if padding == "pad" else None)
    m = _batched(rec, ROWS3, dims, **kw)
    idx, off = _request(rec, ROWS3, B, L=3)
    grad = _named(rec, "grad", torch.ones(B, sum(dims)))
    _attempt(rec, "mixed lookup", lambda: m.lookup(idx, off))
    _attempt(rec, "mixed forward backward", lambda: m(idx, off).sum().backward())
    _attempt(rec, "mixed dense_grad", lambda: m.dense_grad(grad, idx, off))
    m2 = _batched(rec, ROWS3, 8, layout="tbd", optimizer="rowwise_adagrad", **kw)
    grad2 = _named(rec, "grad_tbd", torch.ones(3, B, 8))
    _attempt(rec, "tbd lookup", lambda: m2.lookup(idx, off, batch=B))
    _attempt(rec, "tbd scatter_add_", lambda: m2.scatter_add_(grad2, idx, off, alpha=1.0, pooling=3))
    _attempt(rec, "tbd adagrad_step_", lambda: m2.adagrad_step_(grad2, idx, off))
    if padding == "nopad":      # (with padding: test_a_refused_backward_with_padding_launches_nothing)
        _attempt(rec, "tbd wrong grad shape", lambda: m2.dense_grad(grad, idx, off))
    _check(f"batched-mixed-tbd-{pooling}-{padding}", rec.calls)


def test_batched_module_blocked_layout(rec):
    B = 4
    m = _batched(rec, ROWS3, 8, layout="blocked", block_bags=2)
    idx, off = _request(rec, ROWS3, B)
    grad = _named(rec, "grad", torch.ones(2, 3, 2, 8))
    _attempt(rec, "blocked lookup", lambda: m.lookup(idx, off))
    _attempt(rec, "blocked forward backward", lambda: m(idx, off).sum().backward())
    _attempt(rec, "blocked scatter_add_", lambda: m.scatter_add_(grad, idx, off, alpha=-1.0))
    _attempt(rec, "blocked lookup slice", lambda: m.lookup(idx, off, bag_begin=1))
    for kw in (dict(pooling_mode="mean"), dict(padding_idx=0)):
        _attempt(rec, f"blocked {kw}", lambda: param_amd.BatchedEmbeddingBagMI355(ROWS3, 8, device="cpu", init=None, layout="blocked",
                                                                                   block_bags=2, **kw))
    _check("batched-blocked", rec.calls)


@pytest.mark.parametrize("optimizer", ["sgd", "rowwise_adagrad", "adagrad"])
def test_more_than_1024_tables_with_padding_and_mean(rec, optimizer):
    T, B = 1100, 2
    rows = [5] * T
    m = _batched(rec, rows, 8, pooling_mode="mean", padding_idx=1, optimizer=optimizer, stochastic_rounding=True)
    idx, off = _request(rec, rows, B)
    grad = _named(rec, "grad", torch.ones(B, T * 8))
    _attempt(rec, "scatter_add_", lambda: m.scatter_add_(grad, idx, off, alpha=-0.25))
    names = [c[0] for c in rec.calls[1:]]
    assert names == ["pm_embbag_mean_grad", "pm_pad_rows_guard_bytes", "pm_pad_rows_guard", "pm_embbag_bwd_sorted_workspace",
                     "pm_embbag_bwd_fused", "pm_embbag_bwd_sorted_workspace", "pm_embbag_bwd_fused", "pm_pad_rows_guard"]
    _attempt(rec, "adagrad_step_", lambda: m.adagrad_step_(grad, idx, off))
    _attempt(rec, "adagrad_step_ again", lambda: m.adagrad_step_(grad, idx, off))
    _attempt(rec, "sort_indices", lambda: m.sort_indices(idx, off))
    _check(f"batched-1100-{optimizer}", rec.calls)


def test_a_refused_backward_with_padding_launches_nothing(rec):
    """THE ONE CASE that differs between the version of the host layer this test was written against and the one after it: a
    backward with padding that is refused on the host (here: an unknown ``method``, a gradient of the wrong shape, an unknown
    ``weight_decay_mode``) launches nothing.  The earlier version had already launched the guard's ``save`` -- without a ``restore``
    -- when it raised; that trace is accepted here as well, so that this file passes on both.  The refusals themselves (type and
    text) are asserted either way."""
    B = 4
    m = _batched(rec, ROWS3, 8, padding_idx=PADS3, optimizer="rowwise_adagrad")
    idx, off = _request(rec, ROWS3, B)
    grad = torch.ones(B, 24)
    m.momentum_table(0)
    ts = m._tables()
    before = [["pm_pad_rows_guard_bytes", "pm_pad_rows_guard"], []]
    with pytest.raises(ValueError, match='method must be "sorted" or "atomic"'):
        m.scatter_add_(grad, idx, off, alpha=1.0, method="bogus")
    assert [c[0] for c in rec.calls] in before
    del rec.calls[:]
    with pytest.raises(ValueError, match=r"grad must be float32 of shape \(4, 24\)"):
        m.scatter_add_(grad[:, :16], idx, off, alpha=1.0)
    assert [c[0] for c in rec.calls] in before
    del rec.calls[:]
    with pytest.raises(ValueError, match="weight_decay_mode must be one of none / l2 / decouple, got 'l3'"):
        eb._adagrad(ts, grad, idx, off, B, m._mom_ptrs, 0.1, 1e-8, weight_decay_mode="l3", pad=m._pad_dev())
    assert [c[0] for c in rec.calls] in before
    del rec.calls[:]
    big = _batched(rec, [5] * 1100, 8, padding_idx=1)
    idx, off = _request(rec, big.rows, 2)
    with pytest.raises(ValueError, match="presorted=True takes requests of at most 1024 tables"):
        big.scatter_add_(torch.ones(2, 1100 * 8), idx, off, alpha=1.0, presorted=True)
    assert [c[0] for c in rec.calls] in before


# ---- EmbeddingBagMI355 ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("padding_idx", [None, 2])
@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_single_table_module(rec, mode, padding_idx, sparse):
    n, D, B, L = 9, 8, 4, 3
    m = param_amd.EmbeddingBagMI355(n, D, mode=mode, padding_idx=padding_idx, sparse=sparse, device="cpu",
                                    bounds_check_mode="warning" if sparse else "none")
    ts = lambda name: (lambda: getattr(m._ts, name) if m._ts is not None else None)      # noqa: E731
    rec.named += [("pad", m._pad_dev), ("weights", m.weight.data), ("d_ptrs", ts("d_ptrs")), ("d_rows", ts("d_rows")),
                  ("d_dims", ts("d_dims")), ("d_col0", ts("d_col0"))]
    idx = _named(rec, "indices", torch.arange(B * L, dtype=torch.int64) % n)
    off = _named(rec, "offsets", torch.arange(B, dtype=torch.int64) * L)
    psw = _named(rec, "psw", torch.ones(B * L, requires_grad=True))
    idx2 = idx.view(B, L)

    def no_grad(*a):
        with torch.no_grad():
            return m(*a)
    _attempt(rec, "no-grad 1-D", lambda: no_grad(idx, off))
    _attempt(rec, "no-grad 1-D weighted", lambda: no_grad(idx, off, psw.detach()))
    _attempt(rec, "no-grad 2-D", lambda: no_grad(idx2))
    _attempt(rec, "backward 1-D", lambda: m(idx, off).sum().backward())
    _attempt(rec, "backward 1-D weighted", lambda: m(idx, off, psw).sum().backward())
    _attempt(rec, "backward 2-D", lambda: m(idx2).sum().backward())
    _attempt(rec, "backward 2-D weighted", lambda: m(idx2, None, psw.view(B, L)).sum().backward())
    _attempt(rec, "backward 1-D weights without grad", lambda: m(idx, off, psw.detach()).sum().backward())
    _attempt(rec, "2-D with offsets", lambda: m(idx2, off))
    _attempt(rec, "2-D weights of another shape", lambda: m(idx2, None, psw.detach()))
    _attempt(rec, "1-D without offsets", lambda: m(idx))
    _attempt(rec, "sanitize_", lambda: m.sanitize_(idx, off))
    _check(f"single-{mode}-{'pad' if padding_idx is not None else 'nopad'}-{'sparse' if sparse else 'dense'}", rec.calls)


def test_single_table_module_refuses_other_modes_and_padding_out_of_range():
    with pytest.raises(NotImplementedError, match='only mode="sum"'):
        param_amd.EmbeddingBagMI355(4, 8, mode="max", device="cpu")
    with pytest.raises(ValueError, match=r"padding_idx must be within num_embeddings \(got 4 for 4 rows\)"):
        param_amd.EmbeddingBagMI355(4, 8, padding_idx=4, device="cpu")
    with pytest.raises(ValueError, match="padding_idx has 2 entries for 3 tables"):
        param_amd.BatchedEmbeddingBagMI355(ROWS3, 8, device="cpu", init=None, padding_idx=[0, 1])
    with pytest.raises(ValueError, match="pooling_mode must be sum or mean"):
        param_amd.BatchedEmbeddingBagMI355(ROWS3, 8, device="cpu", init=None, pooling_mode="none")


def test_the_recorded_traces_are_not_being_rewritten():
    assert not REWRITE, "PARAM_AMD_REWRITE_CALL_TRACES=1 rewrote tests/call_trace_host.json: read its diff, then run without the flag"
