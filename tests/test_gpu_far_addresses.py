"""64-bit addressing of the newer lookup and backward paths: table rows, output rows and gradient rows whose offset from their base
pointer reaches 2^31 and 2^32, in bytes and in elements.

* Host tests (not marked ``gpu``): tests/far_rows.py -- the probe rows straddle the four thresholds for every format used below,
  ``compact`` round-trips, and on a SMALL full table every rule used below gives the same bits on the full table and on its compacted
  twin.
* ``test_far_*`` -- far TABLE rows: one module per table format holds ``[guard, far]`` in one slab: ``guard`` spans 2^31 bytes and
  is never looked up (an offset wrongly sign-extended from 32 bits lands there, one wrongly truncated lands inside ``far``: a wrong value,
  not a fault), ``far`` is zero but for its probe rows and their neighbours.  Every result is compared as BITS with the existing rule on
  the twin; updates also with the same entry point on a small twin module, and the whole slab is scanned for stray writes.
* ``test_out_*`` / ``test_grad_*`` -- far OUTPUT and GRADIENT rows: 64-row tables, bags of one lookup, D = 1024, and an output or gradient of more than 2^32
  elements, checked whole on the device and around the thresholds against the rule modules on the host.  Max pooling's
  ``max_indices`` and expanded gradient ``g_seq`` are such tensors too (``test_out_and_grad_of_a_max_module``).

Not covered here: more than 2^31 LOOKUPS through the newer paths (17 GB of indices; tests/test_gpu_parity.py has that for the original
forward and the sorted backward)."""
import contextlib
import functools
import time

import numpy as np
import pytest
import torch

from tests import elem_adagrad_rules as A
from tests import embedding_rules as E
from tests import far_rows as F
from tests import max_rules as X
from tests import mean_rules as M
from tests import out16_rules as O
from tests import padding_rules as P
from tests import psw_grad_rules as G
from tests import qgather_rules as Q
from tests import qrows_rules as R
from tests import sequence_grad_rules as S

gpu = pytest.mark.gpu
DEV = "cuda"
GIB = 1 << 30
B = len(F.STAGED_LENS)
IDT = {"i32": torch.int32, "i64": torch.int64}
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
# the narrowest tables that reach 2^32 ELEMENTS: format -> (D, element size | None, bits | None)
FLOATS = {"f32": (4, 4, None), "bf16": (8, 2, None), "f16": (8, 2, None)}
QUANTS = {"q8x4": (4, None, 8), "q8x1024": (1024, None, 8), "q4x8": (8, None, 4), "q4x1024": (1024, None, 4)}
FORMATS = {**FLOATS, **QUANTS}
LENS = {"staged": F.STAGED_LENS, "unstaged": F.UNSTAGED_LENS, "update": F.UPDATE_LENS}
EXACT_RUN = 256      # kExactRun of the sorted apply: a row looked up more often is summed as ordered chunk partials


def probes_of(fmt):
    return F.probe_rows(*FORMATS[fmt])


@functools.lru_cache(maxsize=None)
def far_request(fmt, which, omit=()):
    """(indices int64, offsets int64 [2 B + 1], psw fp32) over ``[guard, far]``: built once per case and never modified"""
    probes = probes_of(fmt)
    keep = np.array([r for r in probes if int(r) not in omit], dtype=np.int64)
    idx, off = F.request(keep, LENS[which], seed=17 + len(which), guard_bags=B)
    assert off[B] == 0 and off[-1] == idx.size == sum(LENS[which])
    psw = (np.random.default_rng(5).standard_normal(idx.size) * 1.5).astype(np.float32)
    return idx, off, psw


def content(fmt, n, seed):
    """``n`` distinct rows: fp32 values ``[n, D]`` without a zero element (float formats; rounded to the format by the caller) or
    quantised rows uint8 ``[n, row_bytes]``"""
    from oracle import rowquant
    D, es, bits = FORMATS[fmt]
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, D)) * (rng.random((n, 1)) * 4 + 0.25)).astype(np.float32)
    x[np.abs(x) < 0.01] = 0.5
    if bits is None:
        return x
    q = rowquant.quantize_rows(x, bits)
    assert q.shape == (n, F.row_bytes(D, bits=bits))
    return q


# =========================================================================================================================================
# host tests
# =========================================================================================================================================

@pytest.mark.parametrize("fmt", list(FORMATS))
def test_probes_straddle_every_threshold(fmt):
    """Of the rows around a threshold X, ``c`` is the first that starts at or above X and ``c - 1`` starts below it (and ends AT it where
    the row size divides X; 12-, 516- and 1032-byte rows contain X instead): both, and ``c + 1``, are probes."""
    D, es, bits = FORMATS[fmt]
    probes = probes_of(fmt)
    assert np.array_equal(probes, np.unique(probes)) and set(probes[:3]) == {0, 1, 2}
    assert len(probes) <= sum(F.STAGED_LENS), "the staged request reaches every probe"
    rows = F.table_rows(probes)
    assert rows - 1 == probes[-1] and rows < 2 ** 31
    seen = set()
    for what, X, stride, c in F.threshold_rows(D, es, bits):
        assert {c - 1, c, c + 1} <= set(probes.tolist())
        assert (c - 1) * stride < X <= c * stride
        assert stride * 2 > c * stride - X >= 0
        seen.add((what, X))
    assert len(seen) == 4
    rb = F.row_bytes(D, es, bits)
    assert rows * rb > 2 ** 32 and rows * F.row_elems(D, bits) > 2 ** 32
    assert F.guard_rows(D, es, bits) * rb >= 2 ** 31
    sent = F.sentinel_rows(probes)
    assert not set(sent.tolist()) & set(probes.tolist()) and sent.size and sent.max() < rows


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_compact_round_trips(fmt):
    probes = probes_of(fmt)
    for which in LENS:
        idx, off, _ = far_request(fmt, which)
        c = F.compact(probes, idx)
        assert c.dtype == idx.dtype and c.min() == 0 and c.max() == len(probes) - 1
        assert np.array_equal(F.expand(probes, c), idx) and np.array_equal(np.unique(c), np.arange(len(probes)))
        assert F.compact(probes, idx.astype(np.int32)).dtype == np.int32
    assert np.array_equal(F.compact(probes, probes), np.arange(len(probes)))
    with pytest.raises(AssertionError):
        F.compact(probes, np.array([3]))
    with pytest.raises(AssertionError):
        F.compact(probes, np.array([int(probes[-1]) + 1]))


def _small(D, es, bits, seed):
    """a full table small enough for the rules: the helper with thresholds of 2^7 and 2^8 -> (probes, full content, a 3-row guard)"""
    probes = F.probe_rows(D, es, bits, thresholds=(2 ** 7, 2 ** 8))
    fmt = next(k for k, v in FORMATS.items() if v == (D, es, bits))
    full = content(fmt, F.table_rows(probes), seed)
    return probes, full, content(fmt, 3, seed + 1)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _far_arg(probes, twin_arg):
    """the rule's arg-max on the twin as rows of the full table: the probe of every row, -1 where no lookup was kept"""
    a = np.asarray(twin_arg).astype(np.int64)
    return np.where(a >= 0, F.expand(probes, np.maximum(a, 0)), -1)


def test_twin_equals_full_table_for_the_float_rules(coracle):
    """rule(full table, indices) == rule(twin, compact(indices)) bit for bit, for every rule the GPU tests below put on a twin"""
    D, es = 4, 4
    probes, full, guard = _small(D, es, None, 3)
    assert 20 < full.shape[0] < 200
    twin = full[probes]
    for lens in (F.STAGED_LENS, (0, 70, 1, 9, 0, 2)):
        idx, off = F.request(probes, lens, seed=1, guard_bags=B)
        cidx = F.compact(probes, idx)
        psw = np.random.default_rng(2).standard_normal(idx.size).astype(np.float32)
        big, small = [guard, full], [guard[:1], twin]
        pads_b, pads_s = [None, int(probes[-1])], [None, len(probes) - 1]
        for w in (None, psw):
            assert np.array_equal(_u32(coracle.fwd_batched(big, idx, off, B, psw=w)), _u32(coracle.fwd_batched(small, cidx, off, B, psw=w)))
            for pb, ps in (([None, None], [None, None]), (pads_b, pads_s)):
                a, b = P.forward(big, idx, off, B, pb, w), P.forward(small, cidx, off, B, ps, w)
                assert all(np.array_equal(_u32(x), _u32(y)) for x, y in zip(a, b))
                for dt in O.DTYPES:
                    a, b = O.forward(big, idx, off, B, pb, dt, w), O.forward(small, cidx, off, B, ps, dt, w)
                    assert all(np.array_equal(x, y) for x, y in zip(a, b))
        a, b = M.forward(big, idx, off, B, pads_b), M.forward(small, cidx, off, B, pads_s)
        assert all(np.array_equal(_u32(x), _u32(y)) for x, y in zip(a, b))
        a, b = O.forward(big, idx, off, B, pads_b, "bf16", mean=True), O.forward(small, cidx, off, B, pads_s, "bf16", mean=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        # max pooling: the values, and the arg-max after mapping the twin's rows through the probes
        for pb, ps in (([None, None], [None, None]), (pads_b, pads_s)):
            (va, aa), (vb, ab) = X.forward(big, idx, off, B, pb), X.forward(small, cidx, off, B, ps)
            assert all(np.array_equal(_u32(x), _u32(y)) for x, y in zip(va, vb))
            assert (aa[0] == -1).all() and (ab[0] == -1).all() and (ab[1] >= 0).any() and (ab[1] == -1).any()
            assert np.array_equal(aa[1], _far_arg(probes, ab[1])) and aa[1].max() >= 2 ** 7 // (D * es) and not (aa[1] == (pb[1] or -2)).any()
        # the per_sample_weights gradient
        g = np.random.default_rng(4).standard_normal((B, 2 * D)).astype(np.float32)
        gs = [g[:, :D], g[:, D:]]
        a, b = G.restate(big, idx, off, B, gs, 4), G.restate(small, cidx, off, B, gs, 4)
        assert G.same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].all()
        # un-pooled rows, every pair of kinds
        for kin in E.KINDS:
            tb, ts_ = [E.to_bits(x, kin) for x in big], [E.to_bits(x, kin) for x in small]
            for kout in E.KINDS:
                zero = np.zeros((idx.size, D), dtype=E.BITS[kout])
                assert np.array_equal(E.forward(tb, kin, kout, idx, off, B, zero), E.forward(ts_, kin, kout, cidx, off, B, zero))
        # gradients of un-pooled rows: the full result is the twin's at the probes and zero everywhere else
        gn = np.random.default_rng(6).standard_normal((idx.size, D)).astype(np.float32)
        for pb, ps in ((None, None), (int(probes[-1]), len(probes) - 1)):
            a, b = E.dense_grad(full.shape[0], idx, gn, pb), E.dense_grad(len(probes), cidx, gn, ps)
            assert np.array_equal(_u32(a[probes]), _u32(b)) and not np.delete(a, probes, axis=0).any()
        a = S.dense_grad([3, full.shape[0]], [D, D], idx, off[:-1], B, gn)
        b = S.dense_grad([1, len(probes)], [D, D], cidx, off[:-1], B, gn)
        assert np.array_equal(_u32(a[1][probes]), _u32(b[1])) and not np.delete(a[1], probes, axis=0).any() and not a[0].any()
        # the C oracle's sequential scatter-add, one bag per lookup and the pooled request
        one = np.arange(idx.size)
        a, b = coracle.bwd_f32(full.copy(), idx, one, gn, alpha=-0.5), coracle.bwd_f32(twin.copy(), cidx, one, gn, alpha=-0.5)
        assert np.array_equal(_u32(a[probes]), _u32(b)) and np.array_equal(np.delete(a, probes, axis=0), np.delete(full, probes, axis=0))
        loc = off[B:2 * B]
        a, b = coracle.bwd_f32(full.copy(), idx, loc, gs[1], psw, alpha=0.75), coracle.bwd_f32(twin.copy(), cidx, loc, gs[1], psw, alpha=0.75)
        assert np.array_equal(_u32(a[probes]), _u32(b))
        # element-wise Adagrad
        s_full = np.abs(np.random.default_rng(8).standard_normal(full.shape)).astype(np.float32)
        Ga, ca = A.grad_sum_f32(full.shape[0], idx, one, gn)
        Gb, cb = A.grad_sum_f32(len(probes), cidx, one, gn)
        assert np.array_equal(_u32(Ga[probes]), _u32(Gb)) and np.array_equal(ca[probes], cb)
        wa, sa = A.step_f32(full, s_full, Ga, ca > 0, 0.05, 1e-6)
        wb, sb = A.step_f32(twin, s_full[probes], Gb, cb > 0, 0.05, 1e-6)
        assert np.array_equal(_u32(wa[probes]), _u32(wb)) and np.array_equal(_u32(sa[probes]), _u32(sb))


@pytest.mark.parametrize("bits,D", [(8, 4), (8, 40), (4, 8), (4, 40)])
def test_twin_equals_full_table_for_the_quantised_rules(bits, D):
    from oracle import rowquant
    probes = F.probe_rows(D, None, bits, thresholds=(2 ** 9, 2 ** 10))
    rng = np.random.default_rng(bits + D)
    n = F.table_rows(probes)
    assert 10 < n < 600
    full = rowquant.quantize_rows((rng.standard_normal((n, D)) * 3).astype(np.float32), bits)
    guard = full[:3].copy()
    twin = full[probes]
    for lens in (F.STAGED_LENS, (0, 70, 1, 9, 0, 2)):
        idx, off = F.request(probes, lens, seed=1, guard_bags=B)
        cidx = F.compact(probes, idx)
        psw = rng.standard_normal(idx.size).astype(np.float32)
        for w in (None, psw):
            a, b = R.forward([guard, full], [D, D], bits, idx, off, B, w), R.forward([guard[:1], twin], [D, D], bits, cidx, off, B, w)
            assert all(R.same_f32(x, y) and np.array_equal(_u32(x), _u32(y)) for x, y in zip(a, b))
            a = R.forward16([guard, full], [D, D], bits, idx, off, B, "fp16", w)
            b = R.forward16([guard[:1], twin], [D, D], bits, cidx, off, B, "fp16", w)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
        a, b = Q.gather([guard, full], D, bits, idx, off, B), Q.gather([guard[:1], twin], D, bits, cidx, off, B)
        assert np.array_equal(_u32(a[0]), _u32(b[0])) and a[1].all() and b[1].all()


# =========================================================================================================================================
# GPU plumbing
# =========================================================================================================================================

def _bits(t):
    """a tensor's bits as the numpy array the rules compare"""
    t = t.detach().contiguous()
    if t.dtype == torch.uint8:
        return t.cpu().numpy()
    if t.element_size() == 2:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _dev_bits(bits, dtype):
    """numpy bits (uint16 / uint32 / uint8) as a device tensor of ``dtype``"""
    bits = np.ascontiguousarray(bits)
    if dtype == torch.uint8:
        return torch.from_numpy(bits).to(DEV)
    return torch.from_numpy(bits.view(np.int16 if bits.dtype == np.uint16 else np.int32)).to(DEV).view(dtype)


def _rows(t, rows):
    """the rows ``rows`` of a (far) tensor, stacked: one view per row -- the host adds ``r * stride`` to the base pointer in 64 bits --
    and one small concatenation, so that no index kernel of torch's stands between a far row and the comparison"""
    return torch.stack([t[int(r)] for r in rows])


def _put_rows(t, rows, values):
    for i, r in enumerate(rows):
        t[int(r)].copy_(values[i])


def _need(nbytes, what):
    """the skip rule of tests/test_gpu_parity.py: only when the device has less free memory than the test needs plus 8 GiB"""
    import param_amd

    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    param_amd.load_library()
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + 8 * GIB:
        pytest.skip(f"{what}: needs {nbytes / GIB:.1f} GiB + 8 GiB of free HBM, {free / GIB:.0f} GiB available")


def _nonzero(t, chunk=1 << 28):
    """how many elements of a tensor hold a non-zero BIT pattern: one pass over the slab in pieces of 2^28 elements (a reduction over
    the whole tensor would widen it into a temporary several times its size)"""
    v = t.detach().reshape(-1)
    if v.dtype != torch.uint8:
        v = v.view(torch.int16 if v.element_size() == 2 else torch.int32)
    return sum(int((v[a:a + chunk] != 0).sum()) for a in range(0, v.numel(), chunk))


@contextlib.contextmanager
def variant(m, padding_idx=None, pooling_mode=None, output_dtype=None, optimizer=None):
    """The far module under other constructor options for the block.  Every test of a format shares ONE slab (the fixture below): a
    module per option would allocate and zero 18 GiB again, so the options -- plain attributes the constructor sets and the methods
    read at call time -- are set here and put back; the optimizer state a block allocates is freed with it."""
    from param_amd.embedding_bag import _output_dtype
    names = ("padding_idx", "pooling_mode", "_mean", "_max", "output_dtype", "_out16", "optimizer")
    keep = {k: getattr(m, k) for k in names if hasattr(m, k)}      # (the quantised module has the output dtype only)
    try:
        if padding_idx is not None:
            m.padding_idx = list(padding_idx)
        if pooling_mode is not None:
            m.pooling_mode, m._mean, m._max = pooling_mode, pooling_mode == "mean", pooling_mode == "max"
        if output_dtype is not None:
            m.output_dtype = _output_dtype(output_dtype)
            m._out16 = None if m.output_dtype == torch.float32 else m.output_dtype
        if optimizer is not None:
            m.optimizer = optimizer
        m._pad_t = None
        yield m
    finally:
        for k, v in keep.items():
            setattr(m, k, v)
        m._pad_t = None
        if optimizer is not None:
            m.momentum, m._mom_base, m._mom_ptrs = None, None, None
            torch.cuda.empty_cache()


class Far:
    """``[guard, far]`` of one format in one slab, zero but for the far table's probe rows and their neighbours (the sentinels)"""

    def __init__(self, fmt):
        import param_amd

        self.fmt = fmt
        self.D, self.es, self.bits = D, es, bits = FORMATS[fmt]
        self.probes, self.quant = probes_of(fmt), bits is not None
        self.sent = F.sentinel_rows(self.probes)
        self.rows = [F.guard_rows(D, es, bits), F.table_rows(self.probes)]
        self.pad_last = int(self.probes[-1])
        self.pad_byte32 = next(c for what, X, _, c in F.threshold_rows(D, es, bits) if (what, X) == ("bytes", 2 ** 32))
        rb = F.row_bytes(D, es, bits)
        self.slab_bytes = sum(self.rows) * rb
        _need(self.slab_bytes * (2 if fmt == "f32" else 3 if bits is None else 1), f"far tables {fmt}")
        n_p, n_s = len(self.probes), len(self.sent)
        both = content(fmt, n_p + n_s, seed=40 + len(fmt) + D)
        if self.quant:
            self.m = param_amd.QuantizedBatchedEmbeddingBagMI355(self.rows, D, bits, device=DEV)      # (torch.zeros: the slab is zero)
            self.dtype, self.kind = torch.uint8, None
            both_bits = both
        else:
            self.dtype, self.kind = TDT[fmt], fmt
            self.m = param_amd.BatchedEmbeddingBagMI355(self.rows, D, dtype=self.dtype, device=DEV, init=None, fused_update=False,
                                                        learning_rate=0.05, eps=1e-6)
            self.m.weights.data.zero_()
            both_bits = E.to_bits(both, fmt)
        assert len(np.unique(both_bits, axis=0)) == n_p + n_s and both_bits.any(axis=1).all(), "distinct non-zero rows"
        assert self.quant or both_bits.all(), "float rows hold no zero element"
        self.twin_bits, self.sent_bits = both_bits[:n_p].copy(), both_bits[n_p:].copy()
        self._d_twin, self._d_sent = _dev_bits(self.twin_bits, self.dtype), _dev_bits(self.sent_bits, self.dtype)
        self._rules = {}
        self.reset()
        assert _nonzero(self.m.weights) == int(np.count_nonzero(both_bits)), "the slab is zero but for the probes and the sentinels"
        torch.cuda.synchronize()
        self.peak = torch.cuda.max_memory_allocated()

    def rule(self, key, fn):
        """the rule's result for a case, computed once and shared by the index types and output types that must give the same bits"""
        if key not in self._rules:
            self._rules[key] = fn()
        return self._rules[key]

    def reset(self):
        """the probe rows and the sentinels as first written"""
        _put_rows(self.m.table(1), self.probes, self._d_twin)
        _put_rows(self.m.table(1), self.sent, self._d_sent)

    def twin_f32(self):
        """``[one-row guard, twin]`` as fp32 values (16-bit tables widened, which is exact)"""
        return [np.zeros((1, self.D), dtype=np.float32), E.to_f32(self.twin_bits, self.kind)]

    def twin_tables(self):
        """``[one-row guard, twin]`` as the bits the tables hold"""
        return [np.zeros((1,) + self.twin_bits.shape[1:], dtype=self.twin_bits.dtype), self.twin_bits]

    def twin_module(self, **kw):
        """the small module ``[one-row guard, twin]`` with the far module's learning rate and eps"""
        import param_amd

        w = param_amd.BatchedEmbeddingBagMI355([1, len(self.probes)], self.D, dtype=self.dtype, device=DEV, init=None, fused_update=False,
                                               learning_rate=0.05, eps=1e-6, **kw)
        w.weights.data.zero_()
        w.table(1).copy_(self._d_twin)
        return w

    def case(self, which, it, weighted=False, omit=()):
        """host and device forms of a request: (idx_h, cidx_h, off_h, psw_h, idx, off, psw)"""
        idx_h, off_h, psw_h = far_request(self.fmt, which, omit)
        psw_h = psw_h if weighted else None
        return (idx_h, F.compact(self.probes, idx_h), off_h, psw_h, _dev(idx_h, IDT[it]), _dev(off_h, IDT[it]), _dev(psw_h))

    def close(self):
        self.m = self._d_twin = self._d_sent = None
        torch.cuda.empty_cache()


_LIVE = {}
_STATS = {}


def _close_far():
    """free the live far module, if any; its peak of allocated memory (the peak is reset where a module is built) goes to the report"""
    for k in list(_LIVE):
        obj = _LIVE.pop(k)
        _STATS[k] = torch.cuda.max_memory_allocated()
        print(f"far[{k}]: slab {obj.slab_bytes / GIB:.2f} GiB, peak allocated {_STATS[k] / GIB:.2f} GiB")
        obj.close()


@pytest.fixture(scope="module")
def far(request):
    """One far module per format, shared by every test of that format (pytest groups the tests of a module-scoped parameter) and freed
    before the next one is built: at most one slab is live at a time."""
    fmt = request.param
    if fmt not in _LIVE:
        _close_far()
        torch.cuda.reset_peak_memory_stats()
        _LIVE[fmt] = Far(fmt)
    yield _LIVE[fmt]
    _close_far()


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    print(f"tests/test_gpu_far_addresses.py: {time.time() - t0:.1f} s; peak GiB per fixture: "
          f"{ {k: round(v / GIB, 2) for k, v in _STATS.items()} }")


def on_floats(fn):
    return pytest.mark.parametrize("far", list(FLOATS), indirect=True)(gpu(fn))


def on_quants(fn):
    return pytest.mark.parametrize("far", list(QUANTS), indirect=True)(gpu(fn))


def assert_path(plan, which, what):
    """The staged request: every tile's lookups fit the LDS index tile (``row_offset<true>``, int32 indices in LDS).  The unstaged one:
    its longest BAG alone does not, so whatever tile holds it reads its indices from the request (``row_offset<false>``)."""
    n, longest = sum(LENS[which]), max(LENS[which])
    print(f"{what} {which}: idx_cap {plan['idx_cap']}, lookups of the far table {n}, longest bag {longest}, "
          f"tiles_per_table {plan['tiles_per_table']}, bags_per_block {plan['bags_per_block']}, stage_out {plan['stage_out']}")
    if which == "staged":
        assert plan["idx_cap"] >= n
    else:
        assert plan["idx_cap"] < longest


def float_plan(far, kind, idx, off, psw):
    from param_amd import _lib
    return _lib.embbag_plan(far.m._tables().request(idx, off, B, psw, 0, None, forward=True), kind)


def cat(tables):
    """the rule's per-table ``[B, D]`` list as the ``[B, 2 D]`` result of the ``bd`` layout"""
    return np.concatenate(tables, axis=1)


WHICH = pytest.mark.parametrize("which", ["staged", "unstaged"])
IT = pytest.mark.parametrize("it", ["i32", "i64"])
WEIGHTED = pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])


# =========================================================================================================================================
# 2. far table rows: lookups
# =========================================================================================================================================

@on_floats
@WHICH
@IT
@WEIGHTED
def test_far_lookup(far, which, it, weighted, coracle):
    """the plain forward: the baseline for this shape"""
    from param_amd import _lib
    idx_h, cidx, off_h, psw_h, idx, off, psw = far.case(which, it, weighted)
    assert_path(float_plan(far, _lib.PM_PLAN_FORWARD, idx, off, psw), which, "pm_embbag_fwd")
    got = far.m.lookup(idx, off, psw, batch=B)
    want = far.rule(("fwd", which, weighted), lambda: coracle.fwd_batched(far.twin_f32(), cidx, off_h, B, psw=psw_h))
    assert got.shape == (B, 2 * far.D) and np.array_equal(_bits(got), _u32(want))
    assert not got[:, :far.D].any() and got[:, far.D:].any()


@on_floats
@pytest.mark.parametrize("pad", ["last", "byte32"])
@WHICH
@IT
@WEIGHTED
def test_far_lookup_padded(far, pad, which, it, weighted):
    """``padding_idx`` on the far table's last row (the constructor's -1) and on the first row at or beyond 2^32 bytes"""
    from param_amd import _lib
    from param_amd.embedding_bag import _normalize_padding_idx
    k = far.pad_last if pad == "last" else far.pad_byte32
    idx_h, cidx, off_h, psw_h, idx, off, psw = far.case(which, it, weighted)
    assert (idx_h == k).any() and k * far.D * far.es >= 2 ** 32
    ck = int(F.compact(far.probes, np.array([k]))[0])
    assert pad != "last" or _normalize_padding_idx(-1, far.rows[1]) == k
    with variant(far.m, padding_idx=[None, k]) as m:
        assert_path(float_plan(far, _lib.PM_PLAN_PADDED, idx, off, psw), which, "pm_embbag_fwd_padded")
        got = m.lookup(idx, off, psw, batch=B)
    want = far.rule(("pad", ck, which, weighted), lambda: cat(P.forward(far.twin_f32(), cidx, off_h, B, [None, ck], psw_h)))
    assert np.array_equal(_bits(got), _u32(want))
    plain = far.rule(("pad", None, which, weighted), lambda: cat(P.forward(far.twin_f32(), cidx, off_h, B, [None, None], psw_h)))
    assert not np.array_equal(_u32(plain), _u32(want)), "the padding row is looked up and left out"


@on_floats
@WHICH
@IT
def test_far_lookup_mean(far, which, it):
    from param_amd import _lib
    idx_h, cidx, off_h, _, idx, off, _ = far.case(which, it)
    with variant(far.m, pooling_mode="mean") as m:
        assert_path(float_plan(far, _lib.PM_PLAN_PADDED, idx, off, None), which, "pm_embbag_fwd_mean")
        got = m.lookup(idx, off, batch=B)
    want = far.rule(("mean", which), lambda: cat(M.forward(far.twin_f32(), cidx, off_h, B, [None, None])))
    assert np.array_equal(_bits(got), _u32(want))


@on_floats
@pytest.mark.parametrize("pad", ["none", "byte32"])
@WHICH
@IT
def test_far_lookup_max(far, pad, which, it):
    """``pm_embbag_fwd_max`` on the far module (the max flag set for the block: no second slab): the staged walk's ``row_offset<true>``,
    the unstaged walk's ``row_offset<false>``; ``max_indices`` holds the far row numbers themselves"""
    from param_amd import _lib
    k = None if pad == "none" else far.pad_byte32
    idx_h, cidx, off_h, _, idx, off, _ = far.case(which, it)
    ck = None if k is None else int(F.compact(far.probes, np.array([k]))[0])
    assert k is None or ((idx_h == k).any() and k * far.D * far.es >= 2 ** 32)
    with variant(far.m, pooling_mode="max", padding_idx=None if k is None else [None, k]) as m:
        assert m._max and not m._mean
        assert_path(float_plan(far, _lib.PM_PLAN_PADDED, idx, off, None), which, "pm_embbag_fwd_max")
        got, arg = m.lookup(idx, off, batch=B, return_max_indices=True)
        plain = m.lookup(idx, off, batch=B)
    assert not far.m._max and far.m.pooling_mode == "sum"
    want_v, want_a = far.rule(("max", ck, which), lambda: X.forward(far.twin_f32(), cidx, off_h, B, [None, ck]))
    assert got.shape == (B, 2 * far.D) and np.array_equal(_bits(got), _u32(cat(want_v))) and np.array_equal(_bits(plain), _bits(got))
    a = arg.cpu().numpy().astype(np.int64)
    assert arg.dtype == torch.int32 and np.array_equal(a, cat([_far_arg(far.probes, w) for w in want_a]))
    assert (a[:, :far.D] == -1).all() and a.max() * far.D * far.es >= 2 ** 32 and (a[LENS[which].index(0)] == -1).all()
    if k is not None:      # (looked up, asserted above, and never the arg-max; whether it would win a column is the content's accident)
        assert not (a == k).any()


@on_floats
@pytest.mark.parametrize("odt", ["bf16", "fp16"])
@WHICH
@IT
@WEIGHTED
def test_far_lookup_out16(far, odt, which, it, weighted):
    from param_amd import _lib
    idx_h, cidx, off_h, psw_h, idx, off, psw = far.case(which, it, weighted)
    with variant(far.m, output_dtype=odt) as m:
        assert_path(float_plan(far, _lib.PM_PLAN_PADDED16, idx, off, psw), which, "pm_embbag_fwd_out16")
        got = m.lookup(idx, off, psw, batch=B)
    want = O.round16(far.rule(("pad", None, which, weighted), lambda: cat(P.forward(far.twin_f32(), cidx, off_h, B, [None, None], psw_h))), odt)
    assert np.array_equal(want, far.rule(("out16", odt, which, weighted), lambda: cat(O.forward(far.twin_f32(), cidx, off_h, B, [None, None], odt, psw_h))))
    assert got.dtype == {"bf16": torch.bfloat16, "fp16": torch.float16}[odt] and O.same_bits(_bits(got), want, odt)
    assert np.array_equal(_bits(got), want)


@on_floats
@WHICH
@IT
@WEIGHTED
def test_far_lookup_split_bags(far, which, it, weighted, coracle):
    """``split_bags=True`` is "not bit-equal" by its own docstring: the comparison and the bound of
    tests/test_gpu_parity.py::test_split_bag_forward_long_bags -- within 1e-5 of sum |row| of the oracle's sequential sum, and the same
    bits on a second call"""
    idx_h, cidx, off_h, psw_h, idx, off, psw = far.case(which, it, weighted)
    got = far.m.lookup(idx, off, psw, batch=B, split_bags=True)
    tabs = far.twin_f32()
    exp = coracle.fwd_batched(tabs, cidx, off_h, B, psw=psw_h)
    mag = coracle.fwd_batched([np.abs(x) for x in tabs], cidx, off_h, B, psw=None if psw_h is None else np.abs(psw_h))
    assert (np.abs(got.cpu().numpy() - exp) <= 1e-5 * mag + 1e-30).all()
    assert torch.equal(got, far.m.lookup(idx, off, psw, batch=B, split_bags=True))
    assert mag[:, far.D:].sum() > 0 and not mag[:, :far.D].any()


@on_floats
@WHICH
@IT
def test_far_psw_grad(far, which, it):
    """``per_sample_weights_grad`` reads the far table's rows (every lookup is staged in LDS pieces: there is one path)"""
    idx_h, cidx, off_h, _, idx, off, _ = far.case(which, it)
    g = np.random.default_rng(12).standard_normal((B, 2 * far.D)).astype(np.float32)
    got = far.m.per_sample_weights_grad(_dev(g), idx, off, batch=B).cpu().numpy()
    ref, written, _, _ = G.restate(far.twin_f32(), cidx, off_h, B, [g[:, :far.D], g[:, far.D:]], G.vec_of(far.fmt))
    assert written.all() and G.same_bits(got, ref) and got.any()


SEQ_OUT = {"f32": (None, "bf16"), "bf16": ("bf16",), "f16": (None,)}      # the pairs tests/test_gpu_embedding.py crosses


@on_floats
@WHICH
@IT
def test_far_lookup_sequence(far, which, it):
    from param_amd import _lib
    idx_h, cidx, off_h, _, idx, off, _ = far.case(which, it)
    for out in SEQ_OUT[far.fmt]:
        kout = "f32" if out is None else out
        with variant(far.m, output_dtype=out or "fp32") as m:
            plan = _lib.embedding_gather_plan(m._tables().request(idx, off, B, None, 0, None))
            assert plan["grid"] == -(-idx_h.size // plan["tile"]) and plan["lds_borders"] == 1
            got = m.lookup_sequence(idx, off, batch=B)
        zero = np.zeros((idx_h.size, far.D), dtype=E.BITS[kout])
        want = E.forward(far.twin_tables(), far.fmt, kout, cidx, off_h, B, zero)
        assert got.dtype == TDT[kout] and E.same(_bits(got), want, far.fmt, kout) and np.array_equal(_bits(got), want), (far.fmt, kout)


QOUT = pytest.mark.parametrize("odt", ["fp32", "bf16", "fp16"])


@on_quants
@QOUT
@WHICH
@IT
@WEIGHTED
def test_far_quantised_lookup(far, odt, which, it, weighted):
    idx_h, cidx, off_h, psw_h, idx, off, psw = far.case(which, it, weighted)
    with variant(far.m, output_dtype=odt) as m:
        assert_path(m.plan(idx, off, psw, batch=B), which, "pm_embbag_fwd_qrows")
        got = m.lookup(idx, off, psw, batch=B)
    want = far.rule(("qfwd", which, weighted), lambda: cat(R.forward(far.twin_tables(), [far.D, far.D], far.bits, cidx, off_h, B, psw_h)))
    if odt == "fp32":
        assert R.same_f32(got.cpu().numpy(), want) and np.array_equal(_bits(got), _u32(want))
    else:
        assert np.array_equal(_bits(got), O.round16(want, odt))
    assert got[:, far.D:].any()


@on_quants
@QOUT
@WHICH
@IT
def test_far_quantised_lookup_sequence(far, odt, which, it):
    idx_h, cidx, off_h, _, idx, off, _ = far.case(which, it)
    with variant(far.m, output_dtype=odt) as m:
        plan = m.sequence_plan(idx, off, batch=B)
        assert plan["grid"] == -(-idx_h.size // plan["tile"]) and plan["col_passes"] == (2 if (far.bits, far.D) == (8, 1024) else 1)
        got = m.lookup_sequence(idx, off, batch=B)
    want, written = far.rule(("qseq", which), lambda: Q.gather(far.twin_tables(), far.D, far.bits, cidx, off_h, B))
    assert written.all()
    if odt == "fp32":
        assert R.same_f32(got.cpu().numpy(), want) and np.array_equal(_bits(got), _u32(want))
    else:
        assert np.array_equal(_bits(got), O.round16(want, odt))


# =========================================================================================================================================
# 2. far table rows: updates that WRITE them
# =========================================================================================================================================

def _omitted(far):
    """two probes no update looks up: row 1 and the row behind the 2^32-byte threshold"""
    return (1, far.pad_byte32 + 1)


def _state_rows(m, rows):
    return _rows(m.momentum_table(1), rows)


def _run_update(far, which, it, apply, optimizer=None, pad=None, state=False):
    """``apply(module, idx, off, twin: bool)`` on the far module and on the twin module; then every probe row (and its optimizer state)
    of the far table holds the twin's bits; the probes that were not looked up, the padding row, the sentinels (and their state) hold
    what was written; and the slab (the state buffer) holds exactly as many non-zero elements as those rows account for -- nothing
    else was written anywhere in ``guard`` or ``far``.  Returns (far rows before, twin rows after, state before, twin state after)
    as numpy bits / values for the rule checks of the caller."""
    omit = _omitted(far)
    idx_h, cidx, off_h, _, idx, off, _ = far.case(which, it, omit=omit)
    counts = np.bincount(cidx, minlength=len(far.probes))
    assert counts.max() <= EXACT_RUN and set(np.nonzero(counts == 0)[0]) == set(F.compact(far.probes, np.array(omit)).tolist())
    cpad = None if pad is None else int(F.compact(far.probes, np.array([pad]))[0])
    assert pad is None or counts[cpad] > 0, "the padding row is looked up"
    far.reset()
    twin = far.twin_module(optimizer=optimizer or "sgd", padding_idx=None if pad is None else [None, cpad])
    P_, S_ = len(far.probes), len(far.sent)
    with variant(far.m, optimizer=optimizer or "sgd", padding_idx=None if pad is None else [None, pad]) as m:
        s0 = s0_sent = None
        if state:
            rng = np.random.default_rng(77)
            shape = (far.D,) if optimizer == "adagrad" else ()
            s0 = (rng.random((P_,) + shape) + 0.5).astype(np.float32)
            s0_sent = (rng.random((S_,) + shape) + 0.5).astype(np.float32)
            m.momentum_table(0), twin.momentum_table(0)
            _put_rows(m.momentum_table(1), far.probes, _dev(s0))
            _put_rows(m.momentum_table(1), far.sent, _dev(s0_sent))
            twin.momentum_table(1).copy_(_dev(s0))
        apply(m, idx, off, False)
        apply(twin, _dev(cidx, IDT[it]), off, True)
        got = _bits(_rows(m.table(1), far.probes))
        want = _bits(twin.table(1))
        looked = counts > 0
        if cpad is not None:
            looked[cpad] = False
        assert np.array_equal(got, want), "probe rows"
        assert np.array_equal(got[~looked], far.twin_bits[~looked]) and (got[looked] != far.twin_bits[looked]).any()
        assert np.array_equal(_bits(_rows(m.table(1), far.sent)), far.sent_bits), "sentinel rows"
        assert _nonzero(m.weights) == int(np.count_nonzero(want)) + far.sent_bits.size, "a row outside the probes was written"
        gs = ws = None
        if state:
            gs, ws = _state_rows(m, far.probes).cpu().numpy(), twin.momentum_table(1).cpu().numpy()
            assert np.array_equal(_u32(gs), _u32(ws)), "state of the probe rows"
            assert np.array_equal(gs[~looked], s0[~looked]) and (gs[looked] != s0[looked]).reshape(int(looked.sum()), -1).any(axis=1).all()
            assert np.array_equal(_state_rows(m, far.sent).cpu().numpy(), s0_sent), "state of the sentinel rows"
            assert _nonzero(m.momentum) == int(np.count_nonzero(ws)) + s0_sent.size, "state outside the probes was written"
    far.reset()
    return idx_h, cidx, off_h, want, s0, ws


UPD = pytest.mark.parametrize("which", ["staged", "update"])


@on_floats
@UPD
@IT
def test_far_sequence_scatter_add(far, which, it, coracle):
    n = sum(LENS[which])
    g = np.random.default_rng(21).standard_normal((n, far.D)).astype(np.float32)
    _, cidx, _, want, _, _ = _run_update(far, which, it, lambda m, idx, off, twin: m.sequence_scatter_add_(_dev(g), idx, off, -0.5, batch=B))
    if far.fmt == "f32":      # the C oracle's sequential scatter-add on the request "one bag per lookup"
        rule = coracle.bwd_f32(far.twin_f32()[1].copy(), cidx, np.arange(n), g, alpha=-0.5)
        assert np.array_equal(want, _u32(rule))


@on_floats
@pytest.mark.parametrize("optimizer", ["sgd", "rowwise_adagrad", "adagrad"])
@UPD
@IT
def test_far_sequence_optimizer_step(far, optimizer, which, it, coracle):
    """the state rows are far too: ``r * 4`` bytes reach 2^32 for the row-wise state of the fp32 table, ``r * D * 4`` for the element-wise"""
    n = sum(LENS[which])
    g = np.random.default_rng(22).standard_normal((n, far.D)).astype(np.float32)
    state = optimizer != "sgd"
    _, cidx, _, want, s0, ws = _run_update(far, which, it, lambda m, idx, off, twin: m.sequence_optimizer_step_(_dev(g), idx, off, batch=B),
                                           optimizer=optimizer, state=state)
    if far.fmt != "f32":
        return
    w0 = far.twin_f32()[1]
    if optimizer == "sgd":
        assert np.array_equal(want, _u32(coracle.bwd_f32(w0.copy(), cidx, np.arange(n), g, alpha=-0.05)))
    elif optimizer == "adagrad":      # tests/elem_adagrad_rules.py at the bars tests/test_gpu_elem_adagrad.py holds the kernels to
        Gs, count = A.grad_sum_f32(len(far.probes), cidx, np.arange(n), g)
        w_exp, s_exp = A.step_f32(w0, s0, Gs, count > 0, 0.05, 1e-6)
        assert np.allclose(ws, s_exp, rtol=A.STATE_RTOL, atol=0) and np.allclose(want.view(np.float32), w_exp, rtol=A.W_RTOL, atol=A.W_ATOL)


@on_floats
@UPD
@IT
def test_far_sequence_dense_grad(far, which, it):
    """the gradient buffers have the tables' rows: their rows are far rows too"""
    omit = _omitted(far)
    idx_h, cidx, off_h, _, idx, off, _ = far.case(which, it, omit=omit)
    g = np.random.default_rng(23).standard_normal((idx_h.size, far.D)).astype(np.float32)
    outs = far.m.sequence_dense_grad(_dev(g), idx, off, batch=B)
    want = S.dense_grad([1, len(far.probes)], [far.D] * 2, cidx, off_h[:-1], B, g)[1]
    assert [tuple(o.shape) for o in outs] == [(r, far.D) for r in far.rows] and outs[0].dtype == torch.float32
    assert np.array_equal(_bits(_rows(outs[1], far.probes)), _u32(want))
    assert not _rows(outs[1], far.sent).any() and not _rows(outs[1], omit).any()
    assert _nonzero(outs[1]) == int(np.count_nonzero(_u32(want))) and _nonzero(outs[0]) == 0
    del outs
    torch.cuda.empty_cache()


@on_floats
@pytest.mark.parametrize("step", ["scatter_add", "rowwise_adagrad", "adagrad"])
@UPD
@IT
def test_far_pooled_update_keeps_the_padding_row(far, step, which, it, coracle):
    """``padding_idx=-1``: the guard saves and restores a row (and its state) beyond 2^32 bytes"""
    g = np.random.default_rng(24).standard_normal((B, 2 * far.D)).astype(np.float32)

    def apply(m, idx, off, twin):
        if step == "scatter_add":
            m.scatter_add_(_dev(g), idx, off, alpha=-0.5, batch=B)
        else:
            m.adagrad_step_(_dev(g), idx, off, batch=B)

    assert far.pad_last * far.D * far.es >= 2 ** 32
    idx_h, cidx, off_h, want, _, _ = _run_update(far, which, it, apply, optimizer=None if step == "scatter_add" else step,
                                                 pad=far.pad_last, state=step != "scatter_add")
    if far.fmt == "f32" and step == "scatter_add":      # the oracle on the request without its padded lookups
        ck = len(far.probes) - 1
        fi, fo, _ = P.filtered_request(cidx, off_h, 2, B, [None, ck])
        rule = coracle.bwd_f32(far.twin_f32()[1].copy(), fi, fo[B:2 * B], g[:, far.D:], alpha=-0.5)
        assert np.array_equal(want, _u32(rule)) and np.array_equal(rule[ck], far.twin_f32()[1][ck])


# =========================================================================================================================================
# 3. far output and gradient rows
# =========================================================================================================================================

ROWS3, D3 = 64, 1024
N3 = 2 ** 32 // D3 + 64                                       # rows of an output of more than 2^32 elements
CHUNK = 1 << 18


def _idx3(dtype=torch.int64):
    """N3 lookups of a 64-row table in which neighbours differ and rows 2^20 and 2^22 apart -- 2^32 bytes and 2^32 elements of fp32
    rows of 1024 -- differ too"""
    j = torch.arange(N3, device=DEV, dtype=torch.int64)
    return ((j * 37 + j // 64 + j // (1 << 20) * 5) % ROWS3).to(dtype)


def _threshold_rows3(es):
    """output rows around the byte and element thresholds, 64 each"""
    out = []
    for X in F.THRESHOLDS:
        for stride in {D3 * es, D3}:
            c = X // stride
            if 32 <= c and c + 32 <= N3:
                out.append(c)
    return sorted(set(out))


def _check_far_output(out, idx, table, rule_rows, what):
    """``out [N3, D3]`` against ``table[idx]`` on the device, chunk by chunk (``table`` holds the expected output row of every table row,
    in the output's dtype: small offsets only); then 64 rows around every threshold on the host against ``rule_rows(row numbers)``"""
    assert tuple(out.shape) == (N3, D3) and out.dtype == table.dtype
    ib = torch.int16 if out.element_size() == 2 else torch.int32
    bad = 0
    for a in range(0, N3, CHUNK):
        b = min(N3, a + CHUNK)
        bad += int((out[a:b].view(ib) != table[idx[a:b].long()].view(ib)).any(dim=1).sum())
    assert bad == 0, f"{what}: {bad} of {N3} output rows differ"
    idx_h = idx.cpu().numpy().astype(np.int64)
    cs = _threshold_rows3(out.element_size())
    assert len(cs) >= 3
    for c in cs:
        got = _bits(out[c - 32:c + 32])
        assert np.array_equal(got, rule_rows(idx_h[c - 32:c + 32])), (what, c)


def _table3(seed):
    x = np.random.default_rng(seed).standard_normal((ROWS3, D3)).astype(np.float32)
    x[np.abs(x) < 0.01] = 0.5
    return x


@gpu
@pytest.mark.parametrize("kind,out", [("f32", None), ("bf16", "bf16")])
def test_out_lookup_sequence(kind, out):
    import param_amd

    _close_far()
    es = 4 if out is None else 2
    _need(N3 * D3 * es + N3 * 8 + 2 * GIB, "lookup_sequence output")
    bits = E.to_bits(_table3(1), kind)
    m = param_amd.BatchedEmbeddingBagMI355([ROWS3], D3, dtype=TDT[kind], device=DEV, init=None, fused_update=False, output_dtype=out)
    m.table(0).copy_(_dev_bits(bits, TDT[kind]))
    idx = _idx3()
    off = torch.tensor([0, N3], dtype=torch.int64, device=DEV)
    got = m.lookup_sequence(idx, off, batch=1)
    _check_far_output(got, idx, m.table(0), lambda r: bits[r], f"lookup_sequence {kind}")
    del got
    torch.cuda.empty_cache()


def _qmodule3(bits, out=None):
    import param_amd
    from oracle import rowquant

    q = rowquant.quantize_rows(_table3(2 + bits), bits)
    m = param_amd.QuantizedBatchedEmbeddingBagMI355([ROWS3], D3, bits, device=DEV, output_dtype=out)
    m.table(0).copy_(torch.from_numpy(q).to(DEV))
    # the expected output row of every table row: the un-pooled lookup of rows 0 .. 63 (small offsets), itself held to the rule
    ar = torch.arange(ROWS3, device=DEV)
    deq = m.lookup_sequence(ar, torch.tensor([0, ROWS3], device=DEV), batch=1)
    want = Q.rows(q, D3, bits, np.arange(ROWS3))
    assert np.array_equal(_bits(deq), _u32(want))
    return m, q, deq, want


@gpu
@pytest.mark.parametrize("bits", [8, 4])
def test_out_quantised_lookup_sequence(bits):
    _close_far()
    _need(N3 * D3 * 4 + N3 * 8 + 2 * GIB, "quantised lookup_sequence output")
    m, q, deq, want = _qmodule3(bits)
    idx = _idx3()
    got = m.lookup_sequence(idx, torch.tensor([0, N3], dtype=torch.int64, device=DEV), batch=1)
    _check_far_output(got, idx, deq, lambda r: _u32(want[r]), f"quantised lookup_sequence {bits}")
    del got
    torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize("burst", [True, False], ids=["burst", "row-stores"])
@pytest.mark.parametrize("bits", [8, 4])
def test_out_quantised_lookup(bits, burst):
    """bags of one lookup: a pooled row is ``fmaf(scale, code, +0.0 + bias)``, the un-pooled rule; with the output burst and without"""
    from param_amd import _lib

    _close_far()
    _need(N3 * D3 * 4 + 2 * N3 * 8 + 2 * GIB, "quantised lookup output")
    m, q, deq, want = _qmodule3(bits)
    idx = _idx3()
    off = torch.arange(N3 + 1, dtype=torch.int64, device=DEV)
    try:
        _lib.set_forward_tuning(stage_out=-1 if burst else 0)
        plan = m.plan(idx, off, batch=N3)
        assert plan["stage_out"] == (D3 if burst else 0) and plan["tiles_per_table"] * plan["bags_per_block"] >= N3
        got = m.lookup(idx, off, batch=N3)
    finally:
        _lib.set_forward_tuning()
    _check_far_output(got, idx, deq, lambda r: _u32(want[r]), f"quantised lookup {bits} burst={burst}")
    del got
    torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize("out", [None, "bf16", "fp16"], ids=["padded-fp32", "bf16", "fp16"])
def test_out_padded_and_out16_forward(out):
    """the padded forward (fp32 output, a padding row that every 64th bag looks up: its pooled row is +0.0) and the 16-bit-output
    forward (one rounding of the table row)"""
    import param_amd
    from param_amd import _lib

    _close_far()
    es = 4 if out is None else 2
    _need(N3 * D3 * es + 2 * N3 * 8 + 2 * GIB, "pooled output")
    x = _table3(9)
    pad = 5 if out is None else None
    m = param_amd.BatchedEmbeddingBagMI355([ROWS3], D3, device=DEV, init=None, fused_update=False, padding_idx=pad, output_dtype=out)
    m.table(0).copy_(_dev(x))
    idx = _idx3()
    off = torch.arange(N3 + 1, dtype=torch.int64, device=DEV)
    plan = _lib.embbag_plan(m._tables().request(idx, off, N3, None, 0, None, forward=True), _lib.PM_PLAN_PADDED if out is None else _lib.PM_PLAN_PADDED16)
    print(f"far output {out}: {plan}")
    assert plan["tiles_per_table"] * plan["bags_per_block"] >= N3
    got = m.lookup(idx, off, batch=N3)
    if out is None:
        x[pad] = 0.0
        table, rule = _dev(x), (lambda r: _u32(x[r]))
        assert (idx == pad).any()
    else:
        table, rule = _dev(x).to(got.dtype), (lambda r: O.round16(x[r], out))
    _check_far_output(got, idx, table, rule, f"pooled output {out}")
    del got
    torch.cuda.empty_cache()


def _grad_expectation(idx):
    """gradient row b holds ``float(b % 7)`` in every column: every table row's sum is an integer below 2^24 -- exact in fp32 in any
    order -- and equal to a weighted ``np.bincount``"""
    idx_h = idx.cpu().numpy().astype(np.int64)
    want = np.bincount(idx_h, weights=(np.arange(N3) % 7).astype(np.float64), minlength=ROWS3)
    assert want.max() < 2 ** 24 and want.min() > 0
    return want.astype(np.float32)


def _grad3(dtype):
    g = torch.empty((N3, D3), dtype=dtype, device=DEV)
    for a in range(0, N3, CHUNK):
        b = min(N3, a + CHUNK)
        g[a:b] = (torch.arange(a, b, device=DEV) % 7).to(dtype)[:, None]
    return g


def _assert_row_sums(outs, want):
    got = outs[0].cpu().numpy()
    assert got.shape == (ROWS3, D3) and np.array_equal(got, np.broadcast_to(want[:, None], got.shape))


@gpu
def test_grad_sequence_dense_grad():
    import param_amd

    _close_far()
    _need(N3 * D3 * 4 + 4 * GIB, "sequence gradient")
    m = param_amd.BatchedEmbeddingBagMI355([ROWS3], D3, device=DEV, init=None, fused_update=False)
    idx = _idx3()
    g = _grad3(torch.float32)
    outs = m.sequence_dense_grad(g, idx, torch.tensor([0, N3], dtype=torch.int64, device=DEV), batch=1)
    _assert_row_sums(outs, _grad_expectation(idx))
    del g
    torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize("out", ["bf16", None], ids=["mean-bf16-widen", "mean-fp32"])
def test_grad_dense_grad_of_a_mean_module(out):
    """a far ``grad`` through ``pm_embbag_grad_widen`` (bf16 output) and through ``pm_embbag_mean_grad`` (fp32); bags of one lookup: the
    mean's factor is 1"""
    import param_amd

    _close_far()
    gdt = torch.float32 if out is None else torch.bfloat16
    _need(N3 * D3 * (gdt.itemsize + 4) + 4 * GIB, "pooled gradient and its fp32 copy")
    m = param_amd.BatchedEmbeddingBagMI355([ROWS3], D3, device=DEV, init=None, fused_update=False, pooling_mode="mean", output_dtype=out)
    idx = _idx3()
    off = torch.arange(N3 + 1, dtype=torch.int64, device=DEV)
    g = _grad3(gdt)
    outs = m.dense_grad(g, idx, off, batch=N3)
    _assert_row_sums(outs, _grad_expectation(idx))
    del g
    torch.cuda.empty_cache()


@gpu
def test_out_and_grad_of_a_max_module():
    """max pooling's four new address computations beyond 2^32 elements: the bf16 values and the int32 ``max_indices`` of
    ``pm_embbag_fwd_max`` (``arg_out + out_offsets[t] + (bag0 + bg) * out_stride + c``), then ``grad``, ``max_indices`` and ``g_seq`` of
    ``pm_embbag_max_grad`` (``row + c4 * 4``, ``g_seq + j * g_stride``).  Bags of one lookup: a value is one rounding of the table row and
    its arg-max the looked-up row in every column (+0.0 and -1 for the bags that look up the padding row); a gradient row lands whole in
    that row, so the sums are the exact integers of ``_grad_expectation`` without the padded bags."""
    import param_amd
    from param_amd import _lib

    _close_far()
    # the values (2 bytes) next to max_indices (4); then, the values freed, max_indices (4), grad (2) and g_seq (4): 40 GiB
    _need(N3 * D3 * (4 + 2 + 4) + 2 * N3 * 8 + 4 * GIB, "max pooling: max_indices, grad and g_seq")
    x = _table3(11)
    pad = 5
    m = param_amd.MaxBatchedEmbeddingBagMI355([ROWS3], D3, device=DEV, init=None, fused_update=False, padding_idx=pad, output_dtype="bf16")
    m.table(0).copy_(_dev(x))
    idx = _idx3()
    off = torch.arange(N3 + 1, dtype=torch.int64, device=DEV)
    plan = _lib.embbag_plan(m._tables().request(idx, off, N3, None, 0, None, forward=True), _lib.PM_PLAN_PADDED16)
    print(f"far max output: {plan}")
    assert plan["tiles_per_table"] * plan["bags_per_block"] >= N3 and N3 * D3 > 2 ** 32
    got, arg = m.lookup(idx, off, batch=N3, return_max_indices=True)
    padded = idx == pad
    n_pad = int(padded.sum())
    assert 0 < n_pad < N3 // 32
    x[pad] = 0.0
    _check_far_output(got, idx, _dev(x).to(torch.bfloat16), lambda r: O.round16(x[r], "bf16"), "max pooled output bf16")
    del got
    torch.cuda.empty_cache()
    # max_indices: every column of row b is idx[b], -1 for a padded bag -- whole on the device, around the thresholds on the host
    assert tuple(arg.shape) == (N3, D3) and arg.dtype == torch.int32
    want_arg = torch.where(padded, torch.full_like(idx, -1), idx).to(torch.int32)
    bad = 0
    for a in range(0, N3, CHUNK):
        b = min(N3, a + CHUNK)
        bad += int((arg[a:b] != want_arg[a:b, None]).any(dim=1).sum())
    assert bad == 0, f"max_indices: {bad} of {N3} rows differ"
    want_h = want_arg.cpu().numpy()
    cs = _threshold_rows3(4)
    assert {(2 ** 31) // D3, (2 ** 32) // D3} <= set(cs)
    for c in cs:
        assert np.array_equal(arg[c - 32:c + 32].cpu().numpy(), np.broadcast_to(want_h[c - 32:c + 32, None], (64, D3))), ("max_indices", c)
    # the gradient: grad and max_indices read, g_seq written and read, beyond 2^32 elements each
    g = _grad3(torch.bfloat16)
    outs = m.dense_grad(g, idx, off, batch=N3, max_indices=arg)
    want = _grad_expectation(idx)
    want[pad] = 0.0
    _assert_row_sums(outs, want)
    del g, arg, outs
    torch.cuda.empty_cache()
