"""Runs one group of tests/plan_sweep.py on the GPU: for every case the knobs are set, ``pm_embbag_plan`` (``pm_embedding_gather_plan``)
must report the row pinned in tests/plan_sweep_host.json, the entry point runs -- int64 and int32 indices, layouts ``bd`` and ``tbd``
where the dims are equal -- and its output must equal the rule of the operation bit for bit.  The FP8 entries (``f8``, ``f8_gather``) build ``Float8BatchedEmbeddingBagMI355``
modules, are asked through ``pm_embbag_f8_plan`` / ``pm_embedding_gather_f8_plan`` and compare with tests/f8_rules.py; the scaled ones
(``f8s``, ``f8s_gather``) build the same class with ``scale=``, exponents as tests/test_gpu_f8s.py draws them, are asked through
``pm_embbag_f8_scaled_plan`` / ``pm_embedding_gather_f8_plan`` and compare with tests/f8s_rules.py; the mixed-format ones (``anyfmt``,
``anyfmt_gather``) build ``MixedBatchedEmbeddingBagMI355`` over the tables of tests/anyfmt_cases.py, are asked through
``pm_embbag_anyfmt_plan`` / ``pm_embedding_gather_anyfmt_plan`` and compare with tests/anyfmt_rules.py.

tests/test_gpu_plan_sweep.py calls ``run_group`` in its own process; for the groups with an environment setting it starts
``python -m tests.plan_sweep_worker GROUP`` with that setting, because the switches are read once per process.  Exit status 0: every
comparison held; 1: the failures are on stdout."""
import json
import os
import sys

import numpy as np

from tests import anyfmt_cases as AC
from tests import anyfmt_rules as AR
from tests import embedding_rules as ER
from tests import f8_rules as F8
from tests import f8s_rules as F8S
from tests import mean_rules as M
from tests import out16_rules as O16
from tests import padding_rules as P
from tests import plan_sweep as S
from tests import psw_grad_rules as PG
from tests.qrows_rules import same_f32 as _same_f32_or_nan

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
_PINNED = None
_cache = {}


def pinned(name):
    global _PINNED
    if _PINNED is None:
        _PINNED = json.load(open(os.path.join(HERE, "plan_sweep_host.json")))["rows"]
    return _PINNED[name]["plan"]


def _torch():
    import torch

    return torch


def _t(a, dtype=None):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _bits16(t):
    """a bf16 / fp16 tensor as uint16 bits"""
    return t.contiguous().view(_torch().int16).cpu().numpy().view(np.uint16)


def variants(c):
    """(index dtype, layout) pairs a case runs"""
    if c.entry in S.GATHER_ENTRIES or len(set(c.dims)) > 1:
        return [("i64", "bd"), ("i32", "bd")]
    if c.request.startswith("auto") or c.group.startswith("base"):
        return [("i64", "bd"), ("i32", "tbd")]
    return [("i64", "bd"), ("i32", "tbd"), ("i32", "bd"), ("i64", "tbd")]


def _pads(c):
    return c.req.pads if c.entry in ("padded", "mean", "out16", "mean_grad", "max") or (c.entry == "widen" and c.mean) else None


def module(c, layout):
    """the module of a case and its tables as fp32 values (16-bit tables widened: exact); one per distinct set of options"""
    torch = _torch()
    from param_amd import BatchedEmbeddingBagMI355, MaxBatchedEmbeddingBagMI355

    td = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
    od = {None: None, "bf16": torch.bfloat16, "fp16": torch.float16}
    pads = _pads(c)
    out16 = c.out16 if c.entry != "gather" else {"f32": None, "bf16": "bf16", "f16": "fp16"}[c.kind]
    is_max = c.entry == "max"
    key = ("module", c.kind, tuple(c.dims), tuple(c.req.rows), layout, None if pads is None else tuple(pads), c.mean, out16, is_max)

    def make():
        cls, mode = (MaxBatchedEmbeddingBagMI355, "max") if is_max else (BatchedEmbeddingBagMI355, "mean" if c.mean else "sum")
        m = cls(c.req.rows, c.dims, dtype=td[c.kind], device=DEV, layout=layout, init="normal", seed=7, fused_update=False,
                padding_idx=pads, pooling_mode=mode, output_dtype=od[out16])
        return m, [m.table(t).float().cpu().numpy().copy() for t in range(c.req.T)]
    return _memo(key, make)


def _assemble(outs, layout):
    return np.concatenate(outs, axis=1) if layout == "bd" else np.stack(outs)


def reference(c, layout, coracle, tabs):
    """the whole batch's output by the rule of the case's operation (fp32 values; 16-bit outputs: uint16 bits), computed once"""
    r, w = c.req, c.weighted
    psw = r.psw if w else None
    if c.entry in ("fwd", "quantized"):
        return _memo(("fwd", c.request, c.kind, tuple(c.dims), w, layout), lambda: coracle.fwd_batched(tabs, r.idx, r.off, r.B, psw=psw, layout=layout))
    pads = _pads(c)
    if c.mean:
        outs = _memo(("mean", c.request, c.kind, tuple(c.dims)), lambda: M.forward(tabs, r.idx, r.off, r.B, pads))
    else:
        outs = _memo(("padded", c.request, c.kind, tuple(c.dims), w), lambda: P.forward(tabs, r.idx, r.off, r.B, pads, psw))
    if c.entry == "out16":
        outs = [O16.round16(o, c.out16) for o in outs]
    return _assemble(outs, layout)


def _sel(layout, b0, n):
    return (slice(b0, b0 + n),) if layout == "bd" else (slice(None), slice(b0, b0 + n))


def _same_f32(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _first_diff(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} elements differ, the first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}" if len(bad) else "shapes differ"


def check_plan(c, op):
    from param_amd import _lib

    if c.entry == "f8":
        got = list(_lib.embbag_f8_plan(op, S.OUT16_CODE[c.out16]).values())
    elif c.entry == "f8s":
        got = list(_lib.embbag_f8_scaled_plan(op, S.OUT16_CODE[c.out16], c.mean, c.scale == "row").values())
    elif c.entry in ("f8_gather", "f8s_gather"):
        got = list(_lib.embedding_gather_f8_plan(op).values())
    elif c.entry == "anyfmt":
        got = list(_lib.embbag_anyfmt_plan(op, S.OUT16_CODE[c.out16]).values())
    elif c.entry == "anyfmt_gather":
        got = list(_lib.embedding_gather_anyfmt_plan(op).values())
    elif c.plan_kind == "gather":
        got = list(_lib.embedding_gather_plan(op).values())
    else:
        got = list(_lib.embbag_plan(op, S.KIND[c.plan_kind]).values())
    assert got == pinned(c.name), f"pm_embbag_plan reports {got}, tests/plan_sweep_host.json pins {pinned(c.name)}"


def run_forward(c, idt, layout, coracle):
    """fwd, padded, mean, out16: the whole batch, or a slice into a NaN canvas"""
    torch = _torch()
    r, (b0, n) = c.req, c.bags
    m, tabs = module(c, layout)
    it = torch.int64 if idt == "i64" else torch.int32
    idx_t, off_t = _t(r.idx, it), _t(r.off, it)
    psw_t = _t(r.psw) if c.weighted else None
    check_plan(c, m._tables().request(idx_t, off_t, r.B, psw_t, b0, n if c.bag_slice else None, forward=True))
    want = reference(c, layout, coracle, tabs)
    shape = (r.B, sum(c.dims)) if layout == "bd" else (r.T, r.B, c.dims[0])
    if c.entry == "out16":
        canvas = torch.full(shape, float("nan"), dtype=m.output_dtype, device=DEV)
        m.lookup(idx_t, off_t, psw_t, out=canvas, batch=r.B, bag_begin=b0, bag_count=n)
        got, blank = _bits16(canvas), _bits16(torch.full((1,), float("nan"), dtype=m.output_dtype))[0]
        sel = _sel(layout, b0, n)
        assert O16.same_bits(got[sel], want[sel], c.out16), _first_diff(got[sel], want[sel])
        rest = np.ones(shape, dtype=bool)
        rest[sel] = False
        assert (got[rest] == blank).all(), "written outside the slice"
        return
    canvas = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    m.lookup(idx_t, off_t, psw_t, out=canvas, batch=r.B, bag_begin=b0, bag_count=n)
    got = canvas.cpu().numpy()
    sel = _sel(layout, b0, n)
    assert _same_f32(got[sel], want[sel]), _first_diff(got[sel], want[sel])
    rest = np.ones(shape, dtype=bool)
    rest[sel] = False
    assert np.isnan(got[rest]).all(), "written outside the slice"


def max_reference(c, tabs):
    """(values, args) of tests/max_rules.py for the whole batch, per table; a Python loop over the lookups: computed once per
    (request, table dtype, dims) and shared by the knobs, index types, layouts and output types"""
    from tests import max_rules as MX

    r = c.req

    def make():
        vals, args = MX.forward(tabs, r.idx, r.off, r.B, _pads(c))
        held = S.max_conditions(r, vals, args)                     # what the request is there for, on the tables that are compared
        assert held == (c.request != "pad_lumpy", True, True), f"{c.request} on these tables: all padded / first padded / winner twice = {held}"
        return vals, args
    return _memo(("max", c.request, c.kind, tuple(c.dims)), make)


def run_max(c, idt, layout, coracle):
    """pm_embbag_fwd_max: values and ``max_indices`` of the slice into a NaN canvas and a canvas of -77, both equal to the rule bit
    for bit and untouched elsewhere; then the lookup without ``max_indices`` (the WITH_ARG = false instances): the same value bits"""
    from tests import max_rules as MX

    torch = _torch()
    r, (b0, n) = c.req, c.bags
    m, tabs = module(c, layout)
    it = torch.int64 if idt == "i64" else torch.int32
    idx_t, off_t = _t(r.idx, it), _t(r.off, it)
    check_plan(c, m._tables().request(idx_t, off_t, r.B, None, b0, n if c.bag_slice else None, forward=True))
    want_v, want_a = max_reference(c, tabs)
    want_a = _assemble(want_a, layout)
    shape = (r.B, sum(c.dims)) if layout == "bd" else (r.T, r.B, c.dims[0])
    sel = _sel(layout, b0, n)
    rest = np.ones(shape, dtype=bool)
    rest[sel] = False
    odt = torch.float32 if c.out16 is None else m.output_dtype
    assert (c.out16 is None) == (m.output_dtype in (None, torch.float32))
    arg_canvas = torch.full(shape, -77, dtype=torch.int32, device=DEV)
    canvas = torch.full(shape, float("nan"), dtype=odt, device=DEV)
    res = m.lookup(idx_t, off_t, out=canvas, batch=r.B, bag_begin=b0, bag_count=n, max_indices=arg_canvas)
    assert res[0] is canvas and res[1] is arg_canvas
    plain = torch.full(shape, float("nan"), dtype=odt, device=DEV)
    assert m.lookup(idx_t, off_t, out=plain, batch=r.B, bag_begin=b0, bag_count=n) is plain
    if c.out16 is None:
        want = _assemble(want_v, layout)
        for what, t in (("values", canvas), ("values without max_indices", plain)):
            got = t.cpu().numpy()
            assert _same_f32(got[sel], want[sel]), f"{what}: {_first_diff(got[sel].view(np.uint32), want[sel].view(np.uint32))}"
            assert np.isnan(got[rest]).all(), f"{what}: written outside the slice"
    else:
        want = _assemble(MX.round_out(want_v, c.out16), layout)
        blank = _bits16(torch.full((1,), float("nan"), dtype=odt))[0]
        for what, t in (("values", canvas), ("values without max_indices", plain)):
            got = _bits16(t)
            assert O16.same_bits(got[sel], want[sel], c.out16), f"{what}: {_first_diff(got[sel], want[sel])}"
            assert (got[rest] == blank).all(), f"{what}: written outside the slice"
        assert np.array_equal(_bits16(canvas), _bits16(plain)), "with and without max_indices"
    got_a = arg_canvas.cpu().numpy()
    assert np.array_equal(got_a[sel], want_a[sel]), f"max_indices: {_first_diff(got_a[sel], want_a[sel])}"
    assert (got_a[rest] == -77).all(), "max_indices written outside the slice"


def run_quantized(c, idt, layout, coracle):
    """the bytes under the case's knobs: the rowquant reference of the oracle's forward, and the default-knob bytes of the same request"""
    import param_amd
    from oracle import rowquant as orq

    torch = _torch()
    r = c.req
    m, tabs = module(c, layout)
    it = torch.int64 if idt == "i64" else torch.int32
    idx_t, off_t = _t(r.idx, it), _t(r.off, it)
    check_plan(c, m._tables().request(idx_t, off_t, r.B, None, 0, None, forward=True))
    got = m.lookup_quantized(idx_t, off_t, c.bits, batch=r.B).cpu().numpy()
    D = c.dims[0]
    exp = reference(c, layout, coracle, tabs).reshape(-1, D)
    want = orq.quantize_rows(exp, c.bits)
    assert np.array_equal(got.reshape(want.shape), want), _first_diff(got.reshape(want.shape), want)
    param_amd.set_tuning()
    param_amd.set_forward_tuning()
    default = m.lookup_quantized(idx_t, off_t, c.bits, batch=r.B).cpu().numpy()
    assert np.array_equal(got, default), "the bytes differ from the default-knob bytes"


def run_gather(c, idt, layout, coracle):
    torch = _torch()
    r, (b0, n) = c.req, c.bags
    m, _ = module(c, layout)
    it = torch.int64 if idt == "i64" else torch.int32
    idx_t, off_t = _t(r.idx, it), _t(r.off, it)
    check_plan(c, m._tables().request(idx_t, off_t, r.B, None, b0, n if c.bag_slice else None))
    D = c.dims[0]
    if c.kind == "f32":
        bits = [m.table(t).cpu().numpy().view(np.uint32) for t in range(r.T)]
        canvas = torch.full((r.N, D), float("nan"), dtype=torch.float32, device=DEV)
        as_bits = lambda x: x.cpu().numpy().view(np.uint32)                                   # noqa: E731
    else:
        bits = [_bits16(m.table(t)) for t in range(r.T)]
        canvas = torch.full((r.N, D), float("nan"), dtype=m.output_dtype, device=DEV)
        as_bits = _bits16
    before = as_bits(canvas).copy()
    m.lookup_sequence(idx_t, off_t, batch=r.B, out=canvas, bag_begin=b0, bag_count=n)
    want = ER.forward(bits, c.kind, c.kind, r.idx, r.off, r.B, before, b0, n)
    got = as_bits(canvas)
    assert np.array_equal(got, want), _first_diff(got, want)
    if c.bag_slice:
        assert (want == before).any() and (want != before).any()


def run_base(c, idt, layout, coracle):
    """an entry point on the base plan: the same bits under the case's knobs, under the default knobs and by its rule (the atomic
    backward: within the fuzz test's bar, BASELINE north_star's 1e-5 of the summed magnitudes)"""
    import param_amd
    from param_amd import _lib

    torch = _torch()
    r = c.req
    T, B, dims, rows = r.T, r.B, c.dims, r.rows
    it = torch.int64 if idt == "i64" else torch.int32
    idx_t, off_t = _t(r.idx, it), _t(r.off, it)
    psw_t = _t(r.psw) if c.weighted else None
    m, tabs = module(c, layout)
    shape = (B, sum(dims)) if layout == "bd" else (T, B, dims[0])
    g32 = np.random.default_rng(900 + len(c.name)).standard_normal(shape).astype(np.float32)
    if c.entry == "widen":
        g16 = O16.round16(g32, c.out16)
        g32 = O16.widen(g16, c.out16)
        g_t = _t(g16.view(np.int16)).view(m.output_dtype)
    else:
        g_t = _t(g32)
    grads = [np.ascontiguousarray(g32[:, sum(dims[:t]):sum(dims[:t + 1])] if layout == "bd" else g32[t]) for t in range(T)]
    op_psw = psw_t if c.entry in ("widen", "atomic") else None

    def run(pinned_plan=True):                                     # (the default-knob run has a plan of its own: not compared)
        check = lambda: pinned_plan and check_plan(c, m._tables().request(idx_t, off_t, B, op_psw, 0, None))  # noqa: E731
        if c.entry == "psw_grad":
            check()
            return [m.per_sample_weights_grad(g_t, idx_t, off_t, batch=B).cpu().numpy()]
        if c.entry == "atomic":
            with _lib.use_alternates():                            # (the atomic kernel lives in the alternates build, whose knobs are its own)
                param_amd.set_tuning(*c.tuning_args())
                check()
                try:
                    return [d.cpu().numpy() for d in m.dense_grad(g_t, idx_t, off_t, psw_t, batch=B, method="atomic")]
                finally:
                    param_amd.set_tuning()
        check()
        return [d.cpu().numpy() for d in m.dense_grad(g_t, idx_t, off_t, psw_t, batch=B)]

    got = run()
    if c.entry == "atomic":
        for t in range(T):
            s, e = r.off[t * B], r.off[(t + 1) * B]
            bag_of = np.repeat(np.arange(B), r.lens[t * B:(t + 1) * B])
            contrib = grads[t].astype(np.float64)[bag_of] * r.psw[s:e].astype(np.float64)[:, None]
            truth, mag = np.zeros((rows[t], dims[t])), np.zeros((rows[t], dims[t]))
            np.add.at(truth, r.idx[s:e], contrib)
            np.add.at(mag, r.idx[s:e], np.abs(contrib))
            cnt = np.bincount(r.idx[s:e], minlength=rows[t]).astype(np.float64)[:, None]
            tol_atomic = np.maximum(1e-5, cnt * 2.0 ** -23) * mag + 1e-30                     # tests/test_gpu_fuzz.py
            assert (np.abs(got[t] - truth) <= tol_atomic).all(), ("atomic backward", t, float(np.abs(got[t] - truth).max()))
        return
    knobs = (c.tuning_args(), c.forward_args())
    param_amd.set_tuning()
    param_amd.set_forward_tuning()
    try:
        default = run(pinned_plan=False)
    finally:
        param_amd.set_tuning(*knobs[0])
        param_amd.set_forward_tuning(*knobs[1])
    for a, b in zip(got, default):
        assert _same_f32(a, b), "the bits differ from the default-knob bits"
    pads = _pads(c)
    if c.entry == "psw_grad":
        want, written, _, _ = PG.restate(tabs, r.idx, r.off, B, grads, S.VEC[c.kind])
        assert written.all() and PG.same_bits(got[0], want), _first_diff(got[0], want)
    elif c.mean:
        want = M.dense_grad(rows, dims, r.idx, r.off, B, pads, grads)
        for t in range(T):
            assert _same_f32(got[t], want[t]), (t, _first_diff(got[t], want[t]))
    else:
        for t in range(T):
            s, e = r.off[t * B], r.off[(t + 1) * B]
            assert np.bincount(r.idx[s:e], minlength=rows[t]).max() <= 256       # (the sorted apply's exact-run limit)
            want = coracle.bwd_f32(np.zeros((rows[t], dims[t]), np.float32), r.idx[s:e], r.off[t * B:(t + 1) * B] - s, grads[t],
                                   r.psw[s:e] if c.weighted else None)
            assert _same_f32(got[t], want), (t, _first_diff(got[t], want))


def f8_tables(c):
    """the uint8 code tables of an FP8 case, one set per (format, rows, dims): finite codes from a fixed seed (the non-finite ones are
    tests/test_gpu_f8.py's), and in every row one of the format's zeros and subnormals, at a column that moves with the row"""
    def make():
        mbits = 3 if c.kind == "e4m3" else 2
        special = np.array([s | m for s in (0, 0x80) for m in range(1 << mbits)], dtype=np.uint8)          # +-0 and the subnormals
        tabs = []
        for t, (rows, D) in enumerate(zip(c.req.rows, c.dims)):
            tab = F8.finite_codes(np.random.default_rng(7000 + t), c.kind, (rows, D))
            r = np.arange(rows)
            tab[r, r % D] = special[r % special.size]
            assert not F8.is_nan_code(tab, c.kind).any() and np.isfinite(F8.dec(tab, c.kind)).all() and set(special) <= set(np.unique(tab).tolist())
            tabs.append(tab)
        return tabs
    return _memo(("f8 tables", c.kind, tuple(c.req.rows), tuple(c.dims)), make)


def f8_module(c, layout):
    """the Float8BatchedEmbeddingBagMI355 of a case, one per distinct set of options, filled through ``copy_from_``"""
    torch = _torch()
    from param_amd import Float8BatchedEmbeddingBagMI355

    pads = None if c.entry in S.GATHER_ENTRIES else c.req.pads
    key = ("f8 module", c.kind, tuple(c.dims), tuple(c.req.rows), layout, None if pads is None else tuple(pads), c.mean, c.out16, c.scale)

    def make():
        m = Float8BatchedEmbeddingBagMI355(c.req.rows, c.dims, c.kind, device=DEV, layout=layout, pooling_mode="mean" if c.mean else "sum",
                                           padding_idx=pads, output_dtype={None: None, "bf16": torch.bfloat16, "fp16": torch.float16}[c.out16],
                                           scale=c.scale)
        for t, tab in enumerate(f8_tables(c)):
            if c.scale is None:
                m.copy_from_(t, _t(tab))
            else:
                E, er = f8s_exps(c)[t]
                m.copy_from_(t, _t(tab), exponents=E if c.scale == "table" else _t(er))
        return m
    return _memo(key, make)


def run_f8(c, idt, layout, coracle):
    """pm_embbag_fwd_f8: the batch, or a slice of it, into a NaN canvas that must equal tests/f8_rules.py: forward on bits (a 16-bit
    output: its one rounding) and stay NaN elsewhere"""
    torch = _torch()
    r, (b0, n) = c.req, c.bags
    m, tabs = f8_module(c, layout), f8_tables(c)
    it = torch.int64 if idt == "i64" else torch.int32
    idx_t, off_t = _t(r.idx, it), _t(r.off, it)
    psw_t = _t(r.psw) if c.weighted else None
    check_plan(c, m._request(idx_t, off_t, psw_t, b0, n if c.bag_slice else None, r.B, False)[2])
    outs = _memo(("f8", c.request, c.kind, tuple(c.dims), c.weighted, c.mean),
                 lambda: F8.forward(tabs, c.kind, r.idx, r.off, r.B, r.pads, r.psw if c.weighted else None, c.mean))
    assert all(np.isfinite(o).all() for o in outs)
    shape = (r.B, sum(c.dims)) if layout == "bd" else (r.T, r.B, c.dims[0])
    sel = _sel(layout, b0, n)
    rest = np.ones(shape, dtype=bool)
    rest[sel] = False
    canvas = torch.full(shape, float("nan"), dtype=m.output_dtype, device=DEV)
    assert m.lookup(idx_t, off_t, psw_t, out=canvas, batch=r.B, bag_begin=b0, bag_count=n) is canvas
    if c.out16 is None:
        got, want = canvas.cpu().numpy(), _assemble(outs, layout)
        assert _same_f32_or_nan(got[sel], want[sel]), _first_diff(got[sel].view(np.uint32), want[sel].view(np.uint32))
        assert np.isnan(got[rest]).all(), "written outside the slice"
    else:
        got, want = _bits16(canvas), _assemble([O16.round16(o, c.out16) for o in outs], layout)
        assert F8.same16(got[sel], want[sel], c.out16), _first_diff(got[sel], want[sel])
        assert (got[rest] == _bits16(torch.full((1,), float("nan"), dtype=m.output_dtype))[0]).all(), "written outside the slice"


def run_f8_gather(c, idt, layout, coracle):
    """pm_embedding_gather_f8 into a NaN canvas: tests/f8_rules.py: sequence on bits where the rule writes, NaN elsewhere"""
    torch = _torch()
    r, (b0, n) = c.req, c.bags
    m, tabs = f8_module(c, layout), f8_tables(c)
    it = torch.int64 if idt == "i64" else torch.int32
    idx_t, off_t = _t(r.idx, it), _t(r.off, it)
    check_plan(c, m._request(idx_t, off_t, None, b0, n if c.bag_slice else None, r.B, False)[2])
    want, written = _memo(("f8 rows", c.request, c.kind, tuple(c.dims), b0, n), lambda: F8.sequence(tabs, c.kind, r.idx, r.off, r.B, b0, n))
    assert written.any() and (written.all() != bool(c.bag_slice))
    canvas = torch.full((r.N, c.dims[0]), float("nan"), dtype=m.output_dtype, device=DEV)
    assert m.lookup_sequence(idx_t, off_t, batch=r.B, out=canvas, bag_begin=b0, bag_count=n) is canvas
    if c.out16 is None:
        got = canvas.cpu().numpy()
        assert _same_f32_or_nan(got[written], want[written]), _first_diff(got[written].view(np.uint32), want[written].view(np.uint32))
        assert np.isnan(got[~written]).all(), "written outside the slice"
    else:
        got, want16 = _bits16(canvas), F8.sequence16(want, c.out16)
        assert F8.same16(got[written], want16[written], c.out16), _first_diff(got[written], want16[written])
        assert (got[~written] == _bits16(torch.full((1,), float("nan"), dtype=m.output_dtype))[0]).all(), "written outside the slice"


def f8s_exps(c):
    """the exponents of a scaled case's tables, ``[(E_t | None, e_rows | None)]`` as tests/f8s_rules.py takes them, drawn as
    tests/test_gpu_f8s.py: make_exps draws them -- row mode: one per row in [-30, 10], no two neighbours equal; table mode: one value;
    a different set per table"""
    def make():
        if c.scale == "table":
            return [((13 * t + 5) % 41 - 30, None) for t in range(c.req.T)]
        return [(None, ((np.arange(rows) * 7 + (11 * t + 3) % 41) % 41 - 30).astype(np.int64)) for t, rows in enumerate(c.req.rows)]
    exps = _memo(("f8s exps", c.scale, tuple(c.req.rows)), make)
    if c.scale == "row":
        assert all((np.diff(er) != 0).all() for _, er in exps) and (c.req.T == 1 or not np.array_equal(exps[0][1][:100], exps[1][1][:100]))
    else:
        assert len({E for E, _ in exps}) == c.req.T and all(E for E, _ in exps)
    return exps


def run_f8s(c, idt, layout, coracle):
    """pm_embbag_fwd_f8_scaled: run_f8 with exponents -- ``pm_embbag_f8_scaled_plan`` must report the pinned row (plan_f8's with the
    restated f8s_stage_out), the NaN canvas must equal tests/f8s_rules.py: forward on bits and stay NaN elsewhere"""
    torch = _torch()
    r, (b0, n) = c.req, c.bags
    m, tabs, exps = f8_module(c, layout), f8_tables(c), f8s_exps(c)
    assert m.scale == c.scale
    it = torch.int64 if idt == "i64" else torch.int32
    idx_t, off_t = _t(r.idx, it), _t(r.off, it)
    psw_t = _t(r.psw) if c.weighted else None
    check_plan(c, m._request(idx_t, off_t, psw_t, b0, n if c.bag_slice else None, r.B, False)[2])
    outs = _memo(("f8s", c.request, c.kind, tuple(c.dims), c.weighted, c.mean, c.scale),
                 lambda: F8S.forward(tabs, c.kind, exps, r.idx, r.off, r.B, r.pads, r.psw if c.weighted else None, c.mean))
    assert all(np.isfinite(o).all() for o in outs)
    shape = (r.B, sum(c.dims)) if layout == "bd" else (r.T, r.B, c.dims[0])
    sel = _sel(layout, b0, n)
    rest = np.ones(shape, dtype=bool)
    rest[sel] = False
    canvas = torch.full(shape, float("nan"), dtype=m.output_dtype, device=DEV)
    assert m.lookup(idx_t, off_t, psw_t, out=canvas, batch=r.B, bag_begin=b0, bag_count=n) is canvas
    if c.out16 is None:
        got, want = canvas.cpu().numpy(), _assemble(outs, layout)
        assert _same_f32_or_nan(got[sel], want[sel]), _first_diff(got[sel].view(np.uint32), want[sel].view(np.uint32))
        assert np.isnan(got[rest]).all(), "written outside the slice"
    else:
        got, want = _bits16(canvas), _assemble([F8S.round16(o, c.out16) for o in outs], layout)
        assert F8S.same16(got[sel], want[sel], c.out16), _first_diff(got[sel], want[sel])
        assert (got[rest] == _bits16(torch.full((1,), float("nan"), dtype=m.output_dtype))[0]).all(), "written outside the slice"


def run_f8s_gather(c, idt, layout, coracle):
    """pm_embedding_gather_f8_scaled into a NaN canvas: tests/f8s_rules.py: sequence on bits where the rule writes, NaN elsewhere"""
    torch = _torch()
    r, (b0, n) = c.req, c.bags
    m, tabs, exps = f8_module(c, layout), f8_tables(c), f8s_exps(c)
    assert m.scale == c.scale
    it = torch.int64 if idt == "i64" else torch.int32
    idx_t, off_t = _t(r.idx, it), _t(r.off, it)
    check_plan(c, m._request(idx_t, off_t, None, b0, n if c.bag_slice else None, r.B, False)[2])
    if _memo(("f8 unscaled twin asked", c.group), lambda: [c.name, idt])[:] == [c.name, idt]:
        # once per group: pm_embedding_gather_f8_scaled launches on plan_gather_f8, a scaled module's ``sequence_plan`` is an unscaled one's
        from param_amd import Float8BatchedEmbeddingBagMI355

        plain = _memo(("f8 unscaled twin", c.kind, tuple(c.dims), tuple(r.rows), layout),
                      lambda: Float8BatchedEmbeddingBagMI355(r.rows, c.dims, c.kind, device=DEV, layout=layout))
        assert plain.scale is None
        args = dict(batch=r.B, bag_begin=b0, bag_count=n if c.bag_slice else None)
        assert m.sequence_plan(idx_t, off_t, **args) == plain.sequence_plan(idx_t, off_t, **args) and list(m.sequence_plan(idx_t, off_t, **args).values()) == pinned(c.name)
    want, written = _memo(("f8s rows", c.request, c.kind, tuple(c.dims), c.scale, b0, n),
                          lambda: F8S.sequence(tabs, c.kind, exps, r.idx, r.off, r.B, b0, n))
    assert written.any() and (written.all() != bool(c.bag_slice)) and np.isfinite(want).all()
    canvas = torch.full((r.N, c.dims[0]), float("nan"), dtype=m.output_dtype, device=DEV)
    assert m.lookup_sequence(idx_t, off_t, batch=r.B, out=canvas, bag_begin=b0, bag_count=n) is canvas
    if c.out16 is None:
        got = canvas.cpu().numpy()
        assert _same_f32_or_nan(got[written], want[written]), _first_diff(got[written].view(np.uint32), want[written].view(np.uint32))
        assert np.isnan(got[~written]).all(), "written outside the slice"
    else:
        got, want16 = _bits16(canvas), F8S.round16(want, c.out16)
        assert F8S.same16(got[written], want16[written], c.out16), _first_diff(got[written], want16[written])
        assert (got[~written] == _bits16(torch.full((1,), float("nan"), dtype=m.output_dtype))[0]).all(), "written outside the slice"


_ANY_KIND = {None: "f32", "bf16": "bf16", "fp16": "f16"}           # a case's ``out16`` as tests/anyfmt_rules.py spells the output kind


def anyfmt_tables(c):
    """the tables of a mixed-format case as tests/anyfmt_rules.py: Table (the bytes the module stores), from tests/anyfmt_cases.py: one
    set per (formats, rows, dims); every FP8 table carries a table exponent that is not 0, neighbours' differ"""
    def make():
        tabs = AC.tables(c.formats, c.req.rows, c.dims, 7100, exps=[(-2, 3, -5, 1)[t % 4] for t in range(c.req.T)])
        assert all(tab.exp != 0 for tab in tabs if tab.fmt.startswith("fp8"))
        return tabs
    return _memo(("anyfmt tables", tuple(c.formats), tuple(c.req.rows), tuple(c.dims)), make)


def anyfmt_module(c, layout):
    """the MixedBatchedEmbeddingBagMI355 of a case, one per distinct set of options; float and FP8 tables go in through ``copy_from_``
    (FP8: uint8 codes and the exponent), quantised rows through the table view"""
    torch = _torch()
    from param_amd import MixedBatchedEmbeddingBagMI355

    key = ("anyfmt module", tuple(c.formats), tuple(c.dims), tuple(c.req.rows), layout, c.out16)
    view = {"fp32": np.float32, "bf16": np.int16, "fp16": np.int16}
    tdt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}

    def make():
        m = MixedBatchedEmbeddingBagMI355(c.req.rows, c.dims, c.formats, device=DEV, layout=layout,
                                          output_dtype={None: None, "bf16": torch.bfloat16, "fp16": torch.float16}[c.out16])
        for t, tab in enumerate(anyfmt_tables(c)):
            if tab.fmt in view:
                m.copy_from_(t, _t(tab.data.view(view[tab.fmt]).reshape(-1, tab.dim)).view(tdt[tab.fmt]))
            elif tab.fmt.startswith("fp8"):
                m.copy_from_(t, _t(tab.data), exponent=tab.exp)
            else:
                m.table(t).copy_(_t(tab.data))
        assert m.formats == c.formats and m.table_exponents.tolist() == [tab.exp for tab in anyfmt_tables(c)]
        return m
    return _memo(key, make)


def run_anyfmt(c, idt, layout, coracle):
    """pm_embbag_fwd_anyfmt: the batch, or a slice of it, into a NaN canvas that must equal tests/anyfmt_rules.py: forward_bits (every
    table by its own format's rule; a 16-bit output: the one rounding) and stay NaN elsewhere.  The padded requests' indices are plain
    indices here: the module has no padding row."""
    torch = _torch()
    r, (b0, n) = c.req, c.bags
    m, tabs, kind = anyfmt_module(c, layout), anyfmt_tables(c), _ANY_KIND[c.out16]
    it = torch.int64 if idt == "i64" else torch.int32
    idx_t, off_t = _t(r.idx, it), _t(r.off, it)
    psw_t = _t(r.psw) if c.weighted else None
    check_plan(c, m._request(idx_t, off_t, psw_t, b0, n if c.bag_slice else None, r.B, False)[2])
    outs = _memo(("anyfmt", c.request, tuple(c.formats), tuple(c.dims), c.weighted),
                 lambda: AR.forward(tabs, r.idx, r.off, r.B, r.psw if c.weighted else None))
    assert all(np.isfinite(o).all() for o in outs)
    want = _assemble([AR.to_kind(o, kind) for o in outs], layout)
    shape = (r.B, sum(c.dims)) if layout == "bd" else (r.T, r.B, c.dims[0])
    sel = _sel(layout, b0, n)
    rest = np.ones(shape, dtype=bool)
    rest[sel] = False
    canvas = torch.full(shape, float("nan"), dtype=m.output_dtype, device=DEV)
    assert m.lookup(idx_t, off_t, psw_t, out=canvas, batch=r.B, bag_begin=b0, bag_count=n) is canvas
    got = canvas.cpu().numpy().view(np.uint32) if c.out16 is None else _bits16(canvas)
    assert AR.same(got[sel], want[sel], kind), _first_diff(got[sel], want[sel])
    assert AR.is_nan(got[rest], kind).all(), "written outside the slice"


def run_anyfmt_gather(c, idt, layout, coracle):
    """pm_embedding_gather_anyfmt into a NaN canvas: tests/anyfmt_rules.py: sequence on bits where the rule writes (a 16-bit row to
    its own type: a bit copy), NaN elsewhere"""
    torch = _torch()
    r, (b0, n) = c.req, c.bags
    m, tabs, kind = anyfmt_module(c, layout), anyfmt_tables(c), _ANY_KIND[c.out16]
    it = torch.int64 if idt == "i64" else torch.int32
    idx_t, off_t = _t(r.idx, it), _t(r.off, it)
    check_plan(c, m._request(idx_t, off_t, None, b0, n if c.bag_slice else None, r.B, False)[2])
    want, written, copied = _memo(("anyfmt rows", c.request, tuple(c.formats), tuple(c.dims), kind, b0, n),
                                  lambda: AR.sequence(tabs, r.idx, r.off, r.B, kind, b0, n))
    assert written.any() and (written.all() != bool(c.bag_slice)) and (copied.any() or kind == "f32" and "fp32" not in c.formats)
    canvas = torch.full((r.N, c.dims[0]), float("nan"), dtype=m.output_dtype, device=DEV)
    assert m.lookup_sequence(idx_t, off_t, batch=r.B, out=canvas, bag_begin=b0, bag_count=n) is canvas
    got = canvas.cpu().numpy().view(np.uint32) if c.out16 is None else _bits16(canvas)
    assert AR.same(got[written], want[written], kind, copied[written]), _first_diff(got[written], want[written])
    assert AR.is_nan(got[~written], kind).all(), "written outside the slice"


RUN = {"fwd": run_forward, "padded": run_forward, "mean": run_forward, "out16": run_forward, "quantized": run_quantized, "gather": run_gather,
       "psw_grad": run_base, "mean_grad": run_base, "widen": run_base, "atomic": run_base, "max": run_max, "f8": run_f8, "f8_gather": run_f8_gather,
       "f8s": run_f8s, "f8s_gather": run_f8s_gather, "anyfmt": run_anyfmt, "anyfmt_gather": run_anyfmt_gather}


def run_group(group, coracle, log=None):
    """every case of ``group`` under its knobs -> the list of failures (empty: all held).  The knobs are left at their defaults."""
    import param_amd

    assert _torch().cuda.is_available(), "the plan sweep needs a ROCm device"
    param_amd.load_library()
    cases = [c for c in S.CASES if c.group == group]
    assert cases, group
    for c in cases:                                                # the child of an environment group must have been given its setting
        for name in S.ENV:
            assert os.environ.get(name) == (None if name not in c.env else str(c.env[name])), (name, os.environ.get(name), c.env)
    failures = []
    try:
        for c in cases:
            for idt, layout in variants(c):
                param_amd.set_tuning(*c.tuning_args())
                param_amd.set_forward_tuning(*c.forward_args())
                verdict = "ok"
                try:
                    RUN[c.entry](c, idt, layout, coracle)
                except AssertionError as e:                        # (a HIP error is no comparison: it ends the group)
                    failures.append(f"{c.name} [{idt}, {layout}]: {e}")
                    verdict = "FAILED"
                if log:
                    log(f"{c.name} [{idt}, {layout}] {verdict}")
    finally:
        param_amd.set_tuning()
        param_amd.set_forward_tuning()
    return failures


def host_plans(group):
    """{case: what the plan query reports for the case's sizes under its knobs}.  Needs no GPU: the query dereferences no pointer of the
    request, so every pointer is a non-NULL dummy.  (tests/test_plan_sweep_host.py: the library and launch_plan_dump agree.)"""
    import param_amd
    from param_amd import _lib

    res = {}
    try:
        for c in (c for c in S.CASES if c.group == group):
            r, (b0, n) = c.req, c.bags
            op = _lib.pm_embbag_batch()
            op.num_tables, op.weight_dtype, op.index_dtype = r.T, c.dtype_code, _lib.PM_I64
            op.max_dim, op.min_dim, op.out_stride = max(c.dims), min(c.dims), sum(c.dims)
            op.batch, op.num_indices, op.bag_begin, op.bag_count = r.B, r.N, b0, n
            op.tables = op.rows = op.dims = op.out_offsets = op.indices = op.offsets = 8
            op.per_sample_weights = 8 if c.plan_weighted else None
            param_amd.set_tuning(*c.tuning_args())
            param_amd.set_forward_tuning(*c.forward_args())
            if c.entry == "f8":
                plan = _lib.embbag_f8_plan(op, S.OUT16_CODE[c.out16])
            elif c.entry == "f8s":
                plan = _lib.embbag_f8_scaled_plan(op, S.OUT16_CODE[c.out16], c.mean, c.scale == "row")
            elif c.entry in ("f8_gather", "f8s_gather"):
                plan = _lib.embedding_gather_f8_plan(op)
            elif c.entry == "anyfmt":
                plan = _lib.embbag_anyfmt_plan(op, S.OUT16_CODE[c.out16])
            elif c.entry == "anyfmt_gather":
                plan = _lib.embedding_gather_anyfmt_plan(op)
            else:
                plan = _lib.embedding_gather_plan(op) if c.plan_kind == "gather" else _lib.embbag_plan(op, S.KIND[c.plan_kind])
            res[c.name] = list(plan.values())
    finally:
        param_amd.set_tuning()
        param_amd.set_forward_tuning()
    return res


def main(argv):
    if argv[1] == "--plans":
        print(json.dumps(host_plans(argv[2])))
        return 0
    from oracle.embbag_oracle import COracle

    failures = run_group(argv[1], COracle(), log=print if "-v" in argv else None)
    for f in failures:
        print(f)
    print(f"{argv[1]}: {len(failures)} failures")
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
