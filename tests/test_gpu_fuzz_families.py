"""Randomised parity sweep over the module families beyond the base module (the base one: tests/test_gpu_fuzz.py): whole requests and
module configurations drawn by tests/fuzz_cases.py -- table count, dims, dtypes and formats, index type, ragged / empty / one very long
bag, weights, layout, batch slice, offsets with or without the trailing entry, and every option of the family together -- each held to
the family's numpy rule ON BITS.  The only bound is the base fuzz's hot-row bound for rows of more than 256 lookups in the sorted
backward (``fuzz_cases.hot_row_bound``).  Seeds are fixed: a failure reproduces with ``fuzz_cases.case(family, seed)``.
``PARAM_AMD_FUZZ_SEEDS=k`` multiplies every family's default seed count for a one-off soak."""
import os

import numpy as np
import pytest
import torch

from tests import bounds_rules as BR
from tests import embedding_rules as E
from tests import fuzz_cases as FC
from tests import max_direct_rules as MD
from tests import max_rules as MX
from tests import mean_rules as MR
from tests import out16_rules as O
from tests import padding_rules as P
from tests import psw_grad_rules as PG
from tests import sequence_grad_rules as SG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
ODT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
IDT = {"i32": torch.int32, "i64": torch.int64}
KOUT = {"fp32": "f32", "bf16": "bf16", "fp16": "f16"}
_MULT = int(os.environ.get("PARAM_AMD_FUZZ_SEEDS", "1"))      # one-off soak runs: PARAM_AMD_FUZZ_SEEDS=20


def _seeds(family):
    return range(FC.SEEDS[family] * _MULT)


def _dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _bits(t):
    t = t.detach().contiguous()
    if t.element_size() == 2:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _dev_bits(bits, dtype):
    """a device tensor of ``dtype`` holding the uint16 / uint32 bit patterns ``bits``"""
    b = np.ascontiguousarray(bits)
    raw = torch.from_numpy(b.view(np.int16 if b.dtype == np.uint16 else np.int32)).to(DEV)
    return raw.view(dtype)


def _request(c, idx=None, off=None):
    i, o = FC.request_arrays(c) if idx is None else (idx, off)
    return _dev(i), _dev(o)


def _fill(m, c):
    for t, bits in enumerate(c["tables"]):
        m.table(t).copy_(_dev_bits(bits, TDT[c["wdt"]]))


def _gradient(c, shape, seed_offset=0):
    """(device gradient, its exact fp32 values): fp32, or -- ``grad16`` -- in the module's 16-bit output dtype, widened exactly"""
    g = np.random.default_rng([c["seed"], 77 + seed_offset]).standard_normal(shape).astype(np.float32)
    if c.get("grad16"):
        bits = O.round16(g, c["odt"])
        return _dev_bits(bits, ODT[c["odt"]]), O.widen(bits, c["odt"])
    return _dev(g), g


def _unstaged(c, plan):
    """the long bag is longer than the index tile the plan stages: its tile is really unstaged"""
    if c["long_bag"] is not None and not c.get("damaged"):
        assert int(c["lens"][c["long_bag"]]) > plan["idx_cap"] > 0, plan


def _off_tile(c, plan):
    """the seed that meets the host's ``slice_off_tile`` condition: its slice begins inside a tile of the plan's own size"""
    if c["seed"] == FC.off_tile_seed(c["family"]):
        assert FC.off_tile(c) and c["slice"][0] % plan["bags_per_block"] != 0, plan


def _closed(off, TB, N):
    return np.concatenate([np.asarray(off).astype(np.int64)[:TB], [N]])


def _sliced_lookup(c, call, want_parts, whole_shape, odt):
    """the slice goes into a caller's ``out`` pre-filled with the sentinel, which stays outside it"""
    b0, n = c["slice"]
    out = torch.full(whole_shape, FC.SENTINEL, dtype=ODT[odt], device=DEV)
    call(out, b0, n)
    part = FC.join([p if p.dtype != np.float32 else FC.out_bits(p, odt) for p in want_parts], c["layout"])
    want = FC.canvas(whole_shape, c["layout"], part, b0, n, FC.sentinel_bits(odt))
    assert FC.same_bits(_bits(out), want, odt), "batch slice"


def _hot_and_cold(got, exact, truth, mag, cnt, what):
    """rows of at most 256 lookups on bits; every row within the base fuzz's bound of the fp64 sum"""
    cold = cnt <= FC.EXACT_RUN
    assert np.array_equal(MX.bits(got)[cold], MX.bits(exact)[cold]), (what, "cold rows")
    assert (np.abs(got.astype(np.float64) - truth) <= FC.hot_row_bound(cnt.astype(np.float64)[:, None], mag)).all(), (what, "hot rows")


# ---- train ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", _seeds("train"))
def test_train(seed, coracle):
    from param_amd import BatchedEmbeddingBagMI355, _lib

    c = FC.case("train", seed)
    T, B, rows, dims, odt = c["T"], c["B"], c["rows"], c["dims"], c["odt"]
    m = BatchedEmbeddingBagMI355(rows, dims, dtype=TDT[c["wdt"]], device=DEV, layout=c["layout"], init=None, fused_update=False,
                                 bounds_check_mode=c["bounds"], padding_idx=c["pads"], pooling_mode="mean" if c["mean"] else "sum",
                                 output_dtype=None if odt == "fp32" else odt)
    _fill(m, c)
    pads = FC.normal_pads(c["pads"], rows)
    assert m.padding_idx == (None if all(k is None for k in pads) else pads)
    psw_t = _dev(c["psw"])
    ridx, roff, report = FC.repaired(c)

    # forward: whole batch; the request is repaired in place, the report is the rule's
    idx_t, off_t = _request(c)
    got = m.lookup(idx_t, off_t, psw_t, batch=B)
    want = FC.train_forward(c)
    whole = FC.join([w if odt != "fp32" else FC.out_bits(w, "fp32") for w in want], c["layout"])
    assert got.dtype == ODT[odt] and FC.same_bits(_bits(got), whole, odt), "forward"
    assert np.array_equal(idx_t.cpu().numpy(), ridx) and np.array_equal(off_t.cpu().numpy(), roff), "the request after the call"
    if c["bounds"] == "warning":
        assert m.bounds_report() == BR.report_dict(report)
    kind = _lib.PM_PLAN_PADDED16 if odt != "fp32" else _lib.PM_PLAN_PADDED if (c["mean"] or m.padding_idx is not None) else _lib.PM_PLAN_FORWARD
    plan = _lib.embbag_plan(m._tables().request(idx_t, off_t, B, psw_t, 0, None, forward=True), kind)
    _unstaged(c, plan)
    _off_tile(c, plan)

    # forward: the batch slice, on a fresh copy of the request as it was handed over
    if c["slice"] is not None:
        i2, o2 = _request(c)
        _sliced_lookup(c, lambda out, b0, n: m.lookup(i2, o2, psw_t, out=out, batch=B, bag_begin=b0, bag_count=n),
                       FC.train_forward(c, True), tuple(got.shape), odt)
        assert np.array_equal(i2.cpu().numpy(), ridx) and np.array_equal(o2.cpu().numpy(), roff)

    # gradients, on the repaired request
    N = ridx.size
    g_t, g32 = _gradient(c, tuple(got.shape))
    grads = [np.ascontiguousarray(p) for p in FC.split(g32, dims, c["layout"])]
    W = FC.widened(c)
    if c["psw"] is not None:
        want_psw = P.psw_grad_mask(PG.restate(W, ridx, roff, B, grads, PG.vec_of(c["wdt"]))[0], ridx, roff, T, B, pads)
        assert PG.same_bits(m.per_sample_weights_grad(g_t, idx_t, off_t, batch=B).cpu().numpy(), want_psw), "per_sample_weights_grad"
    scaled = MR.scale_grad(grads, ridx, roff, B, pads) if c["mean"] else grads
    truth = P.dense_grad(rows, dims, ridx, roff, B, pads, scaled, c["psw"])
    mag = P.dense_grad(rows, dims, ridx, roff, B, pads, [np.abs(s) for s in scaled], None if c["psw"] is None else np.abs(c["psw"]))
    keep = ~P.padded_mask(ridx, roff, T, B, pads)
    own = P.table_of(roff, T, B, N)
    if c["psw"] is None:
        exact = MR.sum_dense_grad(rows, dims, ridx, roff, B, pads, scaled)
    else:      # the weighted sequential scatter-add: the C oracle's, on the request without its padded lookups
        fi, fo, fw = P.filtered_request(ridx, roff, T, B, pads, c["psw"])
        fo = _closed(fo, T * B, fi.size)
        exact = []
        for t in range(T):
            s, e = int(fo[t * B]), int(fo[(t + 1) * B])
            exact.append(coracle.bwd_f32(np.zeros((rows[t], dims[t]), np.float32), fi[s:e], fo[t * B:(t + 1) * B] - s, scaled[t], fw[s:e]))
    cnts = [np.bincount(ridx[keep & (own == t)].astype(np.int64), minlength=rows[t]) for t in range(T)]
    dense = m.dense_grad(g_t, idx_t, off_t, psw_t, batch=B)
    sparse = m.sparse_grad(g_t, idx_t, off_t, psw_t, batch=B)
    hit = P.sparse_rows(ridx, roff, T, B, pads)
    for t in range(T):
        _hot_and_cold(dense[t].cpu().numpy(), exact[t], truth[t], mag[t], cnts[t], ("dense_grad", t))
        r, v = sparse[t]
        assert np.array_equal(r.cpu().numpy(), hit[t]), ("sparse_grad rows", t)
        _hot_and_cold(v.cpu().numpy(), exact[t][hit[t]], truth[t][hit[t]], mag[t][hit[t]], cnts[t][hit[t]], ("sparse_grad", t))

    # the in-place update leaves the padding rows' bits -- and every row without a kept lookup -- as they were
    before = [_bits(m.table(t)).copy() for t in range(T)]
    m.scatter_add_(g_t, idx_t, off_t, alpha=-0.125, per_sample_weights=psw_t, batch=B)
    after = [_bits(m.table(t)) for t in range(T)]
    for t, kept in enumerate(P.guard(before, after, pads)):
        assert np.array_equal(kept, after[t]), ("padding row", t)
        assert np.array_equal(after[t][cnts[t] == 0], before[t][cnts[t] == 0]), ("rows without a kept lookup", t)


# ---- max ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", _seeds("max"))
def test_max(seed):
    from param_amd import MaxBatchedEmbeddingBagMI355, _lib

    c = FC.case("max", seed)
    T, B, rows, dims, odt = c["T"], c["B"], c["rows"], c["dims"], c["odt"]
    m = MaxBatchedEmbeddingBagMI355(rows, dims, dtype=TDT[c["wdt"]], device=DEV, layout=c["layout"], init=None, fused_update=False,
                                    padding_idx=c["pads"], output_dtype=None if odt == "fp32" else odt)
    _fill(m, c)
    pads = FC.normal_pads(c["pads"], rows)
    idx, off = FC.request_arrays(c)
    idx_t, off_t = _request(c)
    W = FC.widened(c)
    vals, args = MX.forward(W, idx, off, B, pads)
    got, arg_t = m.lookup(idx_t, off_t, batch=B, return_max_indices=True)
    assert FC.same_bits(_bits(got), FC.join([FC.out_bits(v, odt) for v in vals], c["layout"]), odt), "forward"
    assert arg_t.dtype == torch.int32 and np.array_equal(arg_t.cpu().numpy(), FC.join(args, c["layout"])), "max_indices"
    plan = _lib.embbag_plan(m._tables().request(idx_t, off_t, B, None, 0, None, forward=True),
                            _lib.PM_PLAN_PADDED16 if odt != "fp32" else _lib.PM_PLAN_PADDED)
    _unstaged(c, plan)
    _off_tile(c, plan)
    if c["slice"] is not None:
        b0, n = c["slice"]
        v2, a2 = MX.forward(W, idx, off, B, pads, b0, n)
        got_arg = []
        _sliced_lookup(c, lambda out, b0, n: got_arg.append(m.lookup(idx_t, off_t, out=out, batch=B, bag_begin=b0, bag_count=n,
                                                                     return_max_indices=True)[1]), v2, tuple(got.shape), odt)
        want_arg = FC.canvas(tuple(got.shape), c["layout"], FC.join(a2, c["layout"]), b0, n, np.int32(-1))
        assert np.array_equal(got_arg[0].cpu().numpy(), want_arg), "max_indices of a slice: -1 outside it"

    g_t, g32 = _gradient(c, tuple(got.shape))
    grads = [np.ascontiguousarray(p) for p in FC.split(g32, dims, c["layout"])]
    sums = MD.sums(rows, dims, idx, off, B, grads, args)
    if c["same_dims"]:
        dense = m.dense_grad(g_t, idx_t, off_t, batch=B, method="sorted", max_indices=arg_t)
        exact = MX.dense_grad(rows, dims, grads, args)
        own = P.table_of(off, T, B, idx.size)
        for t in range(T):
            cnt = np.bincount(idx[own == t].astype(np.int64), minlength=rows[t])
            _hot_and_cold(dense[t].cpu().numpy(), exact[t], sums[t][2], sums[t][3], cnt, ("sorted max backward", t))
    for saved in (arg_t, None):
        dense = m.dense_grad(g_t, idx_t, off_t, batch=B, method="direct", max_indices=saved)
        for t in range(T):
            G, won = sums[t][0], sums[t][1]
            want = MD.apply(np.zeros((rows[t], dims[t]), np.uint32), "f32", G, won, 1.0)
            assert np.array_equal(_bits(dense[t]), want), ("direct dense_grad", t, saved is None)
    wkind = {"f32": "f32", "bf16": "bf16", "f16": "fp16"}[c["wdt"]]
    for saved in (arg_t, None):
        _fill(m, c)
        m.scatter_add_(g_t, idx_t, off_t, alpha=0.375, batch=B, method="direct", max_indices=saved)
        for t in range(T):
            want = MD.apply(c["tables"][t], wkind, sums[t][0], sums[t][1], 0.375)
            assert np.array_equal(_bits(m.table(t)), want), ("direct scatter_add_: a row that wins no column keeps its bits", t, saved is None)


# ---- sequence -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", _seeds("sequence"))
def test_sequence(seed):
    from param_amd import BatchedEmbeddingBagMI355

    c = FC.case("sequence", seed)
    T, B, rows, dims, odt = c["T"], c["B"], c["rows"], c["dims"], c["odt"]
    D, kin, kout = dims[0], c["wdt"], KOUT[c["odt"]]
    m = BatchedEmbeddingBagMI355(rows, dims, dtype=TDT[kin], device=DEV, layout=c["layout"], init=None, fused_update=False,
                                 padding_idx=c["pads"], output_dtype=None if odt == "fp32" else odt)
    _fill(m, c)
    pads = FC.normal_pads(c["pads"], rows)
    idx, off = FC.request_arrays(c)
    idx_t, off_t = _request(c)
    N = idx.size
    got = m.lookup_sequence(idx_t, off_t, batch=B)
    want = E.forward(c["tables"], kin, kout, idx, off, B, np.zeros((N, D), dtype=E.BITS[kout]))
    assert got.dtype == ODT[odt] and E.same(_bits(got), want, kin, kout), "lookup_sequence"
    if c["slice"] is not None:
        b0, n = c["slice"]
        out = torch.full((N, D), FC.SENTINEL, dtype=ODT[odt], device=DEV)
        m.lookup_sequence(idx_t, off_t, batch=B, out=out, bag_begin=b0, bag_count=n)
        blank = np.full((N, D), FC.sentinel_bits(odt), dtype=E.BITS[kout])
        assert E.same(_bits(out), E.forward(c["tables"], kin, kout, idx, off, B, blank, b0, n), kin, kout), "sliced lookup_sequence"

    c = dict(c, grad16=odt != "fp32" and seed % 2 == 0)
    g_t, g32 = _gradient(c, (N, D))
    dense = m.sequence_dense_grad(g_t, idx_t, off_t, batch=B)
    # (a request without a lookup: the rule's sums are empty -- its reshape of an empty gradient is not defined)
    exact = SG.dense_grad(rows, dims, idx, off, B, g32, pads) if N else [np.zeros((r, D), dtype=np.float32) for r in rows]
    own = P.table_of(off, T, B, N)
    keep = ~P.padded_mask(idx, off, T, B, pads)
    for t in range(T):
        sel = keep & (own == t)
        truth, mag = np.zeros((rows[t], D)), np.zeros((rows[t], D))
        np.add.at(truth, idx[sel].astype(np.int64), g32[sel].astype(np.float64))
        np.add.at(mag, idx[sel].astype(np.int64), np.abs(g32[sel].astype(np.float64)))
        cnt = np.bincount(idx[sel].astype(np.int64), minlength=rows[t])
        _hot_and_cold(dense[t].cpu().numpy(), exact[t], truth, mag, cnt, ("sequence_dense_grad", t))


# ---- serving families -----------------------------------------------------------------------------------------------------------------

def _quantized_module(c):
    from param_amd import QuantizedBatchedEmbeddingBagMI355

    fam = c["family"]
    kw = dict(device=DEV, layout=c["layout"], output_dtype=None if c["odt"] == "fp32" else c["odt"])
    if fam == "pruned":
        kw["index_remapping"] = [None if r is None else torch.from_numpy(r) for r in c["remaps"]]
    rows = c["phys_rows"] if fam == "pruned" else c["rows"]
    m = QuantizedBatchedEmbeddingBagMI355(rows, c["dims"], c["bits"][0] if fam == "qrows" else c["bits"], **kw)
    host = np.zeros(m.weights.numel(), dtype=np.uint8)
    for t, q in enumerate(c["tables"]):
        host[m._starts[t]:m._starts[t] + q.size] = q.reshape(-1)
    m.weights.copy_(torch.from_numpy(host))
    assert m.pruned == (fam == "pruned") and (m.bitwidth is None) == (len(set(c["bits"])) == 2)
    return m


def _f8_module(c):
    from param_amd import Float8BatchedEmbeddingBagMI355

    dt = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}[c["fmt"]]
    m = Float8BatchedEmbeddingBagMI355(c["rows"], c["dims"], dt, device=DEV, layout=c["layout"], padding_idx=c["pads"],
                                       pooling_mode="mean" if c["pool"] == "mean" else "sum",
                                       output_dtype=None if c["odt"] == "fp32" else c["odt"])
    for t, tab in enumerate(c["tables"]):
        m.copy_from_(t, _dev(tab))
    return m


def _f8s_module(c, tables=None):
    """the case's scaled module (``tables``: only these, unfilled -- the quantiser's target)"""
    from param_amd import Float8BatchedEmbeddingBagMI355

    dt = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}[c["fmt"]]
    if tables is not None:
        return Float8BatchedEmbeddingBagMI355([c["rows"][t] for t in tables], [c["dims"][t] for t in tables], dt, device=DEV, scale=c["scale"])
    m = Float8BatchedEmbeddingBagMI355(c["rows"], c["dims"], dt, device=DEV, layout=c["layout"], padding_idx=c["pads"], scale=c["scale"],
                                       pooling_mode="mean" if c["pool"] == "mean" else "sum",
                                       output_dtype=None if c["odt"] == "fp32" else c["odt"])
    for t, (tab, (E_t, e_rows)) in enumerate(zip(c["tables"], c["exps"])):
        m.copy_from_(t, _dev(tab), exponents=E_t if c["scale"] == "table" else _dev(e_rows))
    return m


def _anyfmt_module(c):
    from param_amd import MixedBatchedEmbeddingBagMI355

    m = MixedBatchedEmbeddingBagMI355(c["rows"], c["dims"], c["fmts"], device=DEV, layout=c["layout"], output_dtype=ODT[c["odt"]])
    m.table_exponents.copy_(torch.tensor(c["exps"], dtype=torch.int32))
    host = np.zeros(m.weights.numel(), dtype=np.uint8)
    for t, tab in enumerate(c["tables"]):
        host[m._starts[t]:m._starts[t] + tab.size] = tab.reshape(-1)
    m.weights.copy_(torch.from_numpy(host))
    return m


def _mx4_module(c, tables=None):
    from param_amd import MX4BatchedEmbeddingBagMI355

    if tables is not None:
        return MX4BatchedEmbeddingBagMI355([c["rows"][t] for t in tables], [c["dims"][t] for t in tables], device=DEV)
    m = MX4BatchedEmbeddingBagMI355(c["rows"], c["dims"], device=DEV, layout=c["layout"], pooling_mode="mean" if c["pool"] == "mean" else "sum",
                                    output_dtype=None if c["odt"] == "fp32" else c["odt"])
    for t, (tab, d) in enumerate(zip(c["tables"], c["dims"])):
        m.copy_from_(t, _dev(tab[:, :d // 2]), _dev(tab[:, d // 2:d // 2 + d // 32]))
    return m


_MODULE = {"f8": _f8_module, "f8s": _f8s_module, "anyfmt": _anyfmt_module, "mx4": _mx4_module}


def _sources(c, t):
    """table t's quantiser source in the case's source dtype, as (name, device tensor) contiguous and as a strided view of a wider tensor;
    and its exact fp32 values"""
    wide = FC.quantiser_source(c, t)
    d, pad = c["dims"][t], FC.SRC_PAD
    xw = _dev(wide).to(ODT[c["src"]])                          # exact: the values are representable in the source dtype
    view = xw[:, pad:pad + d]
    assert view.is_contiguous() == (c["rows"][t] == 1) and view.stride(0) == d + 2 * pad
    x32 = np.ascontiguousarray(wide[:, pad:pad + d])
    assert np.array_equal(view.to(torch.float32).cpu().numpy().view(np.uint32), x32.view(np.uint32))
    return (("contiguous", view.contiguous()), ("strided", view)), x32


def _quantiser_f8s(c):
    """the HIP quantiser on a random source of every table's shape against ``f8s_rules.quantize``: exponents exactly, codes byte for byte, a
    NaN code by class"""
    S = FC.F8S
    for t in range(c["T"]):
        sources, x32 = _sources(c, t)
        e = S.row_exponents(x32, c["fmt"])
        want = S.quantize(x32, c["fmt"], e.astype(np.int64) if c["scale"] == "row" else int(e.max()))
        for name, x in sources:
            m = _f8s_module(c, [t])
            m.quantize_from_(0, x)
            if c["scale"] == "row":
                assert np.array_equal(m.row_exponents_of(0).cpu().numpy(), e), ("quantiser: row exponents", t, name)
            else:
                assert int(m.table_exponents[0]) == int(e.max()), ("quantiser: table exponent", t, name)
            assert S.same_codes(m.table(0).view(torch.uint8).cpu().numpy(), want, c["fmt"]), ("quantiser: codes", t, name)


def _quantiser_mx4(c):
    """the HIP quantiser against ``mx4_rules.quantize``, byte for byte (pad bytes included); a NaN block's code bytes are not compared"""
    for t in range(c["T"]):
        sources, x32 = _sources(c, t)
        d = c["dims"][t]
        want = FC.mx4_quantize(x32)
        nan_codes = np.repeat(want[:, d // 2:d // 2 + d // 32] == 255, 16, axis=1)
        assert nan_codes.any()
        for name, x in sources:
            m = _mx4_module(c, [t])
            m.table(0).fill_(0xAA)
            m.quantize_from_(0, x)
            got = m.table(0).cpu().numpy()
            got[:, :d // 2][nan_codes] = 0
            assert np.array_equal(got, want), ("quantiser", t, name)


def _serving(family, seed):
    c = FC.case(family, seed)
    B, odt = c["B"], c["odt"]
    m = _MODULE.get(family, _quantized_module)(c)
    idx_t, off_t = _request(c)
    psw_t = _dev(c["psw"])
    got = m.lookup(idx_t, off_t, psw_t, batch=B)
    want = FC.join([FC.out_bits(p, odt) for p in FC.serving_forward(c)], c["layout"])
    assert got.dtype == ODT[odt] and FC.same_bits(_bits(got), want, odt), "lookup"
    plan = m.plan(idx_t, off_t, psw_t, batch=B)
    _unstaged(c, plan)
    _off_tile(c, plan)
    if c["slice"] is not None:
        _sliced_lookup(c, lambda out, b0, n: m.lookup(idx_t, off_t, psw_t, out=out, batch=B, bag_begin=b0, bag_count=n),
                       FC.serving_forward(c, True), tuple(got.shape), odt)
    if not c["same_dims"]:
        return
    want, written, copied = FC.serving_sequence_bits(c)
    assert written.all()
    got = m.lookup_sequence(idx_t, off_t, batch=B)
    assert got.dtype == ODT[odt] and FC.same_bits(_bits(got), want, odt), "lookup_sequence"
    assert copied is None or np.array_equal(_bits(got)[copied], want[copied]), "a float row read into its own type is a bit copy"
    if family == "pruned":
        gone = FC.PR.physical(c["remaps"], *FC.request_arrays(c), B) < 0
        assert not _bits(got)[gone].any(), "a pruned lookup gives a row of +0.0"
    if c["slice"] is not None:
        b0, n = c["slice"]
        want, written, copied = FC.serving_sequence_bits(c, True)
        out = torch.full(tuple(got.shape), FC.SENTINEL, dtype=ODT[odt], device=DEV)
        m.lookup_sequence(idx_t, off_t, batch=B, out=out, bag_begin=b0, bag_count=n)
        want = np.where(written[:, None], want, FC.sentinel_bits(odt))
        assert FC.same_bits(_bits(out), want, odt), "sliced lookup_sequence"
        assert copied is None or np.array_equal(_bits(out)[copied], want[copied]), "sliced lookup_sequence: bit copies"


@pytest.mark.parametrize("seed", _seeds("qrows"))
def test_qrows(seed):
    _serving("qrows", seed)


@pytest.mark.parametrize("seed", _seeds("qmixed"))
def test_qmixed(seed):
    _serving("qmixed", seed)


@pytest.mark.parametrize("seed", _seeds("pruned"))
def test_pruned(seed):
    _serving("pruned", seed)


@pytest.mark.parametrize("seed", _seeds("f8"))
def test_f8(seed):
    _serving("f8", seed)


@pytest.mark.parametrize("seed", _seeds("f8s"))
def test_f8s(seed):
    _quantiser_f8s(FC.case("f8s", seed))
    _serving("f8s", seed)


@pytest.mark.parametrize("seed", _seeds("anyfmt"))
def test_anyfmt(seed):
    _serving("anyfmt", seed)


@pytest.mark.parametrize("seed", _seeds("mx4"))
def test_mx4(seed):
    _quantiser_mx4(FC.case("mx4", seed))
    _serving("mx4", seed)
