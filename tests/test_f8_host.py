"""FP8 tables without a device: the rule (tests/f8_rules.py) against torch's CPU engine, live and through the committed fixture
(tests/golden/f8_cases.npz); what the constructors and the four C calls refuse; the two plan calls pinned for a list of requests
(tests/f8_plan_host.json; PARAM_AMD_REWRITE_F8_PLAN=1 rewrites it); the symbols; and that no existing module reaches the new calls."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from param_amd import _lib
from tests import f8_rules as R
from tests import out16_rules as O
from tests.qrows_rules import same_f32

HERE = os.path.dirname(os.path.abspath(__file__))
PINNED = os.path.join(HERE, "f8_plan_host.json")
FIXTURE = os.path.join(HERE, "golden", "f8_cases.npz")
REWRITE = os.environ.get("PARAM_AMD_REWRITE_F8_PLAN") == "1"
DTYPES = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
PM_F8 = {"e4m3": _lib.PM_F8E4M3, "e5m2": _lib.PM_F8E5M2}


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


# ---- dec ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", R.FORMATS)
def test_dec_is_torchs_cast_for_all_256_codes(fmt, fixture):
    codes = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(codes).view(DTYPES[fmt]).to(torch.float32).numpy()
    got = R.dec(codes, fmt)
    assert same_f32(got, want) and same_f32(got, fixture[f"dec_{fmt}"])
    nan = R.is_nan_code(codes, fmt)
    assert np.array_equal(np.isnan(got), nan) and int(nan.sum()) == (2 if fmt == "e4m3" else 6)
    assert np.signbit(got[0x80]) and got[0x80] == 0 and not np.signbit(got[0])
    assert got[0x01] == (2.0 ** -9 if fmt == "e4m3" else 2.0 ** -16)                      # the smallest subnormal
    assert np.nanmax(got[np.isfinite(got)]) == (448.0 if fmt == "e4m3" else 57344.0)
    assert int(np.isinf(got).sum()) == (0 if fmt == "e4m3" else 2)
    # every non-NaN code is exact in bf16 and fp16: rounding and widening give the value back
    for d16 in O.DTYPES:
        assert same_f32(O.widen(O.round16(got[~nan], d16), d16), got[~nan])
    if fmt == "e5m2":                                                                      # code << 8 is the fp16 pattern
        assert same_f32((codes.astype(np.uint16) << 8).view(np.float16).astype(np.float32), got)


# ---- the rule against F.embedding_bag over the widened table -----------------------------------------------------------------------------

CASES = (("sum", False, False), ("sum_pad", False, True), ("weighted", True, False), ("weighted_pad", True, True),
         ("mean", False, False), ("mean_pad", False, True))


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_rule_equals_the_fixture_and_torch_live(fmt, fixture):
    tab, off, psw, pad = fixture[f"table_{fmt}"], fixture[f"offsets_{fmt}"], fixture[f"psw_{fmt}"], int(fixture["pad"])
    W = torch.from_numpy(tab).view(DTYPES[fmt]).to(torch.float32)
    assert same_f32(R.dec(tab, fmt), W.numpy())
    B = off.size
    for name, weighted, padded in CASES:
        idx = fixture[f"indices_weighted_{fmt}" if weighted else f"indices_{fmt}"]
        mean = name.startswith("mean")
        got = R.forward([tab], fmt, idx, off, B, [pad] if padded else None, psw if weighted else None, mean)[0]
        live = F.embedding_bag(torch.from_numpy(idx), W, torch.from_numpy(off), mode="mean" if mean else "sum",
                               per_sample_weights=torch.from_numpy(psw) if weighted else None, padding_idx=pad if padded else None).numpy()
        if name == "weighted_pad":
            # torch's padded weighted CPU path rounds the product and the sum (two roundings per kept lookup), the rule one: after K kept
            # lookups they differ by at most (2K + 2) * 2^-24 * sum |psw * row| per element (tests/test_padding_host.py derives it)
            Wn, keep = W.numpy().astype(np.float64), idx != pad
            end = np.concatenate([off[1:], [idx.size]])
            for b in range(B):
                js = [j for j in range(off[b], end[b]) if keep[j]]
                mag = sum(np.abs(np.float64(psw[j]) * Wn[idx[j]]) for j in js) if js else np.zeros(tab.shape[1])
                for ref in (fixture[f"{name}_{fmt}"], live):
                    assert (np.abs(got[b].astype(np.float64) - ref[b]) <= (2 * len(js) + 2) * 2.0 ** -24 * mag).all(), (fmt, b)
            assert np.array_equal(live.view(np.uint32), fixture[f"{name}_{fmt}"].view(np.uint32))
        else:
            assert same_f32(got, fixture[f"{name}_{fmt}"]), (fmt, name, "fixture")
            assert same_f32(got, live), (fmt, name, "live")
        assert not got[1].any() and not np.signbit(got[1]).any(), "an empty bag is +0.0"
        if padded:
            assert not got[4].any() and not np.signbit(got[4]).any(), "an all-padding bag is +0.0"
    plain = R.forward([tab], fmt, fixture[f"indices_{fmt}"], off, B)[0]
    assert np.isnan(plain[6]).all() and (np.isinf(plain[7]).all() if fmt == "e5m2" else (plain[7] != 0).all())


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_unpooled_rule_equals_torch_embedding(fmt, fixture):
    tab = fixture[f"table_{fmt}"]
    idx = np.arange(tab.shape[0], dtype=np.int64)[::-1].copy()
    rows, written = R.sequence([tab], fmt, idx, np.zeros(1, dtype=np.int64), 1)
    want = F.embedding(torch.from_numpy(idx), torch.from_numpy(tab).view(DTYPES[fmt]).to(torch.float32)).numpy()
    assert written.all() and same_f32(rows, want)
    assert np.array_equal(rows[idx == 16].view(np.uint32)[0, :2], [0x80000000, 0]), "-0.0 leaves as it is stored"
    for d16, tdt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        want16 = torch.from_numpy(want).to(tdt).view(torch.int16).numpy().view(np.uint16)
        assert R.same16(R.sequence16(rows, d16), want16, d16)
    # a batch slice of two tables: only the slice's positions are written
    off = np.array([0, 2, 5, 9, 12, 20], dtype=np.int64)          # T = 2, B = 3 (+ the closing entry)
    idx2 = np.arange(20, dtype=np.int64)
    _, w = R.sequence([tab, tab], fmt, idx2, off, 3, bag_begin=1, bag_count=1)
    assert np.array_equal(np.flatnonzero(w), [2, 3, 4, 12, 13, 14, 15, 16, 17, 18, 19])


# ---- the C calls without a device --------------------------------------------------------------------------------------------------------

def _request(T=2, B=4, N=24, max_dim=32, min_dim=0, weighted=False, wd=_lib.PM_F8E4M3):
    op = _lib.pm_embbag_batch()
    op.num_tables, op.weight_dtype, op.index_dtype, op.max_dim, op.min_dim = T, wd, _lib.PM_I64, max_dim, min_dim
    op.batch, op.num_indices, op.bag_begin, op.bag_count = B, N, 0, B
    op.tables = op.rows = op.dims = op.out_offsets = op.indices = op.offsets = 64      # non-null dummies, never dereferenced on the host
    op.out_stride = max_dim * T
    op.per_sample_weights = 64 if weighted else None
    return op


def test_argument_validation_without_gpu():
    """every refusal is made on the host, before any HIP call (the dummy pointers are never dereferenced)"""
    L = _lib.load()
    OK, INVALID, UNSUPPORTED, F32 = _lib.PM_OK, _lib.PM_ERR_INVALID, _lib.PM_ERR_UNSUPPORTED, _lib.PM_F32
    plan12, plan8 = (ctypes.c_int32 * 12)(), (ctypes.c_int64 * 8)()
    ref = lambda op: None if op is None else ctypes.byref(op)      # noqa: E731

    def pooled(op, odt=F32, out=64, mean=0, pad=None):
        return L.pm_embbag_fwd_f8(ref(op), pad, mean, odt, out, None)

    def pooled_plan(op, odt=F32, **_):
        return L.pm_embbag_f8_plan(ref(op), odt, plan12)

    def gather(op, odt=F32, out=64, stride=None, **_):
        return L.pm_embedding_gather_f8(ref(op), odt, out, (op.max_dim if op is not None else 32) if stride is None else stride, None)

    def gather_plan(op, **_):
        return L.pm_embedding_gather_f8_plan(ref(op), plan8)

    err = L.pm_last_error
    for call in (pooled, pooled_plan, gather, gather_plan):
        assert call(None) == INVALID and b"op is NULL" in err()
        for wd in (_lib.PM_F32, _lib.PM_BF16, _lib.PM_F16, 5, -1, 99, _lib.PM_I32):
            assert call(_request(wd=wd)) == INVALID and b"PM_F8E4M3 or PM_F8E5M2" in err(), wd
        # what pm_embbag_fwd refuses about the request
        for field, val, text in (("num_tables", 0, b"num_tables"), ("index_dtype", 3, b"index_dtype"), ("bag_count", 5, b"bag_begin/bag_count"),
                                 ("offsets", None, b"offsets"), ("indices", None, b"indices"), ("tables", None, b"tables"),
                                 ("fixed_pooling", 5, b"fixed_pooling"), ("out_stride", 62, b"out_stride")):
            op = _request()
            setattr(op, field, val)
            assert call(op) == INVALID or (field == "out_stride" and call(op) == UNSUPPORTED), field
            assert text in err(), field
        assert call(_request(min_dim=6)) == INVALID and b"min_dim" in err()
        # the column rule and the limit
        for d in (4, 8, 12, 24, 40, 100, 2040):
            assert call(_request(max_dim=d)) == UNSUPPORTED and b"multiple of" in err(), d
        assert call(_request(max_dim=32, min_dim=8)) == UNSUPPORTED and b"multiple of 16" in err()
        assert call(_request(max_dim=2064)) == UNSUPPORTED and b"at most 2048" in err()
        for field, val in (("table_group", 2), ("grad_block_shift", 1), ("grad_block_extra", 64)):
            op = _request()
            setattr(op, field, val)
            if field == "grad_block_extra":      # (alone it is what every entry point refuses: a block of one bag)
                assert call(op) == INVALID and b"grad_block_extra" in err()
                op.grad_block_shift = 2
            assert call(op) == UNSUPPORTED and b"blocked layouts" in err(), field
    for plan in (pooled_plan, gather_plan):
        for wd in PM_F8.values():
            assert all(plan(_request(max_dim=d, wd=wd)) == OK for d in range(16, 2049, 16))
    # out_dtype
    for call in (pooled, pooled_plan, gather):
        for odt in (-1, 3, 4, _lib.PM_I32, _lib.PM_I64):
            assert call(_request(), odt=odt) == INVALID and b"out_dtype" in err(), odt
    # weights: the gather, and the mean
    for call in (gather, gather_plan):
        assert call(_request(weighted=True)) == UNSUPPORTED and b"per_sample_weights must be NULL" in err()
    assert pooled(_request(weighted=True), mean=1) == UNSUPPORTED and b"mean pooling is unweighted" in err()
    assert pooled_plan(_request(weighted=True)) == OK
    for mean in (2, -1):
        assert pooled(_request(), mean=mean) == INVALID and b"mean must be 0 or 1" in err()
    # out and out_row_stride
    for stride in (16, 30, 34, -32):
        assert gather(_request(), stride=stride) == INVALID and b"out_row_stride" in err(), stride
    for call in (pooled, gather):
        assert call(_request(), out=None) == INVALID and b"out is NULL" in err()
        assert call(_request(), out=72) == INVALID and b"16-byte aligned" in err()
        for odt in (_lib.PM_BF16, _lib.PM_F16):
            assert call(_request(), odt=odt, out=68) == INVALID and b"8-byte aligned" in err()
    assert L.pm_embbag_f8_plan(ctypes.byref(_request()), F32, None) == INVALID and b"out is NULL" in err()
    assert L.pm_embedding_gather_f8_plan(ctypes.byref(_request()), None) == INVALID and b"out is NULL" in err()
    # an empty request: PM_OK without a launch, whatever `out` is
    empty = _request()
    empty.bag_count = 0
    assert pooled(empty, out=None) == OK and gather(empty, out=None) == OK and pooled(empty, odt=_lib.PM_F16, out=None, mean=1) == OK
    none = _request(N=0)
    none.indices = None
    assert gather(none, out=None) == OK and gather(_request(B=0, N=0), out=None) == OK and pooled(_request(B=0, N=0), out=None) == OK


def test_existing_entry_points_keep_refusing_the_fp8_dtypes():
    L = _lib.load()
    plan12, plan8 = (ctypes.c_int32 * 12)(), (ctypes.c_int64 * 8)()
    for wd in PM_F8.values():
        op = _request(wd=wd)
        for rc in (L.pm_embbag_fwd(ctypes.byref(op), 64, None), L.pm_embbag_fwd_padded(ctypes.byref(op), 64, 64, None),
                   L.pm_embbag_fwd_mean(ctypes.byref(op), None, 64, None), L.pm_embbag_fwd_out16(ctypes.byref(op), None, 0, _lib.PM_BF16, 64, None),
                   L.pm_embedding_gather(ctypes.byref(op), _lib.PM_F32, 64, 32, None), L.pm_embbag_plan(ctypes.byref(op), _lib.PM_PLAN_FORWARD, plan12),
                   L.pm_embedding_gather_plan(ctypes.byref(op), plan8)):
            assert rc == _lib.PM_ERR_INVALID and b"weight/dst dtype must be PM_F32, PM_BF16 or PM_F16" in L.pm_last_error()


def test_symbols_and_struct():
    new = {"pm_embbag_fwd_f8", "pm_embbag_f8_plan", "pm_embedding_gather_f8", "pm_embedding_gather_f8_plan"}
    assert new <= set(_lib.EXPORTED_SYMBOLS) and (_lib.PM_F8E4M3, _lib.PM_F8E5M2) == (3, 4)
    L = _lib.load()
    assert L.pm_abi_version() == 8 and ctypes.sizeof(_lib.pm_embbag_batch) == 144
    alt = _lib.load_alternates()
    assert all(hasattr(alt, s) for s in new)
    header = open(os.path.join(os.path.dirname(HERE), "include", "param_amd.h")).read()
    assert "PM_F8E4M3 = 3" in header and "PM_F8E5M2 = 4" in header and "FP8 TABLES" in header


# ---- the plans -------------------------------------------------------------------------------------------------------------------------------
# name -> (T, B, N, max_dim, weighted, out_dtype, unroll, bags_per_block, stage_out, xcd_affine)
PLAN_REQUESTS = {
    "bench_d128_f32": (16, 8192, 16 * 8192 * 20, 128, False, _lib.PM_F32, 0, 0, -1, -1),
    "bench_d128_f16": (16, 8192, 16 * 8192 * 20, 128, False, _lib.PM_F16, 0, 0, -1, -1),
    "bench_d64": (16, 8192, 16 * 8192 * 20, 64, False, _lib.PM_F32, 0, 0, -1, -1),
    "bench_d512": (16, 8192, 16 * 8192 * 20, 512, False, _lib.PM_F32, 0, 0, -1, -1),
    "d16_small": (1, 7, 31, 16, False, _lib.PM_F32, 0, 0, -1, -1),
    "d256_weighted": (3, 100, 1234, 256, True, _lib.PM_F32, 0, 0, -1, -1),
    "d1024_bf16": (2, 64, 640, 1024, False, _lib.PM_BF16, 0, 0, -1, -1),
    "d2048_two_passes": (2, 64, 640, 2048, False, _lib.PM_F32, 0, 0, -1, -1),
    "unroll_2": (16, 8192, 16 * 8192 * 20, 128, False, _lib.PM_F32, 2, 0, -1, -1),
    "unroll_3": (16, 8192, 16 * 8192 * 20, 128, False, _lib.PM_F32, 3, 0, -1, -1),
    "unroll_6": (16, 8192, 16 * 8192 * 20, 128, False, _lib.PM_F32, 6, 0, -1, -1),
    "unroll_8": (16, 8192, 16 * 8192 * 20, 128, False, _lib.PM_F32, 8, 0, -1, -1),
    "no_burst": (4, 256, 4 * 256 * 8, 128, False, _lib.PM_F32, 0, 0, 0, -1),
    "explicit_tile": (4, 256, 4 * 256 * 8, 128, False, _lib.PM_F32, 0, 64, -1, 0),
    "t300_b1": (300, 1, 300, 64, False, _lib.PM_F32, 1, 0, -1, -1),
}
FIELDS = list(_lib.PLAN_FIELDS) + ["g_" + f for f in _lib.GATHER_PLAN_FIELDS]


def plan_of(name):
    """both plan calls of a listed request under its knobs (dummy pointers; the knobs are put back): the pooled plan's twelve members,
    then the gather plan's eight (of the unweighted request)"""
    T, B, N, max_dim, weighted, odt, unroll, bpb, stage, xcd = PLAN_REQUESTS[name]
    try:
        _lib.set_tuning(unroll=unroll, bags_per_block=bpb, xcd_affine=xcd)
        _lib.set_forward_tuning(stage_out=stage)
        p = _lib.embbag_f8_plan(_request(T, B, N, max_dim, weighted=weighted), odt)
        g = _lib.embedding_gather_f8_plan(_request(T, B, N, max_dim, wd=_lib.PM_F8E5M2))
    finally:
        _lib.set_tuning()
        _lib.set_forward_tuning()
    return [p[f] for f in _lib.PLAN_FIELDS] + [g[f] for f in _lib.GATHER_PLAN_FIELDS]


def test_every_listed_request_plans_its_pinned_row():
    rows = {name: plan_of(name) for name in PLAN_REQUESTS}
    if REWRITE:
        with open(PINNED, "w") as f:
            f.write('{\n "plan_fields": %s,\n "rows": {\n' % json.dumps(FIELDS))
            f.write(",\n".join("  %s: %s" % (json.dumps(name), json.dumps(row)) for name, row in rows.items()))
            f.write("\n }\n}\n")
    pinned = json.load(open(PINNED))
    assert pinned["plan_fields"] == FIELDS and list(pinned["rows"]) == list(PLAN_REQUESTS)
    bad = [(name, pinned["rows"][name], row) for name, row in rows.items() if row != pinned["rows"][name]]
    assert not bad, f"{len(bad)} of {len(rows)} rows differ; the first (request, pinned, planned): {bad[0]}"


def test_the_pinned_rows_are_not_being_rewritten():
    assert not REWRITE, "PARAM_AMD_REWRITE_F8_PLAN=1 rewrote tests/f8_plan_host.json: read its diff, then run without the flag"


def test_what_the_plans_say():
    """properties of the pinned rows from the plans' own rules (launch_plan.h: plan_f8, plan_gather_f8)"""
    rows = {n: dict(zip(FIELDS, r)) for n, r in json.load(open(PINNED))["rows"].items()}
    default = rows["bench_d128_f32"]["unroll"]
    assert default in (2, 4, 8)
    for name, p in rows.items():
        T, B, N, max_dim, weighted, odt, unroll, bpb, stage, xcd = PLAN_REQUESTS[name]
        G = min(64, max(8, 1 << (-(-max_dim // 16) - 1).bit_length()))              # group_lanes(max_dim, 16)
        NG = 256 // G
        assert p["bags_per_block"] >= NG and p["tiles_per_table"] == -(-B // p["bags_per_block"]) and p["idx_cap"] <= 4096
        assert p["unroll"] == (default if unroll == 0 else (8 if unroll >= 8 else 4 if unroll >= 4 else 2))
        ob = 4 if odt == _lib.PM_F32 else 2
        assert p["stage_out"] in (0, max_dim) and (p["stage_out"] == 0 or p["bags_per_block"] * max_dim * ob <= 16384)
        assert p["ordered"] == 0 and p["nt_loads"] == 0 and p["flat_bags"] == 0 and p["stage_bags"] == p["bags_per_block"]
        if bpb:
            assert p["bags_per_block"] == bpb
        if stage == 0:
            assert p["stage_out"] == 0
        Gg = min(64, max(8, 1 << (-(-max_dim // 4) - 1).bit_length()))              # group_lanes(max_dim, 4)
        assert p["g_vec"] == 4 and p["g_group_lanes"] == Gg and p["g_tile"] == 256 and p["g_grid"] == -(-N // 256)
        assert p["g_col_passes"] == -(-max_dim // (Gg * 4))
        assert p["g_unroll"] == (8 if unroll == 0 else max(u for u in (1, 2, 4, 8) if u <= unroll))
        assert p["g_lds_borders"] == (1 if T + 1 <= 256 else 0) and p["g_xcd_contiguous"] == (1 if T > 1 and xcd != 0 else 0)
    assert [rows[n]["g_group_lanes"] for n in ("d16_small", "bench_d64", "bench_d128_f32", "d256_weighted")] == [8, 16, 32, 64]
    assert rows["d2048_two_passes"]["g_col_passes"] == 8 and rows["t300_b1"]["g_lds_borders"] == 0
    assert rows["bench_d128_f32"]["stage_out"] == 128 and rows["bench_d128_f16"]["bags_per_block"] >= rows["bench_d128_f32"]["bags_per_block"]


# ---- the modules without a device --------------------------------------------------------------------------------------------------------

def test_constructors_and_refusals_on_cpu():
    from param_amd import Float8BatchedEmbeddingBagMI355 as FB
    from param_amd import Float8EmbeddingBagMI355 as FE
    from param_amd import Float8EmbeddingMI355 as FS

    m = FB([5, 7], [32, 16], "E5M2", device="cpu", pooling_mode="MEAN", padding_idx=[None, -1], output_dtype="fp16")
    assert m.dtype == torch.float8_e5m2 and m.table(1).shape == (7, 16) and m.table(1).dtype == torch.float8_e5m2
    assert m.padding_idx == [None, 6] and m.pooling_mode == "mean" and m.output_dtype == torch.float16
    assert not list(m.parameters()) and list(m.state_dict()) == ["weights"] and m.weights.dtype == torch.uint8
    assert m.weights.numel() == 512 and not m.weights.any() and "float8_e5m2" in repr(m)
    src = torch.randn(7, 16)
    m.copy_from_(1, src.to(torch.float8_e5m2))
    assert torch.equal(m.table(1).view(torch.uint8), src.to(torch.float8_e5m2).view(torch.uint8))
    m.copy_from_(0, torch.full((5, 32), 0x80, dtype=torch.uint8))
    assert (m.table(0).float() == 0).all() and torch.signbit(m.table(0).float()).all()
    twin = FB([5, 7], [32, 16], torch.float8_e5m2, device="cpu")
    twin.load_state_dict(m.state_dict())
    assert torch.equal(twin.weights, m.weights)
    for bad in (src, src.to(torch.float8_e4m3fn), torch.zeros(7, 32, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="copy_from_"):
            m.copy_from_(1, bad)
    for name, dt in (("e4m3", torch.float8_e4m3fn), ("FP8_E4M3", torch.float8_e4m3fn), ("fp8_e5m2", torch.float8_e5m2)):
        assert FB([4], [16], name, device="cpu").dtype == dt
    # ValueError before anything is allocated (rows that could not be)
    for kw, text in ((dict(dtype=torch.float8_e4m3fnuz), "fnuz"), (dict(dtype=torch.float16), "dtype must be"), (dict(dtype="e3m4"), "dtype must be"),
                     (dict(dims=[24]), "multiple of 16"), (dict(dims=[8]), "multiple of 16"), (dict(dims=[2064]), "2048"),
                     (dict(layout="blocked"), "blocked"), (dict(pooling_mode="max"), "sum or mean"), (dict(pooling_mode="none"), "sum or mean"),
                     (dict(pooling_mode=2), "sum or mean"), (dict(rows=[2**31]), "2\\^31"), (dict(output_dtype="int8"), "output_dtype"),
                     (dict(bounds_check_mode="loud"), "bounds_check_mode"), (dict(padding_idx=2**30), "padding_idx")):
        args = dict(rows=[2**30], dims=[2048], device="cpu")
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            FB(**args)
    with pytest.raises(ValueError, match="one common embedding dim"):
        FB([4, 4], [16, 32], device="cpu", layout="tbd")
    # at call time
    idx, off = torch.zeros(4, dtype=torch.int64), torch.zeros(5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.lookup(idx, off, batch=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.plan(idx, off, batch=2)
    with pytest.raises(TypeError, match="int64 or both int32"):
        m.lookup(idx.float(), off, batch=2)
    with pytest.raises(ValueError, match="unweighted"):
        m.lookup(idx, off, torch.ones(4), batch=2)
    with pytest.raises(ValueError, match="one common embedding dim"):
        m.lookup_sequence(idx, off, batch=2)
    with pytest.raises(ValueError, match="one common embedding dim"):
        m.sequence_plan(idx, off, batch=2)
    # from_float on CPU sources: torch's cast, bit for bit
    for dt in DTYPES.values():
        srcs = [torch.randn(6, 16) * 3, torch.randn(4, 32).to(torch.bfloat16)]
        f = FB.from_float(srcs, dt)
        assert all(torch.equal(f.table(t).view(torch.uint8), s.to(dt).view(torch.uint8)) for t, s in enumerate(srcs)) and f.weights.device.type == "cpu"
    with pytest.raises(TypeError, match="from_float takes"):
        FB.from_float([torch.zeros(4, 16, dtype=torch.int32)])
    # the T = 1 modules
    bag = torch.nn.EmbeddingBag(10, 32, mode="mean", padding_idx=3)
    e = FE.from_float(bag, "e4m3", device="cpu")
    assert (e.num_embeddings, e.embedding_dim, e.mode, e.padding_idx) == (10, 32, "mean", [3])
    assert torch.equal(e.table(0).view(torch.uint8), bag.weight.detach().to(torch.float8_e4m3fn).view(torch.uint8))
    with pytest.raises(ValueError, match="sum or mean"):
        FE(10, 32, mode="max", device="cpu")
    with pytest.raises(ValueError, match="sum or mean"):
        FE.from_float(torch.nn.EmbeddingBag(10, 32, mode="max"), device="cpu")
    with pytest.raises(TypeError, match="EmbeddingBagMI355 or a torch.nn.EmbeddingBag"):
        FE.from_float(torch.nn.Embedding(10, 32))
    with pytest.raises(ValueError, match="weight must be"):
        FE(10, 32, device="cpu", weight=torch.zeros(10, 16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="offsets has to be a 1D"):
        e(idx)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        e(torch.zeros((2, 3), dtype=torch.int64))
    emb = torch.nn.Embedding(10, 32, padding_idx=0)
    s = FS.from_float(emb, torch.float8_e5m2, device="cpu", output_dtype="bf16")
    assert torch.equal(s.table(0).view(torch.uint8), emb.weight.detach().to(torch.float8_e5m2).view(torch.uint8)) and s.padding_idx is None
    with pytest.raises(ValueError, match="max_norm"):
        FS.from_float(torch.nn.Embedding(10, 32, max_norm=1.0))
    with pytest.raises(TypeError, match="EmbeddingMI355 or a torch.nn.Embedding"):
        FS.from_float(bag)
    with pytest.raises(TypeError, match="int32 or int64"):
        s(torch.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s(torch.zeros((2, 0, 3), dtype=torch.int32))


def test_existing_modules_reach_none_of_the_new_calls(monkeypatch):
    """a trap on the four new bindings: constructing the existing modules and driving them as far as a machine without a device lets
    them go touches none of them (they are reached through ``param_amd.float8_bag`` alone)"""
    import param_amd
    from param_amd import embedding_bag, quantized_bag

    L = _lib.load()
    hits = []
    for name in ("pm_embbag_fwd_f8", "pm_embbag_f8_plan", "pm_embedding_gather_f8", "pm_embedding_gather_f8_plan"):
        monkeypatch.setattr(L, name, lambda *a, _n=name: hits.append(_n) or _lib.PM_ERR_INVALID, raising=True)
    for fn in ("embbag_f8_plan", "embedding_gather_f8_plan"):
        monkeypatch.setattr(_lib, fn, lambda *a, _n=fn: hits.append(_n), raising=True)
    for mod in (embedding_bag, quantized_bag):
        src = open(mod.__file__).read()
        assert "_f8" not in src and "float8" not in src, mod.__name__
    idx, off = torch.zeros(4, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    mods = [param_amd.BatchedEmbeddingBagMI355([8], 16, device="cpu", init=None), param_amd.EmbeddingBagMI355(8, 16, device="cpu"),
            param_amd.QuantizedBatchedEmbeddingBagMI355([8], [16], 8, device="cpu"), param_amd.QuantizedEmbeddingBagMI355(8, 16, device="cpu")]
    for m in mods:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(idx, off)
    for m in (param_amd.EmbeddingMI355(8, 16, device="cpu"), param_amd.QuantizedEmbeddingMI355(8, 16, device="cpu")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(idx)
    op = _request(wd=_lib.PM_F32)
    _lib.embbag_plan(op, _lib.PM_PLAN_FORWARD), _lib.embedding_gather_plan(op), _lib.embbag_qrows_plan(op, 8), _lib.embedding_gather_qrows_plan(op, 8)
    assert not hits
    # ... and the trap works: the FP8 module does reach them
    f = param_amd.Float8BatchedEmbeddingBagMI355([8], [16], device="cpu")
    monkeypatch.setattr(param_amd.float8_bag, "_require_device", lambda *a: None)
    monkeypatch.setattr(param_amd.float8_bag, "_stream_ptr", lambda: 0)
    monkeypatch.setattr(quantized_bag, "_require_device", lambda *a: None)
    monkeypatch.setattr(embedding_bag, "_require_device", lambda *a: None)
    with pytest.raises(_lib.ParamAmdError):
        f.lookup(idx, off, batch=2)
    assert hits == ["pm_embbag_fwd_f8"]
