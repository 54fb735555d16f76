"""ROW-QUANTISED TABLES of PER-TABLE FORMAT on the CPU: tests/qmixed_rules.py (the per-table application of tests/qrows_rules.py and
tests/qgather_rules.py) against torch's CPU operators, live, table by table; what the constructor accepts and refuses; the per-table
slab layout; every host-side refusal of the four C calls; their plans pinned in tests/qmixed_plan_host.json; and the compiled kernels'
metadata: no instance of the two new kernels uses scratch memory, and there are as many instances as the launcher ladders name.

``PARAM_AMD_REWRITE_QMIXED_PLAN=1 pytest tests/test_qmixed_host.py`` writes the JSON anew from what the library plans (read the diff: a
changed row is a changed launch geometry)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from param_amd import _lib
from tests import qgather_cases as G
from tests import qmixed_rules as M
from tests import qrows_cases as C
from tests import qrows_rules as R
from tests.test_isa_properties import _kernel_resources, bundles  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
PINNED = os.path.join(HERE, "qmixed_plan_host.json")
REWRITE = os.environ.get("PARAM_AMD_REWRITE_QMIXED_PLAN") == "1"
ODT = {"fp32": _lib.PM_F32, "bf16": _lib.PM_BF16, "fp16": _lib.PM_F16}
FIELDS, GFIELDS = list(_lib.PLAN_FIELDS), list(_lib.GATHER_PLAN_FIELDS)


# ---- the rule against torch ------------------------------------------------------------------------------------------------------------

def three_tables(bits, dim=24):
    """three tables of ``qrows_cases``' rows (seeded per width: the middle one of another width's values), prepacked by torch"""
    xs = [C.float_table(dim), C.float_table(128)[:, :dim].copy(), C.float_table(dim)[::-1].copy()]
    return [C.torch_prepack(x, b) for x, b in zip(xs, bits)]


def three_table_request():
    """qrows_cases' request three times over, table-major: (indices, offsets [3 * B], psw), B = 7"""
    idx, off, psw = C.request()
    n = idx.size
    rng = np.random.default_rng(C.SEED + 1)
    idx3 = np.concatenate([idx, rng.permutation(idx), idx[::-1]])
    return idx3, np.concatenate([off, off + n, off + 2 * n]), np.concatenate([psw, psw[::-1], psw * np.float32(0.5)])


@pytest.mark.parametrize("bits", [(8, 4, 8), (4, 8, 4)], ids=["848", "484"])
def test_rule_equals_torch_operators_table_by_table(bits):
    qt = three_tables(bits)
    idx, off, psw = three_table_request()
    B, n = len(C.LENS), idx.size // 3
    for dt in (np.int32, np.int64):
        for w in (None, psw):
            want = M.forward(qt, [24] * 3, bits, idx.astype(dt), off.astype(dt), B, w)
            for t in range(3):
                live = C.torch_lookup(qt[t], bits[t], idx[t * n:(t + 1) * n].astype(dt), (off[t * B:(t + 1) * B] - t * n).astype(dt),
                                      None if w is None else w[t * n:(t + 1) * n])
                assert want[t].shape == (B, 24) and R.same_f32(live, want[t]), (bits, t, dt, w is not None)
                # ... which is the single-format rule over a request of that table alone
                alone = R.forward([qt[t]], [24], bits[t], idx[t * n:(t + 1) * n], off[t * B:(t + 1) * B] - t * n, B,
                                  None if w is None else w[t * n:(t + 1) * n])[0]
                assert R.same_f32(alone, want[t])
                assert not want[t][[0, 2, 6]].any() and not np.signbit(want[t][[0, 2, 6]]).any()      # empty bags: +0.0
    # a batch slice is the rows of that slice; 16-bit outputs are one rounding of the fp32 result
    whole = M.forward(qt, [24] * 3, bits, idx, off, B, psw)
    part = M.forward(qt, [24] * 3, bits, idx, off, B, psw, bag_begin=2, bag_count=3)
    assert all(R.same_f32(p, w[2:5]) for p, w in zip(part, whole))
    from tests import out16_rules as O
    assert all(np.array_equal(h, O.round16(w, "fp16")) for h, w in zip(M.forward16(qt, [24] * 3, bits, idx, off, B, "fp16", psw), whole))
    # un-pooled: every position's row is torch's lookup of a bag of one in the owner's format
    out, written = M.gather(qt, 24, bits, idx, off, B)
    assert written.all() and out.shape == (idx.size, 24)
    for t in range(3):
        assert R.same_f32(G.torch_rows(qt[t], bits[t], idx[t * n:(t + 1) * n]), out[t * n:(t + 1) * n]), (bits, t)
    _, sl = M.gather(qt, 24, bits, idx, off, B, bag_begin=1, bag_count=3)
    assert sl.sum() == 3 * (5 + 0 + 300) and not sl[n - 3:n].any()


def test_uniform_bits_are_the_single_format_rules():
    for b in (8, 4):
        qt = three_tables((b, b, b))
        idx, off, psw = three_table_request()
        B = len(C.LENS)
        for got, want in zip(M.forward(qt, [24] * 3, (b, b, b), idx, off, B, psw), R.forward(qt, [24] * 3, b, idx, off, B, psw)):
            assert R.same_f32(got, want)
        from tests import qgather_rules as Q
        assert R.same_f32(M.gather(qt, 24, (b, b, b), idx, off, B)[0], Q.gather(qt, 24, b, idx, off, B)[0])


# ---- the module without a device -------------------------------------------------------------------------------------------------------

def test_constructor_accepts_and_refuses_on_cpu():
    from param_amd import QuantizedBatchedEmbeddingBagMI355 as QB

    m = QB([5, 7, 3], [8, 128, 24], [8, 4, 8], device="cpu")
    assert m.bitwidths == [8, 4, 8] and m.bitwidth is None and "bitwidth=[8, 4, 8]" in repr(m)
    # per-table row_bytes (D + 8 | D / 2 + 4) and slab starts padded to 256 B
    assert [tuple(m.table(t).shape) for t in range(3)] == [(5, 16), (7, 68), (3, 32)]
    assert m._starts == [0, 256, 256 + 512] and m.weights.numel() == 256 + 512 + 256 and not m.weights.any()
    assert all(m.table(t).data_ptr() % 4 == 0 and m.table(t).dtype == torch.uint8 for t in range(3))
    assert not list(m.parameters()) and list(m.state_dict()) == ["weights"]
    m2 = QB([5, 7, 3], [8, 128, 24], (4, 8, 4), device="cpu", layout="bd", output_dtype="fp16")
    assert [tuple(m2.table(t).shape) for t in range(3)] == [(5, 8), (7, 136), (3, 16)] and m2.output_dtype == torch.float16
    # state_dict round-trips the bytes, table by table
    m.table(1).copy_(torch.arange(7 * 68, dtype=torch.int64).remainder(251).to(torch.uint8).view(7, 68))
    twin = QB([5, 7, 3], [8, 128, 24], [8, 4, 8], device="cpu")
    twin.load_state_dict(m.state_dict())
    assert torch.equal(twin.table(1), m.table(1)) and torch.equal(twin.weights, m.weights)
    # a sequence whose entries are all equal IS the int: today's module
    for b in (8, 4):
        u, i = QB([5, 7], [8, 128], [b, b], device="cpu"), QB([5, 7], [8, 128], b, device="cpu")
        assert u.bitwidth == i.bitwidth == b and u.bitwidths == i.bitwidths == [b, b] and u._starts == i._starts and repr(u) == repr(i)
    assert QB([5, 7], [4, 20], [8, 8], device="cpu").bitwidth == 8                  # ... with the int's column rule (D % 4)
    assert QB([5], [24], [4], device="cpu").bitwidth == 4 and QB([5, 5], 16, (4, 8), device="cpu", layout="tbd").dims == [16, 16]
    # any sequence of per-table widths, and an array's values
    for seq in ((8, 4), range(8, 0, -4), np.array([8, 4]), torch.tensor([8, 4])):
        assert QB([5, 7], [8, 128], seq, device="cpu").bitwidths == [8, 4]
    assert QB([5, 7], [8, 128], np.array([4, 4]), device="cpu").bitwidth == 4
    # refusals, before anything is allocated (rows that could not be allocated prove it)
    huge = [2**30, 2**30]
    for kw, text in ((dict(bitwidth=[8]), "one entry per table"), (dict(bitwidth=[8, 4, 8]), "one entry per table"), (dict(bitwidth=[]), "one entry per table"),
                     (dict(bitwidth=[8, True]), "bitwidth"), (dict(bitwidth=[True, True]), "bitwidth"), (dict(bitwidth=[8, 2]), "bitwidth"),
                     (dict(bitwidth=[16, 4]), "bitwidth"), (dict(bitwidth=[2, 2]), "bitwidth"), (dict(bitwidth=[8, 4.0]), "bitwidth"),
                     (dict(bitwidth=[8, "4"]), "bitwidth"), (dict(bitwidth="84"), "bitwidth"), (dict(bitwidth=None), "bitwidth"),
                     (dict(bitwidth=[8, 4], dims=[12, 128]), "multiple of 8"), (dict(bitwidth=[4, 8], dims=[128, 12]), "multiple of 8"),
                     (dict(bitwidth=[8, 4], dims=[4, 128]), "multiple of 8"), (dict(bitwidth=[8, 4], dims=[4104, 128]), "4096"),
                     (dict(bitwidth=[8, 4], layout="blocked"), "blocked"), (dict(bitwidth=[8, 4], pooling_mode="mean"), "sum pooling"),
                     (dict(bitwidth=[8, 4], padding_idx=0), "padding_idx"), (dict(bitwidth=[8, 4], dims=[8, 16], layout="tbd"), "common embedding dim")):
        args = dict(dims=[1024, 1024], device="cpu")
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            QB(huge, **args)
    # call time: no CPU fallback; the un-pooled lookup needs one common dim as today
    idx, off = torch.zeros(4, dtype=torch.int64), torch.zeros(7, dtype=torch.int64)
    for call in (m.lookup, m.plan):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(idx, off, batch=2)
    with pytest.raises(ValueError, match="one common embedding dim"):
        m.lookup_sequence(idx, off, batch=2)
    with pytest.raises(ValueError, match="one common embedding dim"):
        m.sequence_plan(idx, off, batch=2)
    s = QB([5, 7], [24, 24], [4, 8], device="cpu", layout="tbd")
    for call in (s.lookup_sequence, s.sequence_plan):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(idx, torch.zeros(5, dtype=torch.int64), batch=2)
    with pytest.raises(TypeError, match="int64 or both int32"):
        m.lookup(idx.float(), off)
    with pytest.raises(TypeError):
        m.quantize_from_(1, torch.zeros(7, 128, dtype=torch.float16))
    with pytest.raises(ValueError):
        m.quantize_from_(1, torch.zeros(7, 64))


def test_from_float_argument_checks():
    from param_amd import QuantizedBatchedEmbeddingBagMI355 as QB

    xs = [torch.zeros(5, 8), torch.zeros(7, 128)]
    with pytest.raises(ValueError, match="one entry per table"):
        QB.from_float(xs, bitwidth=[8, 4, 8], device="cpu")
    with pytest.raises(ValueError, match="bitwidth"):
        QB.from_float(xs, bitwidth=[8, 2], device="cpu")
    with pytest.raises(ValueError, match="multiple of 8"):
        QB.from_float([torch.zeros(5, 12), torch.zeros(7, 128)], bitwidth=[8, 4], device="cpu")
    with pytest.raises(TypeError, match="sequence of 2-D float32"):
        QB.from_float([torch.zeros(5, 8, dtype=torch.float16)], bitwidth=[8])
    with pytest.raises(TypeError, match="sequence of 2-D float32"):
        QB.from_float([], bitwidth=[])
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # accepted; the quantising kernel then needs a device
        QB.from_float(xs, bitwidth=[8, 4], device="cpu")


# ---- the C calls without a device ------------------------------------------------------------------------------------------------------

def _request(T=2, B=4, N=24, max_dim=8, min_dim=0, weighted=False):
    op = _lib.pm_embbag_batch()
    op.num_tables, op.weight_dtype, op.index_dtype, op.max_dim, op.min_dim = T, 99, _lib.PM_I64, max_dim, min_dim      # weight_dtype is not read
    op.batch, op.num_indices, op.bag_begin, op.bag_count = B, N, 0, B
    op.tables = op.rows = op.dims = op.out_offsets = op.indices = op.offsets = 64      # non-null dummies, never dereferenced on the host
    op.out_stride = max_dim * T
    op.per_sample_weights = 64 if weighted else None
    return op


def test_symbols_are_declared_exported_and_bound():
    names = ("pm_embbag_fwd_qrows_mixed", "pm_embbag_qrows_mixed_plan", "pm_embedding_gather_qrows_mixed", "pm_embedding_gather_qrows_mixed_plan")
    header = open(os.path.join(os.path.dirname(HERE), "include", "param_amd.h")).read()
    L, A = _lib.load(), _lib.load_alternates()
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name) and hasattr(A, name) and f"int {name}(" in header, name
    assert L.pm_abi_version() == 8 and ctypes.sizeof(_lib.pm_embbag_batch) == 144
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert L.pm_embbag_fwd_qrows_mixed.argtypes[1:] == [vp, i32, vp, vp]
    assert L.pm_embbag_qrows_mixed_plan.argtypes[1:] == [i32, ctypes.POINTER(i32)]
    assert L.pm_embedding_gather_qrows_mixed.argtypes[1:] == [vp, i32, vp, i64, vp]
    assert L.pm_embedding_gather_qrows_mixed_plan.argtypes[1:] == [ctypes.POINTER(i64)]


def test_argument_validation_without_gpu():
    """every refusal is made on the host, before any HIP call (the dummy pointers are never dereferenced)"""
    L = _lib.load()
    INVALID, UNSUPPORTED, OK, F32 = _lib.PM_ERR_INVALID, _lib.PM_ERR_UNSUPPORTED, _lib.PM_OK, _lib.PM_F32
    plan_out, gplan_out = (ctypes.c_int32 * 12)(), (ctypes.c_int64 * 8)()
    ref = lambda op: None if op is None else ctypes.byref(op)      # noqa: E731

    def fwd(op, odt=F32, out=64, bits=64, **_):
        return L.pm_embbag_fwd_qrows_mixed(ref(op), bits, odt, out, None)

    def plan(op, odt=F32, **_):
        return L.pm_embbag_qrows_mixed_plan(ref(op), odt, plan_out)

    def gather(op, odt=F32, out=64, bits=64, stride=None):
        stride = (op.max_dim if op is not None else 8) if stride is None else stride
        return L.pm_embedding_gather_qrows_mixed(ref(op), bits, odt, out, stride, None)

    def gplan(op, **_):
        return L.pm_embedding_gather_qrows_mixed_plan(ref(op), gplan_out)

    err = L.pm_last_error
    for call in (fwd, plan, gather, gplan):
        assert call(None) == INVALID and b"op is NULL" in err()
        # what pm_embbag_fwd refuses about the request
        for field, val, text in (("num_tables", 0, b"num_tables"), ("index_dtype", 3, b"index_dtype"), ("bag_count", 5, b"bag_begin/bag_count"),
                                 ("offsets", None, b"offsets"), ("indices", None, b"indices"), ("tables", None, b"tables"),
                                 ("fixed_pooling", 5, b"fixed_pooling")):
            op = _request()
            setattr(op, field, val)
            assert call(op) == INVALID and text in err(), field
        op = _request()
        op.out_stride = 18
        assert call(op) == UNSUPPORTED and b"out_stride" in err()
        # the column rule: a multiple of 8 for every table (max_dim and min_dim), at most 4096
        for d in (4, 12, 20, 6, 1020):
            assert call(_request(max_dim=d)) == UNSUPPORTED and b"multiple of 8" in err(), d
        for d in (4, 12, 20):
            assert call(_request(max_dim=128, min_dim=d)) == UNSUPPORTED and b"multiple of 8" in err(), d
        assert call(_request(max_dim=16, min_dim=24)) == INVALID and b"min_dim" in err()
        assert call(_request(max_dim=0)) == UNSUPPORTED and call(_request(max_dim=-8)) == UNSUPPORTED
        assert call(_request(max_dim=4104)) == UNSUPPORTED and b"at most 4096" in err()
        # blocked layouts
        for field, val in (("table_group", 2), ("grad_block_shift", 1), ("grad_block_extra", 64)):
            op = _request()
            setattr(op, field, val)
            if field == "grad_block_extra":      # (alone it is what every entry point refuses: a block of one bag)
                assert call(op) == INVALID and b"grad_block_extra" in err()
                op.grad_block_shift = 2
            assert call(op) == UNSUPPORTED and b"blocked layouts" in err(), field
    # accepted requests are asked of the plan queries only: they launch nothing
    for p in (plan, gplan):
        assert all(p(_request(max_dim=d)) == OK for d in range(8, 1025, 8)) and p(_request(max_dim=4096)) == OK
        assert p(_request(max_dim=128, min_dim=8)) == OK
    # table_bits: NULL (the launching calls; the plan queries take none)
    for call in (fwd, gather):
        assert call(_request(), bits=None) == INVALID and b"table_bits is NULL" in err()
        for odt in (-1, 3, _lib.PM_I32, _lib.PM_I64):
            assert call(_request(), odt=odt) == INVALID and b"out_dtype" in err()
        assert call(_request(), out=None) == INVALID and b"out is NULL" in err()
        assert call(_request(), out=72) == INVALID and b"16-byte aligned" in err()
        assert call(_request(), odt=_lib.PM_BF16, out=68) == INVALID and b"8-byte aligned" in err()
        assert call(_request(), odt=_lib.PM_F16, out=68) == INVALID and b"8-byte aligned" in err()
    for odt in (-1, 3, _lib.PM_I32):
        assert plan(_request(), odt=odt) == INVALID and b"out_dtype" in err()
    assert L.pm_embbag_qrows_mixed_plan(ctypes.byref(_request()), F32, None) == INVALID and b"out is NULL" in err()
    assert L.pm_embedding_gather_qrows_mixed_plan(ctypes.byref(_request()), None) == INVALID and b"out is NULL" in err()
    # un-pooled: weights, the row stride
    for call in (gather, gplan):
        assert call(_request(weighted=True)) == UNSUPPORTED and b"per_sample_weights must be NULL" in err()
    for stride in (4, 7, 10, -8):
        assert gather(_request(), stride=stride) == INVALID and b"out_row_stride" in err(), stride
    assert plan(_request(weighted=True)) == OK
    # nothing to do: PM_OK without a launch, whatever `out` is
    empty = _request()
    empty.bag_count = 0
    for call in (fwd, gather):
        assert call(empty, out=None) == OK and call(empty, odt=_lib.PM_F16, out=None) == OK and call(_request(B=0, N=0), out=None) == OK
    none = _request(N=0)
    none.indices = None
    assert gather(none, out=None) == OK


# ---- the plans ---------------------------------------------------------------------------------------------------------------------------
# name: (T, B, N, max_dim, min_dim, weighted, slice, out dtype, (unroll, bags_per_block), stage_out)
BENCH = (16, 8192, 16 * 8192 * 20, 128)
PLAN_REQUESTS = {
    "bench_shape": BENCH + (0, False, None, "fp32", (0, 0), -1),
    "serving_shape": (64, 256, 64 * 256 * 10, 64, 0, False, None, "fp32", (0, 0), -1),
    "d8": (3, 5, 43, 8, 0, False, None, "fp32", (0, 0), -1),
    "d1024": (2, 6, 80, 1024, 0, False, None, "fp32", (0, 0), -1),
    "d1024_bf16": (2, 6, 80, 1024, 0, False, None, "bf16", (0, 0), -1),
    "d4096": (1, 3, 273, 4096, 0, False, None, "fp32", (0, 0), -1),
    "mixed_dims": (3, 5, 43, 128, 8, False, None, "fp32", (0, 0), -1),
    "weighted": BENCH + (0, True, None, "fp32", (0, 0), -1),
    "batch_slice": (2, 10, 100, 128, 0, False, (3, 4), "fp32", (0, 0), -1),
    "tile_longer_than_index_tile": (2, 4, 12000, 128, 0, False, None, "fp32", (0, 0), -1),
    "out_fp16": BENCH + (0, False, None, "fp16", (0, 0), -1),
    "forced_tile_no_burst": (3, 5, 43, 128, 0, False, None, "fp32", (2, 64), -1),
    "no_stage_unroll8": (3, 5, 43, 128, 0, False, None, "fp32", (8, 0), 0),
    "tables_300": (300, 1, 900, 24, 0, False, None, "fp32", (0, 0), -1),
    "tables_1100": (1100, 2, 6600, 8, 0, False, None, "fp32", (0, 0), -1),
}


def plans_of(name):
    """``[pm_embbag_qrows_mixed_plan, pm_embedding_gather_qrows_mixed_plan]`` of a listed request under its knobs (dummy pointers; the
    knobs are put back); the second is None for a weighted request, which the un-pooled calls refuse"""
    T, B, N, max_dim, min_dim, weighted, sl, odt, (unroll, bpb), stage = PLAN_REQUESTS[name]
    op = _request(T, B, N, max_dim, min_dim, weighted)
    if sl is not None:
        op.bag_begin, op.bag_count = sl
    try:
        _lib.set_tuning(unroll=unroll, bags_per_block=bpb)
        _lib.set_forward_tuning(stage_out=stage)
        p = _lib.embbag_qrows_mixed_plan(op, ODT[odt])
        g = None if weighted else _lib.embedding_gather_qrows_mixed_plan(op)
    finally:
        _lib.set_tuning()
        _lib.set_forward_tuning()
    return [[p[f] for f in FIELDS], None if g is None else [g[f] for f in GFIELDS]]


def test_every_listed_request_plans_its_pinned_rows():
    rows = {name: plans_of(name) for name in PLAN_REQUESTS}
    if REWRITE:
        with open(PINNED, "w") as f:
            f.write('{\n "plan_fields": %s,\n "gather_plan_fields": %s,\n "rows": {\n' % (json.dumps(FIELDS), json.dumps(GFIELDS)))
            f.write(",\n".join("  %s: %s" % (json.dumps(name), json.dumps(row)) for name, row in rows.items()))
            f.write("\n }\n}\n")
    pinned = json.load(open(PINNED))
    assert pinned["plan_fields"] == FIELDS and pinned["gather_plan_fields"] == GFIELDS and list(pinned["rows"]) == list(PLAN_REQUESTS)
    bad = [(name, pinned["rows"][name], row) for name, row in rows.items() if row != pinned["rows"][name]]
    assert not bad, f"{len(bad)} of {len(rows)} rows differ; the first (request, pinned, planned): {bad[0]}"


def test_the_pinned_rows_are_not_being_rewritten():
    assert not REWRITE, "PARAM_AMD_REWRITE_QMIXED_PLAN=1 rewrote tests/qmixed_plan_host.json: read its diff, then run without the flag"


def test_what_the_plans_say():
    """properties of the pinned rows from the plans' own rules (launch_plan.h: plan_qmixed, plan_gather_qmixed): eight columns per lane
    for both formats -- the 8-bit single-format plans, whatever formats the tables have"""
    pinned = json.load(open(PINNED))["rows"]
    for name, (prow, grow) in pinned.items():
        T, B, N, max_dim, min_dim, weighted, sl, odt, (unroll, bpb), stage = PLAN_REQUESTS[name]
        p = dict(zip(FIELDS, prow))
        e = 4 if odt == "fp32" else 2
        count = B if sl is None else sl[1]
        lanes = min(64, max(8, 1 << (-(-max_dim // 8) - 1).bit_length()))
        assert p["tiles_per_table"] == -(-count // p["bags_per_block"]) and p["stage_bags"] == p["bags_per_block"]
        assert p["bags_per_block"] % (256 // lanes) == 0
        assert p["ordered"] == p["nt_loads"] == p["flat_bags"] == p["flat_target"] == p["flat_compact"] == 0
        assert p["unroll"] == (2 if 0 < unroll < 4 else 4)
        assert p["stage_out"] in (0, max_dim) and (p["stage_out"] == 0 or p["bags_per_block"] * max_dim * e <= 16384) and (stage != 0 or p["stage_out"] == 0)
        assert 512 <= p["idx_cap"] <= 4096 and p["idx_cap"] % 256 == 0
        if bpb:
            assert p["bags_per_block"] == bpb
        # the plan of the 8-bit single-format call for the same request: the same lane of eight columns
        op = _request(T, B, N, max_dim, min_dim, weighted)
        if sl is not None:
            op.bag_begin, op.bag_count = sl
        try:
            _lib.set_tuning(unroll=unroll, bags_per_block=bpb)
            _lib.set_forward_tuning(stage_out=stage)
            assert [_lib.embbag_qrows_plan(op, 8, ODT[odt])[f] for f in FIELDS] == prow, name
            if grow is not None:
                assert [_lib.embedding_gather_qrows_plan(op, 8)[f] for f in GFIELDS] == grow, name
        finally:
            _lib.set_tuning()
            _lib.set_forward_tuning()
        assert (grow is None) == weighted
        if grow is not None:
            g = dict(zip(GFIELDS, grow))
            assert g["vec"] == 8 and g["tile"] == 256 and g["grid"] == -(-N // 256) and g["group_lanes"] == lanes
            assert g["col_passes"] == -(-max_dim // (lanes * 8)) and g["unroll"] == (8 if unroll in (0, 8) else 2) and lanes % g["unroll"] == 0
            assert g["lds_borders"] == (1 if T + 1 <= 256 else 0) and g["xcd_contiguous"] == (1 if T > 1 else 0)
    rows = {n: dict(zip(FIELDS, r[0])) for n, r in pinned.items()}
    assert rows["bench_shape"]["bags_per_block"] == 32 and rows["bench_shape"]["stage_out"] == 128 and rows["bench_shape"]["idx_cap"] == 1280
    assert rows["out_fp16"]["bags_per_block"] == 64 and rows["weighted"]["bags_per_block"] == 32
    assert rows["tile_longer_than_index_tile"]["tiles_per_table"] == 1 and rows["tile_longer_than_index_tile"]["idx_cap"] < 6000
    assert rows["d1024"]["stage_out"] == 1024 and rows["d1024"]["bags_per_block"] == 4
    assert rows["forced_tile_no_burst"]["stage_out"] == 0 and rows["forced_tile_no_burst"]["unroll"] == 2
    assert rows["batch_slice"]["tiles_per_table"] == 1
    gath = {n: dict(zip(GFIELDS, r[1])) for n, r in pinned.items() if r[1] is not None}
    assert gath["d1024"]["col_passes"] == 2 and gath["d4096"]["col_passes"] == 8 and gath["bench_shape"]["group_lanes"] == 16
    assert gath["tables_300"]["lds_borders"] == 0 and gath["tables_1100"]["lds_borders"] == 0 and gath["d8"]["lds_borders"] == 1


# ---- the compiled kernels --------------------------------------------------------------------------------------------------------------

def test_no_instance_of_the_new_kernels_uses_scratch(bundles):  # noqa: F811
    """code-object metadata (llvm-readelf --notes; no GPU): the launcher ladders name 4 lane-group widths x weighted or not x 3 output
    types x 2 depths of the pooled kernel and 3 output types x 4 widths x 4 depths of the un-pooled one; none has a private segment;
    the un-pooled kernel's LDS is its four arrays; every instance keeps two waves per SIMD at least"""
    res = _kernel_resources(bundles)
    pooled = {n: v for n, v in res.items() if "17qmixed_fwd_kernel" in n}
    gather = {n: v for n, v in res.items() if "20qmixed_gather_kernel" in n}
    assert len(pooled) == 4 * 2 * 3 * 2 and len(gather) == 3 * 4 * 4, (len(pooled), len(gather))
    for name, (vgpr, _sgpr, scratch, lds) in pooled.items():
        assert scratch == 0 and lds == 0 and vgpr <= 128, (name, vgpr, scratch, lds)          # (the tile's LDS is dynamic)
    for name, (vgpr, _sgpr, scratch, lds) in gather.items():
        assert scratch == 0 and lds == 256 * 8 + 256 * 4 + 256 * 8 + 256 * 4 and vgpr <= 256, (name, vgpr, scratch, lds)
    # the existing kernels keep their names and counts (tests/test_isa_qgather.py counts this one)
    assert len([n for n in res if "29embedding_gather_qrows_kernel" in n]) == 2 * 3 * 4 * 4
    assert len([n for n in res if "16qrows_fwd_kernel" in n]) == 2 * 4 * 2 * 3 * 2
