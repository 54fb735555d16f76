"""MIXED-FORMAT TABLES on the CPU: tests/anyfmt_rules.py (the existing restatements applied table by table) against torch's CPU
operators on one request that holds all seven formats; what the constructor accepts and refuses; the slab layout and the ``state_dict``
round trip; every host-side refusal of the four C calls; their plans pinned in tests/anyfmt_plan_host.json and identical for any
permutation of the formats; and the compiled kernels' metadata: no instance of the new kernels uses scratch memory.

``PARAM_AMD_REWRITE_ANYFMT_PLAN=1 pytest tests/test_anyfmt_host.py`` writes the JSON anew from what the library plans (read the diff: a
changed row is a changed launch geometry)."""
import ctypes
import enum
import json
import os

import numpy as np
import pytest
import torch

from param_amd import _lib
from tests import anyfmt_cases as AC
from tests import anyfmt_rules as A
from tests import embedding_rules as E
from tests import qgather_cases as G
from tests import qrows_cases as C
from tests import qrows_rules as R
from tests.test_isa_properties import _kernel_resources, bundles  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
PINNED = os.path.join(HERE, "anyfmt_plan_host.json")
REWRITE = os.environ.get("PARAM_AMD_REWRITE_ANYFMT_PLAN") == "1"
ODT = {"fp32": _lib.PM_F32, "bf16": _lib.PM_BF16, "fp16": _lib.PM_F16}
FIELDS, GFIELDS = list(_lib.PLAN_FIELDS), list(_lib.GATHER_PLAN_FIELDS)
TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16, "fp8_e4m3": torch.float8_e4m3fn, "fp8_e5m2": torch.float8_e5m2}


# ---- the rule against torch ------------------------------------------------------------------------------------------------------------

def torch_fp32_table(tab):
    """the fp32 table torch's CPU casts give for a float or FP8 table's bytes (times 2^E_t)"""
    w = torch.from_numpy(tab.data.copy()).view(TORCH_DT[tab.fmt]).reshape(-1, tab.dim).to(torch.float32)
    return w * (2.0 ** tab.exp) if tab.exp else w


def test_rule_equals_torch_operators_table_by_table():
    rows, B, D = AC.rows_for(7, 1, 20, 40), 5, 16
    exps = [0, 0, 0, -3, 5, 0, 0]
    tabs = AC.tables(AC.SEVEN, rows, [D] * 7, 2, exps)
    idx, off, psw = AC.request(3, rows, B)
    assert tabs[3].exp == -3 and tabs[4].exp == 5 and off.size == 7 * B + 1
    for dt in (np.int32, np.int64):
        for w in (None, psw):
            want = A.forward(tabs, idx.astype(dt), off.astype(dt), B, w)
            for t, tab in enumerate(tabs):
                lo, hi = int(off[t * B]), int(off[(t + 1) * B])
                i_t, o_t = idx[lo:hi], off[t * B:(t + 1) * B] - lo
                w_t = None if w is None else w[lo:hi]
                if tab.fmt in ("int8", "int4"):
                    live = C.torch_lookup(tab.data, 8 if tab.fmt == "int8" else 4, i_t, o_t, w_t)
                else:
                    live = torch.nn.functional.embedding_bag(torch.from_numpy(i_t), torch_fp32_table(tab), torch.from_numpy(o_t), mode="sum",
                                                             per_sample_weights=None if w_t is None else torch.from_numpy(w_t)).numpy()
                assert want[t].shape == (B, D) and R.same_f32(live, want[t]), (tab.fmt, dt, w is not None)
    # a batch slice is the rows of that slice; a 16-bit output is one rounding of the fp32 result
    whole = A.forward(tabs, idx, off, B, psw)
    part = A.forward(tabs, idx, off, B, psw, bag_begin=1, bag_count=3)
    assert all(R.same_f32(p, w[1:4]) for p, w in zip(part, whole))
    for kind, tdt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        for got, w in zip(A.forward_bits(tabs, idx, off, B, kind, psw), whole):
            assert np.array_equal(got, torch.from_numpy(w).to(tdt).view(torch.int16).numpy().view(np.uint16))
    # un-pooled: every position's row is torch's lookup in the owner's format; a float table to its own type is its bits
    for kind, tdt in (("f32", torch.float32), ("bf16", torch.bfloat16), ("f16", torch.float16)):
        out, written, copied = A.sequence(tabs, idx, off, B, kind)
        assert written.all() and out.shape == (idx.size, D)
        for t, tab in enumerate(tabs):
            lo, hi = int(off[t * B]), int(off[(t + 1) * B])
            if tab.fmt in ("int8", "int4"):
                live32 = torch.from_numpy(G.torch_rows(tab.data, 8 if tab.fmt == "int8" else 4, idx[lo:hi]))
            else:
                live32 = torch.nn.functional.embedding(torch.from_numpy(idx[lo:hi]), torch_fp32_table(tab))
            live = live32.to(tdt).contiguous().view(torch.int32 if kind == "f32" else torch.int16).numpy().view(E.BITS[kind])
            assert A.same(out[lo:hi], live, kind), (tab.fmt, kind)
            assert copied[lo:hi].all() == (A._KIND.get(tab.fmt) == kind) and copied[lo:hi].any() == (A._KIND.get(tab.fmt) == kind)
            if copied[lo:hi].all():
                assert np.array_equal(out[lo:hi], A.float_bits(tab)[idx[lo:hi]])
    _, sl, _ = A.sequence(tabs, idx, off, B, "f32", bag_begin=1, bag_count=3)
    assert sl.sum() == sum(int(off[t * B + 4] - off[t * B + 1]) for t in range(7))


# ---- the module without a device -------------------------------------------------------------------------------------------------------

class SparseType(enum.Enum):      # fbgemm's, by shape
    FP32 = "fp32"
    FP16 = "fp16"
    FP8 = "fp8"
    INT8 = "int8"
    INT4 = "int4"
    INT2 = "int2"
    BF16 = "bf16"


def test_constructor_accepts_and_refuses_on_cpu():
    from param_amd import MixedBatchedEmbeddingBagMI355 as MB
    from param_amd.mixed_bag import table_format

    m = MB([5, 7, 3, 4, 6, 9, 2], [8, 128, 24, 16, 32, 8, 64], AC.SEVEN, device="cpu")
    assert m.formats == AC.SEVEN and m.format_codes == [0, 1, 2, 3, 4, 5, 6] == [A.CODES[f] for f in AC.SEVEN]
    # typed views: float dtypes and float8 as [rows, D], quantised rows as uint8 [rows, row_bytes]
    assert [(tuple(m.table(t).shape), m.table(t).dtype) for t in range(7)] == [
        ((5, 8), torch.float32), ((7, 128), torch.bfloat16), ((3, 24), torch.float16), ((4, 16), torch.float8_e4m3fn),
        ((6, 32), torch.float8_e5m2), ((9, 16), torch.uint8), ((2, 36), torch.uint8)]
    # the slab: table starts padded to 256 B, zero-filled; two buffers, no parameters
    assert m._starts == [0, 256, 256 + 1792, 2048 + 256, 2304 + 256, 2560 + 256, 2816 + 256] and m.weights.numel() == 3072 + 256
    assert not m.weights.any() and m.weights.dtype == torch.uint8 and m.table_exponents.dtype == torch.int32 and not m.table_exponents.any()
    assert not list(m.parameters()) and list(m.state_dict()) == ["weights", "table_exponents"]
    assert all(m.table(t).data_ptr() % 16 == 0 for t in range(7))
    # every spelling of a format
    assert [table_format(s) for s in ("FP32", "Bf16", "fp16", "FP8_E4M3", "fp8_e5m2", "INT8", "int4")] == AC.SEVEN
    assert [table_format(s) for s in (torch.float32, torch.bfloat16, torch.float16, torch.float8_e4m3fn, torch.float8_e5m2, torch.int8)] == AC.SEVEN[:6]
    assert [table_format(s) for s in (SparseType.FP32, SparseType.BF16, SparseType.FP16, SparseType.FP8, SparseType.INT8, SparseType.INT4)] == \
        ["fp32", "bf16", "fp16", "fp8_e4m3", "int8", "int4"]
    assert MB([5, 5], 16, [SparseType.FP8, torch.float16], device="cpu", layout="tbd", output_dtype="bf16").formats == ["fp8_e4m3", "fp16"]
    # state_dict round-trips the bytes and the exponents
    m.copy_from_(3, torch.arange(64, dtype=torch.uint8).view(4, 16), exponent=-7)
    m.copy_from_(0, torch.arange(40, dtype=torch.float32).view(5, 8))
    m.copy_from_(5, torch.arange(9 * 16, dtype=torch.int64).remainder(251).to(torch.uint8).view(9, 16))
    m.quantize_from_(1, torch.full((7, 128), 1.5))                       # a float format: a cast, no device needed
    assert m.table_exponents.tolist() == [0, 0, 0, -7, 0, 0, 0] and m.table(0)[4, 7] == 39.0 and (m.table(1) == 1.5).all()
    assert torch.equal(m.dequantized_table(3), m.table(3).float() * 2.0 ** -7) and torch.equal(m.dequantized_table(1), torch.full((7, 128), 1.5))
    twin = MB([5, 7, 3, 4, 6, 9, 2], [8, 128, 24, 16, 32, 8, 64], AC.SEVEN, device="cpu")
    twin.load_state_dict(m.state_dict())
    assert torch.equal(twin.weights, m.weights) and torch.equal(twin.table_exponents, m.table_exponents)
    assert all(torch.equal(twin.table(t).view(torch.uint8), m.table(t).view(torch.uint8)) for t in range(7))
    # copy_from_ checks its arguments: the exponent is an FP8 table's, in [-64, 64]
    for t, e in ((3, 65), (3, -65), (3, 1.0), (3, True), (0, 1), (5, -1)):
        with pytest.raises(ValueError, match="exponent"):
            m.copy_from_(t, m.table(t).clone(), exponent=e)
    m.copy_from_(4, m.table(4).clone(), exponent=64)
    assert m.table_exponents[4] == 64
    with pytest.raises(ValueError, match="copy_from_"):
        m.copy_from_(0, torch.zeros(5, 8, dtype=torch.float16))
    with pytest.raises(ValueError, match="copy_from_"):
        m.copy_from_(5, torch.zeros(9, 8, dtype=torch.uint8))
    # refusals, before anything is allocated (rows that could not be allocated prove it)
    huge = [2**30, 2**30]
    for kw, text in ((dict(formats=["fp32"]), "one entry per table"), (dict(formats=["fp32"] * 3), "one entry per table"), (dict(formats=[]), "one entry per table"),
                     (dict(formats="fp32"), "sequence of one format"), (dict(formats=["fp32", "int2"]), "table format"),
                     (dict(formats=["fp32", SparseType.INT2]), "table format"), (dict(formats=["fp32", torch.float8_e4m3fnuz]), "table format"),
                     (dict(formats=["fp32", 8]), "table format"), (dict(formats=["fp32", None]), "table format"),
                     (dict(formats=["fp32", "int8"], dims=[12, 128]), "multiple of 8"), (dict(formats=["int4", "int8"], dims=[128, 4]), "multiple of 8"),
                     (dict(formats=["bf16", "fp16"], dims=[128, 20]), "multiple of 8"), (dict(formats=["fp32", "fp8_e4m3"], dims=[8, 24]), "multiple of 16"),
                     (dict(formats=["fp8_e5m2", "int4"], dims=[8, 8]), "multiple of 16"), (dict(formats=["fp32", "int4"], dims=[2056, 8]), "2048"),
                     (dict(formats=["fp32", "int8"], dims=[8, 4096]), "2048"), (dict(formats=["fp32", "int8"], layout="blocked"), "blocked"),
                     (dict(formats=["fp32", "int8"], layout="dbt"), "layout"), (dict(formats=["fp32", "int8"], dims=[8, 16], layout="tbd"), "common embedding dim"),
                     (dict(formats=["fp32", "int8"], output_dtype="int8"), "output_dtype")):
        args = dict(dims=[1024, 1024], device="cpu")
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            MB(huge, **args)
    with pytest.raises(ValueError, match="rows < 2\\^31"):
        MB([5, 2**31], [8, 8], ["fp32", "int4"], device="cpu")
    # call time: no CPU fallback; the un-pooled lookup needs one common dim
    idx, off = torch.zeros(4, dtype=torch.int64), torch.zeros(14, dtype=torch.int64)
    for call in (m.lookup, m.plan, m.forward):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(idx, off, batch=2)
    with pytest.raises(ValueError, match="one common embedding dim"):
        m.lookup_sequence(idx, off, batch=2)
    with pytest.raises(ValueError, match="one common embedding dim"):
        m.sequence_plan(idx, off, batch=2)
    s = MB([5, 7], [16, 16], ["int4", "fp8_e4m3"], device="cpu", layout="tbd")
    for call in (s.lookup_sequence, s.sequence_plan):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(idx, torch.zeros(5, dtype=torch.int64), batch=2)
    with pytest.raises(TypeError, match="int64 or both int32"):
        m.lookup(idx.float(), off)
    with pytest.raises(TypeError):
        m.quantize_from_(5, torch.zeros(9, 8, dtype=torch.float16))
    with pytest.raises(ValueError):
        m.quantize_from_(5, torch.zeros(9, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # accepted; the quantising kernels then need a device
        m.quantize_from_(3, torch.zeros(4, 16))


def test_from_modules_argument_checks():
    from param_amd import Float8BatchedEmbeddingBagMI355 as F8B
    from param_amd import MixedBatchedEmbeddingBagMI355 as MB
    from param_amd import QuantizedBatchedEmbeddingBagMI355 as QB

    q = QB([5, 7], [8, 16], [8, 4], device="cpu")
    f = F8B([4], [16], "e5m2", device="cpu", scale="table")
    q.table(1).copy_(torch.arange(7 * 12, dtype=torch.uint8).view(7, 12))
    f.copy_from_(0, torch.arange(64, dtype=torch.uint8).view(4, 16), exponents=-9)
    m = MB.from_modules([q, f])
    assert m.formats == ["int8", "int4", "fp8_e5m2"] and m.rows == [5, 7, 4] and m.dims == [8, 16, 16] and m.layout == "bd"
    assert torch.equal(m.table(1), q.table(1)) and torch.equal(m.table(2).view(torch.uint8), f.table(0).view(torch.uint8))
    assert m.table_exponents.tolist() == [0, 0, -9]
    with pytest.raises(ValueError, match="at least one"):
        MB.from_modules([])
    with pytest.raises(TypeError, match="from_modules takes"):
        MB.from_modules([torch.nn.EmbeddingBag(4, 8)])
    for bad in (F8B([4], [16], "e4m3", device="cpu", scale="row"), F8B([4], [16], "e4m3", device="cpu", pooling_mode="mean"),
                F8B([4], [16], "e4m3", device="cpu", padding_idx=0)):
        with pytest.raises(ValueError, match="from_modules takes a Float8"):
            MB.from_modules([bad])
    with pytest.raises(ValueError, match="pruned"):
        MB.from_modules([QB([5], [8], 8, device="cpu", index_remapping=[torch.tensor([0, -1, 1], dtype=torch.int32)])])


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
    names = ("pm_embbag_fwd_anyfmt", "pm_embbag_anyfmt_plan", "pm_embedding_gather_anyfmt", "pm_embedding_gather_anyfmt_plan")
    header = open(os.path.join(os.path.dirname(HERE), "include", "param_amd.h")).read()
    L, Alt = _lib.load(), _lib.load_alternates()
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name) and hasattr(Alt, name) and f"int {name}(" in header, name
    assert "MIXED-FORMAT TABLES" in header and "PM_Q8 = 5" in header and "PM_Q4 = 6" in header and (_lib.PM_Q8, _lib.PM_Q4) == (5, 6)
    assert L.pm_abi_version() == 8 and ctypes.sizeof(_lib.pm_embbag_batch) == 144
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert L.pm_embbag_fwd_anyfmt.argtypes[1:] == [vp, vp, i32, vp, vp]
    assert L.pm_embbag_anyfmt_plan.argtypes[1:] == [i32, ctypes.POINTER(i32)]
    assert L.pm_embedding_gather_anyfmt.argtypes[1:] == [vp, vp, i32, vp, i64, vp]
    assert L.pm_embedding_gather_anyfmt_plan.argtypes[1:] == [ctypes.POINTER(i64)]


def test_argument_validation_without_gpu():
    """every refusal is made on the host, before any HIP call (the dummy pointers are never dereferenced)"""
    L = _lib.load()
    INVALID, UNSUPPORTED, OK, F32 = _lib.PM_ERR_INVALID, _lib.PM_ERR_UNSUPPORTED, _lib.PM_OK, _lib.PM_F32
    plan_out, gplan_out = (ctypes.c_int32 * 12)(), (ctypes.c_int64 * 8)()
    ref = lambda op: None if op is None else ctypes.byref(op)      # noqa: E731

    def fwd(op, odt=F32, out=64, fmts=64, exps=None, **_):
        return L.pm_embbag_fwd_anyfmt(ref(op), fmts, exps, odt, out, None)

    def plan(op, odt=F32, **_):
        return L.pm_embbag_anyfmt_plan(ref(op), odt, plan_out)

    def gather(op, odt=F32, out=64, fmts=64, exps=None, stride=None):
        stride = (op.max_dim if op is not None else 8) if stride is None else stride
        return L.pm_embedding_gather_anyfmt(ref(op), fmts, exps, odt, out, stride, None)

    def gplan(op, **_):
        return L.pm_embedding_gather_anyfmt_plan(ref(op), gplan_out)

    err = L.pm_last_error
    for call in (fwd, plan, gather, gplan):
        assert call(None) == INVALID and b"op is NULL" in err()
        # everything the per-table-format calls refuse about the request
        for field, val, text in (("num_tables", 0, b"num_tables"), ("index_dtype", 3, b"index_dtype"), ("bag_count", 5, b"bag_begin/bag_count"),
                                 ("offsets", None, b"offsets"), ("indices", None, b"indices"), ("tables", None, b"tables"),
                                 ("fixed_pooling", 5, b"fixed_pooling")):
            op = _request()
            setattr(op, field, val)
            assert call(op) == INVALID and text in err(), field
        op = _request()
        op.out_stride = 18
        assert call(op) == UNSUPPORTED and b"out_stride" in err()
        # the column rule: a multiple of 8 for every table (max_dim and min_dim), at most 2048
        for d in (4, 12, 20, 6, 1020):
            assert call(_request(max_dim=d)) == UNSUPPORTED and b"multiple of 8" in err(), d
        for d in (4, 12, 20):
            assert call(_request(max_dim=128, min_dim=d)) == UNSUPPORTED and b"multiple of 8" in err(), d
        assert call(_request(max_dim=16, min_dim=24)) == INVALID and b"min_dim" in err()
        assert call(_request(max_dim=0)) == UNSUPPORTED and call(_request(max_dim=-8)) == UNSUPPORTED
        for d in (2056, 4096, 4104):
            assert call(_request(max_dim=d)) == UNSUPPORTED and (b"at most 2048" in err() or b"at most 4096" in err()), d
        assert call(_request(max_dim=2056)) == UNSUPPORTED and b"at most 2048" in err()
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
        assert all(p(_request(max_dim=d)) == OK for d in range(8, 2049, 8))
        assert p(_request(max_dim=128, min_dim=8)) == OK
    # table_formats: NULL (the launching calls; the plan queries take none); table_exp may be NULL
    for call in (fwd, gather):
        assert call(_request(), fmts=None) == INVALID and b"table_formats is NULL" in err()
        assert call(_request(), fmts=None, exps=64) == INVALID and b"table_formats is NULL" in err()
        for odt in (-1, 3, 5, 6, _lib.PM_I32, _lib.PM_I64):
            assert call(_request(), odt=odt) == INVALID and b"out_dtype" in err()
        assert call(_request(), out=None) == INVALID and b"out is NULL" in err()
        assert call(_request(), out=72) == INVALID and b"16-byte aligned" in err()
        assert call(_request(), odt=_lib.PM_BF16, out=68) == INVALID and b"8-byte aligned" in err()
        assert call(_request(), odt=_lib.PM_F16, out=68) == INVALID and b"8-byte aligned" in err()
    for odt in (-1, 3, _lib.PM_I32):
        assert plan(_request(), odt=odt) == INVALID and b"out_dtype" in err()
    assert L.pm_embbag_anyfmt_plan(ctypes.byref(_request()), F32, None) == INVALID and b"out is NULL" in err()
    assert L.pm_embedding_gather_anyfmt_plan(ctypes.byref(_request()), None) == INVALID and b"out is NULL" in err()
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
    "seven_d64_b5": (7, 5, 150, 64, 0, False, None, "fp32", (0, 0), -1),
    "seven_d64_b70": (7, 70, 2200, 64, 0, False, None, "fp32", (0, 0), -1),
    "d8": (3, 5, 43, 8, 0, False, None, "fp32", (0, 0), -1),
    "d1024": (2, 6, 80, 1024, 16, False, None, "fp32", (0, 0), -1),
    "d1024_bf16": (2, 6, 80, 1024, 0, False, None, "bf16", (0, 0), -1),
    "d2048": (1, 3, 273, 2048, 0, False, None, "fp32", (0, 0), -1),
    "mixed_dims": (7, 5, 143, 256, 8, False, None, "fp32", (0, 0), -1),
    "weighted": BENCH + (0, True, None, "fp32", (0, 0), -1),
    "batch_slice": (2, 10, 100, 128, 0, False, (3, 4), "fp32", (0, 0), -1),
    "tile_longer_than_index_tile": (2, 4, 12000, 128, 0, False, None, "fp32", (0, 0), -1),
    "out_fp16": BENCH + (0, False, None, "fp16", (0, 0), -1),
    "forced_tile_no_burst": (3, 5, 43, 128, 0, False, None, "fp32", (2, 64), -1),
    "no_stage_unroll8": (3, 5, 43, 128, 0, False, None, "fp32", (8, 0), 0),
    "tables_300": (300, 1, 900, 24, 0, False, None, "fp32", (0, 0), -1),
}


def _plan_op(name):
    T, B, N, max_dim, min_dim, weighted, sl, _odt, _knobs, _stage = PLAN_REQUESTS[name]
    op = _request(T, B, N, max_dim, min_dim, weighted)
    if sl is not None:
        op.bag_begin, op.bag_count = sl
    return op


def plans_of(name):
    """``[pm_embbag_anyfmt_plan, pm_embedding_gather_anyfmt_plan]`` of a listed request under its knobs (dummy pointers; the knobs are put
    back); the second is None for a weighted request, which the un-pooled calls refuse"""
    _T, _B, _N, _max_dim, _min_dim, weighted, _sl, odt, (unroll, bpb), stage = PLAN_REQUESTS[name]
    op = _plan_op(name)
    try:
        _lib.set_tuning(unroll=unroll, bags_per_block=bpb)
        _lib.set_forward_tuning(stage_out=stage)
        p = _lib.embbag_anyfmt_plan(op, ODT[odt])
        g = None if weighted else _lib.embedding_gather_anyfmt_plan(op)
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
    assert not REWRITE, "PARAM_AMD_REWRITE_ANYFMT_PLAN=1 rewrote tests/anyfmt_plan_host.json: read its diff, then run without the flag"


def test_what_the_plans_say():
    """properties of the pinned rows from the plans' own rules (launch_plan.h: plan_anyfmt, plan_gather_anyfmt): eight columns per lane
    whatever the format -- the per-table-format plan of the same request but for the rows in flight, which are the kernel's"""
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
        assert p["unroll"] == 0                                       # a compile-time value per format: the knob is not read
        assert p["stage_out"] in (0, max_dim) and (p["stage_out"] == 0 or p["bags_per_block"] * max_dim * e <= 16384) and (stage != 0 or p["stage_out"] == 0)
        assert 512 <= p["idx_cap"] <= 4096 and p["idx_cap"] % 256 == 0
        if bpb:
            assert p["bags_per_block"] == bpb
        op = _plan_op(name)
        try:
            _lib.set_tuning(unroll=unroll, bags_per_block=bpb)
            _lib.set_forward_tuning(stage_out=stage)
            q = _lib.embbag_qrows_mixed_plan(op, ODT[odt])
            assert [0 if f == "unroll" else q[f] for f in FIELDS] == prow, name
        finally:
            _lib.set_tuning()
            _lib.set_forward_tuning()
        assert (grow is None) == weighted
        if grow is not None:
            g = dict(zip(GFIELDS, grow))
            assert g["vec"] == 8 and g["tile"] == 256 and g["grid"] == -(-N // 256) and g["group_lanes"] == lanes
            assert g["col_passes"] == -(-max_dim // (lanes * 8)) and g["unroll"] == 4 and lanes % g["unroll"] == 0
            assert g["lds_borders"] == (1 if T + 1 <= 256 else 0) and g["xcd_contiguous"] == (1 if T > 1 else 0)
    rows = {n: dict(zip(FIELDS, r[0])) for n, r in pinned.items()}
    assert rows["bench_shape"]["bags_per_block"] == 32 and rows["bench_shape"]["stage_out"] == 128
    assert rows["seven_d64_b70"]["bags_per_block"] == 32 and rows["seven_d64_b70"]["tiles_per_table"] == 3      # (tests/test_gpu_anyfmt.py: case 2)
    assert rows["tile_longer_than_index_tile"]["tiles_per_table"] == 1 and rows["tile_longer_than_index_tile"]["idx_cap"] < 6000
    assert rows["forced_tile_no_burst"]["stage_out"] == 0 and rows["batch_slice"]["tiles_per_table"] == 1
    gath = {n: dict(zip(GFIELDS, r[1])) for n, r in pinned.items() if r[1] is not None}
    assert gath["d1024"]["col_passes"] == 2 and gath["d2048"]["col_passes"] == 4 and gath["bench_shape"]["group_lanes"] == 16
    assert gath["tables_300"]["lds_borders"] == 0 and gath["d8"]["lds_borders"] == 1


def test_the_plan_is_identical_for_any_permutation_of_the_formats():
    """the plan queries have no argument through which a format could reach them (request, out_dtype, result), and what a module hands
    them -- the request's sizes -- is the same for every permutation of its formats; tests/test_gpu_anyfmt.py asks the modules' ``plan``
    on the device"""
    from param_amd import MixedBatchedEmbeddingBagMI355 as MB

    L = _lib.load()
    assert len(L.pm_embbag_anyfmt_plan.argtypes) == 3 and len(L.pm_embedding_gather_anyfmt_plan.argtypes) == 2
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(4):
        m = MB([50] * 7, [64] * 7, [AC.SEVEN[i] for i in rng.permutation(7)], device="cpu")
        seen.add((tuple(m.rows), tuple(m.dims), m.layout, m.output_dtype))
    assert len(seen) == 1
    for name in ("seven_d64_b5", "mixed_dims"):
        assert plans_of(name) == plans_of(name)


# ---- the compiled kernels --------------------------------------------------------------------------------------------------------------

def test_no_instance_of_the_new_kernels_uses_scratch(bundles):  # noqa: F811
    """code-object metadata (llvm-readelf --notes; no GPU): the launcher ladders name 4 lane-group widths x weighted or not x 3 output
    types of the pooled kernel and 3 output types x 4 widths of the un-pooled one; none has a private segment; the un-pooled kernel's
    LDS is its four arrays; every instance keeps two waves per SIMD at least"""
    res = _kernel_resources(bundles)
    pooled = {n: v for n, v in res.items() if "17anyfmt_fwd_kernel" in n}
    gather = {n: v for n, v in res.items() if "20anyfmt_gather_kernel" in n}
    assert len(pooled) == 4 * 2 * 3 and len(gather) == 3 * 4, (len(pooled), len(gather))
    for name, (vgpr, _sgpr, scratch, lds) in pooled.items():
        assert scratch == 0 and lds == 0 and vgpr <= 128, (name, vgpr, scratch, lds)          # (the tile's LDS is dynamic)
    for name, (vgpr, _sgpr, scratch, lds) in gather.items():
        assert scratch == 0 and lds == 256 * 8 + 256 * 8 + 256 * 4 + 256 * 4 and vgpr <= 256, (name, vgpr, scratch, lds)
    print("anyfmt_fwd_kernel VGPRs", sorted({v[0] for v in pooled.values()}), "anyfmt_gather_kernel VGPRs", sorted({v[0] for v in gather.values()}))
    # the kernels they stand in for keep their names and counts
    assert len([n for n in res if "17qmixed_fwd_kernel" in n]) == 4 * 2 * 3 * 2 and len([n for n in res if "20qmixed_gather_kernel" in n]) == 3 * 4 * 4
