"""ROW-QUANTISED TABLES on the CPU: the numpy restatement (tests/qrows_rules.py) against torch's two CPU lookup operators -- live and
through the committed fixture tests/golden/qrows_cases.npz --, every host-side refusal of ``pm_embbag_fwd_qrows`` /
``pm_embbag_qrows_plan``, the plans pinned in tests/qrows_plan_host.json, and what the two modules refuse without a device.

``PARAM_AMD_REWRITE_QROWS_PLAN=1 pytest tests/test_qrows_host.py`` writes the JSON anew from what the library plans (read the diff: a
changed row is a changed launch geometry)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from param_amd import _lib
from tests import qrows_cases as C
from tests import qrows_rules as R

HERE = os.path.dirname(os.path.abspath(__file__))
PINNED = os.path.join(HERE, "qrows_plan_host.json")
REWRITE = os.environ.get("PARAM_AMD_REWRITE_QROWS_PLAN") == "1"
ODT = {"fp32": _lib.PM_F32, "bf16": _lib.PM_BF16, "fp16": _lib.PM_F16}


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(HERE, "golden", "qrows_cases.npz"))


# ---- the rule against torch ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", C.BITS)
@pytest.mark.parametrize("dim", C.DIMS)
def test_rule_equals_torch_operators_live_and_fixture(fixture, bits, dim):
    idx, off, psw = C.request()
    q = C.torch_prepack(C.float_table(dim), bits)
    assert q.shape == (C.ROWS, R.row_bytes(dim, bits)) and np.array_equal(q, fixture[f"q_{bits}_{dim}"])
    for it in ("i32", "i64"):
        dt = np.int32 if it == "i32" else np.int64
        for weighted in (False, True):
            w = psw if weighted else None
            want = R.forward([q], [dim], bits, idx.astype(dt), off.astype(dt), len(off), w)[0]
            live = C.torch_lookup(q, bits, idx.astype(dt), off.astype(dt), w)
            assert want.shape == (len(C.LENS), dim)
            assert R.same_f32(live, want), (bits, dim, it, weighted)
            assert R.same_f32(fixture[C.key(bits, dim, it, weighted)], want), (bits, dim, it, weighted)
            assert not want[[0, 2, 6]].any() and not np.signbit(want[[0, 2, 6]]).any()      # empty bags: +0.0


@pytest.mark.parametrize("bits", C.BITS)
def test_rule_with_a_trailing_offset_and_a_slice(bits):
    """``include_last_offset=True`` is the same request with one more offsets entry; a batch slice is the rows of that slice"""
    idx, off, psw = C.request()
    q = C.torch_prepack(C.float_table(24), bits)
    closed = np.concatenate([off, [idx.size]])
    whole = R.forward([q], [24], bits, idx, off, len(off), psw)[0]
    assert R.same_f32(C.torch_lookup(q, bits, idx, closed, psw, include_last_offset=True), whole)
    assert R.same_f32(R.forward([q], [24], bits, idx, closed, len(off), psw)[0], whole)
    assert R.same_f32(R.forward([q], [24], bits, idx, off, len(off), psw, bag_begin=2, bag_count=3)[0], whole[2:5])


@pytest.mark.parametrize("bits", C.BITS)
def test_rule_on_inf_and_nan_tails(fixture, bits):
    """hand-built rows whose scale or bias is Inf / NaN: NaN positions as a mask, everything else as bits"""
    q = R.special_rows(8, bits)
    assert np.array_equal(q, fixture[f"special_q_{bits}"])
    si, so = C.special_request()
    want = R.forward([q], [8], bits, si, so, len(so))[0]
    assert R.same_f32(C.torch_lookup(q, bits, si, so), want) and R.same_f32(fixture[f"special_out_{bits}"], want)
    assert np.isnan(want).any() and np.isinf(want).any() and not want[5].any()
    codes, scale, bias = R.unpack(q, 8, bits)
    assert np.isinf(scale[0]) and np.isinf(bias[1]) and np.isnan(scale[2]) and np.isnan(bias[3]) and codes[0, 1] == 1


def test_fmaf_is_one_rounding():
    """a case where an fp64 multiply-add followed by the cast rounds twice: (1 + 2^-23) * 6 = 6 + 1.5 ulp is a tie of two fp32
    neighbours; minus 2^-60 the exact value lies BELOW the tie (-> 6 + ulp), but fp64 drops the 2^-60 and the cast ties to even (-> 6 + 2 ulp)"""
    a, b, c = np.float32(1 + 2.0**-23), np.float32(6.0), np.float32(-2.0**-60)
    naive = np.float32(float(a) * float(b) + float(c))
    got = R.fmaf(np.array([a]), np.array([b]), np.array([c]))[0]
    assert got == np.float32(6 + 2.0**-21) and naive == np.float32(6 + 2.0**-20)
    assert R.fmaf(np.array([a]), np.array([b]), np.array([-c]))[0] == np.float32(6 + 2.0**-20)
    assert R.fmaf(np.float32(np.inf), np.float32(0), np.float32(1)).item() != R.fmaf(np.float32(np.inf), np.float32(0), np.float32(1)).item()      # NaN
    assert R.fmaf(np.float32(3e38), np.float32(255), np.float32(0)).item() == np.inf


def test_bag_of_one_equals_dequantize_rows():
    from oracle import rowquant

    for bits in C.BITS:
        q = C.torch_prepack(C.float_table(24), bits)
        one = R.forward([q], [24], bits, np.arange(C.ROWS), np.arange(C.ROWS), C.ROWS)[0]
        assert np.array_equal(one, rowquant.dequantize_rows(q, 24, bits))      # as values (+0.0 == -0.0)


def test_fixture_is_small_and_complete(fixture):
    assert os.path.getsize(os.path.join(HERE, "golden", "qrows_cases.npz")) < 128 * 1024
    assert all(C.key(*c) in fixture.files for c in C.case_names()) and len(C.case_names()) == 40


# ---- the C calls without a device ------------------------------------------------------------------------------------------------------

def _request(T=2, B=4, N=24, max_dim=8, min_dim=0, weighted=False):
    op = _lib.pm_embbag_batch()
    op.num_tables, op.weight_dtype, op.index_dtype, op.max_dim, op.min_dim = T, 99, _lib.PM_I64, max_dim, min_dim      # weight_dtype is not read
    op.batch, op.num_indices, op.bag_begin, op.bag_count = B, N, 0, B
    op.tables = op.rows = op.dims = op.out_offsets = op.indices = op.offsets = 64      # non-null dummies, never dereferenced on the host
    op.out_stride = max_dim * T
    op.per_sample_weights = 64 if weighted else None
    return op


def test_argument_validation_without_gpu():
    """every refusal is made on the host, before any HIP call (the dummy pointers are never dereferenced)"""
    L = _lib.load()
    INVALID, UNSUPPORTED, F32 = _lib.PM_ERR_INVALID, _lib.PM_ERR_UNSUPPORTED, _lib.PM_F32
    plan_out = (ctypes.c_int32 * 12)()
    fwd = lambda op, bits=8, odt=F32, out=64: L.pm_embbag_fwd_qrows(None if op is None else ctypes.byref(op), bits, odt, out, None)      # noqa: E731
    plan = lambda op, bits=8, odt=F32, out=64: L.pm_embbag_qrows_plan(None if op is None else ctypes.byref(op), bits, odt, plan_out)     # noqa: E731
    err = L.pm_last_error
    for call in (fwd, plan):
        assert call(None) == INVALID and b"op is NULL" in err()
        # bits
        for bits in (2, 16):
            assert call(_request(), bits=bits) == UNSUPPORTED and b"payload format" in err() and str(bits).encode() in err()
        for bits in (0, 1, 3, 7, 32, -8):
            assert call(_request(), bits=bits) == INVALID and b"bits must be 8 or 4" in err()
        # what pm_embbag_fwd refuses about the request
        op = _request()
        op.num_tables = 0
        assert call(op) == INVALID and b"num_tables" in err()
        op = _request()
        op.index_dtype = 3
        assert call(op) == INVALID and b"index_dtype" in err()
        op = _request()
        op.bag_count = 5
        assert call(op) == INVALID and b"bag_begin/bag_count" in err()
        op = _request()
        op.offsets = None
        assert call(op) == INVALID and b"offsets" in err()
        op = _request()
        op.indices = None
        assert call(op) == INVALID and b"indices" in err()
        op = _request()
        op.tables = None
        assert call(op) == INVALID and b"tables" in err()
        op = _request()
        op.out_stride = 18
        assert call(op) == UNSUPPORTED and b"out_stride" in err()
        op = _request(min_dim=6)
        assert call(op) == INVALID and b"min_dim" in err()
        op = _request()
        op.fixed_pooling = 5
        assert call(op) == INVALID and b"fixed_pooling" in err()
        # the column rules: D % 4 (8 bits), D % 8 (4 bits)
        assert call(_request(max_dim=6)) == UNSUPPORTED and b"multiple of 4" in err()
        assert plan(_request(max_dim=4)) == _lib.PM_OK      # (accepted requests are asked of the plan query only: it launches nothing)
        assert call(_request(max_dim=12), bits=4) == UNSUPPORTED and b"multiple of 8" in err()
        assert call(_request(max_dim=4), bits=4) == UNSUPPORTED and b"multiple of 8" in err()
        assert call(_request(max_dim=16, min_dim=12), bits=4) == INVALID and b"min_dim" in err()
        # every width up to 1024 that keeps the column rule is accepted; the limit is 4096
        assert all(plan(_request(max_dim=d)) == _lib.PM_OK for d in range(4, 1025, 4))
        assert all(plan(_request(max_dim=d), bits=4) == _lib.PM_OK for d in range(8, 1025, 8))
        assert plan(_request(max_dim=4096)) == _lib.PM_OK and plan(_request(max_dim=4096), bits=4) == _lib.PM_OK
        assert call(_request(max_dim=4100)) == UNSUPPORTED and b"at most 4096" in err()
        assert call(_request(max_dim=4104), bits=4) == UNSUPPORTED and b"at most 4096" in err()
        # out_dtype
        for odt in (-1, 3, _lib.PM_I32, _lib.PM_I64):
            assert call(_request(), odt=odt) == INVALID and b"out_dtype" in err()
        # blocked layouts
        for field, val in (("table_group", 2), ("grad_block_shift", 1), ("grad_block_extra", 64)):
            op = _request()
            setattr(op, field, val)
            if field == "grad_block_extra":      # (alone it is what every entry point refuses: a block of one bag)
                assert call(op) == INVALID and b"grad_block_extra" in err()
                op.grad_block_shift = 2
            assert call(op) == UNSUPPORTED and b"blocked layouts" in err(), field
    # the lookup's own: out.  NULL, misaligned (16 bytes fp32, 8 bytes 16-bit)
    assert fwd(_request(), out=None) == INVALID and b"out is NULL" in err()
    assert fwd(_request(), out=72) == INVALID and b"16-byte aligned" in err()
    assert fwd(_request(), odt=_lib.PM_BF16, out=68) == INVALID and b"8-byte aligned" in err()
    assert fwd(_request(), odt=_lib.PM_F16, out=68) == INVALID and b"8-byte aligned" in err()
    assert L.pm_embbag_qrows_plan(ctypes.byref(_request()), 8, F32, None) == INVALID and b"out is NULL" in err()
    # bag_count == 0: PM_OK without a launch, whatever `out` is
    empty = _request()
    empty.bag_count = 0
    assert fwd(empty, out=None) == _lib.PM_OK and fwd(empty, bits=4, odt=_lib.PM_F16, out=None) == _lib.PM_OK
    none = _request(B=0, N=0)
    assert fwd(none, out=None) == _lib.PM_OK


def test_symbols_are_exported():
    assert {"pm_embbag_fwd_qrows", "pm_embbag_qrows_plan"} <= set(_lib.EXPORTED_SYMBOLS)
    L = _lib.load()
    assert L.pm_abi_version() == 8 and ctypes.sizeof(_lib.pm_embbag_batch) == 144
    assert L.pm_embbag_fwd_qrows.argtypes[1:3] == [ctypes.c_int32, ctypes.c_int32]


# ---- the plans ---------------------------------------------------------------------------------------------------------------------------

def plan_of(name):
    """``pm_embbag_qrows_plan`` of a listed request under its knobs (dummy pointers; the knobs are put back)"""
    bits, T, B, N, max_dim, min_dim, weighted, sl, odt, (unroll, bpb), stage = C.PLAN_REQUESTS[name]
    op = _request(T, B, N, max_dim, min_dim, weighted)
    if sl is not None:
        op.bag_begin, op.bag_count = sl
    try:
        _lib.set_tuning(unroll=unroll, bags_per_block=bpb)
        _lib.set_forward_tuning(stage_out=stage)
        p = _lib.embbag_qrows_plan(op, bits, ODT[odt])
    finally:
        _lib.set_tuning()
        _lib.set_forward_tuning()
    return [p[f] for f in _lib.PLAN_FIELDS]


def test_every_listed_request_plans_its_pinned_row():
    rows = {name: plan_of(name) for name in C.PLAN_REQUESTS}
    if REWRITE:
        with open(PINNED, "w") as f:
            f.write('{\n "plan_fields": %s,\n "rows": {\n' % json.dumps(list(_lib.PLAN_FIELDS)))
            f.write(",\n".join("  %s: %s" % (json.dumps(name), json.dumps(row)) for name, row in rows.items()))
            f.write("\n }\n}\n")
    pinned = json.load(open(PINNED))
    assert pinned["plan_fields"] == list(_lib.PLAN_FIELDS) and list(pinned["rows"]) == list(C.PLAN_REQUESTS)
    bad = [(name, pinned["rows"][name], row) for name, row in rows.items() if row != pinned["rows"][name]]
    assert not bad, f"{len(bad)} of {len(rows)} rows differ; the first (request, pinned, planned): {bad[0]}"


def test_the_plan_header_alone_plans_the_pinned_rows_under_sanitizers(tmp_path):
    """``plan_qrows`` is pure host code: a stand-alone program over launch_plan.h, built with AddressSanitizer and
    UndefinedBehaviorSanitizer, plans the pinned rows -- the library's query and the header agree, and the header's arithmetic is clean"""
    import shutil
    import subprocess

    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "qrows_plan_dump")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-I", os.path.join(root, "include"), "-I", os.path.join(root, "param_amd", "csrc"),
                    os.path.join(HERE, "qrows_plan_dump.cpp"), "-o", exe], check=True)
    lines = []
    for bits, T, B, N, max_dim, min_dim, weighted, sl, odt, (unroll, bpb), stage in C.PLAN_REQUESTS.values():
        begin, count = (0, B) if sl is None else sl
        lines.append(" ".join(map(str, (bits, T, B, N, max_dim, min_dim, int(weighted), begin, count, 4 if odt == "fp32" else 2, unroll, bpb, stage, 2))))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    assert got == list(json.load(open(PINNED))["rows"].values())


def test_the_pinned_rows_are_not_being_rewritten():
    assert not REWRITE, "PARAM_AMD_REWRITE_QROWS_PLAN=1 rewrote tests/qrows_plan_host.json: read its diff, then run without the flag"


def test_what_the_plans_say():
    """properties of the pinned rows that the GPU tests rely on, from the plan's own rules (launch_plan.h: plan_qrows)"""
    rows = {n: dict(zip(_lib.PLAN_FIELDS, r)) for n, r in json.load(open(PINNED))["rows"].items()}
    for name, p in rows.items():
        bits, T, B, N, max_dim, _, _, sl, odt, (unroll, bpb), stage = C.PLAN_REQUESTS[name]
        e = 4 if odt == "fp32" else 2
        count = B if sl is None else sl[1]
        assert p["tiles_per_table"] == -(-count // p["bags_per_block"]) and p["stage_bags"] == p["bags_per_block"]
        assert p["ordered"] == p["nt_loads"] == p["flat_bags"] == p["flat_target"] == p["flat_compact"] == 0
        assert p["unroll"] == (2 if 0 < unroll < 4 else 4)
        assert p["stage_out"] in (0, max_dim) and (p["stage_out"] == 0 or p["bags_per_block"] * max_dim * e <= 16384)
        assert 512 <= p["idx_cap"] <= 4096 and p["idx_cap"] % 256 == 0
        if bpb:
            assert p["bags_per_block"] == bpb
    # lane groups: two dwords of codes per lane -- D = 128 is 16 lanes (8 bits) / 8 lanes (4 bits): 16 / 32 bags per round, tiles of 4
    # rounds unless the burst buffer holds fewer rows (32 fp32 rows of 128 floats are its 16 KB; 64 fp16 rows fit)
    assert rows["even_8bit_d128"]["bags_per_block"] == 32 and rows["even_4bit_d128"]["bags_per_block"] == 32
    assert rows["out_fp16"]["bags_per_block"] == 64 and rows["out_fp16"]["stage_out"] == 128
    assert rows["even_8bit_d128"]["idx_cap"] == 1280 and rows["even_8bit_d128"]["stage_out"] == 128
    # 4 x 1500 lookups in one tile: more than the 4096-entry index tile can hold -- the unstaged path
    assert rows["tile_longer_than_index_tile"]["tiles_per_table"] == 1 and rows["tile_longer_than_index_tile"]["idx_cap"] < 6000
    # D = 1024: 4 bags of 4 KB fill the 16 KB burst buffer exactly (fp32); 16-bit outputs leave room
    assert rows["d1024_8bit"]["stage_out"] == 1024 and rows["d1024_8bit"]["bags_per_block"] == 4
    assert rows["forced_tile_no_burst"]["stage_out"] == 0 and rows["forced_tile_no_burst"]["unroll"] == 4


# ---- the modules without a device ------------------------------------------------------------------------------------------------------

def test_constructors_and_refusals_on_cpu():
    from param_amd import QuantizedBatchedEmbeddingBagMI355 as QB
    from param_amd import QuantizedEmbeddingBagMI355 as QE

    m = QB([5, 7], [4, 128], 8, device="cpu")
    assert m.table(0).shape == (5, 12) and m.table(1).shape == (7, 136) and m.table(1).dtype == torch.uint8 and not m.weights.any()
    assert m.table(1).data_ptr() % 4 == 0 and not list(m.parameters()) and "weights" in m.state_dict()
    m4 = QB([5, 7], [8, 128], 4, device="cpu", layout="bd", output_dtype="fp16")
    assert m4.table(0).shape == (5, 8) and m4.table(1).shape == (7, 68) and m4.output_dtype == torch.float16
    assert QB([3, 3], 16, 4, device="cpu", layout="tbd").dims == [16, 16]
    # state_dict round-trips the bytes
    m.table(1).copy_(torch.arange(7 * 136, dtype=torch.int64).remainder(251).to(torch.uint8).view(7, 136))
    twin = QB([5, 7], [4, 128], 8, device="cpu")
    twin.load_state_dict(m.state_dict())
    assert torch.equal(twin.table(1), m.table(1)) and torch.equal(twin.weights, m.weights)
    # refusals, before anything is allocated (rows that could not be allocated prove it)
    huge = [2**30]
    for kw, text in ((dict(bitwidth=2), "bitwidth"), (dict(bitwidth=16), "bitwidth"), (dict(bitwidth=True), "bitwidth"),
                     (dict(bitwidth=8, dims=[6]), "multiple of 4"), (dict(bitwidth=4, dims=[12]), "multiple of 8"),
                     (dict(bitwidth=4, dims=[4]), "multiple of 8"), (dict(bitwidth=8, dims=[4100]), "4096"),
                     (dict(bitwidth=8, layout="blocked"), "blocked"), (dict(bitwidth=8, pooling_mode="mean"), "sum pooling"),
                     (dict(bitwidth=8, pooling_mode=1), "sum pooling"), (dict(bitwidth=8, padding_idx=0), "padding_idx"),
                     (dict(bitwidth=8, output_dtype="int8"), "output_dtype"), (dict(bitwidth=8, bounds_check_mode="loud"), "bounds_check_mode")):
        args = dict(dims=[1024], device="cpu")
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            QB(huge, **args)
    with pytest.raises(ValueError, match="common embedding dim"):
        QB([3, 3], [8, 16], 8, device="cpu", layout="tbd")
    # call time: no CPU fallback; floating-point indices
    idx, off = torch.zeros(4, dtype=torch.int64), torch.arange(0, 5, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.lookup(idx, torch.zeros(5, dtype=torch.int64), batch=2)
    with pytest.raises(TypeError, match="int64 or both int32"):
        m.lookup(idx.float(), off)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.plan(idx, torch.zeros(5, dtype=torch.int64), batch=2)
    with pytest.raises(TypeError):
        m.quantize_from_(0, torch.zeros(5, 4, dtype=torch.float16))
    with pytest.raises(ValueError):
        m.quantize_from_(0, torch.zeros(4, 4))
    # the single-table module
    e = QE(10, 24, device="cpu")
    assert e.bitwidth == 8 and e.table(0).shape == (10, 32) and e.num_embeddings == 10 and e.embedding_dim == 24
    packed = torch.ops.quantized.embedding_bag_4bit_prepack(torch.randn(10, 24))
    e4 = QE(10, 24, 4, device="cpu", weight=packed)
    assert torch.equal(e4.table(0), packed)
    with pytest.raises(ValueError, match="packed uint8 rows"):
        QE(10, 24, 8, device="cpu", weight=packed)
    with pytest.raises(ValueError, match="sum pooling"):
        QE(10, 24, device="cpu", mode="mean")
    with pytest.raises(ValueError, match="padding_idx"):
        QE(10, 24, device="cpu", padding_idx=3)
    with pytest.raises(ValueError, match="sum pooling"):
        QE.from_float(torch.nn.EmbeddingBag(10, 24, mode="mean"))
    with pytest.raises(ValueError, match="padding_idx"):
        QE.from_float(torch.nn.EmbeddingBag(10, 24, mode="sum", padding_idx=1))
    with pytest.raises(TypeError):
        QE.from_float(torch.nn.Embedding(10, 24))
    with pytest.raises(ValueError, match="offsets has to be"):
        e.forward(idx)
    with pytest.raises(ValueError, match="offsets has to be None"):
        e.forward(idx.view(2, 2), off)
