"""UN-POOLED lookups over ROW-QUANTISED TABLES on the CPU: the numpy restatement (tests/qgather_rules.py) against torch's CPU operators
-- ``quantized::embedding_bag_{byte,4bit}_rowwise_offsets`` over bags of one and ``torch.ao.nn.quantized.Embedding``, live and through
the committed fixture tests/golden/qgather_cases.npz --, every host-side refusal of ``pm_embedding_gather_qrows`` /
``pm_embedding_gather_qrows_plan``, the plans pinned in tests/qgather_plan_host.json, and what the modules refuse without a device.

``PARAM_AMD_REWRITE_QGATHER_PLAN=1 pytest tests/test_qgather_host.py`` writes the JSON anew from what the library plans (read the diff: a
changed row is a changed launch geometry)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from param_amd import _lib
from tests import qgather_cases as G
from tests import qgather_rules as Q
from tests import qrows_cases as C
from tests import qrows_rules as R

HERE = os.path.dirname(os.path.abspath(__file__))
PINNED = os.path.join(HERE, "qgather_plan_host.json")
FIXTURE = os.path.join(HERE, "golden", "qgather_cases.npz")
REWRITE = os.environ.get("PARAM_AMD_REWRITE_QGATHER_PLAN") == "1"


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


# ---- the rule against torch ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", G.BITS)
@pytest.mark.parametrize("dim", C.DIMS)
def test_rule_equals_torch_operators_over_bags_of_one(bits, dim):
    """live, every width of qrows_cases: repeated rows, both index types; and the pooled rule over the same bags of one"""
    q = C.torch_prepack(C.float_table(dim), bits)
    idx = G.indices()
    want = Q.rows(q, dim, bits, idx)
    assert want.shape == (G.N, dim) and want.dtype == np.float32
    for dt in (np.int32, np.int64):
        assert R.same_f32(G.torch_rows(q, bits, idx.astype(dt)), want), (bits, dim, dt)
    assert R.same_f32(R.forward([q], [dim], bits, idx, np.arange(G.N), G.N)[0], want)
    assert np.array_equal(want[7], want[3]) and np.array_equal(want[8], want[6])          # a repeated row is the same row
    out, written = Q.gather([q], dim, bits, idx, np.zeros(1, dtype=np.int64), 1)
    assert written.all() and R.same_f32(out, want)                                        # one table, one bag, offsets = [0]


@pytest.mark.parametrize("bits", G.BITS)
def test_rule_on_signed_zero_rows_is_torchs_and_not_a_plain_fmaf(bits):
    """tails (0.5, -0.0), (-0.25, 0.0), (-0.25, -0.0), (0.0, -0.0), (-0.0, 1.0) and a code-0 column: the rule, the pooled rule over bags
    of one and torch agree bit for bit and hold no -0.0; ``fmaf(scale, code, bias)`` does"""
    q = Q.signed_zero_rows(8, bits)
    r = np.arange(5)
    want = Q.rows(q, 8, bits, r)
    codes, scale, bias = R.unpack(q, 8, bits)
    assert (codes[:, 0] == 0).all() and np.signbit(bias[[0, 2, 3]]).all() and np.signbit(scale[4]) and scale[4] == 0
    assert R.same_f32(G.torch_rows(q, bits, r), want) and R.same_f32(R.forward([q], [8], bits, r, r, 5)[0], want)
    assert Q.negative_zeros(want) == 0 and (want == 0).sum() == 3 + 8      # column 0 of rows 0 .. 2, all of row 3
    plain = R.fmaf(scale[:, None], codes.astype(np.float32), bias[:, None])
    assert Q.negative_zeros(plain) > 0 and not R.same_f32(plain, want) and np.array_equal(plain, want)      # equal as values only


def test_rule_equals_quantized_embedding_module():
    """``torch.ao.nn.quantized.Embedding`` (``quantized::embedding_byte``) on the weight as its accessors give it"""
    idx = G.indices()
    for dim in (4, 24, 128):
        got, packed = G.torch_embedding(C.float_table(dim), idx)
        assert packed.shape == (C.ROWS, R.row_bytes(dim, 8))
        assert R.same_f32(got, Q.rows(packed, dim, 8, idx)), dim


def test_fixture_matches_the_rule_and_is_small_and_complete(fixture):
    assert os.path.getsize(FIXTURE) <= os.path.getsize(os.path.join(HERE, "golden", "qrows_cases.npz"))
    idx = fixture["indices"]
    assert np.array_equal(idx, G.indices())
    want_files = {"indices", "embedding_q_8_24", "embedding_out_8_24"}
    for bits in G.BITS:
        for dim in G.DIMS:
            q = fixture[f"q_{bits}_{dim}"]
            assert np.array_equal(q, C.torch_prepack(C.float_table(dim), bits))
            assert R.same_f32(fixture[G.key(bits, dim)], Q.rows(q, dim, bits, idx)), (bits, dim)
            want_files |= {f"q_{bits}_{dim}", G.key(bits, dim)}
        z = fixture[f"zeros_q_{bits}"]
        assert np.array_equal(z, Q.signed_zero_rows(8, bits))
        assert R.same_f32(fixture[f"zeros_out_{bits}"], Q.rows(z, 8, bits, np.arange(5))) and Q.negative_zeros(fixture[f"zeros_out_{bits}"]) == 0
        want_files |= {f"zeros_q_{bits}", f"zeros_out_{bits}"}
    assert R.same_f32(fixture["embedding_out_8_24"], Q.rows(fixture["embedding_q_8_24"], 24, 8, idx))
    assert set(fixture.files) == want_files


@pytest.mark.parametrize("bits", G.BITS)
def test_rule_on_inf_and_nan_tails(bits):
    """``qrows_rules.special_rows`` through the rule: NaN positions as a mask, everything else as bits -- torch's and the pooled rule's"""
    q = R.special_rows(8, bits)
    r = np.arange(4)
    want = Q.rows(q, 8, bits, r)
    assert R.same_f32(G.torch_rows(q, bits, r), want) and R.same_f32(R.forward([q], [8], bits, r, r, 4)[0], want)
    assert np.isnan(want[0, 0]) and np.isposinf(want[0, 1:]).all()      # Inf * code 0 is NaN, Inf * code > 0 is Inf
    assert np.isneginf(want[1]).all() and np.isnan(want[2:]).all()


def test_owners_and_slices():
    """the table of a position and the slice mask: an empty first bag, a table that owns nothing, a position in front of every table"""
    off = np.array([0, 0, 3, 3, 3, 5, 9], dtype=np.int64)               # T = 3, B = 2 (+ a trailing entry): table 1 owns nothing
    table, written = Q.owners(off, 3, 2, 10)
    assert table.tolist() == [0, 0, 0, 2, 2, 2, 2, 2, 2, 2] and written.all()
    _, sl = Q.owners(off, 3, 2, 10, bag_begin=1, bag_count=1)
    assert sl.tolist() == [True] * 3 + [False] * 2 + [True] * 5
    _, none = Q.owners(off, 3, 2, 10, bag_begin=1, bag_count=0)
    assert not none.any()
    table, written = Q.owners(np.array([2, 4]), 1, 2, 6)
    assert table.tolist() == [-1, -1, 0, 0, 0, 0] and written.tolist() == [False, False, True, True, True, True]


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
    plan_out = (ctypes.c_int64 * 8)()

    def lookup(op, bits=8, odt=F32, out=64, stride=None):
        stride = (op.max_dim if op is not None else 8) if stride is None else stride
        return L.pm_embedding_gather_qrows(None if op is None else ctypes.byref(op), bits, odt, out, stride, None)

    def plan(op, bits=8, **_):
        return L.pm_embedding_gather_qrows_plan(None if op is None else ctypes.byref(op), bits, plan_out)

    err = L.pm_last_error
    for call in (lookup, plan):
        assert call(None) == INVALID and b"op is NULL" in err()
        # bits
        for bits in (2, 16):
            assert call(_request(), bits=bits) == UNSUPPORTED and b"payload format" in err() and str(bits).encode() in err()
        for bits in (0, 1, 3, 7, 32, -8):
            assert call(_request(), bits=bits) == INVALID and b"bits must be 8 or 4" in err()
        # what pm_embbag_fwd refuses about the request
        for field, val, text in (("num_tables", 0, b"num_tables"), ("index_dtype", 3, b"index_dtype"), ("bag_count", 5, b"bag_begin/bag_count"),
                                 ("offsets", None, b"offsets"), ("indices", None, b"indices"), ("tables", None, b"tables"),
                                 ("fixed_pooling", 5, b"fixed_pooling")):
            op = _request()
            setattr(op, field, val)
            assert call(op) == INVALID and text in err(), field
        assert call(_request(min_dim=6)) == INVALID and b"min_dim" in err()
        # the column rules: D % 4 (8 bits), D % 8 (4 bits); the limit is 4096
        assert call(_request(max_dim=6)) == UNSUPPORTED and b"multiple of 4" in err()
        assert call(_request(max_dim=12), bits=4) == UNSUPPORTED and b"multiple of 8" in err()
        assert call(_request(max_dim=4), bits=4) == UNSUPPORTED and b"multiple of 8" in err()
        assert plan(_request(max_dim=4)) == _lib.PM_OK      # (accepted requests are asked of the plan query only: it launches nothing)
        assert all(plan(_request(max_dim=d)) == _lib.PM_OK for d in range(4, 1025, 4))
        assert all(plan(_request(max_dim=d), bits=4) == _lib.PM_OK for d in range(8, 1025, 8))
        assert plan(_request(max_dim=4096)) == _lib.PM_OK and plan(_request(max_dim=4096), bits=4) == _lib.PM_OK
        assert call(_request(max_dim=4100)) == UNSUPPORTED and b"at most 4096" in err()
        assert call(_request(max_dim=4104), bits=4) == UNSUPPORTED and b"at most 4096" in err()
        # blocked layouts
        for field, val in (("table_group", 2), ("grad_block_shift", 1), ("grad_block_extra", 64)):
            op = _request()
            setattr(op, field, val)
            if field == "grad_block_extra":      # (alone it is what every entry point refuses: a block of one bag)
                assert call(op) == INVALID and b"grad_block_extra" in err()
                op.grad_block_shift = 2
            assert call(op) == UNSUPPORTED and b"blocked layouts" in err(), field
        # what pm_embedding_gather refuses about the request: weights
        assert call(_request(weighted=True)) == UNSUPPORTED and b"per_sample_weights must be NULL" in err()
    # the lookup's own: out_dtype, out_row_stride, out (NULL, misaligned: 16 bytes fp32, 8 bytes 16-bit)
    for odt in (-1, 3, _lib.PM_I32, _lib.PM_I64):
        assert lookup(_request(), odt=odt) == INVALID and b"out_dtype" in err()
    for stride in (4, 7, 10, -8):
        assert lookup(_request(), stride=stride) == INVALID and b"out_row_stride" in err(), stride
    assert lookup(_request(), out=None) == INVALID and b"out is NULL" in err()
    assert lookup(_request(), out=72) == INVALID and b"16-byte aligned" in err()
    assert lookup(_request(), odt=_lib.PM_BF16, out=68) == INVALID and b"8-byte aligned" in err()
    assert lookup(_request(), odt=_lib.PM_F16, out=68) == INVALID and b"8-byte aligned" in err()
    assert L.pm_embedding_gather_qrows_plan(ctypes.byref(_request()), 8, None) == INVALID and b"out is NULL" in err()
    # nothing to do: PM_OK without a launch, whatever `out` is
    empty = _request()
    empty.bag_count = 0
    assert lookup(empty, out=None) == _lib.PM_OK and lookup(empty, bits=4, odt=_lib.PM_F16, out=None) == _lib.PM_OK
    none = _request(N=0)
    none.indices = None
    assert lookup(none, out=None) == _lib.PM_OK and lookup(_request(B=0, N=0), out=None) == _lib.PM_OK


def test_symbols_are_exported():
    assert {"pm_embedding_gather_qrows", "pm_embedding_gather_qrows_plan"} <= set(_lib.EXPORTED_SYMBOLS)
    L = _lib.load()
    assert L.pm_abi_version() == 8 and ctypes.sizeof(_lib.pm_embbag_batch) == 144
    assert L.pm_embedding_gather_qrows.argtypes[1:3] == [ctypes.c_int32, ctypes.c_int32]
    assert hasattr(_lib.load_alternates(), "pm_embedding_gather_qrows")


# ---- the plans ---------------------------------------------------------------------------------------------------------------------------

FIELDS = list(_lib.GATHER_PLAN_FIELDS)


def plan_of(name):
    """``pm_embedding_gather_qrows_plan`` of a listed request under its knobs (dummy pointers; the knobs are put back)"""
    bits, T, N, max_dim, unroll, xcd = G.PLAN_REQUESTS[name]
    op = _request(T, 1, N, max_dim)
    try:
        _lib.set_tuning(unroll=unroll, xcd_affine=xcd)
        p = _lib.embedding_gather_qrows_plan(op, bits)
    finally:
        _lib.set_tuning()
    return [p[f] for f in FIELDS]


def test_every_listed_request_plans_its_pinned_row():
    rows = {name: plan_of(name) for name in G.PLAN_REQUESTS}
    if REWRITE:
        with open(PINNED, "w") as f:
            f.write('{\n "plan_fields": %s,\n "rows": {\n' % json.dumps(FIELDS))
            f.write(",\n".join("  %s: %s" % (json.dumps(name), json.dumps(row)) for name, row in rows.items()))
            f.write("\n }\n}\n")
    pinned = json.load(open(PINNED))
    assert pinned["plan_fields"] == FIELDS and list(pinned["rows"]) == list(G.PLAN_REQUESTS)
    bad = [(name, pinned["rows"][name], row) for name, row in rows.items() if row != pinned["rows"][name]]
    assert not bad, f"{len(bad)} of {len(rows)} rows differ; the first (request, pinned, planned): {bad[0]}"


def test_the_plan_header_alone_plans_the_pinned_rows_under_sanitizers(tmp_path):
    """``plan_gather_qrows`` is pure host code: a stand-alone program over launch_plan.h, built with AddressSanitizer and
    UndefinedBehaviorSanitizer, plans the pinned rows -- the library's query and the header agree, the header's arithmetic is clean --
    and walks every grid: each position lies in exactly one tile of ``gather_block_tile``"""
    import shutil
    import subprocess

    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "qgather_plan_dump")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-I", os.path.join(root, "include"), "-I", os.path.join(root, "param_amd", "csrc"),
                    os.path.join(HERE, "qgather_plan_dump.cpp"), "-o", exe], check=True)
    lines = [" ".join(map(str, (bits, T, N, max_dim, unroll, xcd, 2))) for bits, T, N, max_dim, unroll, xcd in G.PLAN_REQUESTS.values()]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    assert [g[:-1] for g in got] == list(json.load(open(PINNED))["rows"].values())
    assert [g[-1] for g in got] == [req[2] for req in G.PLAN_REQUESTS.values()]          # every position covered exactly once


def test_the_pinned_rows_are_not_being_rewritten():
    assert not REWRITE, "PARAM_AMD_REWRITE_QGATHER_PLAN=1 rewrote tests/qgather_plan_host.json: read its diff, then run without the flag"


def test_what_the_plans_say():
    """properties of the pinned rows from the plan's own rules (launch_plan.h: plan_gather_qrows), and what the list covers"""
    rows = {n: dict(zip(FIELDS, r)) for n, r in json.load(open(PINNED))["rows"].items()}
    default = rows["bench_8bit_d128"]["unroll"]
    assert default in (1, 2, 4, 8) and rows["bench_4bit_d128"]["unroll"] == default          # kQgatherUnroll, one default for both formats
    for name, p in rows.items():
        bits, T, N, max_dim, unroll, xcd = G.PLAN_REQUESTS[name]
        cols = 8 if bits == 8 else 16                                                     # two dwords of codes per lane
        need = -(-max_dim // cols)
        assert p["vec"] == cols and p["tile"] == 256 and p["grid"] == -(-N // 256)
        assert p["group_lanes"] == min(64, max(8, 1 << (need - 1).bit_length())) and p["col_passes"] == -(-max_dim // (p["group_lanes"] * cols))
        assert p["unroll"] == (default if unroll == 0 else max(u for u in (1, 2, 4, 8) if u <= unroll)) and p["group_lanes"] % p["unroll"] == 0
        assert p["lds_borders"] == (1 if T + 1 <= 256 else 0) and p["xcd_contiguous"] == (1 if T > 1 and xcd != 0 else 0)
    assert rows["bench_8bit_d128"]["group_lanes"] == 16 and rows["bench_4bit_d128"]["group_lanes"] == 8
    assert rows["d1024_8bit"]["col_passes"] == 2 and rows["d1024_4bit"]["col_passes"] == 1
    assert rows["d4096_8bit"]["col_passes"] == 8 and rows["d4096_4bit"]["col_passes"] == 4
    reqs = list(G.PLAN_REQUESTS.values())
    assert {r[0] for r in reqs} == {8, 4} and {4, 8, 128, 1024, 4096} <= {r[3] for r in reqs} and {1, 16, 300} <= {r[1] for r in reqs}
    assert {r[4] for r in reqs} == {0, 1, 2, 3, 4, 6, 8} and 0 in {r[5] for r in reqs}


# ---- the modules without a device ------------------------------------------------------------------------------------------------------

def test_constructors_and_refusals_on_cpu():
    from param_amd import EmbeddingMI355
    from param_amd import QuantizedBatchedEmbeddingBagMI355 as QB
    from param_amd import QuantizedEmbeddingMI355 as QE

    m = QB([5, 7], [24, 24], 8, device="cpu", layout="tbd")
    idx, off = torch.zeros(4, dtype=torch.int64), torch.zeros(5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.lookup_sequence(idx, off, batch=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.sequence_plan(idx, off, batch=2)
    with pytest.raises(TypeError, match="int64 or both int32"):
        m.lookup_sequence(idx.float(), off, batch=2)
    for bad in (torch.zeros(4, 24, dtype=torch.float16), torch.zeros(3, 24), torch.zeros(4, 32), torch.zeros(24, 4).t()):
        with pytest.raises(ValueError, match="out must be a contiguous float32 tensor of shape"):
            m.lookup_sequence(idx, off, batch=2, out=bad)
    with pytest.raises(ValueError, match="one common embedding dim"):
        QB([5, 7], [4, 128], 8, device="cpu").lookup_sequence(idx, off, batch=2)
    with pytest.raises(ValueError, match="one common embedding dim"):
        QB([5, 7], [4, 128], 8, device="cpu").sequence_plan(idx, off, batch=2)
    # the single-table module
    e = QE(10, 24, device="cpu")
    assert e.bitwidth == 8 and e.table(0).shape == (10, 32) and (e.num_embeddings, e.embedding_dim) == (10, 24) and e.output_dtype == torch.float32
    assert not list(e.parameters()) and list(e.state_dict()) == ["weights"] and "bitwidth=8" in repr(e)
    packed = torch.ops.quantized.embedding_bag_4bit_prepack(torch.randn(10, 24))
    e4 = QE(10, 24, 4, device="cpu", output_dtype="bf16", weight=packed)
    assert torch.equal(e4.table(0), packed) and e4.output_dtype == torch.bfloat16
    twin = QE(10, 24, 4, device="cpu")
    twin.load_state_dict(e4.state_dict())
    assert torch.equal(twin.table(0), packed)
    with pytest.raises(ValueError, match="packed uint8 rows"):
        QE(10, 24, 8, device="cpu", weight=packed)
    for kw, text in ((dict(bitwidth=2), "bitwidth"), (dict(bitwidth=16), "bitwidth"), (dict(embedding_dim=6), "multiple of 4"),
                     (dict(embedding_dim=12, bitwidth=4), "multiple of 8"), (dict(embedding_dim=4100), "4096"),
                     (dict(output_dtype="int8"), "output_dtype"), (dict(bounds_check_mode="loud"), "bounds_check_mode")):
        args = dict(num_embeddings=2**30, embedding_dim=1024, device="cpu")      # (rows that could not be allocated: refused before)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            QE(**args)
    with pytest.raises(TypeError, match="int32 or int64"):
        e(torch.zeros(3))
    with pytest.raises(TypeError, match="int32 or int64"):
        e([1, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        e(torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        e(torch.zeros((2, 0, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="max_norm"):
        QE.from_float(torch.nn.Embedding(10, 24, max_norm=1.0))
    with pytest.raises(TypeError, match="EmbeddingMI355 or a torch.nn.Embedding"):
        QE.from_float(torch.nn.EmbeddingBag(10, 24, mode="sum"))
    assert not hasattr(EmbeddingMI355(4, 8, device="cpu"), "max_norm")
