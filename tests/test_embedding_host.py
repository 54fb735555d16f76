"""The un-pooled lookup without a GPU: the numpy rule (tests/embedding_rules.py) against torch's CPU ``nn.Embedding``; what
``EmbeddingMI355`` and ``BatchedEmbeddingBagMI355.lookup_sequence`` validate and refuse before they need a device; the host-side
argument checks of ``pm_embedding_gather``; and the launch geometry it plans (tests/gather_plan_dump.cpp around launch_plan.h, pinned
by tests/gather_plan_host.json -- rows written down from the rules of the plan, not printed by it)."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import embedding_rules as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _bits(t):
    t = t.detach().contiguous()
    if t.element_size() == 2:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.view(torch.int32).numpy().view(np.uint32)


def _weight(rows, D, kind, seed):
    """a CPU table of ``kind`` holding ordinary values, -0.0, Inf and a subnormal"""
    w = np.random.default_rng(seed).standard_normal((rows, D)).astype(np.float32)
    w[1, :] = -0.0
    w[2, 0], w[2, 1], w[2, 2] = np.inf, -np.inf, 1e-40
    return torch.from_numpy(w).to(TDT[kind])


# ---- 1. the rule is torch's nn.Embedding ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(23,), (4, 5), (2, 3, 4)], ids=["1d", "2d", "3d"])
@pytest.mark.parametrize("pad", [None, 3], ids=["nopad", "pad3"])
@pytest.mark.parametrize("kind", E.KINDS)
def test_forward_rule_is_torch_cpu_bit_for_bit(kind, pad, shape):
    """same dtype in and out -- what torch's module returns: fp32, and 16-bit tables with the table's dtype as output"""
    rows, D = 11, 8
    w = _weight(rows, D, kind, 5)
    idx = torch.from_numpy(np.random.default_rng(6).integers(0, rows, shape))
    want = torch.nn.Embedding.from_pretrained(w, padding_idx=pad)(idx)
    n = idx.numel()
    canvas = np.zeros((n, D), dtype=E.BITS[kind])
    got = E.forward([_bits(w)], kind, kind, idx.numpy().reshape(-1), np.zeros(1, np.int64), 1, canvas)
    assert np.array_equal(got.reshape(*shape, D), _bits(want))


def test_dense_gradient_rule_is_torch_cpu_with_repeated_rows():
    """torch's CPU embedding_dense_backward adds a row's gradients in index order: sequential fp32 adds from zero, the padding row
    zero -- bit for bit on a request in which rows repeat up to a dozen times"""
    rows, D, pad = 13, 8, 4
    rng = np.random.default_rng(7)
    idx = torch.from_numpy(rng.integers(0, rows, (6, 9)))
    assert np.bincount(idx.numpy().reshape(-1), minlength=rows).max() >= 6 and (idx == pad).any()
    m = torch.nn.Embedding(rows, D, padding_idx=pad)
    g = torch.from_numpy(rng.standard_normal((6, 9, D)).astype(np.float32))
    m(idx).backward(g)
    want = E.dense_grad(rows, idx.numpy(), g.numpy(), pad)
    assert np.array_equal(_bits(m.weight.grad), want.view(np.uint32))
    assert not want[pad].any()


def test_sparse_gradient_rule_is_torch_coalesce_without_repeats():
    rows, D, pad = 40, 8, 4
    rng = np.random.default_rng(8)
    idx = torch.from_numpy(rng.permutation(rows)[:24].reshape(4, 6))
    m = torch.nn.Embedding(rows, D, padding_idx=pad, sparse=True)
    g = torch.from_numpy(rng.standard_normal((4, 6, D)).astype(np.float32))
    m(idx).backward(g)
    c = m.weight.grad.coalesce()
    r, v = E.sparse_grad(rows, idx.numpy(), g.numpy(), pad)
    keep = c.indices()[0] != pad            # torch keeps the padding row's slot with a zero value; the rule leaves the row out
    if (idx == pad).any():
        assert not _bits(c.values()[~keep]).any()
    assert np.array_equal(c.indices()[0][keep].numpy(), r) and np.array_equal(_bits(c.values()[keep]), v.view(np.uint32))


def test_conv_follows_the_output_dtype_rule():
    """the converted pairs: exact widening, ONE rounding to nearest even (ties, overflow, subnormals: tests/out16_rules.py)"""
    from tests import out16_rules as O

    f = np.array([1.0, -0.0, 65504.0, 65520.0, 1e-8, 3.0e38, 1.00390625, np.inf], dtype=np.float32)
    assert np.array_equal(E.conv(f.view(np.uint32), "f32", "f16"), O.round16(f, "fp16"))
    assert np.array_equal(E.conv(f.view(np.uint32), "f32", "bf16"), O.round16(f, "bf16"))
    h = np.array([0x0001, 0x8000, 0x7BFF, 0x3C01], dtype=np.uint16)
    assert np.array_equal(E.conv(h, "f16", "f32"), h.view(np.float16).astype(np.float32).view(np.uint32))
    assert np.array_equal(E.conv(h, "f16", "bf16"), O.round16(h.view(np.float16).astype(np.float32), "bf16"))
    assert np.array_equal(E.conv(h, "f16", "f16"), h)


# ---- 2. constructor, validation and refusals on the CPU ---------------------------------------------------------------------------

def test_constructor_and_refusals_without_a_device():
    import param_amd
    from param_amd import EmbeddingMI355

    m = EmbeddingMI355(10, 8, device="cpu", padding_idx=-2)
    assert m.padding_idx == 8 and not m.weight[8].any() and m.weight[7].any() and m.weight.shape == (10, 8)
    assert m.output_dtype == torch.float32 and "10, 8" in repr(m) and "padding_idx=8" in repr(m)
    for bad in (10, -11):
        with pytest.raises(ValueError, match="padding_idx must be within num_embeddings"):
            EmbeddingMI355(10, 8, device="cpu", padding_idx=bad)
    with pytest.raises(TypeError, match="padding_idx must be an int or None"):
        EmbeddingMI355(10, 8, device="cpu", padding_idx=True)
    for spec, want in ((None, torch.float32), ("fp32", torch.float32), ("BF16", torch.bfloat16), (torch.float16, torch.float16), ("fp16", torch.float16)):
        assert EmbeddingMI355(10, 8, device="cpu", output_dtype=spec).output_dtype == want
    with pytest.raises(ValueError, match="output_dtype must be"):
        EmbeddingMI355(10, 8, device="cpu", output_dtype="int8")
    with pytest.raises(ValueError, match="bounds_check_mode"):
        EmbeddingMI355(10, 8, device="cpu", bounds_check_mode="loud")
    with pytest.raises(TypeError):
        EmbeddingMI355(10, 8, device="cpu", max_norm=1.0)                      # not a parameter
    with pytest.raises(TypeError):
        EmbeddingMI355(10, 8, device="cpu", scale_grad_by_freq=True)
    assert "output_dtype=torch.bfloat16" in repr(EmbeddingMI355(10, 8, device="cpu", output_dtype="bf16", sparse=True))
    # a floating-point input is a TypeError; a sound request reaches "no CPU fallback"
    with pytest.raises(TypeError, match="int32 or int64"):
        m(torch.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros((2, 3), dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.sanitize_(torch.zeros(3, dtype=torch.int32))
    assert param_amd.EmbeddingMI355 is EmbeddingMI355


def test_from_pretrained_and_freeze():
    from param_amd import EmbeddingMI355

    w = torch.arange(24, dtype=torch.float32).reshape(6, 4)
    m = EmbeddingMI355.from_pretrained(w, padding_idx=1)
    assert m.weight.data_ptr() == w.data_ptr() and not m.weight.requires_grad and m.padding_idx == 1
    assert m.weight[1].any()                                                     # a caller's weights are left alone
    assert (m.num_embeddings, m.embedding_dim) == (6, 4)
    t = EmbeddingMI355.from_pretrained(w, freeze=False, sparse=True, output_dtype="fp16")
    assert t.weight.requires_grad and t.sparse and t.output_dtype == torch.float16
    with pytest.raises(ValueError, match="2-dimensional"):
        EmbeddingMI355.from_pretrained(torch.zeros(4))


def test_lookup_sequence_refusals_without_a_device():
    from param_amd import BatchedEmbeddingBagMI355

    idx, off = torch.zeros(6, dtype=torch.int64), torch.arange(0, 7, 1, dtype=torch.int64)
    mk = lambda dims=8, **kw: BatchedEmbeddingBagMI355([5, 6, 7], dims, device="cpu", init=None, **kw)      # noqa: E731
    with pytest.raises(ValueError, match='layout="blocked"'):
        mk(layout="blocked", block_bags=2).lookup_sequence(idx, off)
    with pytest.raises(ValueError, match="one common embedding dim"):
        mk(dims=[8, 16, 8]).lookup_sequence(idx, off)
    with pytest.raises(ValueError, match="no un-pooled form"):
        mk(pooling_mode="mean").lookup_sequence(idx, off)
    m = mk()
    for out in (torch.zeros(6, 8, dtype=torch.float16), torch.zeros(5, 8), torch.zeros(6, 16)[:, :8], torch.zeros(6, 4)):
        with pytest.raises(ValueError, match="out must be a contiguous float32 tensor of shape"):
            m.lookup_sequence(idx, off, out=out)
    with pytest.raises(ValueError, match="bfloat16"):
        mk(output_dtype="bf16").lookup_sequence(idx, off, out=torch.zeros(6, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.lookup_sequence(idx, off, out=torch.zeros(6, 8))


# ---- 3. pm_embedding_gather: every host-side refusal, before any HIP call --------------------------------------------------------------

def test_gather_argument_validation_without_gpu():
    from param_amd import _lib

    L = _lib.load()
    F32, BF16, INVALID, UNSUPPORTED = _lib.PM_F32, _lib.PM_BF16, _lib.PM_ERR_INVALID, _lib.PM_ERR_UNSUPPORTED
    op = _lib.pm_embbag_batch()
    call = lambda out_dtype=F32, out=64, stride=8: L.pm_embedding_gather(ctypes.byref(op), out_dtype, out, stride, None)      # noqa: E731
    assert L.pm_embedding_gather(None, F32, 64, 8, None) == INVALID
    assert call() == INVALID and b"num_tables" in L.pm_last_error()              # what pm_embbag_fwd refuses ...
    op.num_tables, op.weight_dtype, op.index_dtype, op.max_dim = 2, F32, _lib.PM_I64, 6
    op.tables = op.rows = op.dims = op.out_offsets = op.indices = op.offsets = 8  # non-null dummies, never dereferenced on the host
    op.batch, op.bag_count, op.num_indices = 4, 4, 100
    assert call() == UNSUPPORTED and b"multiple of 4" in L.pm_last_error()
    op.max_dim, op.index_dtype = 8, 99
    assert call() == INVALID and b"index_dtype" in L.pm_last_error()
    op.index_dtype, op.bag_begin = _lib.PM_I64, 2
    assert call() == INVALID and b"bag_begin" in L.pm_last_error()
    op.bag_begin, op.weight_dtype = 0, 7
    assert call() == INVALID and b"dtype" in L.pm_last_error()
    op.weight_dtype = F32
    # ... and its own
    for bad in (3, 10, -1):
        assert call(out_dtype=bad) == INVALID and b"out_dtype" in L.pm_last_error()
    assert call(out=None) == INVALID and b"out is NULL" in L.pm_last_error()
    assert call(out=64 + 8) == INVALID and b"16-byte aligned" in L.pm_last_error()       # fp32 output: 16 bytes
    assert call(out_dtype=BF16, out=64 + 4) == INVALID and b"8-byte aligned" in L.pm_last_error()
    assert call(stride=4) == INVALID and b"out_row_stride" in L.pm_last_error()          # < max_dim
    assert call(stride=10) == INVALID and b"out_row_stride" in L.pm_last_error()         # not a multiple of 4
    op.per_sample_weights = 8
    assert call() == UNSUPPORTED and b"per_sample_weights" in L.pm_last_error()
    op.per_sample_weights = None
    for field, value in (("table_group", 2), ("grad_block_shift", 2), ("grad_block_extra", 64)):
        setattr(op, field, value)
        if field == "grad_block_extra":
            op.grad_block_shift = 2                                                  # (an extra needs a shift: the request's own rule)
        assert call() == UNSUPPORTED and b"blocked" in L.pm_last_error(), field
        op.table_group = op.grad_block_shift = op.grad_block_extra = 0
    # the empty request: PM_OK without a launch, NULL out allowed with no lookups
    op.num_indices = 0
    assert call(out=None) == _lib.PM_OK
    op.num_indices, op.bag_count = 100, 0
    assert call() == _lib.PM_OK
    op.bag_count = 4
    op.weight_dtype = BF16                                                           # a 16-bit table: dims multiples of 8 ...
    op.max_dim = 12
    assert call(stride=12) == UNSUPPORTED and b"multiple of 8" in L.pm_last_error()


# ---- 4. the gather plan ------------------------------------------------------------------------------------------------------------

SPEC = json.load(open(os.path.join(HERE, "gather_plan_host.json")))


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("gather_plan") / "gather_plan_dump")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "param_amd", "csrc"), os.path.join(HERE, "gather_plan_dump.cpp"), "-o", exe], check=True)

    def run(rows):
        text = "".join(f"{T} {N} {SPEC['shapes'][s]['max_dim']} {SPEC['shapes'][s]['dtype']} {u} {x}\n" for T, N, s, u, x, _ in rows)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(rows)
        return [[int(v) for v in line.split()] for line in out]

    return run


def test_gather_plans_are_the_pinned_ones_and_cover_every_position_once(dump):
    rows = SPEC["rows"]
    got = dump(rows)
    bad = [(r[:5], r[5], g[:-1]) for r, g in zip(rows, got) if g[:-1] != r[5]]
    assert not bad, f"{len(bad)} of {len(rows)} plans differ; the first (case, expected, got): {bad[0]}"
    for r, g in zip(rows, got):
        assert g[-1] == r[1], ("positions covered exactly once", r[:5], g[-1])
        grid, tile = g[SPEC["plan_fields"].index("grid")], g[SPEC["plan_fields"].index("tile")]
        assert (grid - 1) * tile < r[1] <= grid * tile


def test_the_plan_fixture_reaches_every_case_of_the_issue():
    rows = SPEC["rows"]
    assert {r[0] for r in rows} == {1, 3, 1100} and {r[1] for r in rows} == {1, 255, 256, 257, 10000}
    assert {(SPEC["shapes"][r[2]]["max_dim"], SPEC["shapes"][r[2]]["dtype"]) for r in rows} == {(4, 0), (128, 0), (260, 0), (8, 1), (512, 1)}
    plans = [dict(zip(SPEC["plan_fields"], r[5])) for r in rows]
    assert {p["lds_borders"] for p in plans} == {0, 1} and {p["xcd_contiguous"] for p in plans} == {0, 1}
    assert {p["col_passes"] for p in plans} == {1, 2} and {p["unroll"] for p in plans} == {1, 2, 4, 8}
    assert {p["group_lanes"] for p in plans} == {8, 32, 64}
