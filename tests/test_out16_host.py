"""output_dtype, the parts that need no GPU: the numpy restatement of the rounding (tests/out16_rules.py) against torch's CPU casts, bit
for bit on every non-NaN input listed below and by class and sign on NaNs; what the two modules accept and refuse at construction
(``device="cpu"``: nothing is launched); the two new entry points in the header, the binding and both libraries, with the ABI version
and the request struct where they were; their host-side refusals."""
import ctypes
import enum
import os

import numpy as np
import pytest
import torch

import param_amd
from param_amd import _lib
from param_amd.embedding_bag import _output_dtype
from tests import out16_rules as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _torch_round(x32, dtype):
    """torch's CPU cast of an fp32 array, as uint16 bits"""
    return torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(TDT[dtype]).view(torch.int16).numpy().view(np.uint16)


def _check_against_torch(x32, dtype):
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    got, want = O.round16(x32, dtype), _torch_round(x32, dtype)
    nan = np.isnan(x32)
    assert np.array_equal(got[~nan], want[~nan])
    assert not O.is_nan16(got[~nan], dtype).any()
    # NaN: NaN-ness and sign only (torch's own casts do not agree with each other on the payload)
    assert O.is_nan16(got[nan], dtype).all() and O.is_nan16(want[nan], dtype).all()
    assert np.array_equal(got[nan] >> 15, (x32[nan].view(np.uint32) >> 31).astype(np.uint16))
    return got


# ---- round16 / widen against torch ------------------------------------------------------------------------------------------------

def test_bf16_rounding_is_torchs_on_every_upper_half():
    hi = np.arange(65536, dtype=np.uint32) << 16
    for lo in (0, 1, 0x7fff, 0x8000, 0x8001, 0xffff):
        x = (hi | np.uint32(lo)).view(np.float32)
        got = _check_against_torch(x, "bf16")
        if lo == 0:
            assert np.array_equal(got[~np.isnan(x)], (hi >> 16).astype(np.uint16)[~np.isnan(x)])      # representable: unchanged
    # the ties of the GPU test, as torch's CPU cast gives them: to even in both directions
    ties = np.array([1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8], dtype=np.float32)
    assert O.round16(ties, "bf16").tolist() == _torch_round(ties, "bf16").tolist() == [0x3f80, 0x3f82]
    # the NaN convention of the kernels: (u >> 16) | 0x40
    u = np.array([0x7f800001, 0xff800001, 0x7fc12345, 0xffffffff], dtype=np.uint32)
    assert O.round16(u.view(np.float32), "bf16").tolist() == [0x7fc0, 0xffc0, 0x7fc1, 0xffff]


def test_fp16_rounding_is_torchs_on_every_value_its_neighbours_and_the_midpoints():
    pat = np.arange(65536, dtype=np.uint16)
    val = O.widen(pat, "fp16")
    fin = np.isfinite(val)
    xs = [val]
    with np.errstate(all="ignore"):
        xs.append(np.nextafter(val, np.float32(np.inf), dtype=np.float32))
        xs.append(np.nextafter(val, np.float32(-np.inf), dtype=np.float32))
    # the midpoint between every finite fp16 value and the next pattern of its sign (the largest: towards 65536, i.e. +-65520)
    nxt = O.widen(pat[fin] + np.uint16(1), "fp16").astype(np.float64)         # (finite patterns end at 0x7bff / 0xfbff: no wrap)
    nxt = np.where(np.isinf(nxt), np.where(np.signbit(nxt), -65536.0, 65536.0), nxt)
    mid64 = (val[fin].astype(np.float64) + nxt) / 2
    mid = mid64.astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), mid64)                      # every midpoint is an fp32 value
    xs.append(mid)
    big = np.finfo(np.float32).max
    xs.append(np.array([65504.0, 65520.0, -65520.0, 2.0 ** -24, 2.0 ** -25, -2.0 ** -25, big, -big, 65519.996, 65520.004,
                        2.0 ** -25 * (1 + 2.0 ** -23), 2.0 ** -126, 1e-45, -0.0, 0.0], dtype=np.float32))
    for x in xs:
        _check_against_torch(x, "fp16")
    r = lambda v: int(O.round16(np.array([v], dtype=np.float32), "fp16")[0])      # noqa: E731
    assert r(65504.0) == 0x7bff and r(65520.0) == 0x7c00 and r(65519.996) == 0x7bff and r(big) == 0x7c00 and r(-big) == 0xfc00
    assert r(2.0 ** -24) == 0x0001 and r(2.0 ** -25) == 0x0000 and r(2.0 ** -25 * (1 + 2.0 ** -23)) == 0x0001      # tie to even: zero
    assert r(-0.0) == 0x8000 and r(-2.0 ** -25) == 0x8000 and r(2.0 ** -126) == 0 and r(3 * 2.0 ** -25) == 0x0002


@pytest.mark.parametrize("dtype", O.DTYPES)
def test_widen_then_round_is_the_identity_on_every_pattern(dtype):
    pat = np.arange(65536, dtype=np.uint16)
    val = O.widen(pat, dtype)
    want = torch.from_numpy(pat.view(np.int16).copy()).view(TDT[dtype]).float().numpy()
    nan = O.is_nan16(pat, dtype)
    assert np.array_equal(val.view(np.uint32)[~nan], want.view(np.uint32)[~nan]) and np.isnan(val[nan]).all() and np.isnan(want[nan]).all()
    assert nan.sum() == (2 * 0x7f if dtype == "bf16" else 2 * 0x3ff)
    back = O.round16(val, dtype)
    assert np.array_equal(back[~nan], pat[~nan]) and O.same_bits(back, pat, dtype)
    assert not O.same_bits(back ^ np.uint16(0x8000), pat, dtype)              # (same_bits does look at a NaN's sign)


def test_forward_rule_is_the_fp32_rule_rounded_once():
    from tests import mean_rules as M
    from tests import padding_rules as R

    rng = np.random.default_rng(3)
    rows, pads, B = [9, 4, 30], [2, None, 29], 6
    idx, off = R.padded_request(rng, rows, B, pads)
    W = [rng.standard_normal((r, 8)).astype(np.float32) for r in rows]
    psw = rng.standard_normal(idx.size).astype(np.float32)
    for dtype in O.DTYPES:
        for got, want in ((O.forward(W, idx, off, B, pads, dtype), R.forward(W, idx, off, B, pads)),
                          (O.forward(W, idx, off, B, pads, dtype, psw=psw), R.forward(W, idx, off, B, pads, psw)),
                          (O.forward(W, idx, off, B, pads, dtype, mean=True, bag_begin=2, bag_count=3),
                           M.forward(W, idx, off, B, pads, 2, 3))):
            assert all(np.array_equal(g, _torch_round(w, dtype)) for g, w in zip(got, want))


# ---- constructors (device="cpu": nothing is launched) ---------------------------------------------------------------------------

class _SparseType(enum.Enum):      # fbgemm_gpu's enum, by shape
    FP32 = "fp32"
    FP16 = "fp16"
    BF16 = "bf16"
    INT8 = "int8"


class _ByName(enum.IntEnum):       # an enum whose names, not values, say it
    FP32 = 0
    FP16 = 1
    BF16 = 2
    INT4 = 3


SPELLINGS = [(None, torch.float32), (torch.float32, torch.float32), ("fp32", torch.float32), ("FP32", torch.float32),
             (_SparseType.FP32, torch.float32), (_ByName.FP32, torch.float32),
             (torch.bfloat16, torch.bfloat16), ("bf16", torch.bfloat16), ("BF16", torch.bfloat16), ("Bf16", torch.bfloat16),
             (_SparseType.BF16, torch.bfloat16), (_ByName.BF16, torch.bfloat16),
             (torch.float16, torch.float16), ("fp16", torch.float16), ("FP16", torch.float16), (_SparseType.FP16, torch.float16),
             (_ByName.FP16, torch.float16)]
BAD = ["int8", "float16", "half", "", 16, 1, 0, True, 1.0, torch.float64, torch.int8, torch.uint8, _SparseType.INT8, _ByName.INT4,
       (torch.bfloat16,), b"bf16"]


def test_every_spelling_on_both_modules():
    for spec, want in SPELLINGS:
        assert _output_dtype(spec) == want
        one = param_amd.EmbeddingBagMI355(10, 8, device="cpu", output_dtype=spec)
        many = param_amd.BatchedEmbeddingBagMI355([50, 7], 8, device="cpu", init=None, output_dtype=spec)
        for m in (one, many):
            assert m.output_dtype == want and m._out16 == (None if want == torch.float32 else want)
            assert (f"output_dtype={want}" in repr(m)) == (want != torch.float32) and ("output_dtype" in m.extra_repr()) == (want != torch.float32)
    assert param_amd.EmbeddingBagMI355(10, 8, device="cpu").output_dtype == torch.float32
    assert "output_dtype=torch.bfloat16" in repr(param_amd.EmbeddingBagMI355(10, 8, mode="mean", device="cpu", output_dtype="bf16"))


def test_bad_values_and_the_blocked_layout_are_refused():
    for bad in BAD:
        with pytest.raises(ValueError, match="output_dtype"):
            param_amd.EmbeddingBagMI355(10, 8, device="cpu", output_dtype=bad)
        with pytest.raises(ValueError, match="output_dtype"):
            param_amd.BatchedEmbeddingBagMI355([50, 7], 8, device="cpu", init=None, output_dtype=bad)
    with pytest.raises(ValueError, match="output_dtype"):                    # validated before anything is allocated
        param_amd.BatchedEmbeddingBagMI355([2 ** 40], 2 ** 20, device="cpu", init=None, output_dtype="int8")
    with pytest.raises(ValueError, match="output_dtype"):
        param_amd.EmbeddingBagMI355(2 ** 40, 2 ** 20, device="cpu", output_dtype="int8")
    mk = lambda **kw: param_amd.BatchedEmbeddingBagMI355([64, 64], 8, device="cpu", init=None, **kw)      # noqa: E731
    for spec in ("bf16", torch.float16):
        with pytest.raises(ValueError, match="output_dtype.*blocked"):
            mk(layout="blocked", block_bags=4, output_dtype=spec)
    assert mk(layout="blocked", block_bags=4, output_dtype="fp32").output_dtype == torch.float32      # fp32 stays what it was
    m = mk(output_dtype="bf16")
    i, o = torch.zeros(6, dtype=torch.int64), torch.arange(5, dtype=torch.int64)
    with pytest.raises(ValueError, match="output_dtype"):
        m.lookup(i, o, split_bags=True, batch=2)
    with pytest.raises(ValueError, match="output_dtype"):
        m.lookup_quantized(i, o, 16, batch=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.lookup(i, o, batch=2)                                              # a sound request gets as far as the device check


# ---- library surface ----------------------------------------------------------------------------------------------------------

NEW = ("pm_embbag_fwd_out16", "pm_embbag_grad_widen")


def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "param_amd.h")).read()
    assert "OUTPUT DTYPE" in header
    for lib in (_lib.load(), _lib.load_alternates()):
        for name in NEW:
            assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS and name + "(" in header
        assert lib.pm_abi_version() == 8
    assert _lib.PM_ABI_VERSION == 8 and "#define PM_ABI_VERSION 8" in header
    assert ctypes.sizeof(_lib.pm_embbag_batch) == 144
    mk = open(os.path.join(ROOT, "param_amd", "csrc", "Makefile")).read()
    assert all(f in mk for f in ("grad_widen.hip", "embbag_fwd_out16_f32.hip", "embbag_fwd_out16_bf16.hip", "embbag_fwd_out16_f16.hip"))


def _op():
    op = _lib.pm_embbag_batch()
    op.num_tables, op.weight_dtype, op.index_dtype, op.max_dim = 1, _lib.PM_F32, _lib.PM_I64, 8
    op.tables = op.rows = op.dims = op.out_offsets = 16                      # non-null dummies, never dereferenced on the host
    op.batch, op.bag_count, op.num_indices, op.indices, op.offsets = 4, 4, 8, 16, 16
    return op


def test_fwd_out16_refusals_answer_before_a_hip_call():
    L = _lib.load()
    BF, F16, F32 = _lib.PM_BF16, _lib.PM_F16, _lib.PM_F32
    assert L.pm_embbag_fwd_out16(None, None, 0, BF, 16, None) == _lib.PM_ERR_INVALID
    op = _op()
    ref = ctypes.byref(op)
    for bad in (F32, 99):
        assert L.pm_embbag_fwd_out16(ref, None, 0, bad, 16, None) == _lib.PM_ERR_INVALID
        msg = L.pm_last_error()
        assert b"out_dtype" in msg and all(n in msg for n in (b"pm_embbag_fwd,", b"pm_embbag_fwd_padded", b"pm_embbag_fwd_mean"))
    assert L.pm_embbag_fwd_out16(ref, None, 2, BF, 16, None) == _lib.PM_ERR_INVALID and b"mean" in L.pm_last_error()
    assert L.pm_embbag_fwd_out16(ref, None, 0, BF, None, None) == _lib.PM_ERR_INVALID and b"out is NULL" in L.pm_last_error()
    assert L.pm_embbag_fwd_out16(ref, None, 1, F16, 20, None) == _lib.PM_ERR_INVALID and b"aligned" in L.pm_last_error()
    op.per_sample_weights = 16
    assert L.pm_embbag_fwd_out16(ref, None, 1, BF, 16, None) == _lib.PM_ERR_UNSUPPORTED and b"unweighted" in L.pm_last_error()
    op.per_sample_weights = None
    op.table_group = 2                                                       # the blocked forward's request
    assert L.pm_embbag_fwd_out16(ref, None, 0, BF, 16, None) == _lib.PM_ERR_UNSUPPORTED and b"blocked" in L.pm_last_error()
    op.table_group, op.grad_block_shift, op.grad_block_extra = 0, 1, 64      # the blocked gradient
    assert L.pm_embbag_fwd_out16(ref, None, 0, F16, 16, None) == _lib.PM_ERR_UNSUPPORTED and b"blocked" in L.pm_last_error()
    op.grad_block_shift, op.grad_block_extra = 0, 0
    op.weight_dtype = 7
    assert L.pm_embbag_fwd_out16(ref, None, 0, BF, 16, None) == _lib.PM_ERR_INVALID and b"dtype" in L.pm_last_error()
    op.weight_dtype, op.batch, op.bag_count = _lib.PM_F32, 0, 0
    for mean in (0, 1):
        assert L.pm_embbag_fwd_out16(ref, None, mean, BF, None, None) == _lib.PM_OK      # no bags: nothing is launched, no device needed
    assert L.pm_embbag_fwd_out16(ref, None, 0, F32, None, None) == _lib.PM_ERR_INVALID     # ... but fp32 is refused even then


def test_grad_widen_refusals_answer_before_a_hip_call():
    L = _lib.load()
    BF, F16, F32 = _lib.PM_BF16, _lib.PM_F16, _lib.PM_F32
    assert L.pm_embbag_grad_widen(None, None, 0, BF, 16, 32, None) == _lib.PM_ERR_INVALID
    op = _op()
    ref = ctypes.byref(op)
    for bad in (F32, 99):
        assert L.pm_embbag_grad_widen(ref, None, 0, bad, 16, 32, None) == _lib.PM_ERR_INVALID and b"grad_dtype" in L.pm_last_error()
    assert L.pm_embbag_grad_widen(ref, None, -1, BF, 16, 32, None) == _lib.PM_ERR_INVALID and b"mean" in L.pm_last_error()
    assert L.pm_embbag_grad_widen(ref, None, 0, BF, None, 32, None) == _lib.PM_ERR_INVALID and b"NULL" in L.pm_last_error()
    assert L.pm_embbag_grad_widen(ref, None, 1, F16, 16, None, None) == _lib.PM_ERR_INVALID and b"NULL" in L.pm_last_error()
    assert L.pm_embbag_grad_widen(ref, None, 0, BF, 20, 32, None) == _lib.PM_ERR_INVALID and b"aligned" in L.pm_last_error()
    assert L.pm_embbag_grad_widen(ref, None, 0, BF, 16, 24, None) == _lib.PM_ERR_INVALID and b"aligned" in L.pm_last_error()
    assert L.pm_embbag_grad_widen(ref, None, 0, BF, 32, 32, None) == _lib.PM_ERR_INVALID and b"in place" in L.pm_last_error()
    op.per_sample_weights = 16
    assert L.pm_embbag_grad_widen(ref, None, 1, BF, 16, 32, None) == _lib.PM_ERR_UNSUPPORTED and b"unweighted" in L.pm_last_error()
    op.per_sample_weights = None
    op.table_group = 2
    assert L.pm_embbag_grad_widen(ref, None, 0, BF, 16, 32, None) == _lib.PM_ERR_UNSUPPORTED and b"blocked" in L.pm_last_error()
    op.table_group, op.grad_block_shift, op.grad_block_extra = 0, 1, 64
    assert L.pm_embbag_grad_widen(ref, None, 1, F16, 16, 32, None) == _lib.PM_ERR_UNSUPPORTED and b"blocked" in L.pm_last_error()
    op.grad_block_shift, op.grad_block_extra = 0, 0
    op.weight_dtype = 7
    assert L.pm_embbag_grad_widen(ref, None, 0, BF, 16, 32, None) == _lib.PM_ERR_INVALID and b"dtype" in L.pm_last_error()
    op.weight_dtype, op.batch, op.bag_count = _lib.PM_F32, 0, 0
    for mean in (0, 1):
        assert L.pm_embbag_grad_widen(ref, None, mean, F16, None, None, None) == _lib.PM_OK


# ---- the host layer, with the library replaced by a recorder ----------------------------------------------------------------------

class _Rec:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append((name, a))
            return 64 if name.endswith(("_workspace", "_bytes", "_scratch")) else 0
        return fn


@pytest.fixture
def rec(monkeypatch):
    from param_amd import embedding_bag as eb

    r = _Rec()
    monkeypatch.setattr(eb, "_require_device", lambda t, what: None)
    monkeypatch.setattr(eb, "_stream_ptr", lambda: 0)
    monkeypatch.setattr(_lib, "load", lambda: r)
    return r


def test_the_host_layer_routes_a_16_bit_module_through_the_new_entry_points(rec):
    T, B, L, D = 3, 4, 2, 8
    idx, off = torch.zeros(T * B * L, dtype=torch.int64), torch.arange(T * B + 1, dtype=torch.int64) * L
    m = param_amd.BatchedEmbeddingBagMI355([50, 7, 20], D, device="cpu", init=None, fused_update=False, pooling_mode="mean",
                                           padding_idx=1, output_dtype="bf16")
    out = m.lookup(idx, off)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (B, T * D)
    (name, a), = rec.calls
    assert name == "pm_embbag_fwd_out16" and a[2:4] == (1, _lib.PM_BF16) and a[1] == m._pad_dev().data_ptr() and a[4] == out.data_ptr()
    with pytest.raises(ValueError, match="bfloat16"):
        m.lookup(idx, off, out=torch.empty(B, T * D))                       # an fp32 canvas is refused by a bf16 module
    # a bf16 gradient: ONE widening launch (mean fused), then the fp32 chain on the scratch; the caller's tensor is not the one passed on
    rec.calls.clear()
    g16 = torch.zeros(B, T * D, dtype=torch.bfloat16)
    m.scatter_add_(g16, idx, off, alpha=-0.1)
    names = [n for n, _ in rec.calls]
    assert names.count("pm_embbag_grad_widen") == 1 and "pm_embbag_mean_grad" not in names and names[0] == "pm_embbag_grad_widen"
    w = rec.calls[0][1]
    assert w[2:4] == (1, _lib.PM_BF16) and w[4] == g16.data_ptr()
    fused = [a for n, a in rec.calls if n == "pm_embbag_bwd_fused"]
    assert len(fused) == 1 and fused[0][1] == w[5] != g16.data_ptr()
    # an fp32 gradient is always taken, as before: the mean scaling, no widening
    rec.calls.clear()
    m.scatter_add_(torch.zeros(B, T * D), idx, off, alpha=-0.1)
    names = [n for n, _ in rec.calls]
    assert "pm_embbag_grad_widen" not in names and names.count("pm_embbag_mean_grad") == 1
    # any other dtype raises, and a default module keeps refusing 16 bits with its old text
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        m.scatter_add_(torch.zeros(B, T * D, dtype=torch.float16), idx, off, alpha=-0.1)
    d = param_amd.BatchedEmbeddingBagMI355([50, 7, 20], D, device="cpu", init=None, fused_update=False)
    with pytest.raises(ValueError, match=r"^grad must be float32 of shape \(4, 24\)$"):
        d.scatter_add_(g16, idx, off, alpha=-0.1)
    rec.calls.clear()
    assert d.lookup(idx, off).dtype == torch.float32 and [n for n, _ in rec.calls] == ["pm_embbag_fwd"]
