"""output_dtype on the GPU (``pytest -m gpu``): the bf16 / fp16 forward (``pm_embbag_fwd_out16``) against ``round16`` of the GPU's own fp32
forward and against the numpy restatement of the rule (tests/out16_rules.py), bit for bit; the values where rounding is hard; tiling,
the output burst on and off, batch slices; torch's CPU ``embedding_bag(...).to(dtype)``; the widening kernel (``pm_embbag_grad_widen``)
against ``grad16.float()`` and ``pm_embbag_mean_grad``; every backward route fed a 16-bit gradient against the same route fed the widened
one; autograd of the single-table module; and that modules with the default ``output_dtype`` reach neither new entry point."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from tests import out16_rules as O
from tests import padding_rules as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS, PADS, B0 = (50, 7, 1000), (3, None, 999), 37
NONE3 = (None, None, None)
NEW = ("pm_embbag_fwd_out16", "pm_embbag_grad_widen")
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
WDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    import param_amd

    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    param_amd.load_library()
    param_amd.set_hybrid_min_tiles(0)      # the route tests drive the hybrid kernels with small requests
    yield
    param_amd.set_hybrid_min_tiles()


def _bits(t):
    """the bits of a tensor / array of 4- or 2-byte elements as unsigned integers (numpy)"""
    if isinstance(t, torch.Tensor):
        t = t.detach().contiguous()
        if t.element_size() == 2:
            return t.view(torch.int16).cpu().numpy().view(np.uint16)
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    return np.ascontiguousarray(t, dtype=np.float32).view(np.uint32)


def _model(rows, dims, pads=None, mode="sum", dtype=torch.float32, layout="bd", seed=0, out=None, **kw):
    import param_amd

    kw.setdefault("fused_update", False)
    pads = None if pads is None or all(k is None for k in pads) else list(pads)
    return param_amd.BatchedEmbeddingBagMI355(list(rows), dims, dtype=dtype, device=DEV, init="normal", layout=layout, seed=seed,
                                              padding_idx=pads, pooling_mode=mode, output_dtype=out, **kw)


def _twins(rows, dims, pads, mode, out, **kw):
    """a module with ``output_dtype=out`` and its fp32-output twin (``output_dtype=None``), holding the same weights"""
    m, ref = _model(rows, dims, pads, mode, out=out, **kw), _model(rows, dims, pads, mode, out=None, **kw)
    ref.weights.data.copy_(m.weights.data)
    return m, ref


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype=dtype)


def _split(o, dims, layout):
    """an array in the module's output layout as a list of per-table [bags, D_t] arrays"""
    if layout == "tbd":
        return [o[t] for t in range(len(dims))]
    col = np.concatenate([[0], np.cumsum(dims)])
    return [o[:, col[t]:col[t + 1]] for t in range(len(dims))]


def _check_forward(rows, dims, pads, wdt, out, kind, idt, layout, seed, max_len=9, B=B0, slice_=None, long_bag=None):
    """kind: "sum" | "weighted" | "mean".  The 16-bit output equals round16 of the GPU's fp32 forward of the same request and the
    numpy rule, bit for bit (NaN by class and sign); returns what the checks used"""
    rng = np.random.default_rng(seed)
    T = len(rows)
    dims_l = [dims] * T if isinstance(dims, int) else list(dims)
    mode = "mean" if kind == "mean" else "sum"
    m, ref = _twins(rows, dims_l, pads, mode, out, dtype=wdt, layout=layout, seed=seed)
    assert m.output_dtype == TDT[out] and ref.output_dtype == torch.float32
    if long_bag is None:
        idx_h, off_h = R.padded_request(rng, rows, B, pads, share=0.4, max_len=max_len)
        assert (np.diff(off_h) == 0).any()                                   # some bags are empty
    else:
        idx_h, off_h = long_bag
    psw_h = rng.standard_normal(idx_h.size).astype(np.float32) if kind == "weighted" else None
    idx, off, psw = _dev(idx_h, idt), _dev(off_h, idt), _dev(psw_h)
    got = m.lookup(idx, off, psw, batch=B)
    assert got.dtype == TDT[out] and got.is_contiguous()
    want32 = ref.lookup(idx, off, psw, batch=B)
    assert want32.dtype == torch.float32 and tuple(want32.shape) == tuple(got.shape)
    g = _bits(got)
    assert O.same_bits(g, O.round16(want32.cpu().numpy(), out), out), "round16 of the GPU's fp32 forward"
    tabs = [m.table(t).float().cpu().numpy() for t in range(T)]
    rule = O.forward(tabs, idx_h, off_h, B, pads, out, psw=psw_h, mean=kind == "mean")
    for t, (a, b) in enumerate(zip(_split(g, dims_l, layout), rule)):
        assert O.same_bits(a, b, out), ("rule", t)
    if slice_ is not None:
        b0, nb = slice_
        canvas = torch.full(got.shape, 0x7b7b, dtype=torch.int16, device=DEV).view(TDT[out])
        m.lookup(idx, off, psw, out=canvas, bag_begin=b0, bag_count=nb, batch=B)
        for t, (c, a) in enumerate(zip(_split(_bits(canvas), dims_l, layout), _split(g, dims_l, layout))):
            assert np.array_equal(c[b0:b0 + nb], a[b0:b0 + nb]), ("slice", t)
            assert (c[:b0] == 0x7b7b).all() and (c[b0 + nb:] == 0x7b7b).all(), ("outside the slice", t)
    return m, idx, off, psw, got


# ---- 1. forward equals the rule ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("padded", [False, True], ids=["nopad", "padded"])
@pytest.mark.parametrize("kind", ["sum", "weighted", "mean"])
@pytest.mark.parametrize("out", ["bf16", "fp16"])
@pytest.mark.parametrize("wdt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("dims", [8, 128, 256, (16, 128, 64)], ids=["d8", "d128", "d256", "mixed"])
def test_forward_equals_the_rule(dims, wdt, out, kind, padded):
    """T = 3, rows (50, 7, 1000), B = 37: ragged bags of 0 .. 9 lookups, some empty"""
    case = zlib.crc32(repr((dims, wdt, out, kind, padded)).encode()) % 1000
    _check_forward(ROWS, dims, PADS if padded else NONE3, WDT[wdt], out, kind, torch.int64, "bd", seed=3000 + case)


@pytest.mark.parametrize("out", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["sum", "weighted", "mean"])
def test_forward_int32_indices_and_the_tbd_layout_at_one_shape(kind, out):
    _check_forward(ROWS, 128, PADS, torch.float32, out, kind, torch.int32, "tbd", seed=77, slice_=(5, 11))
    _check_forward(ROWS, 64, NONE3, torch.bfloat16, out, kind, torch.int32, "bd", seed=78)


# ---- 2. rounding really happens where it is hard ------------------------------------------------------------------------------------

# one fp32 table, D = 8, every column of a row the same value; row 15 is the padding row and holds NaN
_HARD_ROWS = [1.0, 2.0 ** -8, 2.0 ** -7, 2.0 ** -11, 2.0 ** -10, 40000.0, 65520.0, 3 * 2.0 ** -24, 2.0 ** -127, 2.0 ** -130,
              -2.0 ** -140, np.inf, -np.inf, -0.0, -1e-45, np.nan]
_PADROW = 15
# bag -> (lookups, {dtype: expected bits} where the value is pinned by name; every bag is also held to the twin, the rule and torch)
_HARD_BAGS = [
    ([0, 1], {"bf16": 0x3f80}),                      # 1 + 2^-8: a bf16 tie, to even DOWN (torch's CPU cast gives the same)
    ([0, 2, 1], {"bf16": 0x3f82}),                   # 1 + 2^-7 + 2^-8: a bf16 tie, to even UP
    ([0, 3], {"fp16": 0x3c00}),                      # 1 + 2^-11: an fp16 tie, down
    ([0, 4, 3], {"fp16": 0x3c02}),                   # 1 + 2^-10 + 2^-11: an fp16 tie, up
    ([5, 5], {"fp16": 0x7c00, "bf16": 0x479c}),      # 80000 > 65520: fp16 overflow to +Inf; bf16 rounds 80000 to 79872
    ([6], {"fp16": 0x7c00}),                         # 65520: the tie between 65504 and 2^16 goes to Inf
    ([7], {"fp16": 0x0003}),                         # an fp16 subnormal result
    ([8], {"bf16": 0x0040, "fp16": 0x0000}),         # an fp32-subnormal input (2^-127): a bf16 subnormal, not flushed
    ([9], {"bf16": 0x0008}),                         # 2^-130: a bf16 subnormal
    ([10], {"bf16": 0x8000, "fp16": 0x8000}),        # -2^-140 rounds to -0.0 in both: the sign of zero is kept
    ([13], {"bf16": 0x0000, "fp16": 0x0000}),        # -0.0 in a bag of one lookup: +0.0 + -0.0 = +0.0, as in the fp32 forward
    ([11, 12], {}),                                  # +Inf + -Inf: NaN
    ([11, 0], {"bf16": 0x7f80, "fp16": 0x7c00}),
    ([_PADROW, 0, _PADROW], {"bf16": 0x3f80, "fp16": 0x3c00}),      # the NaN in the padding row reaches no output
    ([_PADROW, _PADROW], {"bf16": 0x0000, "fp16": 0x0000}),
    ([], {"bf16": 0x0000, "fp16": 0x0000}),
]
_NAN_BAG = 11


@pytest.mark.parametrize("out", ["bf16", "fp16"])
def test_rounding_happens_where_it_is_hard(out):
    import param_amd

    D = 8
    W = np.repeat(np.array(_HARD_ROWS, dtype=np.float32)[:, None], D, axis=1)
    idx_h = np.array(sum((b for b, _ in _HARD_BAGS), []), dtype=np.int64)
    off_h = np.cumsum([0] + [len(b) for b, _ in _HARD_BAGS]).astype(np.int64)
    B = len(_HARD_BAGS)
    m, ref = _twins([len(_HARD_ROWS)], D, [_PADROW], "sum", out)
    for mod in (m, ref):
        mod.table(0).copy_(_dev(W))
    idx, off = _dev(idx_h), _dev(off_h)
    g = _bits(m.lookup(idx, off, batch=B))
    want32 = ref.lookup(idx, off, batch=B).cpu().numpy()
    assert O.same_bits(g, O.round16(want32, out), out)
    with np.errstate(invalid="ignore"):                                      # (+Inf + -Inf on the host)
        rule = O.forward([W], idx_h, off_h, B, [_PADROW], out)[0]
    torch_cast = torch.from_numpy(want32).to(TDT[out]).view(torch.int16).numpy().view(np.uint16)
    rest = np.arange(B) != _NAN_BAG
    assert np.array_equal(g[rest], rule[rest]) and np.array_equal(g[rest], torch_cast[rest])
    assert O.is_nan16(g[_NAN_BAG], out).all() and np.isnan(want32[_NAN_BAG]).all() and not O.is_nan16(g[rest], out).any()
    for b, (_, pinned) in enumerate(_HARD_BAGS):
        if out in pinned:
            assert (g[b] == pinned[out]).all(), (b, [hex(v) for v in g[b]], hex(pinned[out]))
    # mean pooling: (-2^-149 + 0 + 0) / 3 underflows to -0.0 in fp32, and the 16-bit output keeps the sign; 1 / 3 is rounded once
    mm, mref = _twins([len(_HARD_ROWS)], D, [_PADROW], "mean", out)
    W2 = W.copy()
    W2[1] = 0.0
    for mod in (mm, mref):
        mod.table(0).copy_(_dev(W2))
    idx2, off2 = _dev(np.array([14, 1, 1, 0, 1, 1, _PADROW], dtype=np.int64)), _dev(np.array([0, 3, 7], dtype=np.int64))
    g2, w2 = _bits(mm.lookup(idx2, off2, batch=2)), mref.lookup(idx2, off2, batch=2).cpu().numpy()
    assert (_bits(w2[0]) == 0x80000000).all() and (g2[0] == 0x8000).all()
    assert np.array_equal(g2, O.round16(w2, out)) and (g2[1] == O.round16(np.float32(1.0) / np.float32(3.0), out)).all()
    assert param_amd.EmbeddingBagMI355(4, 8, device=DEV, output_dtype=out).output_dtype == TDT[out]


# ---- 3. tiling ------------------------------------------------------------------------------------------------------------------------

def _long_bag_request(rng, rows=7, n=5000):
    long_ = rng.integers(0, rows, n)
    idx_h = np.concatenate([[1, 2, 2], long_, [3, 5, 4, 0]]).astype(np.int64)
    return idx_h, np.array([0, 3, 3 + n, idx_h.size], dtype=np.int64)


@pytest.mark.parametrize("out", ["bf16", "fp16"])
def test_several_tiles_a_bag_longer_than_the_index_tile_the_burst_on_and_off_and_a_slice(out):
    """B = 300, D = 32, fp16 tables, ragged bags of up to 60: several tiles per table, the last one short.  One bag of 5000 lookups
    (the LDS index tile holds at most 4096) between two short ones on a 7-row table: the unstaged walk.  Both with the output burst
    on (default) and off: identical bits.  A batch slice writes only its own bags into a canvas of 0x7b7b."""
    from param_amd import _lib

    rng = np.random.default_rng(13)
    long_rq = _long_bag_request(rng)
    cases = [dict(rows=ROWS, dims=32, pads=PADS, wdt=torch.float16, kind="mean", max_len=60, B=300, slice_=(5, 11), seed=5),
             dict(rows=ROWS, dims=32, pads=NONE3, wdt=torch.float16, kind="weighted", max_len=20, B=100, slice_=(5, 11), seed=5),
             dict(rows=(7,), dims=128, pads=(None,), wdt=torch.float32, kind="sum", B=3, long_bag=long_rq, seed=6),
             dict(rows=(7,), dims=64, pads=(3,), wdt=torch.bfloat16, kind="mean", B=3, long_bag=long_rq, seed=6)]
    for c in cases:
        kw = dict(c)
        args = (kw.pop("rows"), kw.pop("dims"), kw.pop("pads"), kw.pop("wdt"), out, kw.pop("kind"), torch.int64, "bd")
        m, idx, off, psw, burst_on = _check_forward(*args, **kw)
        try:
            _lib.set_forward_tuning(stage_out=0)
            burst_off = m.lookup(idx, off, psw, batch=c["B"])
        finally:
            _lib.set_forward_tuning(stage_out=-1)
        assert np.array_equal(_bits(burst_off), _bits(burst_on)), c
        assert np.array_equal(_bits(m.lookup(idx, off, psw, batch=c["B"])), _bits(burst_on))


# ---- 4. against torch -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("out", ["bf16", "fp16"])
@pytest.mark.parametrize("mode,pad", [("sum", None), ("mean", None), ("sum", 3), ("mean", 3)], ids=["sum", "mean", "sum-padded", "mean-padded"])
def test_fp32_table_equals_torchs_cpu_embedding_bag_cast_to_the_dtype(mode, pad, out):
    import param_amd
    import torch.nn.functional as F

    rng = np.random.default_rng(17)
    n, D, B = 50, 32, 40
    idx_h, off_h = R.padded_request(rng, [n], B, [pad], closed=False)
    m = param_amd.EmbeddingBagMI355(n, D, mode=mode, device=DEV, padding_idx=pad, output_dtype=TDT[out])
    W = m.weight.detach().cpu()
    with torch.no_grad():
        got = m(_dev(idx_h), _dev(off_h))
    want = F.embedding_bag(torch.from_numpy(idx_h), W, torch.from_numpy(off_h), mode=mode, padding_idx=pad).to(TDT[out])
    assert got.dtype == TDT[out] and torch.isfinite(want.float()).all()
    assert np.array_equal(_bits(got), _bits(want))
    # 2-D input: every row a bag
    inp = torch.from_numpy(rng.integers(0, n, (B, 5)))
    with torch.no_grad():
        got2 = m(inp.to(DEV))
    assert np.array_equal(_bits(got2), _bits(F.embedding_bag(inp, W, mode=mode, padding_idx=pad).to(TDT[out])))


def test_fp16_output_is_the_16_bit_quantised_payload():
    """``lookup_quantized(bitwidth=16)`` rows are plain round-to-nearest-even fp16 (csrc/rowquant.hip): on a fixed-pooling request both
    accept, its bytes equal the fp16 ``output_dtype`` bytes"""
    rows, D, B, L = (50, 7, 1000), 64, 64, 5
    m, ref = _twins(rows, D, None, "sum", "fp16", seed=4)
    rng = np.random.default_rng(19)
    idx_h, off_h = R.padded_request(rng, rows, B, NONE3, fixed=L)
    idx, off = _dev(idx_h), _dev(off_h)
    q = ref.lookup_quantized(idx, off, 16, batch=B)
    assert q.dtype == torch.uint8 and tuple(q.shape) == (B, 3, 2 * D)
    got = m.lookup(idx, off, batch=B)
    assert np.array_equal(q.cpu().numpy().reshape(B, -1), got.view(torch.uint8).cpu().numpy().reshape(B, -1))
    with pytest.raises(ValueError, match="output_dtype"):
        m.lookup_quantized(idx, off, 16, batch=B)
    with pytest.raises(ValueError, match="output_dtype"):
        m.lookup(idx, off, batch=B, split_bags=True)


# ---- 5. the widening kernel on its own ----------------------------------------------------------------------------------------------

def _grad16(shape, out, seed):
    """a 16-bit gradient with Inf, -0.0, subnormals and the largest finite value sprinkled in (no NaN: payloads are not part of the rule)"""
    g = torch.randn(shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)).to(TDT[out])
    flat = g.view(-1).view(torch.int16)
    flat[::97] = 0x7f80 if out == "bf16" else 0x7c00
    flat[5::101] = -0x8000
    flat[7::103] = 0x0001
    flat[9::107] = 0x7f7f if out == "bf16" else 0x7bff
    flat[11::109] = -0x8000 + 0x0033
    return g


@pytest.mark.parametrize("layout,dims,idt", [("bd", (16, 128, 64), torch.int64), ("tbd", 8, torch.int32), ("bd", 512, torch.int64)],
                         ids=["bd-mixed", "tbd-d8", "bd-d512"])
@pytest.mark.parametrize("padded", [False, True], ids=["nopad", "padded"])
@pytest.mark.parametrize("out", ["bf16", "fp16"])
def test_grad_widen_equals_the_cast_and_the_mean_scaling_and_a_slice_leaves_the_rest_alone(layout, dims, idt, padded, out):
    from param_amd import _lib
    from param_amd.embedding_bag import _mean_scale, _stream_ptr, _widen

    rng = np.random.default_rng(11)
    pads = PADS if padded else NONE3
    dims_l = [dims] * 3 if isinstance(dims, int) else list(dims)
    m = _model(ROWS, dims_l, pads, "mean", layout=layout, out=out)
    idx_h, off_h = R.padded_request(rng, ROWS, B0, pads, share=0.4, max_len=70)      # bags longer than a lane group, some empty
    idx, off = _dev(idx_h, idt), _dev(off_h, idt)
    shape = (3, B0, dims_l[0]) if layout == "tbd" else (B0, sum(dims_l))
    g16 = _grad16(shape, out, 1)
    keep = g16.clone()
    g32 = g16.float()
    assert np.array_equal(_bits(g32), O.widen(_bits(g16), out).view(np.uint32))      # (torch's widening is the rule's)
    ts, pad_t = m._tables(), m._pad_dev()
    plain = _widen(ts, g16, idx, off, B0, None, pad_t, False)
    assert plain.dtype == torch.float32 and np.array_equal(_bits(plain), _bits(g32))
    scaled = _widen(ts, g16, idx, off, B0, None, pad_t, True)
    assert np.array_equal(_bits(scaled), _bits(_mean_scale(ts, g32, idx, off, B0, pad_t)))
    assert np.array_equal(_bits(g16), _bits(keep))                           # the caller's gradient is never modified
    # a slice: only its bags are written
    b0, nb = 5, 20
    op = ts.request(idx, off, B0, None, b0, nb)
    for mean, full in ((0, plain), (1, scaled)):
        canvas = torch.full(shape, 7.0, device=DEV)
        rc = _lib.load().pm_embbag_grad_widen(ctypes.byref(op), None if pad_t is None else pad_t.data_ptr(), mean, _lib.PM_BF16 if out == "bf16"
                                              else _lib.PM_F16, g16.data_ptr(), canvas.data_ptr(), _stream_ptr())
        assert rc == _lib.PM_OK
        c, w = _bits(canvas), _bits(full)
        for t, (ct, wt) in enumerate(zip(_split(c, dims_l, layout), _split(w, dims_l, layout))):
            assert np.array_equal(ct[b0:b0 + nb], wt[b0:b0 + nb]), (mean, t)
            seven = _bits(np.float32(7.0))
            assert (ct[:b0] == seven).all() and (ct[b0 + nb:] == seven).all(), (mean, t)


# ---- 6. every backward route ----------------------------------------------------------------------------------------------------------

BW_ROWS, BW_PADS, BW_B, BW_L, BW_D = (100_000, 70_000, 100_000), (3, None, 99_999), 1024, 8, 32
_BW = {}


def _bw_request(out):
    """the route tests' request and 16-bit gradient, computed once per dtype and left unchanged"""
    if out not in _BW:
        rng = np.random.default_rng(9)
        idx_h, off_h = R.padded_request(rng, BW_ROWS, BW_B, BW_PADS, share=0.3, fixed=BW_L)
        g16 = torch.randn(BW_B, len(BW_ROWS) * BW_D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)).to(TDT[out])
        psw = torch.randn(idx_h.size, device=DEV, generator=torch.Generator(device=DEV).manual_seed(10))
        _BW[out] = (_dev(idx_h), _dev(off_h), g16, g16.float(), psw)
    return _BW[out]


ROUTES = ["dense_grad", "scatter_add_", "sparse_grad", "adagrad_step_", "optimizer_step_sgd", "optimizer_step_rowwise_adagrad",
          "optimizer_step_adagrad", "fused_backward", "per_sample_weights_grad"]


@pytest.mark.parametrize("padded", [False, True], ids=["nopad", "padded"])
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("route", ROUTES)
def test_every_backward_route_on_a_16_bit_gradient_equals_the_route_on_the_widened_one(route, mode, padded):
    """two identical modules (same weights, same optimizer state): one is handed ``grad16``, the other ``grad16.float()``; tables,
    optimizer state, rows and values come out bit for bit the same.  bf16 and fp16 alternate over the cases."""
    out = ("bf16", "fp16")[(ROUTES.index(route) + (mode == "mean") + padded) % 2]
    idx, off, g16, g32, psw = _bw_request(out)
    keep = g16.clone()
    opt = {"adagrad_step_": "rowwise_adagrad", "optimizer_step_sgd": "sgd", "optimizer_step_rowwise_adagrad": "rowwise_adagrad",
           "optimizer_step_adagrad": "adagrad", "fused_backward": "rowwise_adagrad"}.get(route, "sgd")
    kw = dict(optimizer=opt, learning_rate=0.05, seed=2, fused_update=route == "fused_backward")
    if opt != "sgd":
        kw.update(weight_decay=0.01, weight_decay_mode="l2" if opt == "adagrad" else "decouple")
    pads = BW_PADS if padded else None
    a = _model(BW_ROWS, BW_D, pads, mode, out=out, **kw)
    # (the fused backward runs through autograd, which casts a gradient to the output's dtype: its twin has fp32 output)
    b = _model(BW_ROWS, BW_D, pads, mode, out=None if route == "fused_backward" else out, **kw)
    b.weights.data.copy_(a.weights.data)
    if route == "per_sample_weights_grad" and mode == "mean":      # mean pooling is unweighted: refused for every gradient dtype
        for g in (g16, g32):
            with pytest.raises(ValueError, match="unweighted"):
                a.per_sample_weights_grad(g, idx, off, batch=BW_B)
        return
    if opt != "sgd":
        a.momentum_table(0), b.momentum_table(0)
        a.momentum.uniform_(0.1, 1.0)
        b.momentum.copy_(a.momentum)
    before = a.weights.data.clone()
    w = psw if mode == "sum" and route in ("scatter_add_", "dense_grad", "sparse_grad", "fused_backward") else None
    changed = True
    if route == "dense_grad":
        ga, gb = a.dense_grad(g16, idx, off, w, batch=BW_B), b.dense_grad(g32, idx, off, w, batch=BW_B)
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(ga, gb)) and any(bool(x.any()) for x in ga)
        changed = False
    elif route == "sparse_grad":
        for b0, nb in ((0, None), (5, 200)):
            sa = a.sparse_grad(g16, idx, off, w, batch=BW_B, bag_begin=b0, bag_count=nb)
            sb = b.sparse_grad(g32, idx, off, w, batch=BW_B, bag_begin=b0, bag_count=nb)
            for (ra, va), (rb, vb) in zip(sa, sb):
                assert torch.equal(ra, rb) and np.array_equal(_bits(va), _bits(vb)) and ra.numel() > 0
        changed = False
    elif route == "per_sample_weights_grad":
        pa, pb = a.per_sample_weights_grad(g16, idx, off, batch=BW_B), b.per_sample_weights_grad(g32, idx, off, batch=BW_B)
        assert np.array_equal(_bits(pa), _bits(pb)) and bool(pa.any())
        changed = False
    elif route == "scatter_add_":
        for b0, nb in ((0, None), (5, 200)):
            a.scatter_add_(g16, idx, off, alpha=-0.25, per_sample_weights=w, batch=BW_B, bag_begin=b0, bag_count=nb)
            b.scatter_add_(g32, idx, off, alpha=-0.25, per_sample_weights=w, batch=BW_B, bag_begin=b0, bag_count=nb)
    elif route == "adagrad_step_":
        a.adagrad_step_(g16, idx, off, batch=BW_B)
        b.adagrad_step_(g32, idx, off, batch=BW_B)
    elif route == "fused_backward":
        wa = None if w is None else w.clone().requires_grad_(True)
        wb = None if w is None else w.clone().requires_grad_(True)
        oa, ob = a(idx, off, wa), b(idx, off, wb)
        assert oa.dtype == TDT[out] and ob.dtype == torch.float32 and np.array_equal(_bits(oa), O.round16(ob.detach().cpu().numpy(), out))
        oa.backward(g16)
        ob.backward(g32)
        if w is not None:
            assert np.array_equal(_bits(wa.grad), _bits(wb.grad)) and bool(wa.grad.any())
    else:
        a.optimizer_step_(g16, idx, off, batch=BW_B)
        b.optimizer_step_(g32, idx, off, batch=BW_B)
    assert np.array_equal(_bits(a.weights.data), _bits(b.weights.data))
    assert torch.equal(a.weights.data, before) != changed
    if opt != "sgd":
        assert np.array_equal(_bits(a.momentum), _bits(b.momentum))
    assert np.array_equal(_bits(g16), _bits(keep))                           # the caller's gradient is never modified
    with pytest.raises(ValueError, match="grad must be float32 or"):
        a.dense_grad(g16.to(torch.float16 if out == "bf16" else torch.bfloat16), idx, off, batch=BW_B)


def test_1100_tables_one_widening_launch_around_the_table_chunks(monkeypatch):
    from param_amd import _lib

    T, n, D, B, L = 1100, 16, 8, 4, 3
    rows = [n] * T
    pads = [1 if t % 3 else None for t in range(T)]
    rng = np.random.default_rng(51)
    idx_h, off_h = R.padded_request(rng, rows, B, pads, fixed=L)
    idx, off = _dev(idx_h), _dev(off_h)
    g16 = torch.randn(B, T * D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)).to(torch.bfloat16)
    a = _model(rows, D, pads, "mean", out="bf16", learning_rate=0.1, seed=6)
    b = _model(rows, D, pads, "mean", out="bf16", learning_rate=0.1, seed=6)
    assert np.array_equal(_bits(a.lookup(idx, off, batch=B)), O.round16(_model(rows, D, pads, "mean", seed=6).lookup(idx, off, batch=B).cpu().numpy(), "bf16"))
    real, calls = _lib.load(), []

    class Counting:      # counts CALLS (the chunk loop fetches an entry point once and calls it per table range)
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name not in NEW + ("pm_embbag_bwd_fused", "pm_embbag_mean_grad"):
                return fn
            return lambda *args: (calls.append(name), fn(*args))[1]

    monkeypatch.setattr(_lib, "load", lambda: Counting())
    a.optimizer_step_(g16, idx, off, batch=B)
    assert calls.count("pm_embbag_grad_widen") == 1 and calls.count("pm_embbag_bwd_fused") == 2 and "pm_embbag_mean_grad" not in calls, calls
    b.optimizer_step_(g16.float(), idx, off, batch=B)
    assert calls.count("pm_embbag_grad_widen") == 1 and calls.count("pm_embbag_mean_grad") == 1
    assert np.array_equal(_bits(a.weights.data), _bits(b.weights.data))


# ---- 7. autograd of the single-table module -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("mode,pad,weighted", [("sum", None, False), ("sum", 7, True), ("mean", 7, False)], ids=["sum", "sum-padded-weighted", "mean-padded"])
def test_single_table_autograd_returns_and_receives_bf16(sparse, mode, pad, weighted):
    import param_amd

    rng = np.random.default_rng(41)
    n, D, B = 60, 32, 50
    idx_h, off_h = R.padded_request(rng, [n], B, [pad], closed=False)
    idx, off = _dev(idx_h), _dev(off_h)
    g16 = _grad16((B, D), "bf16", 3)
    keep = g16.clone()
    m = param_amd.EmbeddingBagMI355(n, D, mode=mode, device=DEV, sparse=sparse, padding_idx=pad, output_dtype=torch.bfloat16)
    ref = param_amd.EmbeddingBagMI355(n, D, mode=mode, device=DEV, sparse=sparse, padding_idx=pad, _weight=m.weight.detach().clone())
    psw = torch.randn(idx.numel(), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4)) if weighted else None
    pa = None if psw is None else psw.clone().requires_grad_(True)
    pb = None if psw is None else psw.clone().requires_grad_(True)
    out, out32 = m(idx, off, pa), ref(idx, off, pb)
    assert out.dtype == torch.bfloat16 and out32.dtype == torch.float32 and out.requires_grad
    assert np.array_equal(_bits(out), O.round16(out32.detach().cpu().numpy(), "bf16"))
    out.backward(g16)
    out32.backward(g16.float())
    assert np.array_equal(_bits(g16), _bits(keep))
    ga, gb = m.weight.grad, ref.weight.grad
    if sparse:
        assert ga.is_sparse and ga.is_coalesced() and torch.equal(ga._indices(), gb._indices())
        assert np.array_equal(_bits(ga._values()), _bits(gb._values())) and ga._values().numel() > 0
    else:
        assert np.array_equal(_bits(ga), _bits(gb)) and bool(torch.nan_to_num(ga).any())
    if weighted:
        assert pa.grad.dtype == torch.float32 and np.array_equal(_bits(pa.grad), _bits(pb.grad)) and bool(torch.nan_to_num(pa.grad).any())
    # an fp32 gradient is taken too (autograd casts to the output's dtype itself; the module's own entry points take fp32 as before)
    with torch.no_grad():
        assert m(idx, off).dtype == torch.bfloat16


# ---- 8. the default path --------------------------------------------------------------------------------------------------------------

def test_default_modules_reach_neither_new_entry_point(monkeypatch):
    import param_amd
    from param_amd import _lib

    real = _lib.load()
    calls = []

    class Raising:
        def __getattr__(self, name):
            if name in NEW:
                calls.append(name)
                raise AssertionError(f"{name} reached from a module with the default output_dtype")
            return getattr(real, name)

    monkeypatch.setattr(_lib, "load", lambda: Raising())
    rng = np.random.default_rng(71)
    idx_h, off_h = R.padded_request(rng, ROWS, B0, PADS)
    idx, off = _dev(idx_h), _dev(off_h)
    psw = torch.randn(idx.numel(), device=DEV).requires_grad_(True)
    grad = torch.randn(B0, 48, device=DEV)
    for spec in (None, "fp32"):
        for opt in ("sgd", "rowwise_adagrad", "adagrad"):
            for pads, mode in ((None, "sum"), (PADS, "sum"), (PADS, "mean")):
                m = _model(ROWS, 16, pads, mode, optimizer=opt, fused_update=True, out=spec)
                w = psw if mode == "sum" else None
                out = m(idx, off, w)
                assert out.dtype == torch.float32
                out.backward(grad)
                m.lookup(idx, off)
                m.dense_grad(grad, idx, off)
                m.sparse_grad(grad, idx, off)
                if mode == "sum":
                    m.per_sample_weights_grad(grad, idx, off)
    for sparse in (False, True):
        for mode in ("sum", "mean"):
            sm = param_amd.EmbeddingBagMI355(50, 16, mode=mode, device=DEV, sparse=sparse, padding_idx=3)
            sm(idx[:off_h[B0]], off[:B0]).backward(grad[:, :16])
            sm(torch.randint(0, 50, (8, 5), device=DEV)).sum().backward()
    torch.cuda.synchronize()
    assert calls == []
    # ... and a 16-bit module does reach them
    seen = []

    class Counting:
        def __getattr__(self, name):
            if name in NEW:
                seen.append(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "load", lambda: Counting())
    p = _model(ROWS, 16, PADS, "sum", fused_update=True, out="fp16")
    p(idx, off).backward(grad.to(torch.float16))
    assert set(seen) == set(NEW)
