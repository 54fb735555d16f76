"""Scaled FP8 tables without a device: the rule (tests/f8s_rules.py) against torch's CPU engine, live and through the committed fixture
(tests/golden/f8s_cases.npz, written by tests/golden/gen_f8s_cases.py); what the five C calls and the constructors refuse; the symbols;
and that a module without a scale reaches none of the new calls."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from param_amd import _lib
from tests import f8_rules as R
from tests import f8s_rules as S
from tests.qrows_rules import same_f32
from tests.test_f8_host import _request

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "f8s_cases.npz")
DTYPES = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
NEW = ("pm_f8_row_exponents", "pm_rows_quantize_f8", "pm_embbag_fwd_f8_scaled", "pm_embbag_f8_scaled_plan", "pm_embedding_gather_f8_scaled")
KINDS = ("row", "table")


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


def _exps(fx, fmt, kind):
    e = fx[f"rowexp_{fmt}"].astype(np.int64)
    return (None, e) if kind == "row" else (int(e[:10].max()), None)


# ---- the quantiser's rule ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", S.FORMATS)
def test_cast_is_torchs_cast(fmt):
    """every code's value, every midpoint between neighbouring codes, their fp32 neighbours, the edges above fmax, and random bits"""
    vals = R.dec(np.arange(256, dtype=np.uint8), fmt)
    fin = np.sort(vals[np.isfinite(vals)].astype(np.float64))
    pts = np.concatenate([fin, (fin[1:] + fin[:-1]) / 2, [464, 480, 61440, 65536, -464, -480, -61440, -65536, 1e-45, 1e-39]]).astype(np.float32)
    pts = np.concatenate([pts, np.nextafter(pts, np.float32(np.inf)), np.nextafter(pts, np.float32(-np.inf)),
                          np.float32([np.inf, -np.inf, np.nan, 0.0, -0.0])])
    rng = np.random.default_rng(1)
    y = np.concatenate([pts, rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                        (rng.standard_normal(100000) * S.FMAX[fmt]).astype(np.float32)])
    want = torch.from_numpy(y).to(DTYPES[fmt]).view(torch.uint8).numpy()
    got = S.cast(y, fmt)
    assert S.same_codes(got, want, fmt)
    assert got[y == 0].tolist() == want[y == 0].tolist() and 0x80 in got[y == 0], "a zero keeps its sign"
    fmax = np.float32(S.FMAX[fmt])
    assert S.cast(np.float32([fmax]), fmt)[0] == S._MAXCODE[fmt] and not np.isfinite(R.dec(S.cast(np.float32([np.inf]), fmt), fmt)).any()


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_quantiser_rule_equals_the_fixture_and_torch_live(fmt, fixture):
    x, k = fixture[f"src_{fmt}"], S.FMAX_EXP[fmt]
    e = S.row_exponents(x, fmt)
    assert e.dtype == np.int8 and np.array_equal(e, fixture[f"rowexp_{fmt}"])
    # the exponent is the smallest at which the row does not overflow (where the clamp leaves a choice)
    amax = np.where(np.isfinite(x), np.abs(x), 0).max(axis=1).astype(np.float64)
    assert (e[amax == 0] == -64).all() and e[11] == -64 and e[12] == 64 and e[13] == -64 and e[7] == e[6] + 1
    free = (e > -64) & (e < 64)
    assert (amax[free] <= S.FMAX[fmt] * np.exp2(e[free].astype(np.float64))).all() and (amax[free] > S.FMAX[fmt] * np.exp2(e[free] - 1.0)).all()
    assert 2.0 ** k * 1.75 == S.FMAX[fmt]
    for kind in KINDS:
        E, er = _exps(fixture, fmt, kind)
        s = er if E is None else np.full(x.shape[0], E)
        codes = S.quantize(x, fmt, s)
        live = torch.ldexp(torch.from_numpy(x), -torch.from_numpy(s.astype(np.int32))[:, None]).to(DTYPES[fmt]).view(torch.uint8).numpy()
        assert S.same_codes(codes, fixture[f"codes_{kind}_{fmt}"], fmt) and S.same_codes(codes, live, fmt), (fmt, kind)
        if kind == "row":       # a finite element never overflows at its row's exponent
            fin = np.isfinite(x)
            assert np.isfinite(R.dec(codes, fmt)[fin & (e < 64)[:, None]]).all()
            assert not np.isfinite(R.dec(codes, fmt)[~fin]).any()
        assert same_f32(S.dequant(codes, fmt, E, er)[:10], fixture[f"deq_{kind}_{fmt}"][:10])
    # the reason for all this: the uniform init of 10 M rows is all zeros under the plain e4m3fn cast, and survives with a scale
    plain = torch.from_numpy(x[:3]).to(DTYPES[fmt]).to(torch.float32).numpy()
    scaled = S.dequant(S.quantize(x[:3], fmt, e[:3]), fmt, None, e[:3])
    rel = lambda a: np.abs(a - x[:3]).sum() / np.abs(x[:3]).sum()      # noqa: E731
    assert rel(scaled) < (0.04 if fmt == "e4m3" else 0.08)
    if fmt == "e4m3":
        assert not plain.any() and rel(plain) == 1.0


# ---- the lookups' rule -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", S.FORMATS)
def test_lookup_rules_equal_the_fixture_and_torch_live(fmt, kind, fixture):
    tag = f"{kind}_{fmt}"
    codes, idx, off, psw, pad = fixture[f"codes_{tag}"], fixture["indices"], fixture["offsets"], fixture["psw"], int(fixture["pad"])
    exps = [_exps(fixture, fmt, kind)]
    W = torch.from_numpy(S.dequant(codes[:10], fmt, exps[0][0], None if exps[0][1] is None else exps[0][1][:10]))
    assert same_f32(W.numpy(), fixture[f"deq_{tag}"][:10])
    B, ti, to = off.size, torch.from_numpy(idx), torch.from_numpy(off)
    for name, weighted, padded, mean in (("sum", False, False, False), ("sum_pad", False, True, False), ("weighted", True, False, False),
                                         ("mean", False, False, True), ("mean_pad", False, True, True)):
        got = S.forward([codes], fmt, exps, idx, off, B, [pad] if padded else None, psw if weighted else None, mean)[0]
        live = F.embedding_bag(ti, W, to, mode="mean" if mean else "sum", per_sample_weights=torch.from_numpy(psw) if weighted else None,
                               padding_idx=pad if padded else None).numpy()
        assert same_f32(got, fixture[f"{name}_{tag}"]) and same_f32(got, live), (fmt, kind, name)
        assert not got[1].any() and not np.signbit(got[1]).any(), "an empty bag is +0.0"
        if padded:
            assert not got[4].any() and not np.signbit(got[4]).any(), "an all-padding bag is +0.0"
        if name in ("sum", "mean_pad"):
            for d16 in ("bf16", "fp16"):
                assert S.same16(S.round16(got, d16), fixture[f"{name}_{d16}_{tag}"], d16), (fmt, kind, name, d16)
    rows, written = S.sequence([codes], fmt, exps, np.arange(14), np.zeros(1, dtype=np.int64), 1)
    assert written.all() and same_f32(rows, fixture[f"rows_{tag}"])
    assert same_f32(rows[:10], F.embedding(torch.arange(10), W).numpy())
    assert rows[8].view(np.uint32)[1] == 0x80000000 and rows[8].view(np.uint32)[0] == 0, "-0.0 is stored and leaves as -0.0"


def test_every_code_is_exact_and_normal_at_every_exponent():
    for fmt in S.FORMATS:
        codes = np.tile(np.arange(256, dtype=np.uint8), (129, 1))
        v = S.dequant(codes, fmt, None, np.arange(-64, 65))
        d = R.dec(codes[0], fmt).astype(np.float64)
        fin = np.isfinite(d)
        want = d[None, fin] * np.exp2(np.arange(-64, 65, dtype=np.float64))[:, None]
        assert np.array_equal(v[:, fin].astype(np.float64), want), "v is exact in fp32"
        assert (np.abs(v[:, fin][want != 0]) >= 2.0 ** -126).all() and np.abs(want[want != 0]).min() == (2.0 ** -73 if fmt == "e4m3" else 2.0 ** -80)
        with pytest.raises(AssertionError):
            S.dequant(codes[:1], fmt, 40, np.array([30]))


# ---- the C calls without a device --------------------------------------------------------------------------------------------------------

def test_argument_validation_without_gpu():
    """every refusal is made on the host, before any HIP call (the dummy pointers are never dereferenced)"""
    L = _lib.load()
    OK, INVALID, UNSUPPORTED, F32 = _lib.PM_OK, _lib.PM_ERR_INVALID, _lib.PM_ERR_UNSUPPORTED, _lib.PM_F32
    plan12 = (ctypes.c_int32 * 12)()
    err = L.pm_last_error
    ref = lambda op: None if op is None else ctypes.byref(op)      # noqa: E731

    def pooled(op, odt=F32, out=64, mean=0, te=64, re_=None):
        return L.pm_embbag_fwd_f8_scaled(ref(op), None, mean, odt, te, re_, out, None)

    def plan(op, odt=F32, mean=0, **_):
        return L.pm_embbag_f8_scaled_plan(ref(op), odt, mean, 1, plan12)

    def gather(op, odt=F32, out=64, stride=None, te=None, re_=64, **_):
        return L.pm_embedding_gather_f8_scaled(ref(op), odt, te, re_, out, (op.max_dim if op is not None else 32) if stride is None else stride, None)

    # what pm_embbag_fwd_f8 / pm_embedding_gather_f8 refuse, in their words
    for call in (pooled, plan, gather):
        assert call(None) == INVALID and b"op is NULL" in err()
        for wd in (_lib.PM_F32, _lib.PM_BF16, _lib.PM_F16, 5, -1):
            assert call(_request(wd=wd)) == INVALID and b"PM_F8E4M3 or PM_F8E5M2" in err(), wd
        for field, val, text in (("num_tables", 0, b"num_tables"), ("index_dtype", 3, b"index_dtype"), ("bag_count", 5, b"bag_begin/bag_count"),
                                 ("offsets", None, b"offsets"), ("indices", None, b"indices"), ("tables", None, b"tables")):
            op = _request()
            setattr(op, field, val)
            assert call(op) == INVALID and text in err(), field
        for d in (8, 24, 100, 2040):
            assert call(_request(max_dim=d)) == UNSUPPORTED and b"multiple of" in err(), d
        assert call(_request(max_dim=2064)) == UNSUPPORTED and b"at most 2048" in err()
        op = _request()
        op.table_group = 2
        assert call(op) == UNSUPPORTED and b"blocked layouts" in err()
        for odt in (-1, 3, 4, _lib.PM_I32):
            assert call(_request(), odt=odt) == INVALID and b"out_dtype" in err(), odt
    # no exponents at all is the unscaled call's request
    assert pooled(_request(), te=None, re_=None) == INVALID and b"both NULL" in err()
    assert gather(_request(), te=None, re_=None) == INVALID and b"both NULL" in err()
    assert pooled(_request(weighted=True), mean=1) == UNSUPPORTED and b"mean pooling is unweighted" in err()
    assert gather(_request(weighted=True)) == UNSUPPORTED and b"per_sample_weights must be NULL" in err()
    for mean in (2, -1):
        assert pooled(_request(), mean=mean) == INVALID and b"mean must be 0 or 1" in err()
        assert plan(_request(), mean=mean) == INVALID
    assert L.pm_embbag_f8_scaled_plan(ctypes.byref(_request()), F32, 0, 2, plan12) == INVALID
    assert L.pm_embbag_f8_scaled_plan(ctypes.byref(_request()), F32, 0, 1, None) == INVALID and b"out is NULL" in err()
    for stride in (16, 30, 34, -32):
        assert gather(_request(), stride=stride) == INVALID and b"out_row_stride" in err(), stride
    for call in (pooled, gather):
        assert call(_request(), out=None) == INVALID and b"out is NULL" in err()
        assert call(_request(), out=72) == INVALID and b"16-byte aligned" in err()
        assert call(_request(), odt=_lib.PM_F16, out=68) == INVALID and b"8-byte aligned" in err()
    empty = _request()
    empty.bag_count = 0
    assert pooled(empty, out=None) == OK and gather(empty, out=None) == OK and pooled(_request(B=0, N=0), out=None, re_=64) == OK

    # the quantiser
    def exps(src=64, sdt=F32, n=4, dim=32, stride=None, fdt=_lib.PM_F8E4M3, out=64):
        return L.pm_f8_row_exponents(src, sdt, n, dim, dim if stride is None else stride, fdt, out, None)

    def quant(src=64, sdt=F32, n=4, dim=32, stride=None, fdt=_lib.PM_F8E4M3, out=64):
        return L.pm_rows_quantize_f8(src, sdt, n, dim, dim if stride is None else stride, fdt, None, 64, out, None)

    for call in (exps, quant):
        for sdt in (_lib.PM_F8E4M3, _lib.PM_I32, -1, 7):
            assert call(sdt=sdt) == INVALID and b"src_dtype" in err(), sdt
        for fdt in (F32, _lib.PM_BF16, 5, -1):
            assert call(fdt=fdt) == INVALID and b"f8_dtype" in err(), fdt
        assert call(n=-1) == INVALID and b"n_rows" in err()
        for dim in (0, 8, 24, 40, 2040):
            assert call(dim=dim) == UNSUPPORTED and b"multiple of 16" in err(), dim
        assert call(dim=2064) == UNSUPPORTED and b"at most 2048" in err()
        assert call(stride=16) == INVALID and b"src_row_stride" in err()
        assert call(stride=34) == INVALID and b"src_row_stride" in err()          # fp32: 34 elements are not whole 16-byte pieces
        assert call(sdt=_lib.PM_BF16, stride=36) == INVALID and call(sdt=_lib.PM_BF16, stride=40, n=0) == OK
        assert call(src=None) == INVALID and b"src" in err() and call(src=72) == INVALID and b"16-byte aligned" in err()
        assert call(out=None) == INVALID and b"NULL" in err()
        assert call(n=0, src=None, out=None) == OK, "an empty request is PM_OK without a launch"
    assert quant(out=72) == INVALID and b"dst must be 16-byte aligned" in err()


def test_symbols_and_struct():
    assert set(NEW) <= set(_lib.EXPORTED_SYMBOLS)
    L = _lib.load()
    assert L.pm_abi_version() == 8 and ctypes.sizeof(_lib.pm_embbag_batch) == 144
    alt = _lib.load_alternates()
    assert all(hasattr(L, s) and hasattr(alt, s) for s in NEW)
    header = open(os.path.join(os.path.dirname(HERE), "include", "param_amd.h")).read()
    assert "SCALED FP8 TABLES" in header and all(s + "(" in header for s in NEW)


def test_the_scaled_plan_is_the_unscaled_plan_but_for_the_burst():
    """pm_embbag_f8_scaled_plan: pm_embbag_f8_plan's geometry; the row exponents' LDS bytes drop the burst of explicit weighted tiles of
    512 bags (64 KiB + 8 bytes with it), and of nothing else listed here"""
    dropped = []
    for T, B, N, D, weighted, odt, bpb in ((16, 8192, 16 * 8192 * 20, 128, False, _lib.PM_F32, 0), (16, 8192, 16 * 8192 * 20, 128, False, _lib.PM_F16, 0),
                                           (3, 100, 1234, 256, True, _lib.PM_F32, 0), (2, 64, 640, 2048, False, _lib.PM_F32, 0),
                                           (4, 2048, 4 * 2048 * 8, 16, True, _lib.PM_F16, 512), (4, 2048, 4 * 2048 * 8, 16, False, _lib.PM_F16, 512),
                                           (4, 2048, 4 * 2048 * 8, 16, True, _lib.PM_F16, 256)):
        try:
            _lib.set_tuning(bags_per_block=bpb)
            op = _request(T, B, N, D, weighted=weighted)
            base = _lib.embbag_f8_plan(op, odt)
            table, row = _lib.embbag_f8_scaled_plan(op, odt, False, False), _lib.embbag_f8_scaled_plan(op, odt, False, True)
        finally:
            _lib.set_tuning()
        assert table == base, (T, B, D)
        # the tile's LDS with row exponents: offsets | indices (| weights) | uint16 positions | int8 exponents, rounded to 16, | burst
        tile = (base["bags_per_block"] + 2) // 2 * 2 * 8 + base["idx_cap"] * (4 * (2 if weighted else 1) + 3)
        lds = (tile + 15) // 16 * 16 + base["bags_per_block"] * base["stage_out"] * (4 if odt == _lib.PM_F32 else 2)
        assert row == (dict(base, stage_out=0) if lds > 65536 else base), (base, row, lds)
        dropped.append(lds > 65536 and base["stage_out"] > 0)
    assert dropped == [False, False, False, False, True, False, False], dropped


# ---- the modules without a device --------------------------------------------------------------------------------------------------------

def test_constructors_and_refusals_on_cpu():
    from param_amd import Float8BatchedEmbeddingBagMI355 as FB
    from param_amd import Float8EmbeddingBagMI355 as FE
    from param_amd import Float8EmbeddingMI355 as FS

    plain = FB([5, 7], [32, 16], "e4m3", device="cpu")
    assert plain.scale is None and list(plain.state_dict()) == ["weights"] and "scale" not in repr(plain)
    assert torch.equal(plain.dequantized_table(1), plain.table(1).float())
    tab = FB([5, 7], [32, 16], "e4m3", device="cpu", scale="table")
    row = FB([5, 7], [32, 16], "e5m2", device="cpu", scale="row", pooling_mode="mean")
    assert list(tab.state_dict()) == ["weights", "table_exponents"] and tab.table_exponents.dtype == torch.int32 and tab.table_exponents.shape == (2,)
    assert list(row.state_dict()) == ["weights", "row_exponents"] and row.row_exponents.dtype == torch.int8 and row.row_exponents.shape == (12,)
    assert row.row_exponents_of(1).shape == (7,) and row.row_exponents_of(1).data_ptr() == row.row_exponents.data_ptr() + 5
    assert not list(row.parameters()) and "scale=row" in repr(row) and "scale=table" in repr(tab)
    # prepacked data: codes and exponents, validated at load time
    codes = torch.randint(0, 0x78, (7, 16), dtype=torch.uint8)
    e = torch.arange(-3, 4, dtype=torch.int64)
    row.copy_from_(1, codes, exponents=e)
    tab.copy_from_(1, codes, exponents=-9)
    assert torch.equal(row.row_exponents_of(1), e.to(torch.int8)) and int(tab.table_exponents[1]) == -9 and int(tab.table_exponents[0]) == 0
    for m, fmt, exps in ((row, "e5m2", (None, e.numpy())), (tab, "e4m3", (-9, None))):
        assert same_f32(m.dequantized_table(1).numpy(), S.dequant(codes.numpy(), fmt, *exps))
        twin = FB([5, 7], [32, 16], m.dtype, device="cpu", scale=m.scale)
        twin.load_state_dict(m.state_dict())
        assert torch.equal(twin.dequantized_table(1), m.dequantized_table(1)), "exponents round-trip through state_dict"
    row.copy_from_(1, codes)
    assert torch.equal(row.row_exponents_of(1), e.to(torch.int8)), "codes alone keep the exponents"
    for bad, text in ((torch.full((7,), 65), "lie in"), (torch.full((7,), -65), "lie in"), (torch.zeros(6, dtype=torch.int64), "shape"),
                      (torch.zeros(7), "integer tensor"), (3, "integer tensor")):
        with pytest.raises(ValueError, match=text):
            row.copy_from_(1, codes, exponents=bad)
    for bad, text in ((65, "lie in"), (-100, "lie in"), (torch.zeros(7, dtype=torch.int64), "one int"), (1.5, "one int")):
        with pytest.raises(ValueError, match=text):
            tab.copy_from_(1, codes, exponents=bad)
    with pytest.raises(ValueError, match="exponents need a module with scale"):
        plain.copy_from_(1, codes, exponents=0)
    with pytest.raises(ValueError, match='scale="row"'):
        tab.row_exponents_of(0)
    # scale: ValueError before anything is allocated (rows that could not be)
    for bad in ("tensor", "block", 2.0, "TABLE", True):
        with pytest.raises(ValueError, match="scale must be None"):
            FB([2 ** 30], [2048], device="cpu", scale=bad)
        with pytest.raises(ValueError, match="scale must be None"):
            FE(2 ** 30, 2048, device="cpu", scale=bad)
        with pytest.raises(ValueError, match="scale must be None"):
            FS(2 ** 30, 2048, device="cpu", scale=bad)
        with pytest.raises(ValueError, match="scale must be None"):
            FB.from_float([torch.zeros(4, 16)], scale=bad)
    # the quantiser runs on a ROCm device only; an unscaled module has none
    src = torch.randn(7, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        row.quantize_from_(1, src)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FB.from_float([src], "e4m3", scale="row")
    with pytest.raises(ValueError, match="quantize_from_ needs a module with scale"):
        plain.quantize_from_(1, src)
    for bad in (src.double(), src[:, :8], src.to(torch.float8_e5m2), torch.zeros(7, 16, dtype=torch.int32)):
        with pytest.raises(ValueError, match="quantize_from_: table 1 needs"):
            row.quantize_from_(1, bad)
    # from_float without a scale stays torch's cast, bit for bit
    f = FB.from_float([src], "e4m3")
    assert f.scale is None and torch.equal(f.table(0).view(torch.uint8), src.to(torch.float8_e4m3fn).view(torch.uint8))
    # the T = 1 modules
    e1 = FE(10, 32, "e4m3", mode="mean", device="cpu", scale="row")
    s1 = FS(10, 32, "e5m2", device="cpu", scale="table", output_dtype="bf16")
    assert e1.scale == "row" and e1.row_exponents.shape == (10,) and s1.scale == "table" and s1.table_exponents.shape == (1,)
    idx, off = torch.zeros(4, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    for call in (lambda: e1(idx, off), lambda: s1(idx), lambda: row.lookup(idx, torch.zeros(4, dtype=torch.int64), batch=2),
                 lambda: row.plan(idx, torch.zeros(4, dtype=torch.int64), batch=2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FE.from_float(torch.nn.EmbeddingBag(10, 32, mode="sum"), "e4m3", scale="table", device="cpu")


def test_unscaled_modules_reach_none_of_the_new_calls(monkeypatch):
    """a trap on the new bindings: a module with ``scale=None`` driven through every lookup and plan method touches none of them and
    makes the calls it made before; a scaled module reaches the scaled calls and none of the unscaled lookups"""
    import param_amd
    from param_amd import embedding_bag, quantized_bag

    L = _lib.load()
    hits = []
    old = ("pm_embbag_fwd_f8", "pm_embbag_f8_plan", "pm_embedding_gather_f8", "pm_embedding_gather_f8_plan")
    for name in NEW + old:
        monkeypatch.setattr(L, name, lambda *a, _n=name: hits.append(_n) or _lib.PM_OK, raising=True)
    for mod in (embedding_bag, quantized_bag):
        src = open(mod.__file__).read()
        assert "_scaled" not in src and "quantize_f8" not in src, mod.__name__
    monkeypatch.setattr(param_amd.float8_bag, "_require_device", lambda *a: None)
    monkeypatch.setattr(param_amd.float8_bag, "_stream_ptr", lambda: 0)
    monkeypatch.setattr(quantized_bag, "_require_device", lambda *a: None)
    monkeypatch.setattr(embedding_bag, "_require_device", lambda *a: None)
    idx, off = torch.zeros(4, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)

    def drive(m):
        del hits[:]
        m.lookup(idx, off, batch=2)
        m.plan(idx, off, batch=2)
        m.lookup_sequence(idx, off, batch=2)
        m.sequence_plan(idx, off, batch=2)
        return list(hits)

    assert drive(param_amd.Float8BatchedEmbeddingBagMI355([8], [16], device="cpu")) == list(old)
    bag = param_amd.Float8EmbeddingBagMI355(8, 16, device="cpu")
    del hits[:]
    bag(idx, off)
    assert hits == ["pm_embbag_fwd_f8"]
    emb = param_amd.Float8EmbeddingMI355(8, 16, device="cpu")
    del hits[:]
    emb(idx)
    assert hits == ["pm_embedding_gather_f8"]
    for kind in KINDS:
        m = param_amd.Float8BatchedEmbeddingBagMI355([8], [16], device="cpu", scale=kind)
        assert drive(m) == ["pm_embbag_fwd_f8_scaled", "pm_embbag_f8_scaled_plan", "pm_embedding_gather_f8_scaled", "pm_embedding_gather_f8_plan"]
        del hits[:]
        m.quantize_from_(0, torch.zeros(8, 16))
        assert hits == ["pm_f8_row_exponents", "pm_rows_quantize_f8"]
