"""The family fuzz's generator and composed references on the CPU (tests/fuzz_cases.py; the GPU side is tests/test_gpu_fuzz_families.py):
1. the default seed counts are the smallest that meet the coverage conditions, and every drawn configuration is legal;
2. ``case`` is deterministic;  3. the composed references against torch's CPU operators, bit for bit (NaN by class);
4. the comparison helper notices a deliberately wrong reference."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import embedding_rules as E
from tests import fuzz_cases as FC
from tests import max_rules as MX
from tests import out16_rules as O
from tests import qrows_cases as QC

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
PIN_SEEDS = 6


# ---- 1. coverage and legality -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", FC.FAMILIES)
def test_default_seed_count_is_the_smallest_that_covers(family):
    n = FC.SEEDS[family]
    cs = FC.cases(family)
    cov = FC.coverage(family, cs)
    assert all(cov.values()), [k for k, v in cov.items() if not v]
    short = FC.coverage(family, cs[:n - 1])
    assert not all(short.values()), "one seed fewer still meets every condition: the constant is not the smallest"
    assert FC.smallest_count(family) == n


@pytest.mark.parametrize("family", FC.FAMILIES)
def test_every_drawn_configuration_is_legal(family):
    for c in FC.cases(family, 3 * FC.SEEDS[family]):
        assert FC.problems(c) == [], (family, c["seed"])
        if c["long_bag"] is not None:
            assert c["lens"][c["long_bag"]] >= FC.LONG[0] and np.delete(c["lens"], c["long_bag"]).max(initial=0) <= 40


# ---- 2. determinism ---------------------------------------------------------------------------------------------------------------------

def _equal(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


@pytest.mark.parametrize("family", FC.FAMILIES)
def test_case_is_deterministic(family):
    for seed in (0, 1, FC.SEEDS[family] - 1):
        a, b = FC.case(family, seed), FC.case(family, seed)
        assert a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a), (family, seed)


# ---- 3. the composed references against torch ---------------------------------------------------------------------------------------------

def _table_request(idx, off, t, T, B):
    """table t's stretch of a (repaired) TBE request as torch's one-table request: (indices int64, offsets int64 [B])"""
    off = np.asarray(off).astype(np.int64)
    lo = int(off[t * B])
    hi = int(off[(t + 1) * B]) if t + 1 < T else int(np.asarray(idx).size)
    return torch.from_numpy(np.asarray(idx).astype(np.int64)[lo:hi]), torch.from_numpy(off[t * B:(t + 1) * B] - lo)


def _pinned(family, want):
    """the first PIN_SEEDS seeds of ``family`` that ``want`` accepts"""
    got = []
    for seed in range(10 * FC.SEEDS[family]):
        c = FC.case(family, seed)
        if want(c):
            got.append(c)
            if len(got) == PIN_SEEDS:
                break
    assert len(got) == PIN_SEEDS
    return got


def test_train_reference_against_torch_embedding_bag():
    """fp32 tables: ``F.embedding_bag`` per table on the repaired request, with ``padding_idx`` and ``mode``, then ``.to(dtype)``.  torch's
    weighted path with a padding row rounds twice per lookup (tests/test_f8_host.py bounds it), so a weighted table is pinned where it
    has no padding row."""
    damaged = 0
    for c in _pinned("train", lambda c: c["wdt"] == "f32"):
        idx, off, _ = FC.repaired(c)
        damaged += c["damaged"]
        pads = FC.normal_pads(c["pads"], c["rows"])
        want = FC.train_forward(c)
        for t in range(c["T"]):
            if c["psw"] is not None and pads[t] is not None:
                continue
            i, o = _table_request(idx, off, t, c["T"], c["B"])
            lo = int(np.asarray(off).astype(np.int64)[t * c["B"]])
            w = None if c["psw"] is None else torch.from_numpy(c["psw"][lo:lo + i.numel()])
            ref = F.embedding_bag(i, torch.from_numpy(FC.widened(c)[t]), o, mode="mean" if c["mean"] else "sum", padding_idx=pads[t],
                                  per_sample_weights=w).to(TDT[c["odt"]])
            bits = ref.view(torch.int16).numpy().view(np.uint16) if c["odt"] != "fp32" else ref.numpy().view(np.uint32)
            got = want[t] if c["odt"] != "fp32" else FC.out_bits(want[t], "fp32")
            assert FC.same_bits(got, bits, c["odt"]), (c["seed"], t)
    assert damaged, "a repaired request is among the pinned cases"


def test_max_reference_against_torch_embedding_bag():
    for c in _pinned("max", lambda c: c["wdt"] == "f32"):
        idx, off = FC.request_arrays(c)
        pads = FC.normal_pads(c["pads"], c["rows"])
        vals, _ = MX.forward(FC.widened(c), idx, off, c["B"], pads)
        for t in range(c["T"]):
            i, o = _table_request(idx, off, t, c["T"], c["B"])
            ref = F.embedding_bag(i, torch.from_numpy(FC.widened(c)[t]), o, mode="max", padding_idx=pads[t])
            assert FC.same_bits(FC.out_bits(vals[t], "fp32"), ref.numpy().view(np.uint32), "fp32"), (c["seed"], t)


def test_sequence_reference_against_torch_embedding():
    for c in _pinned("sequence", lambda c: True):
        idx, off = FC.request_arrays(c)
        D, N = c["dims"][0], idx.size
        got = E.forward(c["tables"], c["wdt"], "f32", idx, off, c["B"], np.zeros((N, D), dtype=np.uint32))
        for t in range(c["T"]):
            i, o = _table_request(idx, off, t, c["T"], c["B"])
            lo = int(c["off"][t * c["B"]])
            ref = torch.nn.Embedding.from_pretrained(torch.from_numpy(FC.widened(c)[t]))(i)
            assert np.array_equal(got[lo:lo + i.numel()], ref.numpy().view(np.uint32)), (c["seed"], t)


@pytest.mark.parametrize("family", ("qrows", "qmixed"))
def test_quantized_reference_against_torch_rowwise_offsets(family):
    for c in _pinned(family, lambda c: True):
        idx, off = FC.request_arrays(c)
        want = FC.serving_forward(c)
        for t in range(c["T"]):
            i, o = _table_request(idx, off, t, c["T"], c["B"])      # (rebased: the operators read offsets[0] as 0)
            lo = int(c["off"][t * c["B"]])
            w = None if c["psw"] is None else c["psw"][lo:lo + i.numel()]
            ref = QC.torch_lookup(c["tables"][t], c["bits"][t], i.numpy(), o.numpy(), w)
            assert FC.same_bits(FC.out_bits(want[t], "fp32"), np.ascontiguousarray(ref).view(np.uint32), "fp32"), (c["seed"], t)


def _stored_values(c, t):
    """fp32 ``[rows, D]``: table t's stored values, or None for quantised rows of a mixed-format case (their operator is pinned above)"""
    if c["family"] == "f8s":
        return FC.F8S.dequant(c["tables"][t], c["fmt"], *c["exps"][t])
    if c["family"] == "mx4":
        return FC.M4.dequant(c["tables"][t], c["dims"][t])
    return None if c["fmts"][t] in ("int8", "int4") else FC.A.widened(FC.any_tables(c)[t])


@pytest.mark.parametrize("family", ("f8s", "anyfmt", "mx4"))
def test_stored_value_references_against_torch_embedding_bag(family):
    """torch has no operator over these formats, but it has one over their stored VALUES: ``F.embedding_bag`` per table over the
    dequantised fp32 table, with the case's ``mode``, weights and ``padding_idx`` (a weighted table with a padding row is passed over, as
    in the ``train`` pin), against the composed pooled reference of the whole request"""
    pinned = 0
    for c in _pinned(family, lambda c: True):
        idx, off = FC.request_arrays(c)
        want = FC.serving_forward(c)
        pads = FC.normal_pads(c.get("pads"), c["rows"])
        for t in range(c["T"]):
            W = _stored_values(c, t)
            if W is None or (c["psw"] is not None and pads[t] is not None):
                continue
            i, o = _table_request(idx, off, t, c["T"], c["B"])
            lo = int(c["off"][t * c["B"]])
            w = None if c["psw"] is None else torch.from_numpy(c["psw"][lo:lo + i.numel()])
            ref = F.embedding_bag(i, torch.from_numpy(np.ascontiguousarray(W)), o, mode="mean" if c.get("pool") == "mean" else "sum",
                                  padding_idx=pads[t], per_sample_weights=w)
            assert FC.same_bits(FC.out_bits(want[t], "fp32"), ref.numpy().view(np.uint32), "fp32"), (c["seed"], t)
            pinned += 1
    assert pinned >= PIN_SEEDS


# ---- 4. sensitivity -----------------------------------------------------------------------------------------------------------------------

def _forward_bits(c, use_slice):
    """the family's forward reference as output bits, joined in the case's layout"""
    fam = c["family"]
    if fam == "train":
        parts = FC.train_forward(c, use_slice)
        parts = parts if c["odt"] != "fp32" else [FC.out_bits(p, "fp32") for p in parts]
    elif fam == "max":
        b0, n = FC.slice_of(c, use_slice)
        idx, off = FC.request_arrays(c)
        parts = [FC.out_bits(v, c["odt"]) for v in MX.forward(FC.widened(c), idx, off, c["B"], FC.normal_pads(c["pads"], c["rows"]), b0, n)[0]]
    elif fam == "sequence":
        b0, n = FC.slice_of(c, use_slice)
        idx, off = FC.request_arrays(c)
        kout = {"fp32": "f32", "bf16": "bf16", "fp16": "f16"}[c["odt"]]
        blank = np.full((idx.size, c["dims"][0]), FC.sentinel_bits(c["odt"]), dtype=E.BITS[kout])
        return E.forward(c["tables"], c["wdt"], kout, idx, off, c["B"], blank, b0, n)
    else:
        parts = [FC.out_bits(p, c["odt"]) for p in FC.serving_forward(c, use_slice)]
    return FC.join(parts, c["layout"])


def _last_of_longest_counts(c):
    """the lookup ``drop_last_of_longest`` removes contributes to the output: it is no padding row, is not pruned, and -- under max
    pooling -- its row supplies the maximum of some column"""
    g = int(np.argmax(c["lens"]))
    t, j = g // c["B"], int(c["off"][g + 1]) - 1
    r = int(c["idx"][j])
    if "pads" in c and FC.normal_pads(c["pads"], c["rows"])[t] == r:
        return False
    if c["family"] == "pruned" and c["remaps"][t] is not None and c["remaps"][t][r] < 0:
        return False
    if c["family"] == "max":
        idx, off = FC.request_arrays(c)
        args = MX.forward(FC.widened(c), idx, off, c["B"], FC.normal_pads(c["pads"], c["rows"]))[1][t][g % c["B"]]
        return bool((args == r).any() and (c["idx"][int(c["off"][g]):j] != r).all())
    return True


def _sensitive_case(family):
    for seed in range(20 * FC.SEEDS[family]):
        c = FC.case(family, seed)
        if c.get("damaged") or c.get("nan") or c["slice"] is None or c["slice"][1] == 0 or c["slice"][1] == c["B"] or c["lens"].max() == 0:
            continue
        b0, n = c["slice"]
        sl = c["lens"].reshape(c["T"], c["B"])[:, b0:b0 + n]
        if sl.sum() and (c["B"] - n) and c["lens"].sum() > sl.sum() and _last_of_longest_counts(c):
            return c
    raise AssertionError(family)


@pytest.mark.parametrize("family", FC.FAMILIES)
def test_comparison_notices_a_wrong_reference(family):
    c = _sensitive_case(family)
    right = _forward_bits(c, False)
    assert FC.same_bits(right, _forward_bits(c, False), c["odt"])
    if family == "sequence":      # one row per lookup: a dropped lookup changes the shape
        assert not FC.same_bits(right, _forward_bits(FC.drop_last_of_longest(c), False), c["odt"])
    else:
        wrong = _forward_bits(FC.drop_last_of_longest(c), False)
        assert wrong.shape == right.shape and not FC.same_bits(right, wrong, c["odt"]), "a dropped lookup goes unnoticed"
    sliced, shifted = _forward_bits(c, True), _forward_bits(FC.shift_slice(c), True)
    if family == "sequence":
        assert not FC.same_bits(sliced, shifted, c["odt"]), "a shifted slice goes unnoticed"
    else:
        b0, n = c["slice"]
        s0 = FC.shift_slice(c)["slice"][0]
        whole = right.shape
        a = FC.canvas(whole, c["layout"], sliced, b0, n, FC.sentinel_bits(c["odt"]))
        b = FC.canvas(whole, c["layout"], shifted, s0, n, FC.sentinel_bits(c["odt"]))
        assert not FC.same_bits(a, b, c["odt"]), "a shifted slice goes unnoticed"
        assert not FC.same_bits(a, FC.canvas(whole, c["layout"], shifted, b0, n, FC.sentinel_bits(c["odt"])), c["odt"])


def test_same_bits_compares_nan_by_class():
    a = np.array([1.0, np.nan, -0.0], dtype=np.float32)
    b = a.copy()
    b.view(np.uint32)[1] = 0xffc00001
    assert FC.same_bits(a.view(np.uint32), b.view(np.uint32), "fp32")
    assert not FC.same_bits(a.view(np.uint32), np.array([1.0, np.nan, 0.0], dtype=np.float32).view(np.uint32), "fp32")
    assert not FC.same_bits(a.view(np.uint32), np.array([1.0, 2.0, -0.0], dtype=np.float32).view(np.uint32), "fp32")
    for odt in O.DTYPES:
        assert FC.same_bits(O.round16(a, odt), O.round16(b, odt), odt) and not FC.same_bits(O.round16(a, odt), O.round16(-a, odt), odt)
