"""Random requests and module configurations for the family fuzz (tests/test_gpu_fuzz_families.py on the GPU,
tests/test_fuzz_cases_host.py on the CPU).  Pure numpy: ``case(family, seed)`` draws from ``np.random.default_rng`` seeded by
``(crc32(family), seed)``, so the same call gives the same arrays on every machine.  Dtypes, formats and layouts travel as strings.

Families here: ``train`` (BatchedEmbeddingBagMI355: padding, mean, output_dtype, bounds repair, weights), ``max``
(MaxBatchedEmbeddingBagMI355), ``sequence`` (the un-pooled gather and its backward), and the serving families ``qrows`` (one 8- or
4-bit format), ``qmixed`` (a format per table), ``pruned`` (a remap per table) and ``f8`` (unscaled FP8), ``f8s`` (scaled FP8, row or table exponents), ``anyfmt``
(any of the seven stored formats per table) and ``mx4`` (MXFP4).  ``f8s`` and ``mx4`` also draw the source dtype of a quantiser run
(``quantiser_source``).

The references are the rule files' own functions; what this module adds is the COMPOSITION (bounds repair, then the padding filter, then
mean or weights, then the one rounding of a 16-bit output), which tests/test_fuzz_cases_host.py pins to torch's CPU operators.

Sizes are small on purpose: a launch plan depends on sizes and knobs only, and the numpy rules loop per lookup.  A case holds at most
about 3000 ordinary lookups plus, in the ``long`` mode, ONE bag of ``LONG`` lookups, meant to be longer than the index tile the family stages: whether it is, is
not decided here -- the GPU test reads ``idx_cap`` from the family's plan and asserts that the bag is unstaged."""
import zlib

import numpy as np

from tests import anyfmt_cases as AC
from tests import anyfmt_rules as A
from tests import bounds_rules as BR
from tests import embedding_rules as E
from tests import f8_rules as F8
from tests import f8s_rules as F8S
from tests import mean_rules as MR
from tests import mx4_rules as M4
from tests import out16_rules as O
from tests import padding_rules as P
from tests import pruned_rules as PR
from tests import qmixed_rules as QM

FAMILIES = ("train", "max", "sequence", "qrows", "qmixed", "pruned", "f8", "f8s", "anyfmt", "mx4")
SERVING = FAMILIES[3:]

# Default seed counts: for each family the smallest count at which the cases 0 .. n - 1 meet every condition of ``coverage`` (found by
# ``smallest_count``; tests/test_fuzz_cases_host.py asserts both that the count meets them and that count - 1 does not).
SEEDS = {"train": 17, "max": 9, "sequence": 44, "qrows": 15, "qmixed": 10, "pruned": 12, "f8": 8, "f8s": 9, "anyfmt": 42,
         "mx4": 10}

ROWS = (1, 2, 3, 17, 100, 1000)
BATCHES = (1, 2, 7, 33, 100)
MODES = ("fixed", "ragged", "sparse", "long")
LOOKUPS = 3000                   # ordinary lookups a case may hold (the rules loop per lookup)
LONG = (4200, 5001)              # the one long bag's length, [lo, hi): the GPU test asserts it against the plan's ``idx_cap``
EXPS = (-10, 11)                 # FP8 exponents, [lo, hi): the middle of [-64, 64], so sums stay finite
MX4_SCALES = (120, 135)          # MXFP4 scale bytes, [lo, hi): around 127 (2^0)
SRC_PAD = 32                     # columns either side of a quantiser source inside its wider tensor (the strided view)
SENTINEL = 7.0                   # what a caller's ``out`` holds before a sliced call (exact in bf16 and fp16)
EXACT_RUN = 256                  # rows with more lookups are summed as ordered chunk partials: not bit-pinned by the rules
ODTS = ("fp32", "bf16", "fp16")
WDTS = ("f32", "bf16", "f16")    # table dtypes, as tests/embedding_rules.py spells them
_O16 = {"bf16": "bf16", "f16": "fp16"}

# legal embedding dims per element rule (the constructors' own statements): the smallest, ones that end inside a lane group, a wide one
DIMS = {
    "f32": (4, 8, 12, 28, 32, 56, 64, 128, 132, 256, 512),                # multiples of 4
    "bf16": (8, 16, 24, 56, 64, 112, 128, 264, 512),                     # multiples of 8
    "f16": (8, 16, 24, 56, 64, 112, 128, 264, 512),
    "q8": (4, 8, 20, 24, 64, 100, 128, 260, 1024, 4096),                  # 8-bit rows: multiples of 4, at most 4096
    "q4": (8, 16, 24, 40, 64, 104, 128, 264, 1024, 4096),                 # 4-bit, per-table formats and pruned: multiples of 8
    "f8": (16, 32, 48, 64, 112, 128, 144, 256, 1040, 2048),               # FP8: multiples of 16, at most 2048; 1040: a second column pass
    "mx4": (32, 64, 96, 128, 160, 512, 1024, 2048),                       # MXFP4: multiples of 32, at most 2048 (two column passes)
    "any8": (8, 24, 40, 64, 104, 128, 264, 520, 2048),                    # mixed-format: multiples of 8, at most 2048 ...
    "any16": (16, 48, 64, 112, 128, 144, 528, 1040, 2048),                # ... of 16 for an FP8 table
}
PSW_GRAD_MAX_DIM = {"f32": 256, "bf16": 512, "f16": 512}      # pm_embbag_psw_grad's stated limit per table dtype
_WIDE = 512                      # a case with a dim above this draws fewer lookups (the rules' cost is lookups x dim)


def _rng(family, seed):
    return np.random.default_rng([zlib.crc32(family.encode()), int(seed)])


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


# ---- common draws -----------------------------------------------------------------------------------------------------------------------

def _dims(rng, T, legal, common=None):
    common = (rng.random() < 0.5) if common is None else common
    dims = [int(_pick(rng, legal)) for _ in range(T)]
    if common:
        dims = [dims[0]] * T
    return dims, len(set(dims)) == 1


def _lens(rng, T, B, budget):
    """bag lengths ``[T * B]`` in one of the base fuzz's four modes, then the empty table / first bag / last bag, then the long bag"""
    mode = str(_pick(rng, MODES))
    cap = int(min(40, max(3, budget // (T * B))))
    lens = []
    for _ in range(T):
        if mode == "fixed":
            ln = np.full(B, int(rng.integers(0, min(30, cap) + 1)))
        elif mode == "ragged":
            ln = rng.integers(0, cap + 1, B)
        elif mode == "sparse":
            ln = (rng.random(B) < 0.3) * rng.integers(1, 5, B)
        else:
            ln = rng.integers(0, min(8, cap + 1), B)
        lens.append(np.asarray(ln, dtype=np.int64))
    lens = np.concatenate(lens)
    if rng.random() < 0.2:
        t = int(rng.integers(0, T))
        lens[t * B:(t + 1) * B] = 0
    if rng.random() < 0.3:
        lens[0] = 0
    if rng.random() < 0.3:
        lens[-1] = 0
    long_bag = None
    if mode == "long":
        long_bag = int(rng.integers(0, T * B))
        lens[long_bag] = int(rng.integers(*LONG))
    return mode, lens, long_bag


def _slice(rng, B):
    """None, or ``(bag_begin, bag_count)`` with ``bag_count == 0`` among the draws"""
    if rng.random() < 0.35:
        return None
    b0 = int(rng.integers(0, B))
    n = 0 if rng.random() < 0.2 else int(rng.integers(0, B - b0 + 1))
    return (b0, n)


def _format_dims(rng, fmts):
    """dims of a mixed-format module: per table from its format's legal set, or one dim that is legal for every table"""
    per = [DIMS["any16" if f.startswith("fp8") else "any8"] for f in fmts]
    if rng.random() < 0.35:
        both = sorted(set(per[0]).intersection(*per[1:]))
        dims = [int(_pick(rng, both))] * len(fmts)
    else:
        dims = [int(_pick(rng, p)) for p in per]
    return dims, len(set(dims)) == 1


def _common(rng, legal, common_dims=None, formats=None):
    T = int(rng.integers(1, 8))
    rows = [int(_pick(rng, ROWS)) for _ in range(T)]
    B = int(_pick(rng, BATCHES))
    if formats is not None:
        fmts = [str(_pick(rng, formats)) for _ in range(T)]
        dims, same = _format_dims(rng, fmts)
    else:
        dims, same = _dims(rng, T, legal, common_dims)
    budget = LOOKUPS if max(dims) <= _WIDE else LOOKUPS // 6
    mode, lens, long_bag = _lens(rng, T, B, budget)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    per_table = lens.reshape(T, B).sum(axis=1)
    idx = np.concatenate([rng.integers(0, rows[t], int(per_table[t])) for t in range(T)]).astype(np.int64)
    c = dict(T=T, rows=rows, B=B, dims=dims, same_dims=same, mode=mode, long_bag=long_bag, lens=lens, idx=idx, off=off,
             itype="i64" if rng.random() < 0.6 else "i32", trailing=bool(rng.random() < 0.7),
             layout="tbd" if (same and rng.random() < 0.4) else "bd", slice=_slice(rng, B))
    if formats is not None:
        c["fmts"] = fmts
    return c


def _weights(rng, n):
    return rng.standard_normal(n).astype(np.float32)


def _pads(rng, rows):
    """None, one int for every table (negative values included), or a per-table list with Nones"""
    u = rng.random()
    if u < 0.3:
        return None
    if u < 0.55:
        lo = min(rows)
        return int(rng.integers(-lo, lo))
    if u < 0.7:
        return 0
    pads = [None if rng.random() < 0.4 else int(rng.integers(-r, r)) for r in rows]
    if rng.random() < 0.5:
        pads[int(rng.integers(0, len(rows)))] = 0
    return pads


def normal_pads(pads, rows):
    """``padding_idx`` as the modules normalise it: ``int | None`` per table, negative values counted from the end"""
    if pads is None:
        return [None] * len(rows)
    per = [pads] * len(rows) if isinstance(pads, int) else list(pads)
    return [None if k is None else (k + r if k < 0 else k) for k, r in zip(per, rows)]


def _float_tables(rng, rows, dims, wdt):
    """table BITS of kind ``wdt``: normal values, the padding rows included (a kernel that reads one shows)"""
    return [E.to_bits(rng.standard_normal((r, d)).astype(np.float32), wdt) for r, d in zip(rows, dims)]


def _plant_pads(rng, c, share=0.3):
    """about ``share`` of the lookups of every table with a padding row become that row"""
    pads = normal_pads(c["pads"], c["rows"])
    tab = np.repeat(np.arange(c["T"]), c["lens"].reshape(c["T"], c["B"]).sum(axis=1))
    pad = np.array([-1 if k is None else k for k in pads], dtype=np.int64)[tab]
    hit = (rng.random(c["idx"].size) < share) & (pad >= 0)
    c["idx"][hit] = pad[hit]


# ---- families ---------------------------------------------------------------------------------------------------------------------------

def _train(rng):
    wdt = str(_pick(rng, ("f32", "f32", "bf16", "f16")))
    c = _common(rng, DIMS[wdt])
    c.update(wdt=wdt, pads=_pads(rng, c["rows"]), mean=bool(rng.random() < 0.4), odt=str(_pick(rng, ("fp32", "fp32", "bf16", "fp16"))),
             bounds=str(_pick(rng, ("none", "ignore", "warning"))))
    _plant_pads(rng, c)
    # weights only with sum, and only at dims the per_sample_weights gradient takes (one 16-byte load per lane of a 64-lane group)
    c["psw"] = _weights(rng, c["idx"].size) if (not c["mean"] and max(c["dims"]) <= PSW_GRAD_MAX_DIM[wdt] and rng.random() < 0.5) else None
    c["tables"] = _float_tables(rng, c["rows"], c["dims"], wdt)
    c["grad16"] = bool(c["odt"] != "fp32" and rng.random() < 0.5)          # the gradient arrives in the module's 16-bit dtype
    c["damaged"] = False
    if c["bounds"] != "none" and rng.random() < 0.75:
        idx, off = c["idx"].copy(), c["off"].copy()
        pads = normal_pads(c["pads"], c["rows"])
        zero = [t for t in range(c["T"]) if pads[t] == 0 and c["off"][(t + 1) * c["B"]] > c["off"][t * c["B"]]]
        if zero and rng.random() < 0.6:                                    # a bad index in a table whose padding row is its repair target
            t = int(_pick(rng, zero))
            j = int(rng.integers(c["off"][t * c["B"]], c["off"][(t + 1) * c["B"]]))
            idx[j] = c["rows"][t]
        idx, off = BR.corrupt(rng, idx, off, c["rows"], int(rng.integers(0, 4)), int(rng.integers(0, 3)))
        c["idx"], c["off"], c["damaged"] = idx, off, True
    return c


def _max(rng):
    wdt = str(_pick(rng, ("f32", "f32", "bf16", "f16")))
    c = _common(rng, DIMS[wdt])
    c.update(wdt=wdt, pads=_pads(rng, c["rows"]), odt=str(_pick(rng, ("fp32", "fp32", "bf16", "fp16"))))
    _plant_pads(rng, c)
    # few distinct values: ties between rows (the first wins) and rows that win no column; a stored -0.0 among them
    vals = np.array([-2.0, -0.0, 0.0, 0.5, 1.0, 3.0], dtype=np.float32)
    c["tables"] = [E.to_bits(np.where(rng.random((r, d)) < 0.5, vals[rng.integers(0, vals.size, (r, d))],
                                      rng.standard_normal((r, d)).astype(np.float32)), wdt) for r, d in zip(c["rows"], c["dims"])]
    c["grad16"] = bool(c["odt"] != "fp32" and rng.random() < 0.5)
    return c


def _sequence(rng):
    wdt = str(_pick(rng, WDTS))
    c = _common(rng, DIMS[wdt], common_dims=True)
    c.update(wdt=wdt, odt=str(_pick(rng, ODTS)), pads=_pads(rng, c["rows"]))
    _plant_pads(rng, c)
    c["tables"] = _float_tables(rng, c["rows"], c["dims"], wdt)
    return c


def _quantized_tables(rng, rows, dims, bits):
    from oracle import rowquant

    tabs = []
    for r, d, b in zip(rows, dims, bits):
        x = (rng.standard_normal((r, d)) * (rng.random((r, 1)) * 4 + 0.05)).astype(np.float32)
        tabs.append(rowquant.quantize_rows(x, b))
    return tabs


def _nan_row_q(rng, c):
    """with probability 0.3 one looked-up row's scale becomes a NaN"""
    c["nan"] = False
    if c["idx"].size and rng.random() < 0.3:
        j = int(rng.integers(0, c["idx"].size))
        t = int(P.table_of(c["off"], c["T"], c["B"], c["idx"].size)[j])
        q, d, b = c["tables"][t], c["dims"][t], c["bits"][t]
        r = int(c["idx"][j]) if c.get("remaps") is None or c["remaps"][t] is None else int(c["remaps"][t][c["idx"][j]])
        if r >= 0:
            if b == 8:
                q[r, d:d + 4] = np.array([np.nan], dtype=np.float32).view(np.uint8)
            else:
                q[r, d // 2:d // 2 + 2] = np.array([np.nan], dtype=np.float16).view(np.uint8)
            c["nan"] = True


def _serving_common(rng, c):
    c["odt"] = str(_pick(rng, ODTS))
    c["psw"] = _weights(rng, c["idx"].size) if rng.random() < 0.5 else None


def _qrows(rng):
    bits = int(_pick(rng, (8, 4)))
    c = _common(rng, DIMS["q8" if bits == 8 else "q4"])
    c["bits"] = [bits] * c["T"]
    c["tables"] = _quantized_tables(rng, c["rows"], c["dims"], c["bits"])
    _serving_common(rng, c)
    _nan_row_q(rng, c)
    return c


def _qmixed(rng):
    c = _common(rng, DIMS["q4"])
    c["bits"] = [int(_pick(rng, (8, 4))) for _ in range(c["T"])]
    c["tables"] = _quantized_tables(rng, c["rows"], c["dims"], c["bits"])
    _serving_common(rng, c)
    _nan_row_q(rng, c)
    return c


def _pruned(rng):
    """``rows`` are the LOGICAL rows (the index space); ``phys_rows`` what the tables hold.  Per table a remap with a random pruned share,
    0 % (the identity as an explicit remap, or None) and 100 % (no physical row) included; at least one table carries a remap."""
    c = _common(rng, DIMS["q4"])
    c["bits"] = [int(_pick(rng, (8, 4))) for _ in range(c["T"])]
    remaps, phys = [], []
    force = int(rng.integers(0, c["T"]))
    for t, r in enumerate(c["rows"]):
        u = rng.random()
        if u < 0.25 and t != force:
            remaps.append(None)
            phys.append(r)
            continue
        share = 0.0 if u < 0.4 else 1.0 if u < 0.55 else float(rng.random())
        keep = rng.random(r) >= share if 0.0 < share < 1.0 else np.full(r, share == 0.0)
        m = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        remaps.append(m)
        phys.append(int(keep.sum()))
    c["remaps"], c["phys_rows"] = remaps, phys
    c["tables"] = _quantized_tables(rng, phys, c["dims"], c["bits"])
    _serving_common(rng, c)
    _nan_row_q(rng, c)
    return c


def _f8(rng):
    c = _common(rng, DIMS["f8"])
    c["fmt"] = str(_pick(rng, F8.FORMATS))
    c["tables"] = [F8.finite_codes(rng, c["fmt"], (r, d)) for r, d in zip(c["rows"], c["dims"])]
    c["pads"] = _pads(rng, c["rows"])
    _plant_pads(rng, c)
    c["odt"] = str(_pick(rng, ODTS))
    c["pool"] = str(_pick(rng, ("plain", "weighted", "mean")))
    c["psw"] = _weights(rng, c["idx"].size) if c["pool"] == "weighted" else None
    c["nan"] = False
    if c["idx"].size and rng.random() < 0.3:                               # one NaN row among the looked-up ones
        j = int(rng.integers(0, c["idx"].size))
        t = int(P.table_of(c["off"], c["T"], c["B"], c["idx"].size)[j])
        c["tables"][t][int(c["idx"][j])] = 0x7f
        c["nan"] = True
    return c


def _looked_up(rng, c):
    """(table, row) of one random lookup of the request"""
    j = int(rng.integers(0, c["idx"].size))
    return int(P.table_of(c["off"], c["T"], c["B"], c["idx"].size)[j]), int(c["idx"][j])


def _f8s(rng):
    """the ``f8`` draws, then the exponent kind and the exponents: ``exps[t]`` is ``(E_t, None)`` or ``(None, e_rows)``"""
    c = _f8(rng)
    c["scale"] = str(_pick(rng, ("row", "table")))
    c["exps"] = [(int(rng.integers(*EXPS)), None) if c["scale"] == "table" else (None, rng.integers(*EXPS, r).astype(np.int64))
                 for r in c["rows"]]
    c["src"] = str(_pick(rng, ODTS))
    return c


_NAN16 = {"bf16": 0x7fc0, "fp16": 0x7e00}


def _anyfmt(rng):
    """``tables[t]``: the uint8 bytes ``[rows, row_bytes]`` the module stores (tests/anyfmt_cases.py makes them); ``exps[t]``: an FP8
    table's exponent, 0 otherwise"""
    c = _common(rng, None, formats=A.FORMATS)
    c["exps"] = [int(rng.integers(*EXPS)) if f.startswith("fp8") else 0 for f in c["fmts"]]
    c["tables"] = [AC.table_bytes(f, r, d, rng) for f, r, d in zip(c["fmts"], c["rows"], c["dims"])]
    _serving_common(rng, c)
    c["nan"] = False
    if c["idx"].size and rng.random() < 0.3:      # one NaN row among the looked-up ones: an element, an FP8 code or the row's scale
        t, r = _looked_up(rng, c)
        f, d, row = c["fmts"][t], c["dims"][t], c["tables"][t][r]
        k = int(rng.integers(0, d))
        if f == "fp32":
            row.view(np.uint32)[k] = 0x7fc00000
        elif f in _NAN16:
            row.view(np.uint16)[k] = _NAN16[f]
        elif f.startswith("fp8"):
            row[k] = 0x7f
        elif f == "int8":
            row[d:d + 4] = np.array([np.nan], dtype=np.float32).view(np.uint8)
        else:
            row[d // 2:d // 2 + 2] = np.array([np.nan], dtype=np.float16).view(np.uint8)
        c["nan"] = True
    return c


def _mx4(rng):
    """``tables[t]``: uint8 ``[rows, row_bytes(D)]``: codes of every kind under scale bytes around 127 (tests/test_gpu_mx4.py:
    ``random_table``); one NaN BLOCK (scale byte 255) in a looked-up row with probability 0.3"""
    c = _common(rng, DIMS["mx4"])
    tabs = []
    for r, d in zip(c["rows"], c["dims"]):
        tab = np.zeros((r, M4.row_bytes(d)), dtype=np.uint8)
        tab[:, :d // 2] = rng.integers(0, 256, (r, d // 2))
        tab[:, d // 2:d // 2 + d // M4.BLOCK] = rng.integers(*MX4_SCALES, (r, d // M4.BLOCK))
        tabs.append(tab)
    c["tables"] = tabs
    c["odt"] = str(_pick(rng, ODTS))
    c["pool"] = str(_pick(rng, ("plain", "weighted", "mean")))
    c["psw"] = _weights(rng, c["idx"].size) if c["pool"] == "weighted" else None
    c["nan"] = False
    if c["idx"].size and rng.random() < 0.3:
        t, r = _looked_up(rng, c)
        d = c["dims"][t]
        tabs[t][r, d // 2 + int(rng.integers(0, d // M4.BLOCK))] = 255
        c["nan"] = True
    c["src"] = str(_pick(rng, ODTS))
    return c


_DRAW = {"train": _train, "max": _max, "sequence": _sequence, "qrows": _qrows, "qmixed": _qmixed, "pruned": _pruned, "f8": _f8,
         "f8s": _f8s, "anyfmt": _anyfmt, "mx4": _mx4}


def case(family, seed):
    """one request and one module configuration of ``family``, the same for the same arguments everywhere"""
    c = _DRAW[family](_rng(family, seed))
    c.update(family=family, seed=int(seed))
    return c


def offsets_arg(c):
    """the offsets as the entry point is handed them: with or without the trailing entry"""
    return c["off"] if c["trailing"] else c["off"][:c["T"] * c["B"]]


def np_itype(c):
    return np.int64 if c["itype"] == "i64" else np.int32


def request_arrays(c):
    """(indices, offsets) in the case's index dtype (a damaged value that does not fit int32 wraps, as a caller's cast would)"""
    return c["idx"].astype(np_itype(c)), offsets_arg(c).astype(np_itype(c))


# ---- legality: the constructors' stated rules ------------------------------------------------------------------------------------------

def problems(c):
    """what a constructor or entry point would refuse about the case's configuration (an empty list: legal)"""
    bad = []
    fam, T, dims, rows = c["family"], c["T"], c["dims"], c["rows"]
    if not (1 <= T <= 7 and len(rows) == T and len(dims) == T and all(r >= 1 for r in rows)):
        bad.append("tables")
    if c["layout"] == "tbd" and len(set(dims)) != 1:
        bad.append('layout "tbd" needs one common dim')
    if fam in ("train", "max", "sequence"):
        vec = 4 if c["wdt"] == "f32" else 8
        if any(d % vec for d in dims):
            bad.append("dims must be multiples of %d" % vec)
        pads = c["pads"]
        per = [pads] * T if pads is None or isinstance(pads, int) else list(pads)
        if len(per) != T or any(k is not None and not -r <= k < r for k, r in zip(per, rows)):
            bad.append("padding_idx out of range")
    if fam == "train" and c["mean"] and c["psw"] is not None:
        bad.append("mean pooling is unweighted")
    if fam == "train" and c["psw"] is not None and max(dims) > PSW_GRAD_MAX_DIM[c["wdt"]]:
        bad.append("per_sample_weights_grad: dim beyond its limit")
    if fam == "sequence" and len(set(dims)) != 1:
        bad.append("the un-pooled lookup needs one common dim")
    if fam in ("qrows", "qmixed", "pruned"):
        uniform8 = fam == "qrows" and c["bits"][0] == 8
        mult = 4 if uniform8 else 8
        if any(d < mult or d % mult or d > 4096 for d in dims) or any(b not in (8, 4) for b in c["bits"]):
            bad.append("quantised dims / bitwidths")
        if fam == "qrows" and len(set(c["bits"])) != 1:
            bad.append("one format")
    if fam == "pruned":
        if all(m is None for m in c["remaps"]):
            bad.append("a pruned module needs a remap")
        for m, r, p in zip(c["remaps"], rows, c["phys_rows"]):
            if m is not None and (m.size != r or m.size == 0 or m.min() < -1 or m.max() >= p):
                bad.append("remap values")
    if fam in ("f8", "f8s"):
        if any(d < 16 or d % 16 or d > 2048 for d in dims):
            bad.append("FP8 dims")
    if fam in ("f8", "f8s", "mx4") and c["pool"] == "mean" and c["psw"] is not None:
        bad.append("mean pooling is unweighted")
    if fam == "f8s":
        for (E_t, e_rows), r in zip(c["exps"], rows):
            one = E_t is not None and e_rows is None and F8S.EXP_MIN <= E_t <= F8S.EXP_MAX
            per = E_t is None and e_rows is not None and e_rows.shape == (r,) and F8S.EXP_MIN <= e_rows.min() and e_rows.max() <= F8S.EXP_MAX
            if not (one if c["scale"] == "table" else per):
                bad.append("exponents")
    if fam == "anyfmt":
        for f, d, e, tab, r in zip(c["fmts"], dims, c["exps"], c["tables"], rows):
            mult = 16 if f.startswith("fp8") else 8
            if f not in A.FORMATS or d < mult or d % mult or d > 2048:
                bad.append("mixed-format dims / formats")
            if not F8S.EXP_MIN <= e <= F8S.EXP_MAX or (e != 0 and not f.startswith("fp8")):
                bad.append("exponent")
            if tab.shape != (r, A.row_bytes(f, d)) or tab.dtype != np.uint8:
                bad.append("table bytes")
    if fam == "mx4":
        if any(d < 32 or d % 32 or d > 2048 for d in dims):
            bad.append("MXFP4 dims")
        for tab, r, d in zip(c["tables"], rows, dims):
            sc = tab[:, d // 2:d // 2 + d // 32]
            if tab.shape != (r, M4.row_bytes(d)) or (((sc < 2) | (sc > 252)) & (sc != 255)).any():
                bad.append("MXFP4 table bytes / scale bytes")
    if fam in ("f8s", "mx4") and c["src"] not in ODTS:
        bad.append("quantiser source dtype")
    if c["slice"] is not None:
        b0, n = c["slice"]
        if not (0 <= b0 and 0 <= n and b0 + n <= c["B"]):
            bad.append("batch slice")
    undamaged = not c.get("damaged")
    if undamaged:
        own = P.table_of(c["off"], T, c["B"], c["idx"].size)
        if c["idx"].size and not ((c["idx"] >= 0) & (c["idx"] < np.asarray(rows)[own])).all():
            bad.append("indices out of range in an undamaged request")
        if c["off"][0] != 0 or c["off"][-1] != c["idx"].size or (np.diff(c["off"]) < 0).any():
            bad.append("offsets")
    return bad


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------

def _both(cases, f):
    seen = {bool(f(c)) for c in cases}
    return seen == {True, False}


def _all_of(cases, f, values):
    return {f(c) for c in cases} >= set(values)


def coverage(family, cases):
    """name -> bool for every coverage condition of ``family`` over the generated ``cases``.

    ``slice_off_tile``: a non-empty slice whose ``bag_begin`` is odd (``off_tile``).  Plans tile a batch in powers of two of at least 2
    bags, so such a slice begins inside a tile of the whole batch; the GPU test holds the first such seed (``off_tile_seed``) to the
    ``bags_per_block`` of the plan it reads."""
    cov = {
        "index_types": _all_of(cases, lambda c: c["itype"], ("i32", "i64")),
        "layouts": _all_of(cases, lambda c: c["layout"], ("bd", "tbd")),
        "trailing_offset": _both(cases, lambda c: c["trailing"]),
        "common_dims": _both(cases, lambda c: c["same_dims"]),
        "modes": _all_of(cases, lambda c: c["mode"], MODES),
        "long_bag": any(c["long_bag"] is not None and not c.get("damaged") for c in cases),      # (the GPU test asserts it unstaged)
        "empty_table": any((c["lens"].reshape(c["T"], c["B"]).sum(axis=1) == 0).any() for c in cases),
        "empty_first_bag": _both(cases, lambda c: c["lens"][0] == 0),
        "empty_last_bag": _both(cases, lambda c: c["lens"][-1] == 0),
        "no_slice": _both(cases, lambda c: c["slice"] is None),
        "slice_of_no_bags": any(c["slice"] is not None and c["slice"][1] == 0 for c in cases),
        "slice_off_tile": any(off_tile(c) for c in cases),
    }
    if family == "sequence":
        del cov["common_dims"]
    if family in ("train", "max", "sequence"):
        cov["table_types"] = _all_of(cases, lambda c: c["wdt"], WDTS)
        cov["output_types"] = _all_of(cases, lambda c: c["odt"], ODTS)
        cov["padding_forms"] = _all_of(cases, lambda c: "none" if c["pads"] is None else "int" if isinstance(c["pads"], int) else "list",
                                       ("none", "int", "list"))
        cov["negative_padding"] = any(isinstance(c["pads"], int) and c["pads"] < 0 for c in cases)
    if family in ("train", "max"):
        cov["grad16"] = _both(cases, lambda c: c["grad16"])
    if family == "train":
        cov["mean"] = _both(cases, lambda c: c["mean"])
        cov["weighted"] = _both(cases, lambda c: c["psw"] is not None)
        cov["bounds_modes"] = _all_of(cases, lambda c: c["bounds"], ("none", "ignore", "warning"))
        cov["damaged"] = _both(cases, lambda c: c["damaged"])
        reps = [(c, BR.repair(*request_arrays(c), c["rows"], c["T"], c["B"])[2]) for c in cases if c["damaged"]]
        cov["index_defect"] = any(r[0] > 0 for _, r in reps)
        cov["offset_defect"] = any(r[1] > 0 for _, r in reps)
        cov["padded_mean_out16"] = any(c["pads"] is not None and c["mean"] and c["odt"] != "fp32" for c in cases)
        cov["mean_grad16_mixed_dims_padded"] = any(c["pads"] is not None and c["mean"] and c["grad16"] and not c["same_dims"] for c in cases)
        cov["repair_lands_on_padding_row"] = any(repair_hits_pad_zero(c) for c in cases if c["damaged"])
    if family == "max":
        cov["mixed_dims"] = any(not c["same_dims"] for c in cases)
    if family == "sequence":
        cov["kind_pairs"] = _all_of(cases, lambda c: (c["wdt"], c["odt"]), [(w, o) for w in WDTS for o in ODTS])
    if family in SERVING:
        cov["output_types"] = _all_of(cases, lambda c: c["odt"], ODTS)
        cov["nan_row"] = _both(cases, lambda c: c["nan"])
    if family in ("qrows", "qmixed", "pruned"):
        cov["weighted"] = _both(cases, lambda c: c["psw"] is not None)
        cov["formats"] = {b for c in cases for b in c["bits"]} == {8, 4}
    if family == "qmixed":
        cov["mixed_formats"] = any(len(set(c["bits"])) == 2 for c in cases)
    if family == "pruned":
        shares = [(m < 0).mean() for c in cases for m in c["remaps"] if m is not None]
        cov["pruned_0"] = any(s == 0.0 for s in shares)
        cov["pruned_100"] = any(s == 1.0 for s in shares)
        cov["pruned_part"] = any(0.0 < s < 1.0 for s in shares)
        cov["unpruned_table"] = any(m is None for c in cases for m in c["remaps"])
    if family == "anyfmt":
        cov["weighted"] = _both(cases, lambda c: c["psw"] is not None)
        cov["formats"] = {f for c in cases for f in c["fmts"]} >= set(A.FORMATS)
        cov["widest_formats"] = set().union(*[widest_formats(c) for c in cases]) >= set(A.FORMATS)
    if family in ("f8s", "mx4"):
        cov["source_types"] = _all_of(cases, lambda c: c["src"], ODTS)
    if family == "f8s":
        cov["exponent_kinds"] = _all_of(cases, lambda c: c["scale"], ("row", "table"))
    if family == "mx4":
        cov["pooling"] = _all_of(cases, lambda c: c["pool"], ("plain", "weighted", "mean"))
        cov["two_column_passes"] = any(max(c["dims"]) == 2048 for c in cases)
    if family in ("f8", "f8s"):
        cov["formats"] = _all_of(cases, lambda c: c["fmt"], F8.FORMATS)
        cov["pooling"] = _all_of(cases, lambda c: c["pool"], ("plain", "weighted", "mean"))
        cov["padding"] = _both(cases, lambda c: c["pads"] is not None)
    return cov


def off_tile(c):
    return c["slice"] is not None and c["slice"][0] % 2 == 1 and c["slice"][1] > 0


def off_tile_seed(family):
    """the first seed whose slice meets ``slice_off_tile``"""
    return next(s for s in range(SEEDS[family]) if off_tile(case(family, s)))


def widest_formats(c):
    """the formats of the widest table(s) of a mixed-format case with mixed dims (lane groups are sized for the widest table)"""
    if c["same_dims"]:
        return set()
    return {f for f, d in zip(c["fmts"], c["dims"]) if d == max(c["dims"])}


def repair_hits_pad_zero(c):
    """a bad index of the damaged request is repaired (to row 0) inside a table whose padding row is row 0"""
    idx, off = request_arrays(c)
    idx2, off2, _ = BR.repair(idx, off, c["rows"], c["T"], c["B"])
    changed = np.nonzero(idx2.astype(np.int64) != idx.astype(np.int64))[0]
    if not changed.size:
        return False
    pads = normal_pads(c["pads"], c["rows"])
    own = P.table_of(off2, c["T"], c["B"], idx.size)[changed]
    return any(t >= 0 and pads[t] == 0 for t in own)


def cases(family, n=None):
    return [case(family, s) for s in range(SEEDS[family] if n is None else n)]


def smallest_count(family, limit=400):
    """the smallest n for which ``cases(family, n)`` meets every condition of ``coverage``"""
    got = []
    for s in range(limit):
        got.append(case(family, s))
        if all(coverage(family, got).values()):
            return s + 1
    raise AssertionError(f"{family}: {limit} seeds do not meet {[k for k, v in coverage(family, got).items() if not v]}")


# ---- composed references ---------------------------------------------------------------------------------------------------------------

def widened(c):
    """the case's float tables as fp32 values (exact)"""
    return [E.to_f32(t, c["wdt"]) for t in c["tables"]]


def repaired(c):
    """(indices, offsets, report) the entry point works on: ``bounds_rules.repair`` of the request as handed over under ``ignore`` /
    ``warning``, the request itself (report None) under ``none``; the offsets keep the form they were handed over in"""
    idx, off = request_arrays(c)
    if c.get("bounds", "none") == "none":
        return idx, off, None
    return BR.repair(idx, off, c["rows"], c["T"], c["B"])


def slice_of(c, use_slice):
    if not use_slice or c["slice"] is None:
        return 0, c["B"]
    return c["slice"]


def train_forward(c, use_slice=False):
    """list of T arrays ``[bag_count, D_t]``: fp32 values, or uint16 bits of the 16-bit output -- bounds repair, then the padding filter,
    then mean or weights, then ``round16``"""
    idx, off, _ = repaired(c)
    b0, n = slice_of(c, use_slice)
    pads = normal_pads(c["pads"], c["rows"])
    W = widened(c)
    with np.errstate(all="ignore"):
        if c["odt"] != "fp32":
            return O.forward(W, idx, off, c["B"], pads, c["odt"], c["psw"], c["mean"], b0, n)
        if c["mean"]:
            return MR.forward(W, idx, off, c["B"], pads, b0, n)
        return P.forward(W, idx, off, c["B"], pads, c["psw"], b0, n)


def serving_forward(c, use_slice=False):
    """list of T fp32 arrays ``[bag_count, D_t]`` of a serving family's pooled rule (a 16-bit output is its one rounding: ``out_bits``)"""
    b0, n = slice_of(c, use_slice)
    idx, off = request_arrays(c)
    fam = c["family"]
    if fam in ("qrows", "qmixed"):
        return QM.forward(c["tables"], c["dims"], c["bits"], idx, off, c["B"], c["psw"], b0, n)
    if fam == "pruned":
        return PR.forward(c["tables"], c["dims"], c["bits"], c["remaps"], idx, off, c["B"], c["psw"], b0, n)
    if fam == "f8s":
        return F8S.forward(c["tables"], c["fmt"], c["exps"], idx, off, c["B"], normal_pads(c["pads"], c["rows"]), c["psw"], c["pool"] == "mean",
                           b0, n)
    if fam == "anyfmt":
        return A.forward(any_tables(c), idx, off, c["B"], c["psw"], b0, n)
    if fam == "mx4":      # the MXFP4 rule pools the stored values as the padded family does (tests/test_gpu_mx4.py: ``pool``), no padding row
        W = [M4.dequant(tab, d) for tab, d in zip(c["tables"], c["dims"])]
        with np.errstate(all="ignore"):
            if c["pool"] == "mean":
                return MR.forward(W, idx, off, c["B"], [None] * c["T"], b0, n)
            return P.forward(W, idx, off, c["B"], [None] * c["T"], c["psw"], b0, n)
    assert fam == "f8", fam
    return F8.forward(c["tables"], c["fmt"], idx, off, c["B"], normal_pads(c["pads"], c["rows"]), c["psw"], c["pool"] == "mean", b0, n)


def any_tables(c):
    """a mixed-format case's tables as tests/anyfmt_rules.py takes them"""
    return [A.make_table(f, tab, d, e) for f, tab, d, e in zip(c["fmts"], c["tables"], c["dims"], c["exps"])]


def serving_sequence(c, use_slice=False):
    """(fp32 ``[N, D]``, written bool ``[N]``) of a serving family's un-pooled rule (common dims)"""
    b0, n = slice_of(c, use_slice)
    idx, off = request_arrays(c)
    fam = c["family"]
    if fam in ("qrows", "qmixed"):
        return QM.gather(c["tables"], c["dims"][0], c["bits"], idx, off, c["B"], b0, n)
    if fam == "pruned":
        return PR.gather(c["tables"], c["dims"][0], c["bits"], c["remaps"], idx, off, c["B"], b0, n)
    if fam == "f8s":
        return F8S.sequence(c["tables"], c["fmt"], c["exps"], idx, off, c["B"], b0, n)
    if fam == "mx4":      # every element the stored value: a bit copy of the dequantised table's fp32 rows
        N, D = idx.size, c["dims"][0]
        W = [M4.dequant(tab, D).view(np.uint32) for tab in c["tables"]]
        rows = E.forward(W, "f32", "f32", idx, off, c["B"], np.zeros((N, D), dtype=np.uint32), b0, n)
        return rows.view(np.float32), E.in_slice(off, c["T"], c["B"], N, b0, n)[1]
    assert fam == "f8", fam
    return F8.sequence(c["tables"], c["fmt"], idx, off, c["B"], b0, n)


_KIND = {"fp32": "f32", "bf16": "bf16", "fp16": "f16"}


def serving_sequence_bits(c, use_slice=False):
    """(output bits ``[N, D]`` of the case's output dtype, written bool ``[N]``, copied bool ``[N]`` or None) of a serving family's
    un-pooled rule; ``copied`` (mixed-format float tables read into their own type): the row is a bit copy, NaNs included"""
    if c["family"] == "anyfmt":
        b0, n = slice_of(c, use_slice)
        idx, off = request_arrays(c)
        return A.sequence(any_tables(c), idx, off, c["B"], _KIND[c["odt"]], b0, n)
    rows32, written = serving_sequence(c, use_slice)
    return out_bits(rows32, c["odt"]), written, None


# ---- quantiser sources (``f8s``, ``mx4``) ------------------------------------------------------------------------------------------------

def quantiser_source(c, t):
    """fp32 ``[rows_t, D_t + 2 * SRC_PAD]``, every value exact in the case's source dtype ``c["src"]``: normal values under a power of
    two per row, one NaN inside the middle ``D_t`` columns (the source proper; the GPU test reads it contiguous and as the strided view)"""
    rng = np.random.default_rng([zlib.crc32(b"source"), c["seed"], t])
    r, d = c["rows"][t], c["dims"][t]
    x = (rng.standard_normal((r, d + 2 * SRC_PAD)) * np.exp2(rng.integers(-12, 9, (r, 1)))).astype(np.float32)
    x[int(rng.integers(0, r)), SRC_PAD + int(rng.integers(0, d))] = np.nan
    return x if c["src"] == "fp32" else O.widen(O.round16(x, c["src"]), c["src"])


def mx4_quantize(x32, chunk=64):
    """``mx4_rules.quantize`` a few rows at a time (its intermediate arrays hold eight fp64 values per element)"""
    return np.concatenate([M4.quantize(x32[i:i + chunk]) for i in range(0, x32.shape[0], chunk)])


def out_bits(x32, odt):
    """an fp32 rule output as the bits of the output dtype: uint32, or the one rounding to 16 bits"""
    x = np.ascontiguousarray(x32, dtype=np.float32)
    return x.view(np.uint32) if odt == "fp32" else O.round16(x, odt)


def join(parts, layout):
    """per-table ``[bags, D_t]`` arrays in the output's layout: ``[bags, sum D]`` or ``[T, bags, D]``"""
    return np.stack(parts) if layout == "tbd" else np.concatenate(parts, axis=1)


def split(a, dims, layout):
    """the inverse of ``join``"""
    if layout == "tbd":
        return [a[t] for t in range(len(dims))]
    cols = np.concatenate([[0], np.cumsum(dims)])
    return [a[:, cols[t]:cols[t + 1]] for t in range(len(dims))]


def canvas(whole_shape, layout, part, b0, n, sentinel_bits):
    """the caller's ``out`` after a sliced call: the sentinel everywhere but the slice's bags, which hold ``part`` (joined, ``n`` bags)"""
    out = np.full(whole_shape, sentinel_bits, dtype=part.dtype)
    if layout == "tbd":
        out[:, b0:b0 + n] = part
    else:
        out[b0:b0 + n] = part
    return out


def sentinel_bits(odt):
    return out_bits(np.array([SENTINEL], dtype=np.float32), odt)[0]


# ---- comparison -------------------------------------------------------------------------------------------------------------------------

def is_nan_bits(bits):
    b = np.asarray(bits)
    if b.dtype == np.uint32:
        return (b & 0x7fffffff) > 0x7f800000
    assert b.dtype == np.uint16, b.dtype
    return None


def same_bits(got, want, odt):
    """bit for bit where the rule has no NaN; where it has one, a NaN (its class: sign and payload are not part of the serving rules).
    ``got`` / ``want``: uint32 bits for ``"fp32"``, uint16 for ``"bf16"`` / ``"fp16"``."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if odt == "fp32":
        nan_w, nan_g = is_nan_bits(want), is_nan_bits(got)
    else:
        nan_w, nan_g = O.is_nan16(want, odt), O.is_nan16(got, odt)
    return bool(np.array_equal(got[~nan_w], want[~nan_w]) and nan_g[nan_w].all())


def hot_row_bound(cnt, mag):
    """the bound for the sorted backward against the fp64 sum -- the ONE copy: the base fuzz (tests/test_gpu_fuzz.py, ``tol_sorted``,
    where its derivation is written down) calls it too.  ``cnt``: lookups per row ``[rows, 1]``, ``mag``: the fp64 sum of the
    contributions' magnitudes"""
    return np.maximum(1e-5, (256 + cnt / 32) * 2.0 ** -24) * mag + 1e-30


# ---- deliberately wrong references (tests/test_fuzz_cases_host.py: the comparison must notice them) --------------------------------------

def drop_last_of_longest(c):
    """a copy of the case whose longest bag has lost its last lookup (an undamaged request)"""
    T, B = c["T"], c["B"]
    off = c["off"].astype(np.int64)
    g = int(np.argmax(np.diff(off)))
    j = int(off[g + 1]) - 1
    d = dict(c)
    d["idx"] = np.delete(c["idx"], j)
    d["off"] = off - (np.arange(T * B + 1) > g)
    if c.get("psw") is not None:
        d["psw"] = np.delete(c["psw"], j)
    d["lens"] = np.diff(d["off"])
    return d


def shift_slice(c):
    """a copy of the case whose batch slice begins one bag later (or earlier, at the end of the batch)"""
    b0, n = c["slice"]
    d = dict(c)
    d["slice"] = (b0 + 1, n) if b0 + n < c["B"] else (b0 - 1, n)
    return d
