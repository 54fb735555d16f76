"""numpy restatement of the FP8 TABLES rule (include/param_amd.h, "FP8 TABLES").  Tables travel as uint8 code arrays ``[rows, D]``;
``fmt`` is ``"e4m3"`` (OCP e4m3fn) or ``"e5m2"``.

* ``dec``: the fp32 value of every code, written arithmetically from the format's fields (no cast of any library): sign, exponent
  field ``E`` with its bias, mantissa field ``M`` of ``m`` bits -- ``(-1)^s * 2^(E - bias) * (1 + M / 2^m)`` for ``E > 0``, the
  subnormal ``(-1)^s * 2^(1 - bias) * M / 2^m`` for ``E == 0``; e4m3fn has no infinities and its two all-ones codes are NaN; e5m2 is
  IEEE-like, exponent field 31 is +-Inf (``M == 0``) or NaN.  tests/test_f8_host.py holds it to torch's CPU casts for all 256 codes.
* pooled: the padded family's rule over the decoded table, by import -- tests/padding_rules.py (sum, weighted sum), tests/mean_rules.py
  (mean), tests/out16_rules.py (the one rounding of a 16-bit output).
* un-pooled: ``dec`` of the looked-up row; a 16-bit output is its one rounding (exact: every FP8 value is a bf16 and an fp16 value).

NaN codes must give a NaN; sign and payload are not part of the rule (compare with ``qrows_rules.same_f32`` / ``out16_rules.same_bits``)."""
import numpy as np

from tests import mean_rules as M
from tests import out16_rules as O
from tests import padding_rules as P

FORMATS = ("e4m3", "e5m2")
_FIELDS = {"e4m3": (4, 3, 7), "e5m2": (5, 2, 15)}      # exponent bits, mantissa bits, bias


def dec(codes, fmt):
    """fp32 array of the values of the uint8 array ``codes``"""
    ebits, mbits, bias = _FIELDS[fmt]
    c = np.asarray(codes, dtype=np.uint8).astype(np.int64)
    sign = np.where(c & 0x80, -1.0, 1.0)
    E = (c >> mbits) & ((1 << ebits) - 1)
    Mf = (c & ((1 << mbits) - 1)).astype(np.float64) / (1 << mbits)
    val = np.where(E > 0, np.ldexp(1.0 + Mf, E - bias), np.ldexp(Mf, 1 - bias))       # exact in fp64, and in fp32 after the cast
    if fmt == "e4m3":
        val = np.where((c & 0x7f) == 0x7f, np.nan, val)
    else:
        top = E == (1 << ebits) - 1
        val = np.where(top, np.where((c & 3) == 0, np.inf, np.nan), val)
    with np.errstate(invalid="ignore"):
        out = (sign * val).astype(np.float32)
    # a NaN code's sign bit is the code's (what a conversion that moves the fields gives; not part of the rule)
    out = np.where(np.isnan(out), ((c.astype(np.uint32) & 0x80) << 24 | 0x7fc00000).astype(np.uint32).view(np.float32), out)
    assert np.array_equal(out[np.isfinite(out)].astype(np.float64), (sign * val)[np.isfinite(out)]), "every finite code is exact in fp32"
    return out


def finite_codes(rng, fmt, shape):
    """uint8 codes drawn from ``rng``, all of them finite: a NaN (e5m2: or Inf) code has its top two bits cleared"""
    c = rng.integers(0, 256, shape, dtype=np.uint8)
    bad = (c & 0x7f) == 0x7f if fmt == "e4m3" else (c & 0x7f) >= 0x7c
    return np.where(bad, c & 0x3f, c).astype(np.uint8)


def is_nan_code(codes, fmt):
    c = np.asarray(codes, dtype=np.uint8)
    return (c & 0x7f) == 0x7f if fmt == "e4m3" else (c & 0x7f) > 0x7c


def widened(tables, fmt):
    return [dec(t, fmt) for t in tables]


def forward(tables, fmt, indices, offsets, B, pads=None, psw=None, mean=False, bag_begin=0, bag_count=None):
    """list of T fp32 arrays ``[bag_count, D_t]``: the pooled rule.  ``pads``: None or a list of ``int | None`` per table."""
    pads = [None] * len(tables) if pads is None else pads
    W = widened(tables, fmt)
    with np.errstate(all="ignore"):
        if mean:
            assert psw is None
            return M.forward(W, indices, offsets, B, pads, bag_begin, bag_count)
        return P.forward(W, indices, offsets, B, pads, psw, bag_begin, bag_count)


def forward16(tables, fmt, indices, offsets, B, dtype, pads=None, psw=None, mean=False, bag_begin=0, bag_count=None):
    """the same as uint16 bit patterns of ``dtype`` (``"bf16"`` / ``"fp16"``): one rounding of the fp32 result"""
    return [O.round16(o, dtype) for o in forward(tables, fmt, indices, offsets, B, pads, psw, mean, bag_begin, bag_count)]


def sequence(tables, fmt, indices, offsets, B, bag_begin=0, bag_count=None):
    """(rows fp32 ``[N, D]``, written bool ``[N]``): the un-pooled rule for tables of one common dim -- row j is ``dec`` of row
    ``indices[j]`` of the table that owns position j; positions outside the bag slice are not written (zeros here)"""
    T = len(tables)
    idx = np.asarray(indices).astype(np.int64)
    N = idx.size
    bag_count = B - bag_begin if bag_count is None else bag_count
    owner = P.table_of(offsets, T, B, N)
    start, end = P.bag_bounds(offsets, T, B, N)
    out = np.zeros((N, tables[0].shape[1]), dtype=np.float32)
    written = np.zeros(N, dtype=bool)
    pos = np.arange(N)
    for t in range(T if bag_count else 0):             # (a table at a time: its positions inside the slice, all at once)
        lo, hi = int(start[t * B + bag_begin]), int(end[t * B + bag_begin + bag_count - 1])
        sel = (owner == t) & (pos >= lo) & (pos < hi)
        out[sel] = dec(tables[t][idx[sel]], fmt)
        written[sel] = True
    return out, written


def sequence16(rows32, dtype):
    return O.round16(rows32, dtype)


def same16(got, want, dtype):
    """``qrows_rules.same_f32``'s convention for uint16 bit patterns of ``dtype``: equal bit for bit where ``want`` is not a NaN; where
    it is, ``got`` is a NaN.  ``out16_rules.same_bits`` but for a NaN's sign, which is not part of this rule: neither torch's CPU casts
    nor the hardware conversion promise one."""
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    nan = O.is_nan16(want, dtype)
    return bool(got.shape == want.shape and np.array_equal(got[~nan], want[~nan]) and O.is_nan16(got[nan], dtype).all())
