"""numpy restatement of the SCALED FP8 TABLES rule (include/param_amd.h), on top of tests/f8_rules.py's ``dec``.  Tables travel as
uint8 code arrays ``[rows, D]`` with their exponents ``(E_t, e_rows)``: an int and an int array ``[rows]``, either may be None (= 0).

* ``dequant``: ``v = dec(code) * 2^(E_t + e_r)`` -- ``np.ldexp`` of the fp32 value, exact for ``E_t + e_r`` in [-64, 64].
* pooled / un-pooled: tests/f8_rules.py's rules with ``v`` in the place of ``dec(code)`` (the padded family's rule over the dequantised
  table: tests/padding_rules.py, tests/mean_rules.py, tests/out16_rules.py).
* the quantiser: ``row_exponents`` (the smallest exponent at which a row does not overflow, from ``np.frexp`` of its largest finite
  magnitude -- the library reads the same two fields with integer arithmetic), ``cast`` (round to nearest even into the format, written
  from the format's fields; tests/test_f8s_host.py holds it to torch's CPU cast), ``quantize`` (``cast(x * 2^-s)``).

Sources are fp32 arrays: a bf16 / fp16 source is widened exactly before it gets here.  NaN codes are compared by class only."""
import numpy as np

from tests import f8_rules as R
from tests import mean_rules as M
from tests import out16_rules as O
from tests import padding_rules as P

FORMATS = R.FORMATS
EXP_MIN, EXP_MAX = -64, 64
FMAX_EXP = {"e4m3": 8, "e5m2": 15}                      # fmax = 1.75 * 2^k: 448, 57344
FMAX = {"e4m3": 448.0, "e5m2": 57344.0}
_MAXCODE = {"e4m3": 0x7e, "e5m2": 0x7b}                 # the code of fmax
_OVER = {"e4m3": 0x7f, "e5m2": 0x7c}                    # what the midpoint above fmax and everything beyond gives: NaN | Inf


def exponent_sum(E, e_rows, rows):
    s = np.zeros(rows, dtype=np.int64) + (0 if E is None else int(E))
    if e_rows is not None:
        s = s + np.asarray(e_rows).astype(np.int64)
    assert ((s >= EXP_MIN) & (s <= EXP_MAX)).all()
    return s


def dequant(codes, fmt, E=None, e_rows=None):
    """fp32 ``[rows, D]``: the stored values"""
    codes = np.asarray(codes, dtype=np.uint8)
    s = exponent_sum(E, e_rows, codes.shape[0])
    with np.errstate(invalid="ignore"):
        v = np.ldexp(R.dec(codes, fmt), s[:, None].astype(np.int32)).astype(np.float32)
    finite = np.isfinite(v)
    assert (np.abs(v[finite & (v != 0)]) >= 2.0 ** -126).all(), "every stored value is a normal fp32 number"
    return v


def widened(tables, fmt, exps):
    return [dequant(t, fmt, *e) for t, e in zip(tables, exps)]


def forward(tables, fmt, exps, indices, offsets, B, pads=None, psw=None, mean=False, bag_begin=0, bag_count=None):
    """list of T fp32 arrays ``[bag_count, D_t]``: the pooled rule.  ``exps``: a list of ``(E_t | None, e_rows | None)`` per table"""
    pads = [None] * len(tables) if pads is None else pads
    W = widened(tables, fmt, exps)
    with np.errstate(all="ignore"):
        if mean:
            assert psw is None
            return M.forward(W, indices, offsets, B, pads, bag_begin, bag_count)
        return P.forward(W, indices, offsets, B, pads, psw, bag_begin, bag_count)


def sequence(tables, fmt, exps, indices, offsets, B, bag_begin=0, bag_count=None):
    """(rows fp32 ``[N, D]``, written bool ``[N]``): the un-pooled rule (tests/f8_rules.py: ``sequence``) over the stored values"""
    T = len(tables)
    W = widened(tables, fmt, exps)
    idx = np.asarray(indices).astype(np.int64)
    N = idx.size
    bag_count = B - bag_begin if bag_count is None else bag_count
    owner = P.table_of(offsets, T, B, N)
    start, end = P.bag_bounds(offsets, T, B, N)
    out = np.zeros((N, tables[0].shape[1]), dtype=np.float32)
    written = np.zeros(N, dtype=bool)
    pos = np.arange(N)
    for t in range(T if bag_count else 0):
        lo, hi = int(start[t * B + bag_begin]), int(end[t * B + bag_begin + bag_count - 1])
        sel = (owner == t) & (pos >= lo) & (pos < hi)
        out[sel] = W[t][idx[sel]]
        written[sel] = True
    return out, written


# ---- the quantiser ---------------------------------------------------------------------------------------------------------------------

def row_exponents(x, fmt):
    """int8 ``[rows]``: amax over the row's finite elements = m * 2^q with 1 <= m < 2; e = q - k if m <= 1.75 else q - k + 1, clamped to
    [-64, 64]; -64 for a row of zeros or without a finite element"""
    x = np.asarray(x, dtype=np.float32)
    a = np.where(np.isfinite(x), np.abs(x), np.float32(0.0)).max(axis=1)
    m, q = np.frexp(a.astype(np.float64))               # a = m * 2^q with 0.5 <= m < 1
    m, q = 2.0 * m, q.astype(np.int64) - 1
    e = q - FMAX_EXP[fmt] + (m > 1.75)
    e = np.where(a == 0, EXP_MIN, np.clip(e, EXP_MIN, EXP_MAX))
    return e.astype(np.int8)


def cast(y, fmt):
    """uint8 codes of the fp32 array ``y``: round to nearest even on the format's grid; a NaN -> a NaN code (0x7f with the value's sign);
    what rounds past fmax -- e4m3fn: above the midpoint 464, e5m2: from the midpoint 61440 on (the tie goes to the even code) -- and
    +-Inf -> e4m3fn's NaN 0x7f / e5m2's +-Inf 0x7c: the code that follows fmax's; a zero keeps its sign"""
    _, mbits, bias = R._FIELDS[fmt]
    y = np.asarray(y, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        a = np.abs(y).astype(np.float64)
    grid = R.dec(np.arange(_MAXCODE[fmt] + 1, dtype=np.uint8), fmt).astype(np.float64)      # ascending: code = position
    grid = np.append(grid, FMAX[fmt] + 2.0 ** (FMAX_EXP[fmt] - mbits))      # ... and the value the next code would have: 480, 65536
    with np.errstate(invalid="ignore", divide="ignore"):
        _, q = np.frexp(np.where(np.isfinite(a) & (a > 0), a, 1.0))
        quantum = np.ldexp(1.0, np.maximum(q - 1, 1 - bias) - mbits)              # the spacing of the format's values around |y|
        r = np.rint(a / quantum) * quantum                                        # rint: to nearest, ties to even; exact in fp64
    r = np.where(np.isfinite(a), np.minimum(r, grid[-1]), grid[-1])
    code = np.searchsorted(grid, r).astype(np.int64)
    assert np.array_equal(grid[code], r) and _OVER[fmt] == len(grid) - 1
    code = np.where(np.isnan(y), 0x7f, code)
    return (code | np.where(np.signbit(y), 0x80, 0)).astype(np.uint8)


def quantize(x, fmt, exponents):
    """uint8 ``[rows, D]``: ``cast(x * 2^-s)`` with ``s`` an int (the table's exponent) or an int array ``[rows]``; the product is one
    fp32 multiplication by a power of two"""
    x = np.asarray(x, dtype=np.float32)
    s = np.broadcast_to(np.asarray(exponents, dtype=np.int64), (x.shape[0],))
    assert ((s >= EXP_MIN) & (s <= EXP_MAX)).all()
    inv = np.ldexp(np.float32(1.0), (-s).astype(np.int32)).astype(np.float32)
    with np.errstate(all="ignore"):
        return cast(x * inv[:, None], fmt)


def same_codes(got, want, fmt):
    """equal byte for byte where ``want`` is not a NaN code; where it is, ``got`` is a NaN code"""
    got, want = np.asarray(got, dtype=np.uint8), np.asarray(want, dtype=np.uint8)
    nan = R.is_nan_code(want, fmt)
    return bool(got.shape == want.shape and np.array_equal(got[~nan], want[~nan]) and R.is_nan_code(got[nan], fmt).all())


def same16(got, want, dtype):
    return R.same16(got, want, dtype)


def round16(x32, dtype):
    return O.round16(x32, dtype)
