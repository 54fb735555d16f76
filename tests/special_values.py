"""The one set of non-finite, signed-zero, subnormal and near-overflow values the tests feed the kernels and the oracle (numpy only,
no device), the builders that place them in tables, gradients and per-sample weights, and the two comparisons every such test uses.
Used by tests/golden/gen_special_values.py, tests/test_special_values_host.py and tests/test_gpu_special_values.py.

No tolerance is defined here: ``same_class`` takes the bars of its caller, which are the named ones of tests/elem_adagrad_rules.py,
tests/lowp_rules.py and the fuzz test's ``tol_sorted``.
"""
import numpy as np

F32 = np.float32
FLT_TRUE_MIN = np.array([1], np.uint32).view(F32)[0]             # 1e-45
FLT_SUB_MAX = np.array([0x007FFFFF], np.uint32).view(F32)[0]     # the largest subnormal
FLT_MIN = np.finfo(F32).tiny
FLT_MAX = np.finfo(F32).max

with np.errstate(all="ignore"):
    F32_SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, FLT_TRUE_MIN, -FLT_TRUE_MIN, 1e-40, -1e-40, FLT_SUB_MAX, FLT_MIN, -FLT_MIN,
                             3e38, -3e38, FLT_MAX, -FLT_MAX,
                             1.0, -2.5, 0.375, 1e-3, 123456.0], dtype=F32)      # (the handful of ordinary values)
N_SPECIAL = 16                                                                   # F32_SPECIALS[:N_SPECIAL] are the special ones
F32_FINITE_SPECIALS = F32_SPECIALS[:N_SPECIAL][np.isfinite(F32_SPECIALS[:N_SPECIAL])]
# of one sign and absorbing or exact under addition in any order: what rows beyond the exact-run limit may hold
F32_ONE_SIGN = np.array([3e38, np.inf, np.nan, FLT_TRUE_MIN, 1e-40, FLT_SUB_MAX], dtype=F32)

# table BITS of the 16-bit dtypes: +-0, smallest / largest subnormal, smallest normal, largest finite (both signs), +-Inf, one NaN
BF16_BITS = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x807F, 0x0080, 0x8080, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0], np.uint16)
F16_BITS = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x8400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00], np.uint16)
KINDS = ("f32", "bf16", "f16")


def widen16(bits, kind):
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if kind == "bf16":
        return (bits.astype(np.uint32) << 16).view(F32)
    return bits.view(np.float16).astype(F32)


def is_nan(a, kind="f32"):
    a = np.asarray(a)
    if a.dtype == np.uint16:
        assert kind in ("bf16", "f16")
        return (a & 0x7FFF) > (0x7F80 if kind == "bf16" else 0x7C00)
    return np.isnan(a)


def is_special(a, kind="f32"):
    """elements that are NaN, +-Inf, +-0, subnormal, the smallest normal or within a factor of ~1.13 of the largest finite value of their type"""
    a = np.asarray(a)
    if a.dtype == np.uint16:
        m = a & 0x7FFF
        if kind == "bf16":
            return (m <= 0x0080) | (m >= 0x7F7F)
        return (m <= 0x0400) | (m >= 0x7BFF)
    x = np.abs(a.astype(F32))
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(x) | (x <= FLT_MIN) | (x >= F32(3e38))


def is_subnormal(a):
    x = np.abs(np.asarray(a, dtype=F32))
    with np.errstate(invalid="ignore"):
        return (x > 0) & (x < FLT_MIN)


def same_bits(a, b, kind="f32"):
    """NaN at the same places, every other element equal as raw bits (so the sign of zero and of Inf count); NaN payloads are the one
    thing never compared.  fp32 arrays, or uint16 table bits with ``kind`` "bf16" / "f16"."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = is_nan(a, kind), is_nan(b, kind)
    if not np.array_equal(na, nb):
        return False
    if a.dtype != np.uint16:
        assert a.dtype == F32
        a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    return bool(np.array_equal(a[~na], b[~na]))


def first_difference(a, b, kind="f32"):
    """for assertion messages: index and the two values of the first element ``same_bits`` objects to (None if none)"""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = is_nan(a, kind), is_nan(b, kind)
    ra = a if a.dtype == np.uint16 else np.ascontiguousarray(a).view(np.uint32)
    rb = b if b.dtype == np.uint16 else np.ascontiguousarray(b).view(np.uint32)
    bad = (na != nb) | (~na & ~nb & (ra != rb))
    if not bad.any():
        return None
    i = tuple(int(k) for k in np.argwhere(bad)[0])
    return i, a[i], b[i], int(bad.sum())


def same_class(a, b, rtol, atol):
    """NaN, +Inf and -Inf at the same places; finite elements within ``atol + rtol * |b|`` (``atol`` may be an array: a derived bound
    per element).  The bars are the caller's."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    for pick in (np.isnan, np.isposinf, np.isneginf):
        if not np.array_equal(pick(a), pick(b)):
            return False
    f = np.isfinite(b)
    lim = (np.broadcast_to(np.asarray(atol, dtype=np.float64), b.shape) + rtol * np.abs(np.where(f, b, 0.0)))[f]
    return bool((np.abs(a[f] - b[f]) <= lim).all())


def same_nonfinite(a, b):
    """NaN, +Inf and -Inf at the same places, and nothing more (``same_class`` without bars)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and all(np.array_equal(pick(a), pick(b)) for pick in (np.isnan, np.isposinf, np.isneginf))


# ----------------------------------------------------------------------------- builders
def _ordinary(rng, shape):
    return rng.standard_normal(shape).astype(F32)


def special_rows_f32(D, specials=F32_SPECIALS[:N_SPECIAL]):
    """(const, mixed): ``[n, D]`` rows constant at each special, and ``[n, D]`` rows that alternate the special with ordinary values
    (1.5, -0.75: exact in every table type) in adjacent columns, the special first in even rows of the pair and second in odd ones --
    one 16-byte lane load holds both."""
    n = len(specials)
    const = np.repeat(np.asarray(specials, dtype=F32)[:, None], D, axis=1)
    mixed = np.empty((n, D), F32)
    fill = np.where(np.arange(D) % 4 < 2, F32(1.5), F32(-0.75))
    for k, v in enumerate(specials):
        at = (np.arange(D) % 2) == (k % 2)
        mixed[k] = np.where(at, v, fill)
    return const, mixed


def special_table_f32(rows, D, rng, specials=F32_SPECIALS[:N_SPECIAL]):
    """``[rows, D]`` fp32: rows [0, n) constant specials, [n, 2n) mixed, the rest ordinary (standard normal); n = len(specials)"""
    const, mixed = special_rows_f32(D, specials)
    n = len(specials)
    assert rows >= 2 * n + 1
    return np.concatenate([const, mixed, _ordinary(rng, (rows - 2 * n, D))], axis=0)


def special_table_bits(rows, D, rng, kind):
    """uint16 ``[rows, D]`` table bits of ``kind`` "bf16" / "f16", laid out as ``special_table_f32``: constant rows of each special
    bit pattern, mixed rows (special next to 1.5 / -0.75), ordinary rows (standard normal rounded to the type)"""
    sp = BF16_BITS if kind == "bf16" else F16_BITS
    n = len(sp)
    assert rows >= 2 * n + 1
    const = np.repeat(sp[:, None], D, axis=1)
    one5, m075 = (0x3FC0, 0xBF40) if kind == "bf16" else (0x3E00, 0xBA00)
    fill = np.where(np.arange(D) % 4 < 2, one5, m075).astype(np.uint16)
    mixed = np.stack([np.where((np.arange(D) % 2) == (k % 2), v, fill) for k, v in enumerate(sp)]).astype(np.uint16)
    o = _ordinary(rng, (rows - 2 * n, D))
    if kind == "bf16":
        u = o.view(np.uint32)
        ob = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    else:
        ob = o.astype(np.float16).view(np.uint16)
    return np.concatenate([const, mixed, ob], axis=0)


def special_table(rows, D, rng, kind):
    """(what to copy into the module's table -- fp32 values or uint16 bits, the same values widened to fp32)"""
    if kind == "f32":
        w = special_table_f32(rows, D, rng)
        return w, w
    b = special_table_bits(rows, D, rng, kind)
    return b, widen16(b, kind)


def n_special_rows(kind):
    """rows [0, n) of a special table are constant, [n, 2n) mixed"""
    return N_SPECIAL if kind == "f32" else len(BF16_BITS)


def special_grad(B, D, rng, specials=F32_SPECIALS[:N_SPECIAL]):
    """``[B, D]`` bag gradient: bags [0, n) constant specials, [n, 2n) mixed, the rest ordinary"""
    return special_table_f32(B, D, rng, specials)


PSW_SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-30, 1e-40], dtype=F32)


def special_weights(n, rng, every=5, specials=PSW_SPECIALS):
    """``n`` per-sample weights: every ``every``-th one a special (in turn), the others uniform in [0.5, 1.5)"""
    w = rng.uniform(0.5, 1.5, n).astype(F32)
    at = np.arange(0, n, every)
    w[at] = np.asarray(specials, dtype=F32)[np.arange(len(at)) % len(specials)]
    return w


# finite edge rows of the row-wise quantiser and the rows that mix both zero signs at the minimum
def quant_edge_rows(dim):
    """``[n, dim]`` fp32 finite edge rows for the 8 / 4 / 2-bit quantisers (zeros, where present, all carry ONE sign) and their names"""
    k = np.arange(dim)
    rows = {
        "all_subnormal": (F32(1e-40) * (1 + k % 7)).astype(F32),
        "all_minus_zero": np.full(dim, -0.0, F32),
        "all_plus_zero": np.zeros(dim, F32),
        "range_overflows_f32": np.where(k % 2 == 0, F32(3e38), F32(-3e38)).astype(F32),
        "one_ulp_at_1": np.where(k % 3 == 0, np.nextafter(F32(1), F32(2)), F32(1)).astype(F32),
        "one_subnormal_outlier": np.where(k == dim // 2, F32(1e-40), F32(0.25)).astype(F32),
        "negative_subnormals": (F32(-1e-41) * (1 + k % 5)).astype(F32),
        "pm_30000": np.where(k % 2 == 0, F32(30000), F32(-30000)).astype(F32),
        "range_1e-9_at_5": (F32(5) + F32(1e-9) * (k % 4)).astype(F32),
        "zero_and_one_1e-44": np.where(k == 3, F32(1e-44), F32(0)).astype(F32),
        "minus_zero_and_positive": np.where(k % 2 == 0, F32(-0.0), F32(0.5) + k).astype(F32),
        "ordinary": np.linspace(-3, 7, dim).astype(F32),
    }
    return np.stack(list(rows.values())), list(rows)


def quant_mixed_zero_rows(dim):
    """rows whose minimum is zero and in which BOTH zero signs occur: torch stores the sign of the FIRST zero as the bias"""
    k = np.arange(dim)
    a = np.where(k % 2 == 0, F32(-0.0), F32(0.0)).astype(F32)               # -0 first
    b = np.where(k % 2 == 0, F32(0.0), F32(-0.0)).astype(F32)               # +0 first
    c = np.where(k == 1, F32(-0.0), np.where(k == dim - 1, F32(0.0), F32(1) + k)).astype(F32)    # -0 at 1, +0 last, positives around
    d = np.where(k == 2, F32(0.0), np.where(k == dim - 2, F32(-0.0), F32(2.5))).astype(F32)      # +0 first, -0 late
    return np.stack([a, b, c, d])


# ----------------------------------------------------------------------------- requests
def special_index(kind):
    """row of the constant-special block that holds each named value"""
    if kind == "f32":
        return dict(pz=0, nz=1, pinf=2, ninf=3, nan=4, sub_a=5, sub_b=7, big=12, nbig=13)
    return dict(pz=0, nz=1, pinf=10, ninf=11, nan=12, sub_a=2, sub_b=2, big=8, nbig=9)


def named_bags(kind, weighted, L=None):
    """The single-purpose bags: ``[(name, rows, weights, expected)]``.  ``expected``: "+0" | "nan" | "+inf" | "sum2" (the exact sum of
    two subnormal rows: non-zero, and subnormal in fp32 unless the table is fp16) | a float.  With ``L`` (fixed pooling) every bag is
    padded to L lookups with the +0 row at weight 1 (the -0 bag: with the -0 row) and the empty bag is left out."""
    ix = special_index(kind)
    big3 = 65504.0 if kind == "f16" else "+inf"           # 65504 + 65504 - 65504 stays finite in fp32; 3e38 + 3e38 does not
    bags = [("minus_zero_alone", [ix["nz"]], [1.0], "+0"),
            ("inf_and_minus_inf", [ix["pinf"], ix["ninf"]], [1.0, 1.0], "nan"),
            ("empty_between_specials", [], [], "+0"),
            ("big_big_minus_big", [ix["big"], ix["big"], ix["nbig"]], [1.0, 1.0, 1.0], big3),
            ("two_subnormals", [ix["sub_a"], ix["sub_b"]], [1.0, 1.0], "sum2"),
            ("zero_weight_on_inf", [ix["pinf"]], [0.0], "nan" if weighted else "+inf"),
            ("minus_zero_twice", [ix["nz"], ix["nz"]], [1.0, 1.0], "+0")]
    if L is not None:
        assert L >= 3
        bags = [(n, r + [ix["nz"] if n.startswith("minus_zero") else ix["pz"]] * (L - len(r)), w + [1.0] * (L - len(r)), e)
                for n, r, w, e in bags if r]
    return bags


def check_named_bag(name, expected, got_row, parts):
    """``got_row``: the pooled fp32 row of a named bag (constant rows: every column alike); ``parts``: the fp32 rows it pooled"""
    g = np.asarray(got_row, dtype=F32)
    if expected == "+0":
        ok = bool((g.view(np.uint32) == 0).all())
    elif expected == "nan":
        ok = bool(np.isnan(g).all())
    elif expected == "+inf":
        ok = bool(np.isposinf(g).all())
    elif expected == "sum2":
        want = (parts[0].astype(np.float64) + parts[1].astype(np.float64)).astype(F32)
        ok = bool((want != 0).all()) and same_bits(g, want)
    else:
        ok = bool((g == F32(expected)).all())
    assert ok, (name, expected, g[:4])


def forward_request(kind, rows, B, rng, L=None, weighted=False):
    """TBE request (int64 ``idx``, ``off`` [T*B+1], fp32 ``psw`` or None, the named bags) over special tables of ``rows[t]`` rows each:
    in every table bags [0, k) are the named bags, the others draw half their lookups from the special rows and half from all rows;
    ``L`` lookups each (fixed pooling) or 0 .. 6 (ragged).  Weighted: every fifth weight of the drawn bags is a special one."""
    named = named_bags(kind, weighted, L)
    n2 = 2 * n_special_rows(kind)
    idx, psw, lens = [], [], []
    for r in rows:
        assert B > len(named) and r > n2
        for _, rr, ww, _ in named:
            idx += rr
            psw += ww
            lens.append(len(rr))
        ln = np.full(B - len(named), L) if L is not None else rng.integers(0, 7, B - len(named))
        n = int(ln.sum())
        ix = np.where(rng.random(n) < 0.5, rng.integers(0, n2, n), rng.integers(0, r, n))
        idx += ix.tolist()
        psw += special_weights(n, rng).tolist()
        lens += ln.tolist()
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    with np.errstate(all="ignore"):
        psw = np.asarray(psw, dtype=F32)
    return np.asarray(idx, dtype=np.int64), off, (psw if weighted else None), named


def dyadic_table(rows, D, rng, kind):
    """a special table whose ordinary rows are multiples of 1/8 in [-4, 4] (exact in every table type): sums of such rows, of
    multiples of the smallest subnormal, of zeros, and anything absorbed by an Inf or NaN do not depend on the order of addition"""
    store, w = special_table(rows, D, rng, kind)
    n2 = 2 * n_special_rows(kind)
    o = (rng.integers(-32, 33, (rows - n2, D)) / 8.0).astype(F32)
    w = w.copy()
    w[n2:] = o
    if kind == "f32":
        return w, w
    store = store.copy()
    if kind == "bf16":
        store[n2:] = (o.view(np.uint32) >> 16).astype(np.uint16)
    else:
        store[n2:] = o.astype(np.float16).view(np.uint16)
    assert np.array_equal(widen16(store, kind), w, equal_nan=True)
    return store, w


def long_bag_request(kind, rows, rng, weighted=False):
    """One table, 8 bags of 300 .. 3000 lookups for the one-workgroup-per-bag forward, which adds in another order than the oracle:
    every bag is built so that its sum does not depend on the order (see ``dyadic_table``), hence bit-comparable all the same.
    Bags: dyadic rows and zeros | the same and a +Inf row | the same and a NaN row | only -0 rows | +-smallest-subnormal rows 2 : 1 |
    largest-finite rows and zeros (fp32, bf16: +Inf whatever the order; fp16: an exact multiple of 32) | +Inf and -Inf rows | dyadic rows, and the mixed rows of the zeros.
    Weights (``weighted``): powers of two and zeros of both signs; in bag 1 one weight is +Inf instead of the row."""
    ix = special_index(kind)
    n = n_special_rows(kind)
    lens = [3000, 300, 2049, 301, 1500, 333, 777, 1024]
    dy = lambda k: rng.integers(2 * n, rows, k)                                              # noqa: E731
    bags = [np.concatenate([dy(2900), np.full(50, ix["pz"]), np.full(50, ix["nz"])]),
            np.concatenate([dy(299), [ix["pinf"]]]),
            np.concatenate([dy(2048), [ix["nan"]]]),
            np.full(301, ix["nz"]),
            np.concatenate([np.full(1000, ix["sub_a"]), np.full(500, ix["sub_a"] + 1)]),
            np.concatenate([np.full(300, ix["big"]), np.full(33, ix["pz"])]),
            np.concatenate([np.full(400, ix["pinf"]), np.full(377, ix["ninf"])]),
            np.concatenate([dy(1000), np.full(12, n + ix["pz"]), np.full(12, n + ix["nz"])])]
    assert [len(b) for b in bags] == lens
    bags = [rng.permutation(b) for b in bags]
    idx = np.concatenate(bags).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    psw = None
    if weighted:
        psw = rng.choice(np.array([1.0, 2.0, 0.5, 1.0, 0.0, -0.0], F32), len(idx)).astype(F32)
        for b in (3, 4, 5, 6):                                # signs and sizes must stay what the bag is about
            psw[off[b]:off[b + 1]] = 1.0
        at = off[1] + int(np.flatnonzero(bags[1] == ix["pinf"])[0])
        psw[at] = 1.0
        psw[off[1]] = np.inf if bags[1][0] != ix["pinf"] else 1.0
    return idx, off, psw


# ----------------------------------------------------------------------------- gradients for rows beyond the exact-run limit
def column_grad(B, D, rng):
    """``[B, D]`` bag gradient whose column sums have one class in any order of addition, column d by ``d % 6``: 0 ordinary |
    1 +Inf in every 97th bag | 2 NaN in every 89th | 3 +3e38 in every 5th (their sum overflows to +Inf however it is associated) |
    4 subnormals only (multiples of the smallest one up to 1000: exact sums) | 5 -Inf in every 83rd.  Columns 1, 2, 3, 5 hold
    ordinary values elsewhere.  To be used with weights >= 0 (``hot_weights``)."""
    g = _ordinary(rng, (B, D))
    b = np.arange(B)
    for d in range(D):
        k = d % 6
        if k == 1:
            g[b % 97 == d % 97, d] = np.inf
        elif k == 2:
            g[b % 89 == d % 89, d] = np.nan
        elif k == 3:
            g[b % 5 == d % 5, d] = F32(3e38)
        elif k == 4:
            g[:, d] = (rng.integers(-1000, 1001, B) * np.float64(FLT_TRUE_MIN)).astype(F32)
        elif k == 5:
            g[b % 83 == d % 83, d] = -np.inf
    return g


def hot_weights(n, rng):
    """per-sample weights that keep every contribution's sign: uniform in [0.5, 1.5), every seventh one of 1e-30, 1e-40, 1 (no zero: it
    would turn the Inf columns into NaN ones)"""
    w = rng.uniform(0.5, 1.5, n).astype(F32)
    at = np.arange(0, n, 7)
    w[at] = np.array([1e-30, 1e-40, 1.0], F32)[np.arange(len(at)) % 3]
    return w


N_HOT = 4          # hot rows of ``backward_request``: the table's last four
N_ZERO = 2         # and before them two rows looked up once each, by the +0 and by the -0 gradient bag


def backward_request(kind, rows, B, rng, hot=True):
    """TBE request (``idx``, ``off`` [T*B+1], ``psw``) for gradients made by ``special_grad(B, D)`` (bags [0, 16) constant specials,
    [16, 32) mixed, the rest ordinary) into special tables of ``rows[t]`` rows:
      * ragged bags of 0 .. 6 lookups, half of them into the special table rows, with ``special_weights``; every such row stays
        within the exact-run limit, so the oracle's lookup order defines its bits (cancelling huge values included);
      * row ``r - 5`` is looked up once, by bag 0 (gradient +0), row ``r - 6`` once, by bag 1 (gradient -0), weight 1;
      * ``hot``: the last four rows (ordinary table rows) are looked up more than 256 times, by bags whose contributions have one
        class in any order: 300 ordinary bags each, and the MIXED bag of +Inf (18) | of NaN (20) | of 3e38, three times over (28),
        at weight 1, other weights > 0 -- every other column of these rows stays finite; the fourth only by the subnormal bags
        5, 7, 9, a hundred times each."""
    n2 = 2 * n_special_rows(kind)
    assert B >= 340
    idx, psw, lens = [], [], []
    for r in rows:
        free = r - N_HOT - N_ZERO
        assert free > n2
        per_bag = [[] for _ in range(B)]
        for b in range(B):
            k = int(rng.integers(0, 7))
            ix = np.where(rng.random(k) < 0.5, rng.integers(0, n2, k), rng.integers(0, free, k))
            per_bag[b] = [(int(i), None) for i in ix]
        per_bag[0].append((r - 5, 1.0))
        per_bag[1].append((r - 6, 1.0))
        if hot:
            ordinary = np.arange(2 * N_SPECIAL, B)
            for h, extra in ((r - 1, [(18, 1)]), (r - 2, [(20, 1)]), (r - 3, [(28, 3)])):
                for b in rng.choice(ordinary, 300, replace=False):
                    per_bag[int(b)].append((h, -1.0))
                for b, times in extra:
                    per_bag[b] += [(h, 1.0)] * times
            for b in (5, 7, 9):
                per_bag[b] += [(r - 4, -1.0)] * 100
        for b in range(B):
            order = rng.permutation(len(per_bag[b]))
            idx += [per_bag[b][j][0] for j in order]
            psw += [per_bag[b][j][1] for j in order]
            lens.append(len(per_bag[b]))
    idx = np.asarray(idx, dtype=np.int64)
    n = len(idx)
    cold_w, hot_w = special_weights(n, rng), hot_weights(n, rng)
    with np.errstate(all="ignore"):
        w = np.array([cold_w[j] if p is None else (hot_w[j] if p < 0 else p) for j, p in enumerate(psw)], dtype=F32)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return idx, off, w
