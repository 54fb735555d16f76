"""Probe rows of a FAR table and its compacted twin (host only, numpy): what tests/test_gpu_far_addresses.py stands on.

A far table is one whose rows reach offsets of 2^31 and 2^32 from its base pointer, counted in BYTES and counted in ELEMENTS: an ``int``
element index ``r * D`` overflows at another row than a 32-bit byte offset ``r * row_bytes``.  Only a handful of PROBE rows of such a
table are ever written or looked up:

* rows 0, 1, 2;
* ``ceil(X / row_bytes) + {-1, 0, 1}`` for X in {2^31, 2^32} bytes;
* ``ceil(X / row_elems) + {-1, 0, 1}`` for X in {2^31, 2^32} elements (``row_elems``: D for float and 8-bit rows, D / 2 -- the code
  bytes -- for 4-bit rows);
* the last row.

The table has ``max probe + 1`` rows: its last row IS the highest threshold probe.  (A separate last row would be a 16th probe of the
fp32 D = 4 table, and the staged request of the GPU tests -- bags of 0, 3, 1, 9, 0, 2 lookups -- has 15 lookups in which every probe
has to appear.)

The TWIN of a far table is the small table that holds the probe rows' content in probe order; ``compact`` maps far row numbers to twin
row numbers.  A request that draws its indices from the probes only means the same thing on both: every rule of the project
(tests/*_rules.py, the C oracle) reads ``table[index]`` and nothing else of a table, so rule(far table, indices) is rule(twin,
compact(indices)) -- tests/test_gpu_far_addresses.py proves that on small full tables before any GPU sees a twin."""
import numpy as np

THRESHOLDS = (2 ** 31, 2 ** 32)
STAGED_LENS = (0, 3, 1, 9, 0, 2)            # B = 6 bags of the far table: 15 lookups, staged in LDS by every tiled kernel
UNSTAGED_LENS = (0, 4200, 1, 9, 0, 2)       # one tile of more than 4096 lookups: its indices are read from the request
UPDATE_LENS = (0, 1500, 1, 9, 0, 2)         # the updates' long request: no row is looked up more than 256 times (asserted where used)


def row_bytes(D, es=None, bits=None):
    """bytes per row: ``D * es`` for a float table of element size ``es``, the quantised row of ``bits`` (8 / 4) otherwise"""
    if bits is None:
        return D * es
    return D + 8 if bits == 8 else D // 2 + 4


def row_elems(D, bits=None):
    """elements per row: columns of a float or 8-bit row, code bytes of a 4-bit row"""
    return D // 2 if bits == 4 else D


def _ceil_div(a, b):
    return -(-a // b)


def threshold_rows(D, es=None, bits=None, thresholds=THRESHOLDS):
    """the four rows ``c`` = the first row that STARTS at or above a threshold: ``[(what, X, stride, c)]``, bytes first"""
    rb, re_ = row_bytes(D, es, bits), row_elems(D, bits)
    return [(what, X, s, _ceil_div(X, s)) for what, s in (("bytes", rb), ("elements", re_)) for X in thresholds]


def probe_rows(D, es=None, bits=None, thresholds=THRESHOLDS):
    """ascending distinct int64 probe rows; the table has ``probe_rows(...)[-1] + 1`` rows"""
    rows = {0, 1, 2}
    for _, _, _, c in threshold_rows(D, es, bits, thresholds):
        rows |= {c - 1, c, c + 1}
    p = np.array(sorted(rows), dtype=np.int64)
    assert p[0] == 0
    return p


def table_rows(probes):
    return int(probes[-1]) + 1


def guard_rows(D, es=None, bits=None, span=2 ** 31):
    """rows of the GUARD table in front of a far table: at least ``span`` bytes that no lookup reads"""
    return _ceil_div(span, row_bytes(D, es, bits)) + 1


def sentinel_rows(probes):
    """ascending rows ``probe +- 1`` inside the table that are not probes themselves: written once, never looked up"""
    p = set(int(r) for r in probes)
    n = table_rows(probes)
    s = {r + d for r in p for d in (-1, 1)}
    return np.array(sorted(r for r in s if 0 <= r < n and r not in p), dtype=np.int64)


def compact(probes, indices):
    """far row numbers as twin row numbers ``0 .. len(probes) - 1`` (the input's dtype); every index must be a probe"""
    idx = np.asarray(indices)
    pos = np.searchsorted(probes, idx.astype(np.int64))
    assert ((pos < len(probes)) & (probes[np.minimum(pos, len(probes) - 1)] == idx)).all(), "an index is not a probe row"
    return pos.astype(idx.dtype)


def expand(probes, twin_indices):
    """the inverse of ``compact``"""
    t = np.asarray(twin_indices)
    return np.asarray(probes)[t.astype(np.int64)].astype(np.int64)


def request(probes, lens, seed, guard_bags=None, dtype=np.int64):
    """A TBE request over the tables ``[guard, far]`` (``guard_bags`` None: over the far table alone): ``(indices, offsets [T * B + 1])``
    with ``B = len(lens)``; the guard's ``guard_bags`` (= B) bags are empty, the far table's bags have ``lens`` lookups drawn from the
    probes -- every probe at least once (asserted), the rest uniformly.  The twin's request is the same offsets with ``compact`` of the
    indices, over ``[a one-row guard, twin]``."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    n, P = int(lens.sum()), len(probes)
    assert n >= P, f"{n} lookups cannot reach {P} probes"
    pick = np.concatenate([np.arange(P), rng.integers(0, P, n - P)])
    idx = np.asarray(probes)[rng.permutation(pick)]
    assert np.array_equal(np.unique(idx), probes), "every probe row is looked up"
    far_off = np.concatenate([[0], np.cumsum(lens)])
    off = far_off if guard_bags is None else np.concatenate([np.zeros(guard_bags, dtype=np.int64), far_off])
    return idx.astype(dtype), off.astype(dtype)
