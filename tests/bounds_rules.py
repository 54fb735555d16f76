"""numpy restatement of the bounds-check rule of ``pm_embbag_bounds_check`` (include/param_amd.h): the monotone closure of the
offsets, the table a lookup belongs to, the replacement of out-of-range indices and the report -- what the GPU tests hold the
kernels to bit for bit -- and of the conditions ``embbag_check_kernel`` (``pm_embbag_check``) puts on a request."""
import numpy as np

NONE = np.iinfo(np.int64).max       # PM_BOUNDS_NONE


def repair(indices, offsets, rows, T, B):
    """-> (indices', offsets', report): the arrays as a repairing call leaves them (same dtypes; the inputs are not modified) and
    ``report = (bad_indices, bad_offsets, first_bad_index, first_bad_offset)``, positions ``None`` without a finding.
    ``offsets`` has ``T * B`` or ``T * B + 1`` entries."""
    indices, offsets = np.asarray(indices), np.asarray(offsets)
    rows = np.asarray(rows, dtype=np.int64)
    N, TB = int(indices.size), T * B
    assert offsets.size in (TB, TB + 1) and rows.size == T
    idx, off = indices.copy(), offsets.copy()
    if TB == 0:
        return idx, off, (0, 0, None, None)
    c = np.clip(off[:TB].astype(np.int64), 0, N)
    c[0] = 0
    closed = np.maximum.accumulate(c)                       # o'[k] = max(o'[k - 1], clamp(o[k], 0, N)), o'[0] = 0
    off[:TB] = closed.astype(off.dtype)
    if off.size == TB + 1:
        off[TB] = N
    changed_off = np.nonzero(off.astype(np.int64) != offsets.astype(np.int64))[0]
    borders = closed[::B]                                   # o'[t * B], t = 0 .. T - 1
    table = np.searchsorted(borders, np.arange(N, dtype=np.int64), side="right") - 1      # the last t with o'[t * B] <= j
    wide = idx.astype(np.int64)
    bad = (wide < 0) | (wide >= rows[table]) if N else np.zeros(0, dtype=bool)
    idx[bad] = 0
    bad_pos = np.nonzero(bad)[0]
    first = lambda a: int(a[0]) if a.size else None         # noqa: E731
    return idx, off, (int(bad_pos.size), int(changed_off.size), first(bad_pos), first(changed_off))


def report_array(report):
    """the report as the device int64[4] holds it"""
    bi, bo, fi, fo = report
    return np.array([bi, bo, NONE if fi is None else fi, NONE if fo is None else fo], dtype=np.int64)


def report_dict(report):
    bi, bo, fi, fo = report
    return {"bad_indices": bi, "bad_offsets": bo, "first_bad_index": fi, "first_bad_offset": fo}


def check_errors(indices, offsets, rows, T, B):
    """violations as ``embbag_check_kernel`` counts them for a whole-batch request: bag g of table g // B spans
    [offsets[g], offsets[g + 1]), the very last bag ends at N (a trailing offsets entry is never read); a bag with
    ``start < 0``, ``end < start`` or ``end > N`` is one violation (its lookups are not looked at), otherwise every lookup of it
    outside [0, rows[t]) is one."""
    indices, offsets = np.asarray(indices).astype(np.int64), np.asarray(offsets).astype(np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    N, TB = int(indices.size), T * B
    if TB == 0:
        return 0
    s = offsets[:TB]
    e = np.concatenate([offsets[1:TB], [N]])
    broken = (s < 0) | (e < s) | (e > N)
    bad = int(broken.sum())
    for t in range(T):                                      # lookups of table t's sound bags that are out of table t's range
        ok = ~broken[t * B:(t + 1) * B]
        if not ok.any():
            continue
        before = np.concatenate([[0], np.cumsum((indices < 0) | (indices >= rows[t]))])
        bad += int((before[e[t * B:(t + 1) * B][ok]] - before[s[t * B:(t + 1) * B][ok]]).sum())
    return bad


# ---- requests for the tests ---------------------------------------------------------------------------------------------------

def every_defect_case(closed, dtype=np.int64):
    """T = 3, B = 4, rows = [5, 50, 7], two lookups per bag, with every kind of defect; the expected arrays are written out by hand.
    -> (indices, offsets, rows, T, B, indices', offsets', report)"""
    rows, T, B = [5, 50, 7], 3, 4
    #        offsets[0] != 0   negative            descending pair      > N   wrong trailing entry
    off = [3, 2, -5, 6,        8, 10, 12, 11,      16, 18, 20, 99,      7]
    fix = [0, 2, 2, 6,         8, 10, 12, 12,      16, 18, 20, 24,      24]       # clamp to [0, 24], then the running maximum
    #      table 0: -1 negative, 5 == rows[0], 49 valid for table 1 only | table 1: untouched | table 2: 10 valid for table 1 only, 7 == rows[2]
    idx = [0, -1, 2, 3, 5, 0, 1, 49,      10, 20, 30, 40, 49, 5, 6, 49,      10, 1, 2, 3, 4, 5, 6, 7]
    out = [0, 0, 2, 3, 0, 0, 1, 0,        10, 20, 30, 40, 49, 5, 6, 49,      0, 1, 2, 3, 4, 5, 6, 0]
    n_off = len(off) if closed else T * B
    report = (5, 5 if closed else 4, 1, 0)      # indices 1, 4, 7, 16, 23; offsets 0, 2, 7, 11 (and 12)
    a = lambda v: np.array(v, dtype=dtype)      # noqa: E731
    return a(idx), a(off[:n_off]), rows, T, B, a(out), a(fix[:n_off]), report


def clean_request(rng, rows, B, max_len, dtype=np.int64, closed=True, min_len=0, empty_tables=()):
    """a valid ragged request: bag lengths min_len .. max_len (tables in ``empty_tables`` own no lookup), indices uniform in their
    table's rows -> (indices, offsets)"""
    T = len(rows)
    lens = rng.integers(min_len, max_len + 1, T * B)
    for t in empty_tables:
        lens[t * B:(t + 1) * B] = 0
    ends = np.cumsum(lens)
    N = int(ends[-1]) if T * B else 0
    off = np.concatenate([[0], ends]).astype(dtype)
    per_table = np.repeat(np.asarray(rows, dtype=np.int64), np.add.reduceat(lens, np.arange(0, T * B, B)) if T * B else 0)
    idx = (rng.random(N) * per_table).astype(np.int64).astype(dtype)
    return idx, (off if closed else off[:T * B])


def corrupt(rng, idx, off, rows, n_idx, n_off):
    """copies of the arrays with n_idx indices and n_off offsets overwritten by bad (or at least different) values"""
    idx, off = idx.copy(), off.copy()
    N, big = idx.size, int(max(rows))
    lo = np.iinfo(idx.dtype).min
    if N:
        pos = rng.choice(N, size=min(n_idx, N), replace=False)
        idx[pos] = rng.choice(np.array([-1, lo, big, big + 1, np.iinfo(idx.dtype).max], dtype=np.int64), size=pos.size).astype(idx.dtype)
    if off.size:
        pos = rng.choice(off.size, size=min(n_off, off.size), replace=False)
        off[pos] = rng.choice(np.array([-3, lo, N + 1, N + 1000, 0, N, N // 2, np.iinfo(off.dtype).max], dtype=np.int64),
                              size=pos.size).astype(off.dtype)
    return idx, off
