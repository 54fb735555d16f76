"""numpy restatement of the UN-POOLED rule over row-quantised tables (include/param_amd.h, "ROW-QUANTISED TABLES, UN-POOLED"), on top of
tests/qrows_rules.py (``unpack``, ``fmaf``, ``same_f32``): for every lookup position j of the bag slice, t the table that owns j,
r = indices[j], per column c < D_t::

    out[j, c] = conv( fmaf(scale_r, (float)code[r, c], fl32(+0.0 + bias_r)) )

-- the pooled rule of one unweighted bag of one lookup.  The addition is part of the rule (it is not ``fmaf(scale, code, bias)``).
Table t owns the positions ``[offsets[t * B], offsets[(t + 1) * B])``, the last table ends at N: a position's table is the LAST table
whose first bag starts at or before it (tables that own no position are passed over); the slice ``[bag_begin, bag_begin + bag_count)``
of every table is the stretch ``[offsets[t * B + bag_begin], offsets[t * B + bag_begin + bag_count))``, ``offsets[T * B]`` being N.
tests/test_qgather_host.py holds this module to torch's CPU operators.  16-bit outputs: ``tests/out16_rules.round16`` of the result."""
import numpy as np

from tests import qrows_rules as R


def rows(q, dim, bits, r):
    """fp32 ``[len(r), dim]``: the rule for the rows ``r`` of ONE table ``q`` (uint8 ``[rows, row_bytes(dim, bits)]``)"""
    codes, scale, bias = R.unpack(q, dim, bits)
    r = np.asarray(r, dtype=np.int64)
    with np.errstate(all="ignore"):
        t = (np.float32(0.0) + bias[r]).astype(np.float32)
        return R.fmaf(scale[r][:, None], codes[r].astype(np.float32), t[:, None])


def owners(offsets, T, B, N, bag_begin=0, bag_count=None):
    """(table int64 ``[N]`` -- -1: in front of every table --, written bool ``[N]``: the position lies in the bag slice of its table)"""
    off = np.asarray(offsets).astype(np.int64)
    bag_count = B - bag_begin if bag_count is None else bag_count
    edge = lambda g: off[g] if g < T * B else N      # noqa: E731 -- (a trailing offsets[T * B] entry is never read)
    j = np.arange(N, dtype=np.int64)
    borders = np.array([off[t * B] for t in range(T)], dtype=np.int64)
    table = np.full(N, -1, dtype=np.int64)
    for t in range(T):                               # the last table whose border is at or before j
        table[borders[t] <= j] = t
    written = np.zeros(N, dtype=bool)
    for t in range(T):
        lo, hi = edge(t * B + bag_begin), edge(t * B + bag_begin + bag_count)
        written |= (table == t) & (j >= lo) & (j < hi)
    return table, written


def gather_tables(qtables, dims, bits, indices, offsets, B, bag_begin=0, bag_count=None):
    """per-table lists (mixed dims): ``[(positions int64 [n_t], values fp32 [n_t, D_t])]`` of the WRITTEN positions of every table"""
    idx = np.asarray(indices).astype(np.int64)
    table, written = owners(offsets, len(qtables), B, idx.size, bag_begin, bag_count)
    out = []
    for t, (q, d) in enumerate(zip(qtables, dims)):
        pos = np.nonzero(written & (table == t))[0]
        out.append((pos, rows(q, d, bits, idx[pos])))
    return out


def gather(qtables, dim, bits, indices, offsets, B, bag_begin=0, bag_count=None):
    """(fp32 ``[N, dim]`` -- zeros in the rows that are not written --, written bool ``[N]``) for tables of one common ``dim``"""
    n = np.asarray(indices).size
    out = np.zeros((n, dim), dtype=np.float32)
    written = np.zeros(n, dtype=bool)
    for pos, vals in gather_tables(qtables, [dim] * len(qtables), bits, indices, offsets, B, bag_begin, bag_count):
        out[pos] = vals
        written[pos] = True
    return out, written


def negative_zeros(a):
    """how many elements of the fp32 array ``a`` are -0.0"""
    a = np.asarray(a, dtype=np.float32)
    return int(((a == 0) & np.signbit(a)).sum())


def signed_zero_rows(dim, bits):
    """hand-built rows ``[5, row_bytes]`` whose tails are (scale, bias) = (0.5, -0.0), (-0.25, 0.0), (-0.25, -0.0), (0.0, -0.0), (-0.0, 1.0):
    column 0 holds code 0 in every row (then 1, 2, ..): a plain ``fmaf(scale, code, bias)`` gives -0.0 there for row 2 (-0 + -0), the rule +0.0 everywhere"""
    n = 5
    codes = (np.arange(n * dim, dtype=np.int64).reshape(n, dim) % dim % (256 if bits == 8 else 16)).astype(np.uint8)
    tails = np.array([[0.5, -0.0], [-0.25, 0.0], [-0.25, -0.0], [0.0, -0.0], [-0.0, 1.0]])
    if bits == 8:
        return np.concatenate([codes, tails.astype(np.float32).view(np.uint8).reshape(n, 8)], axis=1)
    packed = (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)
    return np.concatenate([packed, tails.astype(np.float16).view(np.uint8).reshape(n, 4)], axis=1)
