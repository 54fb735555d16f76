"""numpy restatement of the MAX POOLING rule (include/param_amd.h, "MAX POOLING"; torch's ``nn.EmbeddingBag(mode="max")``), per table.
A request is the pooled one: T tables, B bags per table, ``indices`` table-major, bag ``(t, b)`` = the positions
``[offsets[t * B + b], offsets[t * B + b + 1])``, the very last bag ends at N.  ``pads``: ``int | None`` per table.  Tables are fp32 arrays
(a 16-bit table is passed widened: the widening is exact and monotone, so the rule is the same).

* forward: the lookups equal to the table's padding index are removed; per column the first kept lookup sets ``cur``, whatever it
  holds, and a later one replaces it iff ``w > cur`` -- numpy's ``>`` on float32 is the ordered, strict IEEE comparison.  No kept
  lookup: ``+0.0``.
* arg-max: the row index that supplied ``cur`` (int32), ``-1`` where there is no kept lookup.
* expansion: ``g_seq[j, c] = grad(t, bag(j))[c]`` iff ``j`` is the first position of its bag with ``indices[j] == arg(t, bag(j))[c]``,
  else ``+0.0``; positions outside the batch slice are not written.
* dense gradient: ``grad(t, b)[c]`` is added to row ``arg(t, b)[c]`` of a zeroed fp32 buffer, bags in ascending order (sequential fp32
  adds: torch's ``_embedding_bag_dense_backward`` order for max).

The GPU tests hold the kernels to all of it on bits; tests/test_max_host.py holds the rule to torch's CPU module."""
import numpy as np


def bag_bounds(offsets, T, B, N):
    """(start, end) int64 ``[T * B]``: a bag ends where the next one starts, the very last one at N (a trailing offset is not read)"""
    off = np.asarray(offsets).astype(np.int64).reshape(-1)[:T * B]
    return off, np.concatenate([off[1:], np.array([N], dtype=np.int64)])


def forward(tables, indices, offsets, B, pads=None, bag_begin=0, bag_count=None):
    """(values, args): two lists of T arrays ``[bag_count, D_t]``, fp32 and int32"""
    T = len(tables)
    idx = np.asarray(indices).astype(np.int64).reshape(-1)
    pads = [None] * T if pads is None else pads
    bag_count = B - bag_begin if bag_count is None else bag_count
    start, end = bag_bounds(offsets, T, B, idx.size)
    vals, args = [], []
    for t, w in enumerate(tables):
        w = np.asarray(w, dtype=np.float32)
        v = np.zeros((bag_count, w.shape[1]), dtype=np.float32)
        a = np.full((bag_count, w.shape[1]), -1, dtype=np.int32)
        for k in range(bag_count):
            g = t * B + bag_begin + k
            first = True
            for j in range(int(start[g]), int(end[g])):
                r = int(idx[j])
                if pads[t] is not None and r == pads[t]:
                    continue
                with np.errstate(invalid="ignore"):
                    take = np.ones(w.shape[1], dtype=bool) if first else w[r] > v[k]
                v[k] = np.where(take, w[r], v[k])
                a[k] = np.where(take, np.int32(r), a[k])
                first = False
        vals.append(v)
        args.append(a)
    return vals, args


def round_out(vals, dtype):
    """the fp32 result rounded once to ``dtype`` (``"bf16"`` / ``"fp16"``), as uint16 bits: the OUTPUT DTYPE rule's one rounding
    (tests/out16_rules.py; compare with its ``same_bits``: a NaN's payload is not part of that rule)"""
    from tests import out16_rules as O
    return [O.round16(v, dtype) for v in vals]


def expand(indices, offsets, B, grads, args, bag_begin=0, bag_count=None):
    """(g_seq fp32 ``[N, D]``, written bool ``[N]``): ``grads`` / ``args`` are lists of T ``[B, D]`` arrays (whole batch; only the
    slice's bags are read).  Rows of positions that are not written are +0.0 in ``g_seq`` and False in ``written``."""
    T = len(grads)
    D = np.asarray(grads[0]).shape[1]
    idx = np.asarray(indices).astype(np.int64).reshape(-1)
    bag_count = B - bag_begin if bag_count is None else bag_count
    start, end = bag_bounds(offsets, T, B, idx.size)
    g_seq = np.zeros((idx.size, D), dtype=np.float32)
    written = np.zeros(idx.size, dtype=bool)
    for t in range(T):
        g = np.asarray(grads[t], dtype=np.float32)
        a = np.asarray(args[t]).astype(np.int64)
        for b in range(bag_begin, bag_begin + bag_count):
            done = np.zeros(D, dtype=bool)
            for j in range(int(start[t * B + b]), int(end[t * B + b])):
                hit = ~done & (idx[j] == a[b])
                g_seq[j] = np.where(hit, g[b], np.float32(0.0))
                written[j] = True
                done |= hit
    return g_seq, written


def dense_grad(rows, dims, grads, args, bag_begin=0, bag_count=None):
    """list of T fp32 ``[rows_t, dims_t]``: ``grads[t][b, c]`` added to row ``args[t][b, c]``, bags ascending, from zeros"""
    outs = []
    for t, (r, d) in enumerate(zip(rows, dims)):
        g = np.asarray(grads[t], dtype=np.float32)
        a = np.asarray(args[t]).astype(np.int64)
        B = g.shape[0]
        hi = B if bag_count is None else bag_begin + bag_count
        out = np.zeros((r, d), dtype=np.float32)
        cols = np.arange(d)
        with np.errstate(all="ignore"):
            for b in range(bag_begin, hi):
                has = a[b] >= 0
                out[a[b][has], cols[has]] = out[a[b][has], cols[has]] + g[b][has]
        outs.append(out)
    return outs


def bits(x):
    """an fp32 array as its uint32 bits: the compare that tells -0.0 from +0.0 and one NaN from another"""
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)
