"""numpy restatement of the PADDING rule (include/param_amd.h, "PADDING"; torch's ``nn.EmbeddingBag(mode="sum", padding_idx=...)``),
per table: a lookup whose index equals its table's padding index contributes nothing to the forward, its row receives no gradient
and no update, and its ``per_sample_weights`` gradient is +0.0.  ``pads`` is a list of ``int | None`` per table throughout.

What the GPU tests hold the kernels to bit for bit: the forward (sequential fp32 adds from +0.0 in index order; weighted, one
fused multiply-add per kept lookup -- emulated exactly through fp64 below), the rows of the sparse gradient, the mask over the
``per_sample_weights`` gradient and the guard's save / restore."""
import numpy as np


def table_of(offsets, T, B, N):
    """table of every lookup j in [0, N): the last t with offsets[t * B] <= j (tables without lookups own none)"""
    borders = np.asarray(offsets).astype(np.int64)[:T * B:B] if B else np.zeros(0, dtype=np.int64)
    return np.searchsorted(borders, np.arange(N, dtype=np.int64), side="right") - 1


def bag_bounds(offsets, T, B, N):
    """(start, end) of the T * B bags: the next offset, N for the very last bag (a trailing offsets entry is never read)"""
    off = np.asarray(offsets).astype(np.int64)
    return off[:T * B], np.concatenate([off[1:T * B], [N]])


def padded_mask(indices, offsets, T, B, pads):
    """bool [N]: lookup j is PADDED (its index is its table's padding index)"""
    idx = np.asarray(indices).astype(np.int64)
    if idx.size == 0:
        return np.zeros(0, dtype=bool)
    pad = np.array([-1 if k is None else k for k in pads], dtype=np.int64)
    return idx == pad[table_of(offsets, T, B, idx.size)]


def fma32(w, f, acc):
    """fp32 fused multiply-add ``w * f + acc`` with ONE rounding, element-wise.  The product of two fp32 values is exact in fp64;
    the sum is rounded to ODD in fp64 (TwoSum gives the exact residual), which makes the final rounding to fp32 the correctly
    rounded result (53 >= 2 * 24 + 2 bits).  Finite inputs."""
    p = np.asarray(w, dtype=np.float32).astype(np.float64) * np.asarray(f, dtype=np.float32).astype(np.float64)
    a = np.asarray(acc, dtype=np.float32).astype(np.float64)
    p, a = np.broadcast_arrays(p, a)
    s = p + a
    bb = s - p
    err = (p - (s - bb)) + (a - bb)
    bits = s.copy().view(np.int64)
    need = (err != 0) & ((bits & 1) == 0)
    away = (err > 0) == (s > 0)                   # the exact sum lies beyond s in magnitude
    bits = np.where(need, np.where(away, bits + 1, bits - 1), bits)
    return bits.view(np.float64).astype(np.float32)


def forward(tables, indices, offsets, B, pads, psw=None, bag_begin=0, bag_count=None):
    """list of T fp32 arrays ``[bag_count, D_t]``: out(t, b) = sum over the kept lookups of bag (t, b), in index order from +0.0, of
    psw[j] * W_t[indices[j]] -- plain fp32 adds unweighted, one fma per kept lookup weighted.  ``tables``: fp32 arrays (16-bit
    tables widened, which is exact).  The padding row is never read."""
    T = len(tables)
    idx = np.asarray(indices).astype(np.int64)
    N = idx.size
    bag_count = B - bag_begin if bag_count is None else bag_count
    start, end = bag_bounds(offsets, T, B, N)
    skip = padded_mask(idx, offsets, T, B, pads)
    outs = []
    for t in range(T):
        W = np.asarray(tables[t], dtype=np.float32)
        out = np.zeros((bag_count, W.shape[1]), dtype=np.float32)
        for k in range(bag_count):
            g = t * B + bag_begin + k
            acc = np.zeros(W.shape[1], dtype=np.float32)
            for j in range(int(start[g]), int(end[g])):
                if skip[j]:
                    continue
                acc = fma32(np.float32(psw[j]), W[idx[j]], acc) if psw is not None else acc + W[idx[j]]
            out[k] = acc
        outs.append(out)
    return outs


def filtered_request(indices, offsets, T, B, pads, psw=None):
    """the request with the padded lookups REMOVED: (indices', offsets', psw') in the inputs' dtypes; offsets keeps its length (a
    trailing entry becomes the new N).  The product forward on it is what the padded forward must equal bit for bit."""
    indices, offsets = np.asarray(indices), np.asarray(offsets)
    N = indices.size
    keep = ~padded_mask(indices, offsets, T, B, pads)
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)          # kept lookups in front of position j
    new_off = before[np.clip(offsets.astype(np.int64), 0, N)].astype(offsets.dtype)
    return indices[keep], new_off, (None if psw is None else np.asarray(psw)[keep])


def dense_grad(rows, dims, indices, offsets, B, pads, grads, psw=None):
    """list of T fp64 arrays ``[rows_t, D_t]``: the weight gradient, summed in fp64 (a reference for tolerance checks); the padding
    row is exactly zero.  ``grads``: list of T arrays ``[B, D_t]``."""
    T = len(rows)
    idx = np.asarray(indices).astype(np.int64)
    N = idx.size
    start, end = bag_bounds(offsets, T, B, N)
    skip = padded_mask(idx, offsets, T, B, pads)
    outs = [np.zeros((r, d), dtype=np.float64) for r, d in zip(rows, dims)]
    for g in range(T * B):
        t, b = divmod(g, B)
        for j in range(int(start[g]), int(end[g])):
            if not skip[j]:
                outs[t][idx[j]] += (1.0 if psw is None else float(psw[j])) * np.asarray(grads[t][b], dtype=np.float64)
    return outs


def sparse_rows(indices, offsets, T, B, pads, bag_begin=0, bag_count=None):
    """list of T ascending int64 arrays: the distinct rows the kept lookups of the bag slice hit -- the COO rows of the coalesced
    sparse gradient, without the padding row"""
    idx = np.asarray(indices).astype(np.int64)
    bag_count = B - bag_begin if bag_count is None else bag_count
    start, end = bag_bounds(offsets, T, B, idx.size)
    skip = padded_mask(idx, offsets, T, B, pads)
    res = []
    for t in range(T):
        lo, hi = (int(start[t * B + bag_begin]), int(end[t * B + bag_begin + bag_count - 1])) if bag_count else (0, 0)
        res.append(np.unique(idx[lo:hi][~skip[lo:hi]]))
    return res


def psw_grad_mask(values, indices, offsets, T, B, pads, bag_begin=0, bag_count=None):
    """``values`` (the per_sample_weights gradient, fp32 [N]) with +0.0 at the padded lookups of the bag slice; every other entry
    keeps its bits"""
    out = np.array(values, dtype=np.float32, copy=True)
    idx = np.asarray(indices).astype(np.int64)
    bag_count = B - bag_begin if bag_count is None else bag_count
    if idx.size == 0 or bag_count == 0:
        return out
    start, end = bag_bounds(offsets, T, B, idx.size)
    tab = table_of(offsets, T, B, idx.size)
    pos = np.arange(idx.size)
    inside = (pos >= start[tab * B + bag_begin]) & (pos < end[tab * B + bag_begin + bag_count - 1])
    out[padded_mask(idx, offsets, T, B, pads) & inside] = np.float32(0.0)
    return out


def guard(before, after, pads):
    """the guard's save / restore around a backward: per table, ``after`` with its padding row put back from ``before`` (a table
    without a padding row is ``after``).  Works on any per-table arrays whose first axis is the row: weights, optimizer state,
    dense gradient buffers."""
    res = []
    for b, a, k in zip(before, after, pads):
        a = np.array(a, copy=True)
        if k is not None:
            a[k] = np.asarray(b)[k]
        res.append(a)
    return res


# ---- requests for the tests ---------------------------------------------------------------------------------------------------

def padded_request(rng, rows, B, pads, share=0.4, max_len=9, fixed=None, dtype=np.int64, closed=True):
    """a valid request in which about ``share`` of the lookups of every table with a padding row are that row: ragged bags of
    0 .. max_len lookups, or ``fixed`` lookups per bag -> (indices, offsets)"""
    T = len(rows)
    lens = np.full(T * B, fixed, dtype=np.int64) if fixed is not None else rng.integers(0, max_len + 1, T * B)
    ends = np.cumsum(lens)
    N = int(ends[-1]) if T * B else 0
    off = np.concatenate([[0], ends]).astype(dtype)
    tab = np.repeat(np.arange(T), np.add.reduceat(lens, np.arange(0, T * B, B))) if T * B else np.zeros(0, dtype=np.int64)
    idx = (rng.random(N) * np.asarray(rows, dtype=np.int64)[tab]).astype(np.int64)
    pad = np.array([-1 if k is None else k for k in pads], dtype=np.int64)[tab]
    hit = (rng.random(N) < share) & (pad >= 0)
    idx[hit] = pad[hit]
    return idx.astype(dtype), (off if closed else off[:T * B])
