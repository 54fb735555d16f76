"""numpy restatement of the MEAN POOLING rule (include/param_amd.h, "MEAN POOLING"; torch's ``nn.EmbeddingBag(mode="mean")`` on fp32
tables), per table.  ``count(t, b)`` = the lookups of bag (t, b) that are not table t's padding index (``pads``: a list of
``int | None`` per table, as in tests/padding_rules.py).

* forward: ``sum / (float)count`` for ``count >= 1`` -- the sum forward's additions (index order from +0.0, fp32), then ONE correctly
  rounded fp32 division per element (numpy's float32 division is that); ``+0.0`` with no division for ``count == 0``.
* backward: every lookup of bag (t, b) contributes ``grad(t, b) * r``, ``r = float32(1) / float32(count)`` rounded to fp32 FIRST, then
  one fp32 multiplication per element; ``+0.0`` for ``count == 0``.  The contributions are summed as the sum backward sums them: the
  dense and the sparse gradient below are the sum rule on the scaled gradient (a sequential fp32 scatter-add in lookup order).

The GPU tests hold the kernels to all of it bit for bit; tests/test_mean_host.py holds the rule to torch's CPU module."""
import numpy as np

from tests import padding_rules as P


def count(indices, offsets, T, B, pads):
    """int64 ``[T * B]``: kept lookups per bag"""
    idx = np.asarray(indices).astype(np.int64)
    start, end = P.bag_bounds(offsets, T, B, idx.size)
    keep = np.concatenate([[0], np.cumsum(~P.padded_mask(idx, offsets, T, B, pads))]).astype(np.int64)
    lo, hi = np.clip(start, 0, idx.size), np.clip(end, 0, idx.size)
    return np.where(hi > lo, keep[hi] - keep[lo], 0)


def divide(sums, n):
    """``sums [bags, D] / float32(n [bags])`` where ``n >= 1``, the row untouched (+0.0 from the sum rule) where ``n == 0``"""
    out = np.array(sums, dtype=np.float32, copy=True)
    n = np.asarray(n)
    has = n > 0
    with np.errstate(all="ignore"):
        out[has] = out[has] / n[has].astype(np.float32)[:, None]
    return out


def forward(tables, indices, offsets, B, pads, bag_begin=0, bag_count=None):
    """list of T fp32 arrays ``[bag_count, D_t]``: ``padding_rules.forward`` (unweighted), then the division"""
    T = len(tables)
    bag_count = B - bag_begin if bag_count is None else bag_count
    sums = P.forward(tables, indices, offsets, B, pads, None, bag_begin, bag_count)
    n = count(indices, offsets, T, B, pads).reshape(T, B)[:, bag_begin:bag_begin + bag_count]
    return [divide(s, n[t]) for t, s in enumerate(sums)]


def scale_grad(grads, indices, offsets, B, pads):
    """list of T fp32 arrays ``[B, D_t]``: ``grads[t][b] * (float32(1) / float32(count(t, b)))``, +0.0 where the count is 0"""
    T = len(grads)
    n = count(indices, offsets, T, B, pads).reshape(T, B)
    res = []
    for t, g in enumerate(grads):
        g = np.asarray(g, dtype=np.float32)
        out = np.zeros_like(g)
        has = n[t] > 0
        r = np.float32(1.0) / n[t][has].astype(np.float32)
        with np.errstate(all="ignore"):
            out[has] = g[has] * r[:, None]
        res.append(out)
    return res


def sum_dense_grad(rows, dims, indices, offsets, B, pads, grads, bag_begin=0, bag_count=None):
    """the SUM rule's dense weight gradient in fp32: a sequential scatter-add of ``grads[t][bag(j)]`` in lookup order into zeros (what
    the sorted backward equals bit for bit); padded lookups are left out, so a padding row is +0.0"""
    T = len(rows)
    idx = np.asarray(indices).astype(np.int64)
    bag_count = B - bag_begin if bag_count is None else bag_count
    start, end = P.bag_bounds(offsets, T, B, idx.size)
    skip = P.padded_mask(idx, offsets, T, B, pads)
    outs = [np.zeros((r, d), dtype=np.float32) for r, d in zip(rows, dims)]
    with np.errstate(all="ignore"):
        for t in range(T):
            g = np.asarray(grads[t], dtype=np.float32)
            for b in range(bag_begin, bag_begin + bag_count):
                for j in range(int(start[t * B + b]), int(end[t * B + b])):
                    if not skip[j]:
                        outs[t][idx[j]] = outs[t][idx[j]] + g[b]
    return outs


def dense_grad(rows, dims, indices, offsets, B, pads, grads, bag_begin=0, bag_count=None):
    """the mean backward's dense gradient: the sum rule on the scaled gradient"""
    return sum_dense_grad(rows, dims, indices, offsets, B, pads, scale_grad(grads, indices, offsets, B, pads), bag_begin, bag_count)


def sparse_grad(rows, dims, indices, offsets, B, pads, grads, bag_begin=0, bag_count=None):
    """the mean backward's coalesced sparse gradient: list of T ``(rows_t ascending int64, values_t fp32 [U_t, D_t])``"""
    dense = dense_grad(rows, dims, indices, offsets, B, pads, grads, bag_begin, bag_count)
    hit = P.sparse_rows(indices, offsets, len(rows), B, pads, bag_begin, bag_count)
    return [(r, dense[t][r]) for t, r in enumerate(hit)]
