"""numpy restatement of the SEQUENCE GRADIENT rule (include/param_amd.h, "SEQUENCE GRADIENTS"): the batched backward of the un-pooled
lookup.  A sequence request is the request ``lookup_sequence`` takes -- T tables, B bags per table, ``indices`` table-major; table ``t``
owns the positions ``[offsets[t * B], offsets[(t + 1) * B])``, the last table ends at N -- and the gradient is ``grad[N, D]`` fp32,
addressed by lookup position.

For table ``t`` and row ``r``, ``J(t, r)`` = the positions owned by ``t``, inside the bag slice, whose index is ``r``, ascending.  The
dense gradient adds ``grad[j]`` over ``J(t, r)`` in that order, from zero: sequential fp32 adds, which is ``embedding_rules.dense_grad``
(torch's CPU ``embedding_dense_backward``) of every table on its own stretch.  A table's padding row stays zero.  The GPU tests hold
``sequence_dense_grad`` to this bit for bit for rows of at most 256 lookups (``kExactRun``); hotter rows are summed as ordered chunk
partials and are held to the fp64 sum instead."""
import numpy as np

from tests import embedding_rules as E


def table_slices(offsets, T, B, N, bag_begin=0, bag_count=None):
    """per table the position range ``(lo, hi)`` of the bag slice: ``[offsets[t * B + bag_begin], offsets[t * B + bag_begin + bag_count))``
    -- read off ``embedding_rules.in_slice`` (which rests on ``padding_rules.table_of`` / ``bag_bounds``); a table without a position
    in the slice gives ``(0, 0)``.  The positions of a table's slice are contiguous: asserted."""
    tab, inside = E.in_slice(offsets, T, B, N, bag_begin, bag_count)
    out = []
    for t in range(T):
        sel = np.nonzero(inside & (tab == t))[0]
        if sel.size == 0:
            out.append((0, 0))
            continue
        lo, hi = int(sel[0]), int(sel[-1]) + 1
        assert hi - lo == sel.size, "a table's slice is one contiguous stretch of positions"
        out.append((lo, hi))
    return out


def dense_grad(rows, dims, indices, offsets, B, grad32, pads=None, slice=(0, None), init=None):
    """list of T fp32 ``[rows_t, dims_t]``: ``embedding_rules.dense_grad`` of every table on its stretch of the slice.  ``grad32``:
    ``[N, >= D]`` (the first ``dims_t`` columns of a row are read); ``pads``: ``int | None`` per table; ``slice``: ``(bag_begin,
    bag_count)``.  Rows of positions outside the slice are never read (they may hold NaN).  ``init``: fp32 buffers the gradient is
    ADDED to (the ``out=`` rule: the same sequential adds, starting from what the row held; a padding row keeps its bits)."""
    idx = np.asarray(indices).astype(np.int64).reshape(-1)
    g = np.asarray(grad32, dtype=np.float32).reshape(idx.size, -1)
    T = len(rows)
    pads = [None] * T if pads is None else pads
    out = []
    for t, (lo, hi) in enumerate(table_slices(offsets, T, B, idx.size, slice[0], slice[1])):
        if init is not None:
            acc = np.array(init[t], dtype=np.float32, copy=True)
            with np.errstate(all="ignore"):
                for j in range(lo, hi):
                    if idx[j] != pads[t]:
                        acc[idx[j]] = acc[idx[j]] + g[j, :dims[t]]
            out.append(acc)
        elif hi > lo:
            out.append(E.dense_grad(rows[t], idx[lo:hi], np.ascontiguousarray(g[lo:hi, :dims[t]]), pads[t]))
        else:
            out.append(np.zeros((rows[t], dims[t]), dtype=np.float32))
    return out
