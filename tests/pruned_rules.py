"""PRUNED TABLES (include/param_amd.h, "PRUNED TABLES"): no arithmetic of its own.  Table ``t`` may carry a remap -- int array
``[logical_rows_t]`` with values in ``[-1, rows_t)``, ``None``: the table is not pruned (the identity).  Pooled: the lookups of a bag
whose remap value is -1 are DELETED, index and weight alike, the others take their remap value, and the rest is ``tests/qmixed_rules``
table by table.  Un-pooled: a written position whose remap value is -1 is a row of +0.0; every other position ``qmixed_rules``' row of
the remapped index.  tests/test_pruned_host.py holds both to torch's CPU operators called with ``pruned_weights=True``."""
import numpy as np

from tests import out16_rules as O
from tests import qgather_rules as Q
from tests import qmixed_rules as M


def physical(remaps, indices, offsets, B):
    """int64 ``[N]``: the physical row of every lookup position of a TBE request (-1: pruned; positions in front of every table keep
    their index) -- the owner's remap applied, ``None`` the identity"""
    idx = np.asarray(indices).astype(np.int64)
    table, _ = Q.owners(offsets, len(remaps), B, idx.size)
    phys = idx.copy()
    for t, r in enumerate(remaps):
        if r is not None:
            own = table == t
            phys[own] = np.asarray(r).astype(np.int64)[idx[own]]
    return phys


def compact(remaps, indices, offsets, B, psw=None):
    """the request with the pruned lookups deleted and the rest remapped: ``(indices int64, offsets int64 [len(offsets)], psw | None,
    kept bool [N])`` -- what the module without pruning is fed over the physical tables"""
    phys = physical(remaps, indices, offsets, B)
    keep = phys >= 0
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)      # kept lookups in front of every position
    off = before[np.asarray(offsets).astype(np.int64)]
    return phys[keep], off, None if psw is None else np.asarray(psw, dtype=np.float32)[keep], keep


def forward(qtables, dims, bits, remaps, indices, offsets, B, psw=None, bag_begin=0, bag_count=None):
    """list of T fp32 arrays ``[bag_count, D_t]``: ``qmixed_rules.forward`` over the physical tables of the compacted request"""
    idx, off, w, _ = compact(remaps, indices, offsets, B, psw)
    return M.forward(qtables, dims, bits, idx, off, B, w, bag_begin, bag_count)


def forward16(qtables, dims, bits, remaps, indices, offsets, B, dtype, psw=None, bag_begin=0, bag_count=None):
    """the same as uint16 bit patterns of ``dtype`` (``"bf16"`` / ``"fp16"``): ONE rounding of the fp32 result"""
    return [O.round16(o, dtype) for o in forward(qtables, dims, bits, remaps, indices, offsets, B, psw, bag_begin, bag_count)]


def gather(qtables, dim, bits, remaps, indices, offsets, B, bag_begin=0, bag_count=None):
    """(fp32 ``[N, dim]`` -- +0.0 in the rows of pruned positions and in the rows that are not written --, written bool ``[N]``: pruned
    positions inside the slice ARE written) for tables of one common ``dim``"""
    phys = physical(remaps, indices, offsets, B)
    pruned = phys < 0
    # (a pruned position's row is not read: any row of a table that has one stands in, then the zeros; a table without a physical row
    # has only pruned positions and is looked up in an all-zero stand-in of one row)
    stand_in = [q if np.asarray(q).shape[0] else np.zeros((1, np.asarray(q).shape[1]), dtype=np.uint8) for q in qtables]
    out, written = M.gather(stand_in, dim, bits, np.where(pruned, 0, phys), offsets, B, bag_begin, bag_count)
    out[pruned] = 0.0
    return out, written
