"""ROW-QUANTISED TABLES of PER-TABLE FORMAT (include/param_amd.h, "PER-TABLE FORMATS"): no rule of its own.  Table ``t`` has a format
``bits[t]`` (8 or 4); the pooled output of table ``t`` is ``tests/qrows_rules.forward`` of THAT table alone with ``bits[t]`` over that
table's part of the request, and the un-pooled row of position ``j`` is ``tests/qgather_rules.rows`` of the table that owns ``j`` with
that table's bits.  Both modules are held to torch's CPU operators by their own host tests; tests/test_qmixed_host.py holds this
per-table application to the operators once more, live."""
import numpy as np

from tests import out16_rules as O
from tests import qgather_rules as Q
from tests import qrows_rules as R


def table_part(t, T, B, indices, offsets, psw=None):
    """table ``t``'s part of a TBE request as a request over ONE table: ``(indices, offsets [B], psw)`` -- the table's B offsets as they
    are (absolute positions) and the index array cut where the next table begins, so that the table's last bag ends there"""
    idx = np.asarray(indices)
    off = np.asarray(offsets).astype(np.int64)
    end = int(off[(t + 1) * B]) if t + 1 < T else idx.size
    return idx[:end], off[t * B:(t + 1) * B], None if psw is None else np.asarray(psw, dtype=np.float32)[:end]


def forward(qtables, dims, bits, indices, offsets, B, psw=None, bag_begin=0, bag_count=None):
    """list of T fp32 arrays ``[bag_count, D_t]``: ``qrows_rules.forward`` table by table, each with its own ``bits[t]``"""
    T = len(qtables)
    outs = []
    for t in range(T):
        idx, off, w = table_part(t, T, B, indices, offsets, psw)
        outs.append(R.forward([qtables[t]], [dims[t]], bits[t], idx, off, B, w, bag_begin, bag_count)[0])
    return outs


def forward16(qtables, dims, bits, indices, offsets, B, dtype, psw=None, bag_begin=0, bag_count=None):
    """the same as uint16 bit patterns of ``dtype`` (``"bf16"`` / ``"fp16"``): ONE rounding of the fp32 result"""
    return [O.round16(o, dtype) for o in forward(qtables, dims, bits, indices, offsets, B, psw, bag_begin, bag_count)]


def gather_tables(qtables, dims, bits, indices, offsets, B, bag_begin=0, bag_count=None):
    """per-table lists: ``[(positions int64 [n_t], values fp32 [n_t, D_t])]`` of the WRITTEN positions of every table, each dequantised
    by ``qgather_rules.rows`` with its own ``bits[t]``"""
    idx = np.asarray(indices).astype(np.int64)
    table, written = Q.owners(offsets, len(qtables), B, idx.size, bag_begin, bag_count)
    out = []
    for t, (q, d) in enumerate(zip(qtables, dims)):
        pos = np.nonzero(written & (table == t))[0]
        out.append((pos, Q.rows(q, d, bits[t], idx[pos])))
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
