"""numpy restatement of the ROW-QUANTISED TABLES rule (include/param_amd.h, "ROW-QUANTISED TABLES"): sum pooling straight from tables in
the 8- / 4-bit row-wise format, bit for bit what torch's CPU operators ``quantized::embedding_bag_byte_rowwise_offsets`` and
``quantized::embedding_bag_4bit_rowwise_offsets`` compute (tests/test_qrows_host.py holds this module to them, live and through a fixture).

A table is uint8 ``[rows, row_bytes(D, bits)]``: codes first (a 4-bit code of column c in byte c // 2 at bit 4 * (c % 2)), then fp32
``scale, bias`` (8 bits) or fp16 ``scale, bias`` widened exactly (4 bits).  For a bag, per column, over its lookups j in index order
from ``acc = +0.0``::

    sc = fl32(scale_r * w_j)    bi = fl32(bias_r * w_j)          (unweighted: sc = scale_r, bi = bias_r)
    acc = fmaf(sc, (float)code[r, c], fl32(acc + bi))            r = indices[j]

The fused multiply-add is emulated EXACTLY: the product of an fp32 value and a code below 256 is exact in fp64, the fp64 sum is rounded
to odd (TwoSum gives the exact residual), and the cast to fp32 is then the one correct rounding (53 >= 2 * 24 + 2 bits).  A plain fp64
multiply-add would round twice.  Inf and NaN go through as IEEE arithmetic gives them; NaN payloads are not part of the rule
(:func:`same_f32`).  16-bit outputs: ``tests/out16_rules.round16`` of the fp32 result."""
import numpy as np

from tests import out16_rules as O
from tests.padding_rules import bag_bounds

BITS = (8, 4)


def row_bytes(dim, bits):
    return dim + 8 if bits == 8 else dim // 2 + 4


def unpack(q, dim, bits):
    """(codes uint8 ``[n, dim]``, scale fp32 ``[n]``, bias fp32 ``[n]``) of uint8 rows ``[n, row_bytes]``"""
    q = np.ascontiguousarray(q, dtype=np.uint8).reshape(-1, row_bytes(dim, bits))
    n = q.shape[0]
    if bits == 8:
        tail = q[:, dim:dim + 8].copy().view(np.float32).reshape(n, 2)
        return q[:, :dim].copy(), tail[:, 0].copy(), tail[:, 1].copy()
    assert bits == 4, bits
    nb = dim // 2
    codes = np.empty((n, dim), dtype=np.uint8)
    codes[:, 0::2] = q[:, :nb] & 0xf
    codes[:, 1::2] = q[:, :nb] >> 4
    tail = q[:, nb:nb + 4].copy().view(np.float16).reshape(n, 2).astype(np.float32)
    return codes, tail[:, 0].copy(), tail[:, 1].copy()


def fmaf(a, b, c):
    """fp32 ``a * b + c`` with ONE rounding; ``a * b`` must be exact in fp64 (here b is a code below 256)"""
    with np.errstate(all="ignore"):
        p = np.asarray(a, dtype=np.float32).astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64)
        c = np.asarray(c, dtype=np.float32).astype(np.float64)
        p, c = np.broadcast_arrays(p, c)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = s.copy().view(np.int64)
        need = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((bits & 1) == 0)
        away = (err > 0) == (s > 0)                   # the exact sum lies beyond s in magnitude
        # (s == 0 with a residual cannot happen: a zero sum of two fp64 values is exact)
        bits = np.where(need, np.where(away, bits + 1, bits - 1), bits)
        return bits.view(np.float64).astype(np.float32)


def pool(codes, scale, bias, rows_of, w_of):
    """the rule for a list of bags at once: ``rows_of[k]`` the int row array of bag k (``w_of[k]`` its fp32 weights or None) ->
    fp32 ``[len(rows_of), D]``.  Step l joins the l-th lookup of every bag that has one."""
    nb, D = len(rows_of), codes.shape[1]
    acc = np.zeros((nb, D), dtype=np.float32)
    lens = np.array([len(r) for r in rows_of], dtype=np.int64)
    order = np.argsort(-lens, kind="stable")              # bags by falling length: step l joins a prefix
    fcodes = codes.astype(np.float32)
    with np.errstate(all="ignore"):
        for step in range(int(lens.max()) if nb else 0):
            sel = order[:int((lens > step).sum())]
            r = np.array([rows_of[k][step] for k in sel], dtype=np.int64)
            sc, bi = scale[r], bias[r]
            if w_of is not None:
                w = np.array([w_of[k][step] for k in sel], dtype=np.float32)
                sc, bi = sc * w, bi * w
            acc[sel] = fmaf(sc[:, None], fcodes[r], acc[sel] + bi[:, None])
    return acc


def forward(qtables, dims, bits, indices, offsets, B, psw=None, bag_begin=0, bag_count=None):
    """list of T fp32 arrays ``[bag_count, D_t]``: the rule over the bags ``[bag_begin, bag_begin + bag_count)`` of every table.
    ``qtables``: uint8 arrays ``[rows_t, row_bytes(D_t, bits)]``; the request is the TBE request of every pooled entry point."""
    T = len(qtables)
    idx = np.asarray(indices).astype(np.int64)
    bag_count = B - bag_begin if bag_count is None else bag_count
    start, end = bag_bounds(offsets, T, B, idx.size)
    w = None if psw is None else np.asarray(psw, dtype=np.float32)
    outs = []
    for t in range(T):
        codes, scale, bias = unpack(qtables[t], dims[t], bits)
        bags = [(int(start[t * B + bag_begin + k]), int(end[t * B + bag_begin + k])) for k in range(bag_count)]
        outs.append(pool(codes, scale, bias, [idx[s:e] for s, e in bags], None if w is None else [w[s:e] for s, e in bags]))
    return outs


def forward16(qtables, dims, bits, indices, offsets, B, dtype, psw=None, bag_begin=0, bag_count=None):
    """the same as uint16 bit patterns of ``dtype`` (``"bf16"`` / ``"fp16"``): ONE rounding of the fp32 result"""
    return [O.round16(o, dtype) for o in forward(qtables, dims, bits, indices, offsets, B, psw, bag_begin, bag_count)]


def same_f32(got, want):
    """equal bit for bit where ``want`` is not a NaN; where it is, ``got`` is a NaN too (payload and sign are not part of the rule)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)) and np.isnan(got[nan]).all())


def special_rows(dim, bits):
    """hand-built rows ``[4, row_bytes]`` whose tails are not finite: scale +Inf, bias -Inf, scale NaN, bias NaN (codes 0, 1, 2, ..)"""
    n = 4
    codes = (np.arange(n * dim, dtype=np.int64).reshape(n, dim) % (256 if bits == 8 else 16)).astype(np.uint8)
    tails = np.array([[np.inf, 0.5], [0.25, -np.inf], [np.nan, 1.0], [2.0, np.nan]])
    if bits == 8:
        return np.concatenate([codes, tails.astype(np.float32).view(np.uint8).reshape(n, 8)], axis=1)
    packed = (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)
    return np.concatenate([packed, tails.astype(np.float16).view(np.uint8).reshape(n, 4)], axis=1)
