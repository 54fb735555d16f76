"""numpy restatement of the UN-POOLED LOOKUP rule (include/param_amd.h, "UN-POOLED LOOKUPS"; torch's ``nn.Embedding``): one output row
per lookup position.  Everything travels as BITS -- uint32 for fp32, uint16 for bf16 / fp16 (``kind`` is ``"f32"``, ``"bf16"`` or
``"f16"``) -- because the same-dtype rule is a bit copy: ``-0.0``, subnormals, Inf and NaN payloads leave exactly as stored.

* forward: position ``j`` belongs to the last table ``t`` with ``offsets[t * B] <= j`` (tests/padding_rules.py: ``table_of``); inside
  the bag slice ``out[j, :D_t] = conv(table_t[indices[j]])``; every other element of ``out`` keeps what the canvas held.
* ``conv``: same kind in and out -- the bits; 16 bits -> fp32 -- the exact widening; fp32 -> 16 bits and bf16 <-> fp16 -- widened
  exactly, then the ONE rounding of tests/out16_rules.py (``round16``).
* dense gradient of one table: sequential fp32 adds of the gradient rows in lookup order into zeros; the padding row stays zero.
* sparse gradient: the same values at the ascending distinct rows looked up, the padding row absent.

The GPU tests hold the kernel and the module to all of it bit for bit; tests/test_embedding_host.py holds the rule to torch's CPU
``nn.Embedding``: the forward always, the dense ``weight.grad`` on a request WITH repeated rows (torch's CPU kernel adds a row's
gradients in index order, so the pin did not have to be narrowed to requests without repeats), the sparse gradient against torch's
``.coalesce()`` where no row repeats (coalesce sums in an order of its own)."""
import numpy as np

from tests import out16_rules as O
from tests import padding_rules as P

KINDS = ("f32", "bf16", "f16")
_O16 = {"bf16": "bf16", "f16": "fp16"}          # this file's kinds as tests/out16_rules.py spells them
BITS = {"f32": np.uint32, "bf16": np.uint16, "f16": np.uint16}


def to_bits(values32, kind):
    """fp32 values as table bits of ``kind`` (16-bit kinds: rounded to nearest even)"""
    v = np.ascontiguousarray(values32, dtype=np.float32)
    return v.view(np.uint32).copy() if kind == "f32" else O.round16(v, _O16[kind])


def to_f32(bits, kind):
    """the fp32 values table bits of ``kind`` stand for (exact)"""
    if kind == "f32":
        return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)
    return O.widen(bits, _O16[kind])


def conv(bits, kind_in, kind_out):
    """output bits of ``kind_out`` for table bits of ``kind_in``"""
    bits = np.ascontiguousarray(bits, dtype=BITS[kind_in])
    if kind_in == kind_out:
        return bits.copy()
    wide = to_f32(bits, kind_in)
    if kind_out == "f32":
        return np.ascontiguousarray(wide).view(np.uint32).copy()
    return O.round16(wide, _O16[kind_out])


def is_nan(bits, kind):
    b = np.asarray(bits)
    if kind == "f32":
        return (b & 0x7fffffff) > 0x7f800000
    return O.is_nan16(b, _O16[kind])


def same(got, want, kind_in, kind_out):
    """bit for bit; for a CONVERTED output a NaN of the rule only asks for a NaN of its sign (the payload is not part of the rule)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if kind_in == kind_out:
        return bool(np.array_equal(got, want))
    nan = is_nan(want, kind_out)
    sign = 0x80000000 if kind_out == "f32" else 0x8000
    return bool(np.array_equal(got[~nan], want[~nan]) and is_nan(got[nan], kind_out).all() and
                np.array_equal(got[nan] & sign, want[nan] & sign))


def in_slice(offsets, T, B, N, bag_begin=0, bag_count=None):
    """(table of every position, bool: the position belongs to a bag of the slice)"""
    bag_count = B - bag_begin if bag_count is None else bag_count
    tab = P.table_of(offsets, T, B, N)
    if N == 0 or bag_count == 0:
        return tab, np.zeros(N, dtype=bool)
    start, end = P.bag_bounds(offsets, T, B, N)
    pos = np.arange(N, dtype=np.int64)
    t = np.maximum(tab, 0)
    inside = (tab >= 0) & (pos >= start[t * B + bag_begin]) & (pos < end[t * B + bag_begin + bag_count - 1])
    return tab, inside


def forward(tables, kind_in, kind_out, indices, offsets, B, canvas, bag_begin=0, bag_count=None):
    """``canvas`` (bits of ``kind_out``, ``[N, stride]``) with the rule's rows written into it: ``tables`` is a list of T bit arrays
    ``[rows_t, D_t]`` of ``kind_in``"""
    idx = np.asarray(indices).astype(np.int64)
    out = np.array(canvas, dtype=BITS[kind_out], copy=True)
    tab, inside = in_slice(offsets, len(tables), B, idx.size, bag_begin, bag_count)
    for t, w in enumerate(tables):
        sel = np.nonzero(inside & (tab == t))[0]
        if sel.size:
            out[sel, :w.shape[1]] = conv(np.asarray(w)[idx[sel]], kind_in, kind_out)
    return out


def dense_grad(rows, indices, grad32, padding_idx=None):
    """fp32 ``[rows, D]``: ``grad32[j]`` added to row ``indices[j]`` in lookup order, from zeros; the padding row stays zero"""
    idx = np.asarray(indices).astype(np.int64).reshape(-1)
    g = np.asarray(grad32, dtype=np.float32).reshape(idx.size, -1)
    out = np.zeros((rows, g.shape[1]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for j, r in enumerate(idx):
            if r != padding_idx:
                out[r] = out[r] + g[j]
    return out


def sparse_grad(rows, indices, grad32, padding_idx=None):
    """(ascending distinct rows looked up without the padding row, their rows of ``dense_grad``)"""
    idx = np.asarray(indices).astype(np.int64).reshape(-1)
    hit = np.unique(idx[idx != padding_idx]) if padding_idx is not None else np.unique(idx)
    return hit, dense_grad(rows, idx, grad32, padding_idx)[hit]
