"""numpy restatement of the OUTPUT DTYPE rule (include/param_amd.h, "OUTPUT DTYPE"): a bf16 / fp16 pooled output is ``round16`` of the
fp32 output of the same request -- tests/padding_rules.py (sum, weighted sum) or tests/mean_rules.py (mean) -- with ONE rounding to
nearest even per element; a 16-bit gradient is widened exactly.  16-bit values travel as uint16 bit patterns; ``dtype`` is ``"bf16"``
or ``"fp16"``.

* ``round16``: bf16 in integer arithmetic on the fp32 bits ``u``: ``(u + 0x7fff + ((u >> 16) & 1)) >> 16``, which carries into the
  exponent (and to Inf) by itself and keeps subnormals and signed zeros; a NaN gives ``(u >> 16) | 0x40``.  fp16 is numpy's
  float32 -> float16 cast (IEEE round to nearest even, overflow to Inf, subnormals produced).  tests/test_out16_host.py holds both to
  torch's CPU casts bit for bit on every non-NaN input it lists; NaNs are compared by class and sign only (:func:`same_bits`).
* ``widen``: the exact fp32 value of every 16-bit pattern."""
import numpy as np

from tests import mean_rules as M
from tests import padding_rules as P

DTYPES = ("bf16", "fp16")


def round16(x32, dtype):
    """uint16 bits of the fp32 array ``x32`` rounded to ``dtype``"""
    x = np.ascontiguousarray(x32, dtype=np.float32)
    if dtype == "fp16":
        with np.errstate(all="ignore"):
            return x.astype(np.float16).view(np.uint16)
    assert dtype == "bf16", dtype
    u = x.view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def widen(bits, dtype):
    """the fp32 array a uint16 array of ``dtype`` bit patterns stands for (exact)"""
    b = np.ascontiguousarray(bits, dtype=np.uint16)
    if dtype == "fp16":
        return b.view(np.float16).astype(np.float32)
    assert dtype == "bf16", dtype
    return (b.astype(np.uint32) << 16).view(np.float32)


def is_nan16(bits, dtype):
    b = np.asarray(bits, dtype=np.uint16)
    return (b & 0x7fff) > (0x7f80 if dtype == "bf16" else 0x7c00)


def same_bits(got, want, dtype):
    """equal bit for bit where ``want`` is not a NaN; where it is, ``got`` is a NaN of the same sign"""
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    if got.shape != want.shape:
        return False
    nan = is_nan16(want, dtype)
    return bool(np.array_equal(got[~nan], want[~nan]) and is_nan16(got[nan], dtype).all() and
                np.array_equal(got[nan] & 0x8000, want[nan] & 0x8000))


def forward(tables, indices, offsets, B, pads, dtype, psw=None, mean=False, bag_begin=0, bag_count=None):
    """list of T uint16 arrays ``[bag_count, D_t]``: ``round16`` of the fp32 rule's output (``tables``: fp32 arrays, 16-bit tables
    widened)"""
    if mean:
        assert psw is None
        outs = M.forward(tables, indices, offsets, B, pads, bag_begin, bag_count)
    else:
        outs = P.forward(tables, indices, offsets, B, pads, psw, bag_begin, bag_count)
    return [round16(o, dtype) for o in outs]
