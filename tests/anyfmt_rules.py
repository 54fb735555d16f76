"""The MIXED-FORMAT TABLES rule (include/param_amd.h) has NO ARITHMETIC OF ITS OWN, and neither has this file: it applies the existing
restatements table by table --

* fp32 / bf16 / fp16 tables: tests/padding_rules.py (the fp32 sum in index order over the widened table, no padding row) pooled,
  tests/embedding_rules.py un-pooled (same type in and out is a bit copy);
* FP8 tables with their table exponent: tests/f8s_rules.py (on top of tests/f8_rules.py's ``dec``), pooled and un-pooled;
* 8- / 4-bit rows: tests/qrows_rules.py pooled, tests/qgather_rules.py un-pooled;
* a 16-bit output: tests/out16_rules.py's one rounding of the fp32 result.

A table travels as ``Table(fmt, data, dim, exp)``: ``fmt`` one of ``FORMATS``, ``data`` the uint8 bytes ``[rows, row_bytes(fmt, dim)]`` exactly as the
module stores them, ``exp`` the FP8 table exponent (0 otherwise).  Table ``t`` of a request is handed to its family's rule as a ONE-table
request: its own ``B`` offsets and the index array cut at the next table's border (the rules end a request's last bag at N).
Outputs travel as BITS of the output kind (``"f32"`` uint32, ``"bf16"`` / ``"f16"`` uint16).  NaN compares as NaN where the format's own
rule says so: ``same`` is a bit compare but for NaN payloads (and NaN signs), except where the rule is a bit copy."""
from collections import namedtuple

import numpy as np

from tests import embedding_rules as E
from tests import f8s_rules as FS
from tests import out16_rules as O
from tests import padding_rules as P
from tests import qgather_rules as QG
from tests import qrows_rules as Q

FORMATS = ("fp32", "bf16", "fp16", "fp8_e4m3", "fp8_e5m2", "int8", "int4")
CODES = {"fp32": 0, "bf16": 1, "fp16": 2, "fp8_e4m3": 3, "fp8_e5m2": 4, "int8": 5, "int4": 6}      # include/param_amd.h
KINDS = ("f32", "bf16", "f16")
_KIND = {"fp32": "f32", "bf16": "bf16", "fp16": "f16"}          # a float format as tests/embedding_rules.py spells it
_O16 = {"bf16": "bf16", "f16": "fp16"}                          # an output kind as tests/out16_rules.py spells it
_F8 = {"fp8_e4m3": "e4m3", "fp8_e5m2": "e5m2"}
_BITS = {"int8": 8, "int4": 4}

Table = namedtuple("Table", "fmt data dim exp")


def row_bytes(fmt, dim):
    if fmt in _BITS:
        return Q.row_bytes(dim, _BITS[fmt])
    return dim * (4 if fmt == "fp32" else 2 if fmt in _KIND else 1)


def make_table(fmt, data, dim, exp=0):
    data = np.ascontiguousarray(data).view(np.uint8).reshape(-1, row_bytes(fmt, dim))
    assert exp == 0 or fmt in _F8
    return Table(fmt, data, int(dim), int(exp))


def float_bits(tab):
    """a float table's elements as bits ``[rows, dim]`` (uint32 / uint16)"""
    return tab.data.view(E.BITS[_KIND[tab.fmt]]).reshape(-1, tab.dim)


def widened(tab):
    """fp32 ``[rows, dim]`` of a float or FP8 table: the stored values"""
    if tab.fmt in _KIND:
        return np.ascontiguousarray(E.to_f32(float_bits(tab), _KIND[tab.fmt])).reshape(-1, tab.dim)
    return FS.dequant(tab.data, _F8[tab.fmt], tab.exp)


def one_table_request(t, T, indices, offsets, B, psw=None):
    """table ``t``'s part of a request as a request over ONE table: (indices cut at the next border, its B offsets, weights cut alike)"""
    idx, off = np.asarray(indices), np.asarray(offsets)
    end = int(off[(t + 1) * B]) if t + 1 < T else idx.size
    return idx[:end], off[t * B:(t + 1) * B], None if psw is None else np.asarray(psw, dtype=np.float32)[:end]


def to_kind(x32, kind):
    """fp32 values as output bits of ``kind``: themselves, or the one rounding"""
    x = np.ascontiguousarray(x32, dtype=np.float32)
    return x.view(np.uint32).copy() if kind == "f32" else O.round16(x, _O16[kind])


def forward(tables, indices, offsets, B, psw=None, bag_begin=0, bag_count=None):
    """list of T fp32 arrays ``[bag_count, D_t]``: every table pooled by its own family's rule"""
    T, outs = len(tables), []
    for t, tab in enumerate(tables):
        idx, off, w = one_table_request(t, T, indices, offsets, B, psw)
        if tab.fmt in _BITS:
            outs.append(Q.forward([tab.data], [tab.dim], _BITS[tab.fmt], idx, off, B, w, bag_begin, bag_count)[0])
        elif tab.fmt in _F8:
            outs.append(FS.forward([tab.data], _F8[tab.fmt], [(tab.exp, None)], idx, off, B, None, w, False, bag_begin, bag_count)[0])
        else:
            with np.errstate(all="ignore"):
                outs.append(P.forward([widened(tab)], idx, off, B, [None], w, bag_begin, bag_count)[0])
    return outs


def forward_bits(tables, indices, offsets, B, kind, psw=None, bag_begin=0, bag_count=None):
    """the same as output bits of ``kind``"""
    return [to_kind(o, kind) for o in forward(tables, indices, offsets, B, psw, bag_begin, bag_count)]


def sequence(tables, indices, offsets, B, kind, bag_begin=0, bag_count=None):
    """(output bits of ``kind`` ``[N, D]`` -- zeros in the rows that are not written --, written bool ``[N]``, copied bool ``[N]``: the row is a
    bit copy) for tables of one common dim: every position by the un-pooled rule of the table that owns it"""
    T, D = len(tables), tables[0].dim
    N = np.asarray(indices).size
    out = np.zeros((N, D), dtype=E.BITS[kind])
    written, copied = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    for t, tab in enumerate(tables):
        idx, off, _ = one_table_request(t, T, indices, offsets, B)
        n = idx.size
        if tab.fmt in _BITS:
            vals, w = QG.gather([tab.data], D, _BITS[tab.fmt], idx, off, B, bag_begin, bag_count)
            vals = to_kind(vals, kind)
        elif tab.fmt in _F8:
            vals, w = FS.sequence([tab.data], _F8[tab.fmt], [(tab.exp, None)], idx, off, B, bag_begin, bag_count)
            vals = to_kind(vals, kind)
        else:
            vals = E.forward([float_bits(tab)], _KIND[tab.fmt], kind, idx, off, B, np.zeros((n, D), dtype=E.BITS[kind]), bag_begin, bag_count)
            _, w = E.in_slice(off, 1, B, n, bag_begin, bag_count)
            copied[:n] |= w & (_KIND[tab.fmt] == kind)
        assert not (written[:n] & w).any(), "a position has one owner"
        out[:n][w] = vals[w]
        written[:n] |= w
    return out, written, copied


def is_nan(bits, kind):
    return E.is_nan(bits, kind)


def same(got, want, kind, copied=None):
    """bit for bit where ``want`` is not a NaN; where it is, ``got`` is a NaN.  Rows of ``copied`` (bool per row): bit for bit, NaNs included."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = is_nan(want, kind)
    ok = np.array_equal(got[~nan], want[~nan]) and bool(is_nan(got[nan], kind).all())
    if copied is not None:
        ok = ok and np.array_equal(got[copied], want[copied])
    return bool(ok)
