"""Pooled and un-pooled lookups over OCP FP8 embedding tables (``csrc/embbag_fwd_f8_kernel.inc`` through ``pm_embbag_fwd_f8``,
``csrc/embedding_gather_f8.hip`` through ``pm_embedding_gather_f8``), plain or with power-of-two scales (``csrc/f8_quantize.hip``,
``csrc/embbag_fwd_f8s_kernel.inc``, ``csrc/embedding_gather_f8s.hip`` through ``pm_rows_quantize_f8`` / ``pm_embbag_fwd_f8_scaled`` /
``pm_embedding_gather_f8_scaled``).

* :class:`Float8BatchedEmbeddingBagMI355` -- T tables stored as ``torch.float8_e4m3fn`` or ``torch.float8_e5m2`` bytes, one byte per
  element, pooled (sum, weighted sum or mean, with ``padding_idx``) by ONE launch that reads those bytes;
  ``lookup_sequence`` is its un-pooled lookup.  The serving-side sibling of :class:`BatchedEmbeddingBagMI355`; what fbgemm's
  ``IntNBitTableBatchedEmbeddingBagsCodegen`` is for with ``SparseType.FP8`` tables.
* :class:`Float8EmbeddingBagMI355` -- the single-table module with ``nn.EmbeddingBag``'s call.
* :class:`Float8EmbeddingMI355` -- the single-table un-pooled module with ``nn.Embedding``'s call.

The arithmetic is fixed (include/param_amd.h, "FP8 TABLES"): every stored byte widens EXACTLY to fp32 (gfx950 converts both formats in
hardware), and from there the rule is the padded family's -- lookups equal to ``padding_idx`` removed, fp32 additions in index order
from +0.0 (one fmaf per lookup when weighted), one correctly rounded division for the mean, one rounding for a 16-bit ``output_dtype``
-- so the result is ``torch.nn.functional.embedding_bag(indices, table.to(torch.float32), ...)`` on the CPU bit for bit, and the
un-pooled rows are the stored values exactly (``-0.0``, subnormals and +-Inf included; a NaN code gives a NaN).

``scale=None`` (the default) is the plain format: no scale, no bias, ``from_float`` casts with torch's ``.to(dtype)``.  A table of small
values does not survive that cast (the uniform init of 10 M rows, |x| <= 3.2e-4, is all zeros in e4m3fn), so the three modules take
``scale="table"`` or ``scale="row"`` (include/param_amd.h, "SCALED FP8 TABLES"): the stored value is ``dec(code) * 2^(E_t + e_r)`` with
one int32 exponent per table (buffer ``table_exponents``) or one int8 exponent per row (buffer ``row_exponents``), in [-64, 64];
``quantize_from_`` / ``from_float(..., scale=...)`` run the HIP quantiser (the smallest exponent at which a row -- or the table -- does
not overflow, then torch's cast of ``x * 2^-s``), and the lookups are the same rule over the dequantised table, bit for bit.  A module
without a scale makes exactly the calls it made before.

Forward only: the tables are a buffer, nothing requires grad.  There is no CPU path.  Left out, on purpose: scales that are not powers
of two, MX block scales, the ``fnuz`` formats, FP8 output, a format per table, FP8 next to 8- / 4-bit tables in one launch, max pooling,
pruning, any backward, the operator plug-in.
"""
from __future__ import annotations

import ctypes
import operator
from typing import Optional, Sequence

import torch
import torch.nn as nn

from . import _lib
from .embedding_bag import (_IDTYPE, _WDTYPE, BatchedEmbeddingBagMI355, EmbeddingBagMI355, EmbeddingMI355, _BoundsChecked,
                            _check_rows_out, _normalize_padding_idx, _pad_tensor, _require_device, _stream_ptr, bounds_check_mode_name)
from .quantized_bag import _QTableSet

MAX_DIM = 2048      # kF8MaxDim (csrc/launch_plan.h)
_F8 = {torch.float8_e4m3fn: _lib.PM_F8E4M3, torch.float8_e5m2: _lib.PM_F8E5M2}
_SRC = {torch.float32: _lib.PM_F32, torch.bfloat16: _lib.PM_BF16, torch.float16: _lib.PM_F16}      # what the quantiser reads
EXP_MIN, EXP_MAX = -64, 64      # the range of a table's plus a row's exponent (csrc/f8s_elem.h)
_F8_NAMES = {"e4m3": torch.float8_e4m3fn, "fp8_e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2, "fp8_e5m2": torch.float8_e5m2}


def float8_dtype(dtype) -> torch.dtype:
    """``torch.float8_e4m3fn`` / ``torch.float8_e5m2`` from one of the two, or ``"e4m3"`` / ``"e5m2"`` / ``"fp8_e4m3"`` / ``"fp8_e5m2"``
    in any case; anything else -- ``torch.float8_e4m3fnuz`` included -- raises ValueError"""
    dt = _F8_NAMES.get(dtype.lower()) if isinstance(dtype, str) else dtype
    if dt not in _F8:
        raise ValueError(f"dtype must be torch.float8_e4m3fn or torch.float8_e5m2 (or \"e4m3\" / \"e5m2\" / \"fp8_e4m3\" / \"fp8_e5m2\"), got "
                         f"{dtype!r} (the fnuz formats are not implemented; other table dtypes: BatchedEmbeddingBagMI355)")
    return dt


def _scale_kind(scale):
    if scale is not None and scale not in ("table", "row"):
        raise ValueError(f'scale must be None, "table" or "row", got {scale!r} (scales that are not powers of two and MX block scales are not implemented)')
    return scale


def _pow2(exponents: torch.Tensor) -> torch.Tensor:
    """fp32 ``2^e`` for an integer tensor in [-64, 64], built from its bits: exact on every device"""
    return ((exponents.to(torch.int32) + 127) << 23).view(torch.float32)


def _pooling(mode, who: str) -> str:
    name = str(getattr(mode, "name", mode)).lower()
    name = {"0": "sum", "1": "mean"}.get(name, name)
    if name not in ("sum", "mean"):
        raise ValueError(f"{who}: FP8 tables pool by sum or mean (got {mode!r}; max pooling and un-pooled modules of this kind are not implemented: "
                         "lookup_sequence is the un-pooled lookup)")
    return name


def _check_spec(dims: Sequence[int], layout: str) -> None:
    if layout == "blocked":
        raise ValueError('FP8 tables do not take layout="blocked"')
    if layout not in ("bd", "tbd"):
        raise ValueError(f'layout must be "bd" or "tbd", got {layout!r}')
    for d in dims:
        if d < 16 or d % 16 or d > MAX_DIM:
            raise ValueError(f"embedding dim {d}: an FP8 table needs a multiple of 16 in [16, {MAX_DIM}]")
    if layout == "tbd" and len(set(dims)) != 1:
        raise ValueError('layout "tbd" needs one common embedding dim')


def _weight_bytes(weight: torch.Tensor, dtype: torch.dtype, shape, what: str) -> torch.Tensor:
    """``weight`` as the uint8 bytes a table stores: a tensor of the table's float8 dtype or uint8, of ``shape``"""
    if not isinstance(weight, torch.Tensor) or weight.dtype not in (dtype, torch.uint8) or tuple(weight.shape) != tuple(shape):
        raise ValueError(f"{what} must be a {str(dtype).replace('torch.', '')} (or uint8: the same bytes) tensor of shape {tuple(shape)}, got "
                         f"{getattr(weight, 'dtype', type(weight).__name__)} {tuple(getattr(weight, 'shape', ()))}")
    return weight.detach().contiguous().view(torch.uint8)


class Float8BatchedEmbeddingBagMI355(nn.Module, _BoundsChecked):
    """T FP8 embedding tables in one HBM slab, pooled by ONE kernel launch that reads the stored bytes.

    ``Float8BatchedEmbeddingBagMI355(rows, dims, dtype=torch.float8_e4m3fn, device="cuda", layout="bd", output_dtype=None,
    bounds_check_mode="none", pooling_mode="sum", padding_idx=None)``: ``dtype`` one of the two torch float8 dtypes or their names (see
    :func:`float8_dtype`), one format per module; ``dims`` multiples of 16, at most 2048, and may differ per table with ``layout="bd"``
    (lane groups are sized for the widest table).  The tables live in ONE zero-filled uint8 buffer ``weights`` (table starts padded to
    256 B; ``state_dict`` round-trips it): every element starts as +0.0.  ``table(t)`` is the ``[rows_t, D_t]`` view in the float8 dtype;
    ``copy_from_(t, tensor)`` takes a tensor of that dtype, or uint8 bytes, as a bit copy.  ``from_float(source, dtype, **kw)`` builds a
    module from a :class:`BatchedEmbeddingBagMI355` sum / mean module or a list of float tensors with torch's ``.to(dtype)`` on the
    device where the source lives (round to nearest even, saturating to NaN / Inf as torch does: there is no quantiser kernel here).

    ``lookup(indices, offsets, per_sample_weights=None, out=None, bag_begin=0, bag_count=None, batch=None)`` -- and ``forward``, the same
    call -- takes the TBE request of :class:`BatchedEmbeddingBagMI355` and returns ``[B, sum D]`` (``"bd"``) or ``[T, B, D]`` (``"tbd"``) in
    ``output_dtype`` (fp32, or bf16 / fp16: the fp32 value rounded once in the kernel).  ``pooling_mode`` ``"sum"`` / ``"mean"``;
    ``padding_idx`` as in :class:`BatchedEmbeddingBagMI355` (None, one int, or one int | None per table).  ``plan(...)`` is the launch
    geometry of the same request (``pm_embbag_f8_plan``).  ``lookup_sequence(indices, offsets, batch=None, out=None, bag_begin=0,
    bag_count=None)`` is the UN-POOLED lookup: ``[N, D]``, the stored value of every looked-up element, exactly (one common embedding
    dim; ``padding_idx`` does not affect it); ``sequence_plan(...)`` its geometry.  ``bounds_check_mode`` and ``sanitize_``: see
    :class:`_BoundsChecked`.

    ``scale=None | "table" | "row"`` (include/param_amd.h, "SCALED FP8 TABLES"): with a scale the stored value is ``dec(code) * 2^(E_t +
    e_r)`` -- ``"table"``: an int32 ``[T]`` buffer ``table_exponents``; ``"row"``: one int8 slab ``row_exponents`` with the per-table
    view ``row_exponents_of(t)``; every exponent in [-64, 64], all zero at first; both round-trip through ``state_dict``.
    ``quantize_from_(t, tensor)`` fills table ``t`` from an fp32 / bf16 / fp16 tensor on the device with the HIP quantiser,
    ``copy_from_(t, codes, exponents=...)`` takes prepacked codes and exponents, ``dequantized_table(t)`` is the fp32 table, and
    ``from_float(source, dtype, scale=...)`` quantises instead of casting.  ``lookup``, ``forward``, ``lookup_sequence`` and ``plan`` go to
    the scaled calls when ``scale`` is set, and only then; everything else -- ``bounds_check_mode``, ``padding_idx``, mean,
    ``output_dtype``, batch slices, ``out=``, mixed dims -- works as without a scale.  With ``scale=None`` the module has the buffers,
    the ``state_dict`` keys and the calls it had before scales existed.

    No parameters; the output never requires grad.  ValueError before anything is allocated: another dtype (``float8_e4m3fnuz``
    included), a ``scale`` other than the three, dims that are not multiples of 16 or above 2048, ``layout="blocked"``, max / none pooling, ``rows >= 2^31``; a weighted
    mean lookup raises ValueError at the call.  Tensors that are not on a ROCm device raise RuntimeError (no CPU fallback),
    floating-point indices TypeError.
    """

    def __init__(self, rows: Sequence[int], dims, dtype=torch.float8_e4m3fn, device="cuda", layout: str = "bd", output_dtype=None,
                 bounds_check_mode="none", pooling_mode="sum", padding_idx=None, scale=None):
        super().__init__()
        self._init_shared(bounds_check_mode, output_dtype)
        self.dtype = float8_dtype(dtype)
        self.scale = _scale_kind(scale)
        rows = [int(r) for r in rows]
        dims = [int(dims)] * len(rows) if isinstance(dims, int) else [int(d) for d in dims]
        if len(rows) != len(dims) or not rows:
            raise ValueError("rows and dims must name the same tables, at least one")
        _check_spec(dims, layout)
        self.pooling_mode = _pooling(pooling_mode, type(self).__name__)
        self._mean = self.pooling_mode == "mean"
        if any(r < 1 or r >= 2**31 for r in rows):
            raise ValueError("every table needs 1 <= rows < 2^31")
        try:
            pads = [padding_idx if padding_idx is None or isinstance(padding_idx, bool) else operator.index(padding_idx)] * len(rows)
        except TypeError:      # not one integer for every table: one entry per table
            pads = list(padding_idx)
            if len(pads) != len(rows):
                raise ValueError(f"padding_idx has {len(pads)} entries for {len(rows)} tables (None, one int, or one int | None per table)")
        pads = [_normalize_padding_idx(k, r) for k, r in zip(pads, rows)]
        self.padding_idx = pads if any(k is not None for k in pads) else None
        self.rows, self.dims, self.layout = rows, dims, layout
        # table starts padded to 256 B: every row is 16-byte aligned, a D = 128 row is one aligned 128-byte line
        starts, cur = [], 0
        for r, d in zip(rows, dims):
            starts.append(cur)
            cur += (r * d + 255) // 256 * 256
        self._starts = starts
        self.register_buffer("weights", torch.zeros(cur, dtype=torch.uint8, device=device))
        self._ts: Optional[_QTableSet] = None
        # scaled tables: every exponent starts as 0 (with the zero codes: +0.0 everywhere)
        if self.scale == "table":
            self.register_buffer("table_exponents", torch.zeros(len(rows), dtype=torch.int32, device=device))
        elif self.scale == "row":
            self._row_starts = [sum(rows[:t]) for t in range(len(rows))]
            self.register_buffer("row_exponents", torch.zeros(sum(rows), dtype=torch.int8, device=device))
            self._row_ptrs: Optional[torch.Tensor] = None      # device int64 [T]: where each table's exponents start ...
            self._row_ptrs_base = 0                            # ... for the slab at this address

    _TABLES = "weights"

    # -- tables ------------------------------------------------------------------------------
    def _bytes(self, t: int) -> torch.Tensor:
        s, n = self._starts[t], self.rows[t] * self.dims[t]
        return self.weights[s:s + n].view(self.rows[t], self.dims[t])

    def table(self, t: int) -> torch.Tensor:
        """table ``t``: the ``[rows_t, D_t]`` view of the buffer in the module's float8 dtype"""
        return self._bytes(t).view(self.dtype)

    def copy_from_(self, t: int, tensor: torch.Tensor, exponents=None) -> None:
        """fill table ``t`` from a ``[rows_t, D_t]`` tensor of the module's float8 dtype, or of uint8 (the same bytes): a bit copy.
        ``exponents`` (scaled modules; None keeps what the module holds): the table's exponent, an int (``scale="table"``), or an
        integer tensor ``[rows_t]`` of row exponents (``scale="row"``), each in [-64, 64] -- checked here, once, with torch ops"""
        codes = _weight_bytes(tensor, self.dtype, (self.rows[t], self.dims[t]), f"copy_from_: table {t}")
        if exponents is not None:
            if self.scale is None:
                raise ValueError("copy_from_: exponents need a module with scale=\"table\" or scale=\"row\"")
            e = torch.as_tensor(exponents)
            want = () if self.scale == "table" else (self.rows[t],)
            if e.dtype.is_floating_point or e.dtype == torch.bool or tuple(e.shape) != want:
                raise ValueError(f"copy_from_: exponents must be {'one int' if self.scale == 'table' else f'an integer tensor of shape {want}'}, got "
                                 f"{e.dtype} {tuple(e.shape)}")
            if e.numel() and bool(((e < EXP_MIN) | (e > EXP_MAX)).any()):
                raise ValueError(f"copy_from_: exponents must lie in [{EXP_MIN}, {EXP_MAX}]")
            if self.scale == "table":
                self.table_exponents[t] = int(e)
            else:
                self.row_exponents_of(t).copy_(e)
        self._bytes(t).copy_(codes)

    def row_exponents_of(self, t: int) -> torch.Tensor:
        """``scale="row"``: the int8 ``[rows_t]`` view of table ``t``'s row exponents"""
        if self.scale != "row":
            raise ValueError('row_exponents_of needs a module with scale="row"')
        return self.row_exponents[self._row_starts[t]:self._row_starts[t] + self.rows[t]]

    def quantize_from_(self, t: int, tensor: torch.Tensor) -> None:
        """fill table ``t`` of a scaled module from a ``[rows_t, D_t]`` fp32 / bf16 / fp16 tensor on the module's ROCm device with the HIP
        quantiser: the row exponents (``pm_f8_row_exponents``), for ``scale="table"`` their maximum -- taken on the device, nothing
        synchronises --, then the codes (``pm_rows_quantize_f8``).  Rows may be strided (``tensor[:, a:b]`` of a wider tensor)."""
        if self.scale is None:
            raise ValueError("quantize_from_ needs a module with scale=\"table\" or scale=\"row\" (an unscaled table is torch's cast: copy_from_)")
        if not isinstance(tensor, torch.Tensor) or tensor.dtype not in _SRC or tuple(tensor.shape) != (self.rows[t], self.dims[t]):
            raise ValueError(f"quantize_from_: table {t} needs a float32 / bfloat16 / float16 tensor of shape {(self.rows[t], self.dims[t])}, got "
                             f"{getattr(tensor, 'dtype', type(tensor).__name__)} {tuple(getattr(tensor, 'shape', ()))}")
        _require_device(self.weights, f"{type(self).__name__}.weights")
        _require_device(tensor, "tensor")
        src = tensor.detach()
        if src.stride(1) != 1 or src.stride(0) < src.shape[1] or (src.stride(0) * src.element_size()) % 16 or src.data_ptr() % 16:
            src = src.contiguous()
        L, dst, stream = _lib.load(), self._bytes(t), _stream_ptr()
        head = (src.data_ptr(), _SRC[src.dtype], self.rows[t], self.dims[t], src.stride(0), _F8[self.dtype])
        rexp = self.row_exponents_of(t) if self.scale == "row" else torch.empty(self.rows[t], dtype=torch.int8, device=self.weights.device)
        _lib.check(L.pm_f8_row_exponents(*head, rexp.data_ptr(), stream))
        if self.scale == "row":
            _lib.check(L.pm_rows_quantize_f8(*head, None, rexp.data_ptr(), dst.data_ptr(), stream))
        else:
            e_t = self.table_exponents[t:t + 1]
            e_t.copy_(rexp.max().to(torch.int32))
            _lib.check(L.pm_rows_quantize_f8(*head, e_t.data_ptr(), None, dst.data_ptr(), stream))

    def dequantized_table(self, t: int) -> torch.Tensor:
        """table ``t`` as fp32: ``dec(code) * 2^(E_t + e_r)``, exactly (an unscaled module: ``table(t).float()``)"""
        w = self.table(t).to(torch.float32)
        if self.scale == "table":
            return w * _pow2(self.table_exponents[t])
        if self.scale == "row":
            return w * _pow2(self.row_exponents_of(t))[:, None]
        return w

    def _exponent_args(self):
        """(table_exp, row_exp) of the scaled calls: a device pointer or None each"""
        if self.scale == "table":
            return self.table_exponents.data_ptr(), None
        base = self.row_exponents.data_ptr()
        if self._row_ptrs is None or self._row_ptrs_base != base:
            self._row_ptrs = torch.tensor([base + s for s in self._row_starts], dtype=torch.int64).to(self.row_exponents.device)
            self._row_ptrs_base = base
        return None, self._row_ptrs.data_ptr()

    @classmethod
    def from_float(cls, source, dtype=torch.float8_e4m3fn, scale=None, **kw):
        """cast a :class:`BatchedEmbeddingBagMI355` (sum or mean pooling; its ``layout``, ``pooling_mode`` and ``padding_idx`` carry
        over) or a sequence of 2-D floating-point tensors with torch's ``.to(dtype)`` on the device where the source lives -- or, with
        ``scale="table"`` / ``"row"``, quantise it with the HIP quantiser on the module's device (``quantize_from_``); keywords go to
        the constructor (``device`` defaults to the source's)"""
        dt = float8_dtype(dtype)
        _scale_kind(scale)
        if isinstance(source, BatchedEmbeddingBagMI355):
            kw.setdefault("pooling_mode", _pooling(source.pooling_mode, "from_float"))
            kw.setdefault("padding_idx", source.padding_idx)
            kw.setdefault("layout", source.layout)
            tables = [source.table(t) for t in range(len(source.rows))]
        else:
            tables = list(source)
            if not tables or any(not isinstance(x, torch.Tensor) or x.dim() != 2 or not x.dtype.is_floating_point or x.dtype in _F8 for x in tables):
                raise TypeError("from_float takes a BatchedEmbeddingBagMI355 or a sequence of 2-D floating-point tensors")
        kw.setdefault("device", tables[0].device)
        if scale is None:
            m = cls([int(x.shape[0]) for x in tables], [int(x.shape[1]) for x in tables], dt, **kw)
            for t, x in enumerate(tables):
                m.copy_from_(t, x.detach().to(dt))
            return m
        m = cls([int(x.shape[0]) for x in tables], [int(x.shape[1]) for x in tables], dt, scale=scale, **kw)
        for t, x in enumerate(tables):
            x = x.detach().to(m.weights.device)
            m.quantize_from_(t, x if x.dtype in _SRC else x.to(torch.float32))
        return m

    def _tables(self) -> _QTableSet:
        if self._ts is None or self._ts.ptrs[0] != self._bytes(0).data_ptr():
            self._ts = _QTableSet([self._bytes(t) for t in range(len(self.rows))], self.dims, self.layout)
        return self._ts

    def _pad_dev(self) -> Optional[torch.Tensor]:
        if self.padding_idx is None:
            return None
        dev = self.weights.device
        if self._pad_t is None or self._pad_t.device != dev:
            self._pad_t = _pad_tensor(self.padding_idx, dev)
        return self._pad_t

    _batch_of = BatchedEmbeddingBagMI355._batch_of

    # -- ops ---------------------------------------------------------------------------------
    def _request(self, indices, offsets, per_sample_weights, bag_begin, bag_count, batch, sanitize: bool):
        if indices.dtype.is_floating_point or offsets.dtype.is_floating_point:
            raise TypeError(f"indices and offsets must both be int64 or both int32, got {indices.dtype} / {offsets.dtype}")
        if self._mean and per_sample_weights is not None:
            raise ValueError('pooling_mode="mean" is unweighted: per_sample_weights must be None')
        _require_device(self.weights, f"{type(self).__name__}.weights")
        B = self._batch_of(offsets, indices) if batch is None else batch
        ts = self._tables()
        if sanitize and self.bounds_check_mode != "none":
            self._sanitize(ts, indices, offsets, B, self.bounds_check_mode, per_sample_weights, bag_begin, bag_count)
        # the table set's (cached) request names fp32 tables -- what the sanitiser is handed --; the FP8 calls get a copy that names the format
        op = _lib.pm_embbag_batch.from_buffer_copy(ts.request(indices, offsets, B, per_sample_weights, bag_begin, bag_count, forward=True))
        op.weight_dtype = _F8[self.dtype]
        return ts, B, op

    def lookup(self, indices, offsets, per_sample_weights=None, out=None, bag_begin=0, bag_count=None, batch: Optional[int] = None):
        """The pooled forward; ``bag_begin/bag_count`` select a batch slice (bags outside it keep what ``out`` held)."""
        ts, B, op = self._request(indices, offsets, per_sample_weights, bag_begin, bag_count, batch, True)
        _, _, shape = ts.out_desc(B)
        odt = self.output_dtype
        if out is None:
            out = torch.empty(shape, dtype=odt, device=ts.device)
        elif out.dtype != odt or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != ts.device:
            raise ValueError(f"out must be a contiguous {str(odt).replace('torch.', '')} tensor of shape {shape} on {ts.device}")
        pad = self._pad_dev()
        if self.scale is None:
            rc = _lib.load().pm_embbag_fwd_f8(ctypes.byref(op), None if pad is None else pad.data_ptr(), 1 if self._mean else 0, _WDTYPE[odt],
                                              out.data_ptr(), _stream_ptr())
        else:
            rc = _lib.load().pm_embbag_fwd_f8_scaled(ctypes.byref(op), None if pad is None else pad.data_ptr(), 1 if self._mean else 0, _WDTYPE[odt],
                                                     *self._exponent_args(), out.data_ptr(), _stream_ptr())
        if rc:
            _lib.check(rc)
        return out

    def forward(self, indices, offsets, per_sample_weights=None, out=None, bag_begin=0, bag_count=None, batch: Optional[int] = None):
        return self.lookup(indices, offsets, per_sample_weights, out, bag_begin, bag_count, batch)

    def plan(self, indices, offsets, per_sample_weights=None, bag_begin=0, bag_count=None, batch: Optional[int] = None) -> dict:
        """the launch geometry ``lookup`` would use for this request under the knobs as they stand (``_lib.PLAN_FIELDS`` by name;
        ``pm_embbag_f8_plan``, nothing is launched)"""
        _, _, op = self._request(indices, offsets, per_sample_weights, bag_begin, bag_count, batch, False)
        if self.scale is None:
            return _lib.embbag_f8_plan(op, _WDTYPE[self.output_dtype])
        return _lib.embbag_f8_scaled_plan(op, _WDTYPE[self.output_dtype], self._mean, self.scale == "row")

    # -- un-pooled ---------------------------------------------------------------------------
    def _sequence_request(self, indices, offsets, batch, bag_begin, bag_count, sanitize: bool, out=None):
        if len(set(self.dims)) != 1:
            raise ValueError("lookup_sequence needs one common embedding dim (mixed dims are served by pm_embedding_gather_f8, the C call)")
        if out is not None:
            _check_rows_out(out, indices.numel(), self.dims[0], self.output_dtype, self.weights.device)
        return self._request(indices, offsets, None, bag_begin, bag_count, batch, sanitize)

    def lookup_sequence(self, indices, offsets, batch: Optional[int] = None, out=None, bag_begin=0, bag_count=None):
        """The UN-POOLED forward over the module's T tables: ``[N, D]`` in ``output_dtype``, ``N = indices.numel()``, row ``j`` = row
        ``indices[j]`` of the table that owns lookup position ``j`` (table ``t`` owns ``[offsets[t * B], offsets[(t + 1) * B])``), every
        element the stored value exactly -- one launch, ``pm_embedding_gather_f8``.  Runs after ``bounds_check_mode``, like ``lookup``;
        ``padding_idx`` does not affect it.  ``bag_begin/bag_count`` select a batch slice: only the rows of lookups inside it are
        written -- a caller's ``out`` keeps every other row, a tensor allocated here holds zeros there."""
        ts, B, op = self._sequence_request(indices, offsets, batch, bag_begin, bag_count, True, out)
        n, D, odt = indices.numel(), self.dims[0], self.output_dtype
        if out is None:
            whole = bag_begin == 0 and bag_count in (None, B)
            out = (torch.empty if whole else torch.zeros)((n, D), dtype=odt, device=ts.device)
        if n and self.scale is not None:
            rc = _lib.load().pm_embedding_gather_f8_scaled(ctypes.byref(op), _WDTYPE[odt], *self._exponent_args(), out.data_ptr(), D, _stream_ptr())
            if rc:
                _lib.check(rc)
        elif n:
            rc = _lib.load().pm_embedding_gather_f8(ctypes.byref(op), _WDTYPE[odt], out.data_ptr(), D, _stream_ptr())
            if rc:
                _lib.check(rc)
        return out

    def sequence_plan(self, indices, offsets, batch: Optional[int] = None, bag_begin=0, bag_count=None) -> dict:
        """the launch geometry ``lookup_sequence`` would use (``_lib.GATHER_PLAN_FIELDS`` by name; ``pm_embedding_gather_f8_plan``: the
        scaled un-pooled lookup has the unscaled one's geometry)"""
        _, _, op = self._sequence_request(indices, offsets, batch, bag_begin, bag_count, False)
        return _lib.embedding_gather_f8_plan(op)

    def sanitize_(self, indices, offsets, batch: Optional[int] = None, mode=None) -> None:
        """The sanitiser on its own (see :class:`BatchedEmbeddingBagMI355`)."""
        _require_device(self.weights, f"{type(self).__name__}.weights")
        B = self._batch_of(offsets, indices) if batch is None else batch
        mode = bounds_check_mode_name(mode) if mode is not None else self.bounds_check_mode
        self._sanitize(self._tables(), indices, offsets, B, "warning" if mode == "none" else mode)

    def extra_repr(self) -> str:
        return (f"rows={self.rows}, dims={self.dims}, dtype={self.dtype}, layout={self.layout}, pooling_mode={self.pooling_mode}" +
                (f", padding_idx={self.padding_idx}" if self.padding_idx is not None else "") +
                (f", output_dtype={self.output_dtype}" if self._out16 is not None else "") +
                (f", scale={self.scale}" if self.scale is not None else ""))


def _torch_weight(module, kinds, what: str) -> torch.Tensor:
    if not isinstance(module, kinds):
        raise TypeError(f"from_float takes {what}")
    if getattr(module, "max_norm", None) is not None:
        raise ValueError("from_float: max_norm is not implemented (the rows would be renormalised at lookup time)")
    return module.weight.detach()


def _quantized(m, w: torch.Tensor):
    """the single-table modules' ``from_float(..., scale=...)``: the source's weight through the quantiser on the module's device"""
    w = w.to(m.weights.device)
    m.quantize_from_(0, w if w.dtype in _SRC else w.to(torch.float32))
    return m


class Float8EmbeddingBagMI355(Float8BatchedEmbeddingBagMI355):
    """``nn.EmbeddingBag(mode="sum" | "mean")`` over ONE FP8 table, on the HIP kernel.

    ``Float8EmbeddingBagMI355(num_embeddings, embedding_dim, dtype=torch.float8_e4m3fn, mode="sum", padding_idx=None, device="cuda",
    output_dtype=None, bounds_check_mode="none", weight=None)``; ``forward(input, offsets=None, per_sample_weights=None)`` -> ``[B, D]``:
    ``input`` 1-D with ``offsets`` ``[B]`` (``include_last_offset=False``), or 2-D ``[B, L]`` with ``offsets=None``.  ``weight``: a
    ``[num_embeddings, embedding_dim]`` tensor of the float8 dtype or uint8, copied as it is.  ``from_float(m, dtype)`` casts an
    :class:`EmbeddingBagMI355` or a ``torch.nn.EmbeddingBag`` of mode sum / mean (its ``padding_idx`` carries over) with torch's
    ``.to(dtype)``.  Refusals as the batched module's; ``mode="max"`` raises ValueError."""

    def __init__(self, num_embeddings: int, embedding_dim: int, dtype=torch.float8_e4m3fn, mode="sum", padding_idx=None, device="cuda",
                 output_dtype=None, bounds_check_mode="none", weight: Optional[torch.Tensor] = None, scale=None):
        dt = float8_dtype(dtype)
        _scale_kind(scale)
        if weight is not None:
            weight = _weight_bytes(weight, dt, (int(num_embeddings), int(embedding_dim)), "weight")
        super().__init__([num_embeddings], [embedding_dim], dt, device=device, layout="bd", output_dtype=output_dtype,
                         bounds_check_mode=bounds_check_mode, pooling_mode=mode, padding_idx=padding_idx, scale=scale)
        self.num_embeddings, self.embedding_dim, self.mode = int(num_embeddings), int(embedding_dim), self.pooling_mode
        self._off2d: dict = {}
        if weight is not None:
            self._bytes(0).copy_(weight)

    _bags_2d = EmbeddingBagMI355._bags_2d

    @classmethod
    def from_float(cls, module, dtype=torch.float8_e4m3fn, scale=None, **kw):
        w = _torch_weight(module, (EmbeddingBagMI355, nn.EmbeddingBag), "an EmbeddingBagMI355 or a torch.nn.EmbeddingBag")
        dt = float8_dtype(dtype)
        kw.setdefault("mode", _pooling(module.mode, "from_float"))
        kw.setdefault("padding_idx", module.padding_idx)
        kw.setdefault("device", w.device if w.is_cuda else "cuda")
        if _scale_kind(scale) is None:
            return cls(int(w.shape[0]), int(w.shape[1]), dt, weight=w.to(dt), **kw)
        return _quantized(cls(int(w.shape[0]), int(w.shape[1]), dt, scale=scale, **kw), w)

    def forward(self, input, offsets=None, per_sample_weights=None):
        if input.dim() == 2:
            input, offsets, per_sample_weights = self._bags_2d(input, offsets, per_sample_weights)
        elif offsets is None:
            raise ValueError("offsets has to be a 1D Tensor but got None")
        return self.lookup(input, offsets, per_sample_weights, batch=offsets.numel())

    def extra_repr(self) -> str:
        return (f"{self.num_embeddings}, {self.embedding_dim}, dtype={self.dtype}, mode={self.mode}" +
                (f", padding_idx={self.padding_idx[0]}" if self.padding_idx is not None else "") +
                (f", output_dtype={self.output_dtype}" if self._out16 is not None else ""))


class Float8EmbeddingMI355(Float8BatchedEmbeddingBagMI355):
    """``nn.Embedding`` over ONE FP8 table, on the HIP kernel: the un-pooled sibling of :class:`Float8EmbeddingBagMI355`.

    ``Float8EmbeddingMI355(num_embeddings, embedding_dim, dtype=torch.float8_e4m3fn, device="cuda", output_dtype=None,
    bounds_check_mode="none", weight=None)``; ``forward(input)`` takes an int32 / int64 tensor of any shape and returns
    ``[*input.shape, D]`` in ``output_dtype``: the stored value of every element of row ``input[...]``, exactly, moved by ONE launch
    (``pm_embedding_gather_f8``: one table, one bag, ``offsets = [0]``).  An empty input returns an empty result without a launch.
    ``from_float(m, dtype)`` casts a ``torch.nn.Embedding`` or an :class:`EmbeddingMI355` with torch's ``.to(dtype)``; its
    ``padding_idx`` changes nothing here (a forward returns the padding row as stored), ``max_norm`` raises ValueError."""

    def __init__(self, num_embeddings: int, embedding_dim: int, dtype=torch.float8_e4m3fn, device="cuda", output_dtype=None,
                 bounds_check_mode="none", weight: Optional[torch.Tensor] = None, scale=None):
        dt = float8_dtype(dtype)
        _scale_kind(scale)
        if weight is not None:
            weight = _weight_bytes(weight, dt, (int(num_embeddings), int(embedding_dim)), "weight")
        super().__init__([num_embeddings], [embedding_dim], dt, device=device, layout="bd", output_dtype=output_dtype,
                         bounds_check_mode=bounds_check_mode, scale=scale)
        self.num_embeddings, self.embedding_dim = int(num_embeddings), int(embedding_dim)
        self._off0: dict = {}        # the request's offsets [0], one per (dtype, device)
        if weight is not None:
            self._bytes(0).copy_(weight)

    _offsets0 = EmbeddingMI355._offsets0

    @classmethod
    def from_float(cls, module, dtype=torch.float8_e4m3fn, scale=None, **kw):
        w = _torch_weight(module, (EmbeddingMI355, nn.Embedding), "an EmbeddingMI355 or a torch.nn.Embedding")
        dt = float8_dtype(dtype)
        kw.setdefault("device", w.device if w.is_cuda else "cuda")
        if _scale_kind(scale) is None:
            return cls(int(w.shape[0]), int(w.shape[1]), dt, weight=w.to(dt), **kw)
        return _quantized(cls(int(w.shape[0]), int(w.shape[1]), dt, scale=scale, **kw), w)

    def _flat(self, input) -> torch.Tensor:
        if not isinstance(input, torch.Tensor) or input.dtype not in _IDTYPE:
            raise TypeError(f"Float8EmbeddingMI355: input must be an int32 or int64 tensor, got {getattr(input, 'dtype', type(input))}")
        _require_device(self.weights, "Float8EmbeddingMI355.weights")
        _require_device(input, "input")
        return input.reshape(-1).contiguous()

    def forward(self, input):
        indices = self._flat(input)
        if not indices.numel():
            return torch.empty((*input.shape, self.embedding_dim), dtype=self.output_dtype, device=self.weights.device)
        return self.lookup_sequence(indices, self._offsets0(indices), batch=1).view(*input.shape, self.embedding_dim)

    def sanitize_(self, input, mode=None) -> None:
        """The sanitiser on its own: repairs ``input`` in place (it must be contiguous), stream-ordered."""
        if not input.is_contiguous():
            raise ValueError("sanitize_ needs a contiguous input (it is repaired in place)")
        indices = self._flat(input)
        if indices.numel():
            super().sanitize_(indices, self._offsets0(indices), batch=1, mode=mode)

    def extra_repr(self) -> str:
        return f"{self.num_embeddings}, {self.embedding_dim}, dtype={self.dtype}" + (f", output_dtype={self.output_dtype}" if self._out16 is not None else "")
