"""Pooled and un-pooled lookups over embedding tables that are EACH stored in their own format -- fp32, bf16, fp16, OCP FP8 e4m3fn /
e5m2 (with a power-of-two table exponent), 8- or 4-bit quantised rows -- in ONE launch (``csrc/embbag_fwd_anyfmt_kernel.inc`` through
``pm_embbag_fwd_anyfmt``, ``csrc/embedding_gather_anyfmt.hip`` through ``pm_embedding_gather_anyfmt``).

* :class:`MixedBatchedEmbeddingBagMI355` -- T tables, one format per table (fbgemm's ``IntNBitTableBatchedEmbeddingBagsCodegen`` takes
  one ``SparseType`` per table for the same reason: a serving model keeps its huge tables at 4 bits or FP8, the mid-size ones at 8 bits
  and the small or sensitive ones at fp16 or fp32).  Without it such a model is up to three modules -- :class:`BatchedEmbeddingBagMI355`,
  :class:`QuantizedBatchedEmbeddingBagMI355`, :class:`Float8BatchedEmbeddingBagMI355` --, three launches and the strided copies that
  put their results into one ``[B, sum D]`` output.

NO NEW ARITHMETIC (include/param_amd.h, "MIXED-FORMAT TABLES"): the columns of table ``t`` are bit for bit what that format's own
module gives for the same bytes -- fp32 additions in index order from +0.0 (one fmaf per lookup when weighted) for the float and FP8
formats, an FP8 element being ``dec(code) * 2^E_t``; ``fmaf(scale * w, code, acc + bias * w)`` for quantised rows; one rounding for a
16-bit ``output_dtype``.  The un-pooled lookup returns a 16-bit row to the same 16-bit ``output_dtype`` as stored bits.

Forward only: the tables are a buffer, nothing requires grad.  There is no CPU path.  Left out, on purpose: FP8 row exponents, pruning /
``index_remapping``, mean pooling, ``padding_idx``, max pooling, 2-bit rows, a lane-group width per format, any backward, the operator
plug-in.  No existing module is rerouted to this kernel.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch
import torch.nn as nn

from . import _lib, quant
from .embedding_bag import _WDTYPE, BatchedEmbeddingBagMI355, _BoundsChecked, _check_rows_out, _require_device, _stream_ptr, bounds_check_mode_name
from .float8_bag import _F8, _SRC, EXP_MAX, EXP_MIN, Float8BatchedEmbeddingBagMI355, _pow2
from .quantized_bag import QuantizedBatchedEmbeddingBagMI355, _QTableSet

MAX_DIM = 2048      # kAnyfmtMaxDim (csrc/launch_plan.h)
FORMATS = ("fp32", "bf16", "fp16", "fp8_e4m3", "fp8_e5m2", "int8", "int4")
_CODE = {"fp32": _lib.PM_F32, "bf16": _lib.PM_BF16, "fp16": _lib.PM_F16, "fp8_e4m3": _lib.PM_F8E4M3, "fp8_e5m2": _lib.PM_F8E5M2,
         "int8": _lib.PM_Q8, "int4": _lib.PM_Q4}
_TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16, "fp8_e4m3": torch.float8_e4m3fn,
          "fp8_e5m2": torch.float8_e5m2, "int8": torch.int8}
_BY_DTYPE = {v: k for k, v in _TORCH.items()}
_ALIASES = {"fp8": "fp8_e4m3"}      # fbgemm's SparseType.FP8 is e4m3
_BITS = {"int8": 8, "int4": 4}
_COLUMN_RULE = {"fp8_e4m3": 16, "fp8_e5m2": 16}      # the format's own column rule where it is stricter than a lane's eight columns


def table_format(spec) -> str:
    """one of :data:`FORMATS` from its name in any case, the matching torch dtype (``torch.int8`` is ``"int8"``; 4-bit rows have no torch
    dtype), or an enum member read by ``value`` or ``name`` (fbgemm's ``SparseType``; its ``FP8`` is e4m3).  Anything else raises ValueError."""
    if isinstance(spec, torch.dtype):
        if spec in _BY_DTYPE:
            return _BY_DTYPE[spec]
    else:
        for key in (spec, getattr(spec, "value", None), getattr(spec, "name", None)):
            if isinstance(key, str):
                key = _ALIASES.get(key.lower(), key.lower())
                if key in _CODE:
                    return key
    raise ValueError(f"a table format must be one of {' / '.join(FORMATS)} (any case), the matching torch dtype or an enum member of that "
                     f"value or name (fbgemm's SparseType), got {spec!r} (2-bit rows and the fnuz FP8 formats are not implemented)")


def _row_bytes(fmt: str, dim: int) -> int:
    if fmt in _BITS:
        return quant.host_row_bytes(dim, _BITS[fmt])
    return dim * (4 if fmt == "fp32" else 2 if fmt in ("bf16", "fp16") else 1)


class MixedBatchedEmbeddingBagMI355(nn.Module, _BoundsChecked):
    """T embedding tables, EACH in its own stored format, in one HBM slab, pooled (sum, optionally weighted) by ONE kernel launch.

    ``MixedBatchedEmbeddingBagMI355(rows, dims, formats, device="cuda", layout="bd", output_dtype=None, bounds_check_mode="none")``:
    ``formats`` has one entry per table (see :func:`table_format`): ``"fp32" | "bf16" | "fp16" | "fp8_e4m3" | "fp8_e5m2" | "int8" |
    "int4"`` in any case, the matching torch dtype, or an enum member read by name.  ``dims`` are multiples of 8 (a lane holds eight
    columns of a row whatever its format), of 16 for an FP8 table, at most 2048, and may differ per table with ``layout="bd"``.
    The tables live in ONE zero-filled uint8 buffer ``weights`` (table starts padded to 256 B) next to the int32 ``[T]`` buffer
    ``table_exponents`` (zeros; read for FP8 tables only); ``state_dict`` round-trips both.  ``formats`` is the list of names,
    ``format_codes`` the C call's codes.

    ``table(t)`` is the typed view: ``[rows_t, D_t]`` of the float or float8 dtype, uint8 ``[rows_t, row_bytes]`` for quantised rows.
    ``copy_from_(t, tensor, exponent=0)`` is a bit copy of a tensor of that view's dtype and shape (FP8 also takes uint8 codes);
    ``exponent`` sets an FP8 table's ``E_t`` in [-64, 64].  ``quantize_from_(t, fp)`` runs the format's own quantiser -- ``quantize_rows``
    for int8 / int4, the scaled-FP8 quantiser with ``scale="table"`` semantics for FP8, a cast for the float formats --,
    ``dequantized_table(t)`` is the fp32 table, and ``from_modules(modules)`` concatenates the tables of existing modules by copying
    their bytes.

    ``lookup`` / ``forward(indices, offsets, per_sample_weights=None, out=None, bag_begin=0, bag_count=None, batch=None)`` takes the TBE
    request of :class:`BatchedEmbeddingBagMI355` and returns ``[B, sum D]`` (``"bd"``) or ``[T, B, D]`` (``"tbd"``) in ``output_dtype``;
    ``lookup_sequence(indices, offsets, batch=None, out=None, bag_begin=0, bag_count=None)`` is the un-pooled lookup ``[N, D]`` (one
    common dim); ``plan`` / ``sequence_plan`` their launch geometry (no formats enter it); ``bounds_check_mode`` and ``sanitize_``: see
    :class:`_BoundsChecked`.  No parameters; the output never requires grad.

    ValueError before anything is allocated: a wrong length of ``formats`` or an unknown format, a dim that is not a multiple of 8 or
    breaks its format's own rule, a dim above 2048, ``rows >= 2^31``, ``layout="blocked"``.  At call time tensors that are not on a ROCm
    device raise RuntimeError (no CPU fallback), floating-point indices TypeError.
    """

    def __init__(self, rows: Sequence[int], dims, formats, device="cuda", layout: str = "bd", output_dtype=None, bounds_check_mode="none"):
        super().__init__()
        self._init_shared(bounds_check_mode, output_dtype)
        rows = [int(r) for r in rows]
        dims = [int(dims)] * len(rows) if isinstance(dims, int) else [int(d) for d in dims]
        if len(rows) != len(dims) or not rows:
            raise ValueError("rows and dims must name the same tables, at least one")
        if isinstance(formats, (str, bytes, torch.dtype)) or not isinstance(formats, Sequence):
            raise ValueError(f"formats must be a sequence of one format per table, got {formats!r}")
        if len(formats) != len(rows):
            raise ValueError(f"formats names {len(formats)} tables, rows and dims name {len(rows)}: one entry per table")
        formats = [table_format(f) for f in formats]
        if layout == "blocked":
            raise ValueError('mixed-format tables do not take layout="blocked"')
        if layout not in ("bd", "tbd"):
            raise ValueError(f'layout must be "bd" or "tbd", got {layout!r}')
        for d, f in zip(dims, formats):
            mult = _COLUMN_RULE.get(f, 8)
            if d < mult or d % mult or d > MAX_DIM:
                raise ValueError(f"embedding dim {d}: a{'n' if f in _COLUMN_RULE else ''} {f} table of a mixed-format module needs a multiple of "
                                 f"{mult} in [{mult}, {MAX_DIM}]")
        if layout == "tbd" and len(set(dims)) != 1:
            raise ValueError('layout "tbd" needs one common embedding dim')
        if any(r < 1 or r >= 2**31 for r in rows):
            raise ValueError("every table needs 1 <= rows < 2^31")
        self.padding_idx = None
        self.rows, self.dims, self.formats, self.layout = rows, dims, formats, layout
        self.format_codes = [_CODE[f] for f in formats]
        self._row_bytes = [_row_bytes(f, d) for f, d in zip(formats, dims)]
        # table starts padded to 256 B: float and FP8 rows stay 16-byte aligned, quantised rows 4-byte aligned
        starts, cur = [], 0
        for r, rb in zip(rows, self._row_bytes):
            starts.append(cur)
            cur += (r * rb + 255) // 256 * 256
        self._starts = starts
        self.register_buffer("weights", torch.zeros(cur, dtype=torch.uint8, device=device))
        self.register_buffer("table_exponents", torch.zeros(len(rows), dtype=torch.int32, device=device))
        self._ts: Optional[_QTableSet] = None

    _TABLES = "weights"

    # -- tables ------------------------------------------------------------------------------
    def _bytes(self, t: int) -> torch.Tensor:
        """table ``t`` as uint8 ``[rows_t, row_bytes_t]``"""
        s, n = self._starts[t], self.rows[t] * self._row_bytes[t]
        return self.weights[s:s + n].view(self.rows[t], self._row_bytes[t])

    def table(self, t: int) -> torch.Tensor:
        """table ``t``: ``[rows_t, D_t]`` of the float / float8 dtype, or the uint8 ``[rows_t, row_bytes]`` quantised rows"""
        f = self.formats[t]
        return self._bytes(t) if f in _BITS else self._bytes(t).view(_TORCH[f])

    def _set_exponent(self, t: int, exponent) -> None:
        if isinstance(exponent, bool) or not isinstance(exponent, int) or not EXP_MIN <= exponent <= EXP_MAX:
            raise ValueError(f"exponent must be an int in [{EXP_MIN}, {EXP_MAX}], got {exponent!r}")
        if exponent != 0 and not self.formats[t].startswith("fp8"):
            raise ValueError(f"exponent is for FP8 tables only; table {t} is {self.formats[t]}")
        if self.formats[t].startswith("fp8"):
            self.table_exponents[t] = exponent

    def copy_from_(self, t: int, tensor: torch.Tensor, exponent: int = 0) -> None:
        """fill table ``t`` from a tensor of ``table(t)``'s dtype and shape (an FP8 table also takes uint8 codes): a bit copy.
        ``exponent``: an FP8 table's ``E_t``, an int in [-64, 64] (checked; anything but 0 for another format raises ValueError)"""
        view = self.table(t)
        ok = isinstance(tensor, torch.Tensor) and tuple(tensor.shape) == tuple(view.shape) and (
            tensor.dtype == view.dtype or (self.formats[t].startswith("fp8") and tensor.dtype == torch.uint8))
        if not ok:
            raise ValueError(f"copy_from_: table {t} ({self.formats[t]}) needs a {str(view.dtype).replace('torch.', '')} tensor of shape "
                             f"{tuple(view.shape)}, got {getattr(tensor, 'dtype', type(tensor).__name__)} {tuple(getattr(tensor, 'shape', ()))}")
        self._set_exponent(t, exponent)
        src = tensor.detach().contiguous()
        self._bytes(t).copy_(src.view(torch.uint8).view(self.rows[t], self._row_bytes[t]))

    def quantize_from_(self, t: int, source: torch.Tensor) -> None:
        """fill table ``t`` from a ``[rows_t, D_t]`` floating-point tensor with the format's own quantiser: ``quantize_rows`` (int8 / int4;
        fp32 sources, D up to 512), the scaled-FP8 quantiser with ``scale="table"`` semantics -- the smallest table exponent at which no
        finite element overflows, then torch's cast of ``x * 2^-E_t`` -- (FP8; fp32 / bf16 / fp16 sources on the module's device), or
        ``.to(dtype)`` (the float formats)"""
        f = self.formats[t]
        if not isinstance(source, torch.Tensor) or not source.dtype.is_floating_point or tuple(source.shape) != (self.rows[t], self.dims[t]):
            raise ValueError(f"quantize_from_: table {t} needs a floating-point tensor of shape {(self.rows[t], self.dims[t])}, got "
                             f"{getattr(source, 'dtype', type(source).__name__)} {tuple(getattr(source, 'shape', ()))}")
        if f in _BITS:
            if source.dtype != torch.float32:
                raise TypeError(f"quantize_from_: float32 expected for an {f} table, got {source.dtype} (widen 16-bit tables first)")
            _require_device(self.weights, f"{type(self).__name__}.weights")
            quant.quantize_rows(source.detach().contiguous(), self.dims[t], _BITS[f], out=self._bytes(t))
        elif f.startswith("fp8"):
            if source.dtype not in _SRC:
                raise TypeError(f"quantize_from_: float32 / bfloat16 / float16 expected for an {f} table, got {source.dtype}")
            _require_device(self.weights, f"{type(self).__name__}.weights")
            _require_device(source, "source")
            src = source.detach()
            if src.stride(1) != 1 or src.stride(0) < src.shape[1] or (src.stride(0) * src.element_size()) % 16 or src.data_ptr() % 16:
                src = src.contiguous()
            L, stream = _lib.load(), _stream_ptr()
            head = (src.data_ptr(), _SRC[src.dtype], self.rows[t], self.dims[t], src.stride(0), _F8[_TORCH[f]])
            rexp = torch.empty(self.rows[t], dtype=torch.int8, device=self.weights.device)
            _lib.check(L.pm_f8_row_exponents(*head, rexp.data_ptr(), stream))
            e_t = self.table_exponents[t:t + 1]
            e_t.copy_(rexp.max().to(torch.int32))
            _lib.check(L.pm_rows_quantize_f8(*head, e_t.data_ptr(), None, self._bytes(t).data_ptr(), stream))
        else:
            self.table(t).copy_(source.detach().to(_TORCH[f]))

    def dequantized_table(self, t: int) -> torch.Tensor:
        """table ``t`` as fp32: the widened elements, ``dec(code) * 2^E_t``, or ``dequantize_rows`` of the quantised rows"""
        f = self.formats[t]
        if f in _BITS:
            _require_device(self.weights, f"{type(self).__name__}.weights")
            return quant.dequantize_rows(self._bytes(t), self.dims[t], _BITS[f])
        w = self.table(t).to(torch.float32)
        return w * _pow2(self.table_exponents[t]) if f.startswith("fp8") else w

    @classmethod
    def from_modules(cls, modules, **kw):
        """one module over the tables of ``modules``, in order, their bytes (and FP8 table exponents) copied: each a
        :class:`BatchedEmbeddingBagMI355` sum module without padding, a :class:`QuantizedBatchedEmbeddingBagMI355` without pruning, or a
        :class:`Float8BatchedEmbeddingBagMI355` sum module without padding with ``scale=None | "table"``.  Keywords go to the constructor
        (``device`` and ``layout`` default to the first module's)."""
        modules = list(modules)
        if not modules:
            raise ValueError("from_modules needs at least one module")
        rows, dims, formats, sources = [], [], [], []
        for m in modules:
            if isinstance(m, Float8BatchedEmbeddingBagMI355):
                if m.pooling_mode != "sum" or m.padding_idx is not None or m.scale == "row":
                    raise ValueError('from_modules takes a Float8BatchedEmbeddingBagMI355 of sum pooling without padding_idx and with scale=None or "table"')
                fmts = [_BY_DTYPE[m.dtype]] * len(m.rows)
                exps = m.table_exponents.tolist() if m.scale == "table" else [0] * len(m.rows)
                srcs = [(m._bytes(t), int(exps[t])) for t in range(len(m.rows))]
            elif isinstance(m, QuantizedBatchedEmbeddingBagMI355):
                if m.pruned:
                    raise ValueError("from_modules does not take a pruned QuantizedBatchedEmbeddingBagMI355 (index_remapping is not implemented here)")
                fmts = ["int8" if b == 8 else "int4" for b in m.bitwidths]
                srcs = [(m.table(t), 0) for t in range(len(m.rows))]
            elif isinstance(m, BatchedEmbeddingBagMI355):
                if m.pooling_mode != "sum" or m.padding_idx is not None or m.layout == "blocked":
                    raise ValueError('from_modules takes a BatchedEmbeddingBagMI355 of sum pooling without padding_idx (layout "bd" or "tbd")')
                fmts = [_BY_DTYPE[m.weights.dtype]] * len(m.rows)
                srcs = [(m.table(t), 0) for t in range(len(m.rows))]
            else:
                raise TypeError(f"from_modules takes BatchedEmbeddingBagMI355, QuantizedBatchedEmbeddingBagMI355 and Float8BatchedEmbeddingBagMI355 "
                                f"modules, got {type(m).__name__}")
            rows += list(m.rows)
            dims += list(m.dims)
            formats += fmts
            sources += srcs
        kw.setdefault("device", modules[0].weights.device)
        kw.setdefault("layout", modules[0].layout)
        out = cls(rows, dims, formats, **kw)
        for t, (src, e) in enumerate(sources):
            src = src.detach().contiguous()
            out._bytes(t).copy_(src.view(torch.uint8).view(out.rows[t], out._row_bytes[t]))
            if e:
                out.table_exponents[t] = e
        return out

    def _tables(self) -> _QTableSet:
        if self._ts is None or self._ts.ptrs[0] != self._bytes(0).data_ptr():
            self._ts = _QTableSet([self._bytes(t) for t in range(len(self.rows))], self.dims, self.layout, self.format_codes)
        return self._ts

    _batch_of = BatchedEmbeddingBagMI355._batch_of

    # -- ops ---------------------------------------------------------------------------------
    def _request(self, indices, offsets, per_sample_weights, bag_begin, bag_count, batch, sanitize: bool):
        if indices.dtype.is_floating_point or offsets.dtype.is_floating_point:
            raise TypeError(f"indices and offsets must both be int64 or both int32, got {indices.dtype} / {offsets.dtype}")
        _require_device(self.weights, f"{type(self).__name__}.weights")
        _require_device(self.table_exponents, f"{type(self).__name__}.table_exponents")
        B = self._batch_of(offsets, indices) if batch is None else batch
        ts = self._tables()
        if sanitize and self.bounds_check_mode != "none":
            self._sanitize(ts, indices, offsets, B, self.bounds_check_mode, per_sample_weights, bag_begin, bag_count)
        return ts, B, ts.request(indices, offsets, B, per_sample_weights, bag_begin, bag_count, forward=True)

    def lookup(self, indices, offsets, per_sample_weights=None, out=None, bag_begin=0, bag_count=None, batch: Optional[int] = None):
        """The pooled forward; ``bag_begin/bag_count`` select a batch slice (bags outside it keep what ``out`` held)."""
        ts, B, op = self._request(indices, offsets, per_sample_weights, bag_begin, bag_count, batch, True)
        _, _, shape = ts.out_desc(B)
        odt = self.output_dtype
        if out is None:
            out = torch.empty(shape, dtype=odt, device=ts.device)
        elif out.dtype != odt or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != ts.device:
            raise ValueError(f"out must be a contiguous {str(odt).replace('torch.', '')} tensor of shape {shape} on {ts.device}")
        rc = _lib.load().pm_embbag_fwd_anyfmt(ctypes.byref(op), ts.d_bits.data_ptr(), self.table_exponents.data_ptr(), _WDTYPE[odt],
                                              out.data_ptr(), _stream_ptr())
        if rc:
            _lib.check(rc)
        return out

    def forward(self, indices, offsets, per_sample_weights=None, out=None, bag_begin=0, bag_count=None, batch: Optional[int] = None):
        return self.lookup(indices, offsets, per_sample_weights, out, bag_begin, bag_count, batch)

    def plan(self, indices, offsets, per_sample_weights=None, bag_begin=0, bag_count=None, batch: Optional[int] = None) -> dict:
        """the launch geometry ``lookup`` would use for this request under the knobs as they stand (``_lib.PLAN_FIELDS`` by name;
        ``pm_embbag_anyfmt_plan``, nothing is launched; ``unroll`` is 0: the rows in flight are a compile-time value per format)"""
        _, _, op = self._request(indices, offsets, per_sample_weights, bag_begin, bag_count, batch, False)
        return _lib.embbag_anyfmt_plan(op, _WDTYPE[self.output_dtype])

    # -- un-pooled ---------------------------------------------------------------------------
    def _sequence_request(self, indices, offsets, batch, bag_begin, bag_count, sanitize: bool, out=None):
        if len(set(self.dims)) != 1:
            raise ValueError("lookup_sequence needs one common embedding dim (mixed dims are served by pm_embedding_gather_anyfmt, the C call)")
        if out is not None:
            _check_rows_out(out, indices.numel(), self.dims[0], self.output_dtype, self.weights.device)
        return self._request(indices, offsets, None, bag_begin, bag_count, batch, sanitize)

    def lookup_sequence(self, indices, offsets, batch: Optional[int] = None, out=None, bag_begin=0, bag_count=None):
        """The UN-POOLED forward over the module's T tables: ``[N, D]`` in ``output_dtype``, ``N = indices.numel()``, row ``j`` = row
        ``indices[j]`` of the table that owns lookup position ``j`` (table ``t`` owns ``[offsets[t * B], offsets[(t + 1) * B])``), by the
        un-pooled rule of that table's format -- one launch, ``pm_embedding_gather_anyfmt``.  Runs after ``bounds_check_mode``, like
        ``lookup``.  ``bag_begin/bag_count`` select a batch slice: only the rows of lookups inside it are written -- a caller's ``out``
        keeps every other row, a tensor allocated here holds zeros there."""
        ts, B, op = self._sequence_request(indices, offsets, batch, bag_begin, bag_count, True, out)
        n, D, odt = indices.numel(), self.dims[0], self.output_dtype
        if out is None:
            whole = bag_begin == 0 and bag_count in (None, B)
            out = (torch.empty if whole else torch.zeros)((n, D), dtype=odt, device=ts.device)
        if n:
            rc = _lib.load().pm_embedding_gather_anyfmt(ctypes.byref(op), ts.d_bits.data_ptr(), self.table_exponents.data_ptr(), _WDTYPE[odt],
                                                        out.data_ptr(), D, _stream_ptr())
            if rc:
                _lib.check(rc)
        return out

    def sequence_plan(self, indices, offsets, batch: Optional[int] = None, bag_begin=0, bag_count=None) -> dict:
        """the launch geometry ``lookup_sequence`` would use (``_lib.GATHER_PLAN_FIELDS`` by name; ``pm_embedding_gather_anyfmt_plan``)"""
        _, _, op = self._sequence_request(indices, offsets, batch, bag_begin, bag_count, False)
        return _lib.embedding_gather_anyfmt_plan(op)

    def sanitize_(self, indices, offsets, batch: Optional[int] = None, mode=None) -> None:
        """The sanitiser on its own (see :class:`BatchedEmbeddingBagMI355`)."""
        _require_device(self.weights, f"{type(self).__name__}.weights")
        B = self._batch_of(offsets, indices) if batch is None else batch
        mode = bounds_check_mode_name(mode) if mode is not None else self.bounds_check_mode
        self._sanitize(self._tables(), indices, offsets, B, "warning" if mode == "none" else mode)

    def extra_repr(self) -> str:
        return (f"rows={self.rows}, dims={self.dims}, formats={self.formats}, layout={self.layout}" +
                (f", output_dtype={self.output_dtype}" if self._out16 is not None else ""))
