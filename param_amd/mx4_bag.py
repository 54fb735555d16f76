"""Pooled and un-pooled lookups over OCP Microscaling FP4 (MXFP4) embedding tables, and the quantiser that writes them
(``csrc/embbag_fwd_mx4.hip`` through ``pm_embbag_fwd_mx4``, ``csrc/embedding_gather_mx4.hip`` through ``pm_embedding_gather_mx4``,
``csrc/mx4_quantize.hip`` through ``pm_rows_quantize_mx4``).

:class:`MX4BatchedEmbeddingBagMI355` -- T tables whose rows hold ``e2m1`` codes (two columns per byte, column ``c`` in byte ``c / 2`` at
bit ``4 * (c % 2)``: ``torch.float4_e2m1fn_x2``'s order) followed by one ``E8M0`` scale byte per block of 32 columns
(``torch.float8_e8m0fnu``), zero-padded to a multiple of 8 bytes: 72 bytes at D = 128.  The serving-side sibling of
:class:`Float8BatchedEmbeddingBagMI355`; what fbgemm's int-nbit TBE carries as its MX4 type.

The arithmetic is fixed (include/param_amd.h, "MXFP4 TABLES"): the stored value of a column is ``e2m1(code) * 2^(x - 127)`` with its
block's scale byte ``x`` in [2, 252] -- exact and normal in fp32 -- or NaN for ``x == 255``; from there the rule is the FP8 lookup's: fp32
additions in index order from +0.0 (one fmaf per lookup when weighted), one correctly rounded division for the mean, one rounding for a
16-bit ``output_dtype``.  The quantiser is the OCP MX v1.0 conversion with the scale clamped into that range.

Forward only: the tables are a buffer, nothing requires grad.  There is no CPU path.  Left out, on purpose: ``padding_idx``, max pooling,
pruning, membership in the mixed-format launch, MXFP6 / MXFP8, NVFP4-style fp8 scales, the single-table ``nn.EmbeddingBag`` /
``nn.Embedding`` wrappers, MX4 in the quantised all-to-all, the operator plug-in, any backward.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch
import torch.nn as nn

from . import _lib
from .embedding_bag import (_WDTYPE, BatchedEmbeddingBagMI355, _BoundsChecked, _check_rows_out, _require_device, _stream_ptr,
                            bounds_check_mode_name)
from .float8_bag import _SRC, _pooling
from .quantized_bag import _QTableSet

MAX_DIM = 2048      # kMx4MaxDim (csrc/launch_plan.h)
BLOCK = 32          # columns that share a scale byte
SCALE_MIN, SCALE_MAX, SCALE_NAN = 2, 252, 255      # the scale bytes of the contract
_CODE_DTYPES = (torch.uint8,) + ((torch.float4_e2m1fn_x2,) if hasattr(torch, "float4_e2m1fn_x2") else ())
_SCALE_DTYPES = (torch.uint8,) + ((torch.float8_e8m0fnu,) if hasattr(torch, "float8_e8m0fnu") else ())


def row_bytes(dim: int) -> int:
    """bytes of one stored row of ``dim`` columns: ``dim / 2`` code bytes and ``dim / 32`` scale bytes, rounded up to 8"""
    return (dim // 2 + dim // BLOCK + 7) // 8 * 8


def _check_spec(dims: Sequence[int], layout: str) -> None:
    if layout == "blocked":
        raise ValueError('MXFP4 tables do not take layout="blocked"')
    if layout not in ("bd", "tbd"):
        raise ValueError(f'layout must be "bd" or "tbd", got {layout!r}')
    for d in dims:
        if d < BLOCK or d % BLOCK or d > MAX_DIM:
            raise ValueError(f"embedding dim {d}: an MXFP4 table needs a multiple of {BLOCK} in [{BLOCK}, {MAX_DIM}]")
    if layout == "tbd" and len(set(dims)) != 1:
        raise ValueError('layout "tbd" needs one common embedding dim')


class MX4BatchedEmbeddingBagMI355(nn.Module, _BoundsChecked):
    """T MXFP4 embedding tables in one HBM slab, pooled by ONE kernel launch that reads the stored bytes.

    ``MX4BatchedEmbeddingBagMI355(rows, dims, device="cuda", layout="bd", output_dtype=None, bounds_check_mode="none",
    pooling_mode="sum")``: ``dims`` multiples of 32, at most 2048, and may differ per table with ``layout="bd"`` (lane groups are sized for
    the widest table).  The tables live in ONE uint8 buffer ``weights`` (table starts padded to 256 B; ``state_dict`` round-trips it):
    zero codes under scale bytes of 127, so every element starts as +0.0 (all-zero bytes would be outside the scale contract).
    ``table(t)`` is the uint8 ``[rows_t, row_bytes(D_t)]`` view.  ``quantize_from_(t, tensor)`` fills table ``t`` from an fp32 / bf16 /
    fp16 tensor on the device with the HIP quantiser (rows may be strided); ``copy_from_(t, codes, scales)`` packs prepacked codes
    (``[rows_t, D_t / 2]``, uint8 or ``torch.float4_e2m1fn_x2``) and scales (``[rows_t, D_t / 32]``, uint8 or ``torch.float8_e8m0fnu``)
    into rows and checks the scale range once; ``dequantized_table(t)`` is the fp32 table (the un-pooled lookup of every row);
    ``from_float(source, **kw)`` quantises a :class:`BatchedEmbeddingBagMI355` or a list of float tensors.

    ``lookup(indices, offsets, per_sample_weights=None, out=None, bag_begin=0, bag_count=None, batch=None)`` -- and ``forward``, the same
    call -- takes the TBE request of :class:`BatchedEmbeddingBagMI355` and returns ``[B, sum D]`` (``"bd"``) or ``[T, B, D]`` (``"tbd"``) in
    ``output_dtype``.  ``pooling_mode`` ``"sum"`` / ``"mean"``.  ``plan(...)`` is the launch geometry of the same request
    (``pm_embbag_mx4_plan``).  ``lookup_sequence(indices, offsets, batch=None, out=None, bag_begin=0, bag_count=None)`` is the UN-POOLED
    lookup: ``[N, D]``, the stored value of every looked-up element (one common embedding dim); ``sequence_plan(...)`` its geometry.
    ``bounds_check_mode`` and ``sanitize_``: see :class:`_BoundsChecked`.

    No parameters; the output never requires grad.  ValueError before anything is allocated: dims that are not multiples of 32 or above
    2048, ``layout="blocked"``, max / none pooling, ``rows >= 2^31``; a weighted mean lookup raises ValueError at the call.  Tensors that
    are not on a ROCm device raise RuntimeError (no CPU fallback), floating-point indices TypeError.
    """

    _TABLES = "weights"
    padding_idx = None

    def __init__(self, rows: Sequence[int], dims, device="cuda", layout: str = "bd", output_dtype=None, bounds_check_mode="none",
                 pooling_mode="sum"):
        super().__init__()
        self._init_shared(bounds_check_mode, output_dtype)
        rows = [int(r) for r in rows]
        dims = [int(dims)] * len(rows) if isinstance(dims, int) else [int(d) for d in dims]
        if len(rows) != len(dims) or not rows:
            raise ValueError("rows and dims must name the same tables, at least one")
        _check_spec(dims, layout)
        self.pooling_mode = _pooling(pooling_mode, type(self).__name__)
        self._mean = self.pooling_mode == "mean"
        if any(r < 1 or r >= 2**31 for r in rows):
            raise ValueError("every table needs 1 <= rows < 2^31")
        self.rows, self.dims, self.layout = rows, dims, layout
        self.row_bytes = [row_bytes(d) for d in dims]
        # table starts padded to 256 B: every row is 8-byte aligned
        starts, cur = [], 0
        for r, rb in zip(rows, self.row_bytes):
            starts.append(cur)
            cur += (r * rb + 255) // 256 * 256
        self._starts = starts
        self.register_buffer("weights", torch.zeros(cur, dtype=torch.uint8, device=device))
        for t, d in enumerate(dims):
            self.table(t)[:, d // 2:d // 2 + d // BLOCK] = 127
        self._ts: Optional[_QTableSet] = None

    # -- tables ------------------------------------------------------------------------------
    def table(self, t: int) -> torch.Tensor:
        """table ``t``: the uint8 ``[rows_t, row_bytes(D_t)]`` view of the buffer"""
        s, n = self._starts[t], self.rows[t] * self.row_bytes[t]
        return self.weights[s:s + n].view(self.rows[t], self.row_bytes[t])

    def copy_from_(self, t: int, codes: torch.Tensor, scales: torch.Tensor) -> None:
        """fill table ``t`` from prepacked ``codes`` ``[rows_t, D_t / 2]`` (uint8 or ``torch.float4_e2m1fn_x2``: the same bytes) and
        ``scales`` ``[rows_t, D_t / 32]`` (uint8 or ``torch.float8_e8m0fnu``).  The scale bytes must lie in [2, 252] or be 255 (a NaN
        block) -- checked here, once, with torch ops (one synchronisation)."""
        r, d = self.rows[t], self.dims[t]
        for x, kinds, shape, what in ((codes, _CODE_DTYPES, (r, d // 2), "codes"), (scales, _SCALE_DTYPES, (r, d // BLOCK), "scales")):
            if not isinstance(x, torch.Tensor) or x.dtype not in kinds or tuple(x.shape) != shape:
                raise ValueError(f"copy_from_: table {t} needs {what} of shape {shape} and dtype {' / '.join(str(k).replace('torch.', '') for k in kinds)}, "
                                 f"got {getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
        s = scales.detach().contiguous().view(torch.uint8)
        if s.numel() and bool((((s < SCALE_MIN) | (s > SCALE_MAX)) & (s != SCALE_NAN)).any()):
            raise ValueError(f"copy_from_: scale bytes must lie in [{SCALE_MIN}, {SCALE_MAX}] or be {SCALE_NAN} (a NaN block)")
        tab = self.table(t)
        tab[:, :d // 2].copy_(codes.detach().contiguous().view(torch.uint8))
        tab[:, d // 2:d // 2 + d // BLOCK].copy_(s)
        tab[:, d // 2 + d // BLOCK:] = 0

    def quantize_from_(self, t: int, tensor: torch.Tensor) -> None:
        """fill table ``t`` from a ``[rows_t, D_t]`` fp32 / bf16 / fp16 tensor on the module's ROCm device with the HIP quantiser
        (``pm_rows_quantize_mx4``: one launch, the source is read once).  Rows may be strided (``tensor[:, a:b]`` of a wider tensor)."""
        if not isinstance(tensor, torch.Tensor) or tensor.dtype not in _SRC or tuple(tensor.shape) != (self.rows[t], self.dims[t]):
            raise ValueError(f"quantize_from_: table {t} needs a float32 / bfloat16 / float16 tensor of shape {(self.rows[t], self.dims[t])}, got "
                             f"{getattr(tensor, 'dtype', type(tensor).__name__)} {tuple(getattr(tensor, 'shape', ()))}")
        _require_device(self.weights, f"{type(self).__name__}.weights")
        _require_device(tensor, "tensor")
        src = tensor.detach()
        if src.stride(1) != 1 or src.stride(0) < src.shape[1] or (src.stride(0) * src.element_size()) % 16 or src.data_ptr() % 16:
            src = src.contiguous()
        _lib.check(_lib.load().pm_rows_quantize_mx4(src.data_ptr(), _SRC[src.dtype], self.rows[t], self.dims[t], src.stride(0),
                                                    self.table(t).data_ptr(), _stream_ptr()))

    def dequantized_table(self, t: int) -> torch.Tensor:
        """table ``t`` as fp32 ``[rows_t, D_t]``: the un-pooled lookup of rows 0 .. rows_t - 1 (``pm_embedding_gather_mx4``)"""
        _require_device(self.weights, f"{type(self).__name__}.weights")
        dev = self.weights.device
        ts = _QTableSet([self.table(t)], [self.dims[t]], "bd")
        idx = torch.arange(self.rows[t], dtype=torch.int64, device=dev)
        off = torch.zeros(1, dtype=torch.int64, device=dev)
        op = _lib.pm_embbag_batch.from_buffer_copy(ts.request(idx, off, 1, None, 0, None, forward=True))
        op.weight_dtype = _lib.PM_MX4
        out = torch.empty((self.rows[t], self.dims[t]), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().pm_embedding_gather_mx4(ctypes.byref(op), _lib.PM_F32, out.data_ptr(), self.dims[t], _stream_ptr()))
        return out

    @classmethod
    def from_float(cls, source, **kw):
        """quantise a :class:`BatchedEmbeddingBagMI355` (sum or mean pooling; its ``layout`` and ``pooling_mode`` carry over) or a sequence
        of 2-D floating-point tensors with the HIP quantiser on the module's device; keywords go to the constructor (``device`` defaults to
        the source's)"""
        if isinstance(source, BatchedEmbeddingBagMI355):
            if source.padding_idx is not None:
                raise ValueError("from_float: MXFP4 tables have no padding_idx")
            kw.setdefault("pooling_mode", _pooling(source.pooling_mode, "from_float"))
            kw.setdefault("layout", source.layout)
            tables = [source.table(t) for t in range(len(source.rows))]
        else:
            tables = list(source)
            if not tables or any(not isinstance(x, torch.Tensor) or x.dim() != 2 or not x.dtype.is_floating_point for x in tables):
                raise TypeError("from_float takes a BatchedEmbeddingBagMI355 or a sequence of 2-D floating-point tensors")
        kw.setdefault("device", tables[0].device)
        m = cls([int(x.shape[0]) for x in tables], [int(x.shape[1]) for x in tables], **kw)
        for t, x in enumerate(tables):
            x = x.detach().to(m.weights.device)
            m.quantize_from_(t, x if x.dtype in _SRC else x.to(torch.float32))
        return m

    def _tables(self) -> _QTableSet:
        if self._ts is None or self._ts.ptrs[0] != self.table(0).data_ptr():
            self._ts = _QTableSet([self.table(t) for t in range(len(self.rows))], self.dims, self.layout)
        return self._ts

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
        # the table set's (cached) request names fp32 tables -- what the sanitiser is handed --; the MXFP4 calls get a copy that names the format
        op = _lib.pm_embbag_batch.from_buffer_copy(ts.request(indices, offsets, B, per_sample_weights, bag_begin, bag_count, forward=True))
        op.weight_dtype = _lib.PM_MX4
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
        rc = _lib.load().pm_embbag_fwd_mx4(ctypes.byref(op), 1 if self._mean else 0, _WDTYPE[odt], out.data_ptr(), _stream_ptr())
        if rc:
            _lib.check(rc)
        return out

    def forward(self, indices, offsets, per_sample_weights=None, out=None, bag_begin=0, bag_count=None, batch: Optional[int] = None):
        return self.lookup(indices, offsets, per_sample_weights, out, bag_begin, bag_count, batch)

    def plan(self, indices, offsets, per_sample_weights=None, bag_begin=0, bag_count=None, batch: Optional[int] = None) -> dict:
        """the launch geometry ``lookup`` would use for this request under the knobs as they stand (``_lib.PLAN_FIELDS`` by name;
        ``pm_embbag_mx4_plan``, nothing is launched)"""
        _, _, op = self._request(indices, offsets, per_sample_weights, bag_begin, bag_count, batch, False)
        return _lib.embbag_mx4_plan(op, _WDTYPE[self.output_dtype])

    # -- un-pooled ---------------------------------------------------------------------------
    def _sequence_request(self, indices, offsets, batch, bag_begin, bag_count, sanitize: bool, out=None):
        if len(set(self.dims)) != 1:
            raise ValueError("lookup_sequence needs one common embedding dim")
        if out is not None:
            _check_rows_out(out, indices.numel(), self.dims[0], self.output_dtype, self.weights.device)
        return self._request(indices, offsets, None, bag_begin, bag_count, batch, sanitize)

    def lookup_sequence(self, indices, offsets, batch: Optional[int] = None, out=None, bag_begin=0, bag_count=None):
        """The UN-POOLED forward over the module's T tables: ``[N, D]`` in ``output_dtype``, ``N = indices.numel()``, row ``j`` = row
        ``indices[j]`` of the table that owns lookup position ``j`` (table ``t`` owns ``[offsets[t * B], offsets[(t + 1) * B])``), every
        element the stored value -- one launch, ``pm_embedding_gather_mx4``.  Runs after ``bounds_check_mode``, like ``lookup``.
        ``bag_begin/bag_count`` select a batch slice: only the rows of lookups inside it are written -- a caller's ``out`` keeps every
        other row, a tensor allocated here holds zeros there."""
        ts, B, op = self._sequence_request(indices, offsets, batch, bag_begin, bag_count, True, out)
        n, D, odt = indices.numel(), self.dims[0], self.output_dtype
        if out is None:
            whole = bag_begin == 0 and bag_count in (None, B)
            out = (torch.empty if whole else torch.zeros)((n, D), dtype=odt, device=ts.device)
        if n:
            rc = _lib.load().pm_embedding_gather_mx4(ctypes.byref(op), _WDTYPE[odt], out.data_ptr(), D, _stream_ptr())
            if rc:
                _lib.check(rc)
        return out

    def sequence_plan(self, indices, offsets, batch: Optional[int] = None, bag_begin=0, bag_count=None) -> dict:
        """the launch geometry ``lookup_sequence`` would use (``_lib.GATHER_PLAN_FIELDS`` by name; ``pm_embedding_gather_mx4_plan``)"""
        _, _, op = self._sequence_request(indices, offsets, batch, bag_begin, bag_count, False)
        return _lib.embedding_gather_mx4_plan(op)

    def sanitize_(self, indices, offsets, batch: Optional[int] = None, mode=None) -> None:
        """The sanitiser on its own (see :class:`BatchedEmbeddingBagMI355`)."""
        _require_device(self.weights, f"{type(self).__name__}.weights")
        B = self._batch_of(offsets, indices) if batch is None else batch
        mode = bounds_check_mode_name(mode) if mode is not None else self.bounds_check_mode
        self._sanitize(self._tables(), indices, offsets, B, "warning" if mode == "none" else mode)

    def extra_repr(self) -> str:
        return (f"rows={self.rows}, dims={self.dims}, layout={self.layout}, pooling_mode={self.pooling_mode}" +
                (f", output_dtype={self.output_dtype}" if self._out16 is not None else ""))
