"""Pooled and un-pooled lookups over 8- and 4-bit ROW-QUANTISED embedding tables (``csrc/embbag_fwd_qrows.hip`` through
``pm_embbag_fwd_qrows``, ``csrc/embedding_gather_qrows.hip`` through ``pm_embedding_gather_qrows``; tables of PER-TABLE format in one
launch: ``csrc/embbag_fwd_qmixed.hip`` / ``csrc/embedding_gather_qmixed.hip`` through ``pm_embbag_fwd_qrows_mixed`` /
``pm_embedding_gather_qrows_mixed``).

* :class:`QuantizedBatchedEmbeddingBagMI355` -- T tables stored as the bytes ``quantize_rows`` writes (torch's
  ``quantized::embedding_bag_{byte,4bit}_prepack`` layout), pooled by ONE launch that reads those bytes: no fp32 copy of a table exists.
  The serving-side sibling of :class:`BatchedEmbeddingBagMI355`; what fbgemm's ``IntNBitTableBatchedEmbeddingBagsCodegen`` is for.
  ``lookup_sequence`` is its un-pooled lookup (``PoolingMode.NONE``): one dequantised row per lookup position, one launch.
  ``bitwidth`` is one int or one int PER TABLE (that class's ``weights_tys``): tables of either format share the launch, each pooled
  by its own format's rule -- no new arithmetic.
* :class:`QuantizedEmbeddingBagMI355` -- the single-table module with ``nn.EmbeddingBag``'s call; what
  ``torch.ao.nn.quantized.EmbeddingBag`` is for.
* :class:`QuantizedEmbeddingMI355` -- the single-table un-pooled module with ``nn.Embedding``'s call; what
  ``torch.ao.nn.quantized.Embedding`` is for.

The arithmetic is fixed (include/param_amd.h, "ROW-QUANTISED TABLES") and equals torch's CPU operators
``quantized::embedding_bag_{byte,4bit}_rowwise_offsets`` bit for bit: per element and lookup, in index order from +0.0,
``acc = fmaf(scale * w, code, acc + bias * w)``.  It is NOT bit-identical to the fp32 forward over ``dequantized_table(t)`` (which rounds
every dequantised element first); the two agree within summation rounding.  A bag of exactly one unweighted lookup equals
``dequantize_rows`` of that row as a value -- and that bag of one is the un-pooled rule: per lookup and column
``out = fmaf(scale, code, +0.0 + bias)`` (the addition is part of it: the result equals ``dequantize_rows`` as a value, not on the sign
of zeros), rounded once for a 16-bit ``output_dtype``; bit for bit ``quantized::embedding_byte`` / the two operators above over bags of one.

Forward only: the tables are buffers, nothing requires grad.  There is no CPU path.  Left out, on purpose: 2-bit tables, fp16 / bf16 /
fp32 rows next to quantised ones, mean pooling, ``padding_idx``, per-position weights of the un-pooled lookup, mixed dims of the un-pooled lookup from Python (the C call serves them),
a padded row stride, per-table lane sub-groups for mixed dims, a lane width per format, the operator plug-in, any backward.

PRUNED TABLES (``index_remapping=``; ``csrc/embbag_fwd_qpruned.hip`` / ``csrc/embedding_gather_qpruned.hip`` through
``pm_embbag_fwd_qrows_pruned`` / ``pm_embedding_gather_qrows_pruned``): a request addresses a table's LOGICAL rows and an int32 array per
table maps each to a physical row or to -1, "pruned" (fbgemm's ``index_remappings_array``, torch's ``compressed_indices_mapping``).  A
pooled bag drops its pruned lookups -- index and weight alike -- and pools the rest from their physical rows by the rule above; an
un-pooled pruned position is a row of +0.0.  Left out there: fbgemm's hash-based remap, pruned fp32 / bf16 training tables, 8-bit dims
that are multiples of 4 but not 8.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch
import torch.nn as nn

from . import _lib, quant
from .embedding_bag import (_IDTYPE, _WDTYPE, BatchedEmbeddingBagMI355, EmbeddingBagMI355, EmbeddingMI355, _BoundsChecked, _TableSet,
                            _check_rows_out, _require_device, _stream_ptr, bounds_check_mode_name)

BITWIDTHS = (8, 4)
MAX_DIM = 4096      # kQrowsMaxDim (csrc/launch_plan.h)


def _check_spec(bitwidth, dims: Sequence[int], layout: str) -> None:
    """what the constructors refuse, before anything is allocated"""
    if bitwidth not in BITWIDTHS or isinstance(bitwidth, bool):
        raise ValueError(f"bitwidth must be 8 or 4, got {bitwidth!r} (2-bit tables are not implemented; 16 bits is a table dtype of "
                         "BatchedEmbeddingBagMI355)")
    if layout == "blocked":
        raise ValueError('row-quantised tables do not take layout="blocked"')
    if layout not in ("bd", "tbd"):
        raise ValueError(f'layout must be "bd" or "tbd", got {layout!r}')
    mult = 4 if bitwidth == 8 else 8
    for d in dims:
        if d < mult or d % mult or d > MAX_DIM:
            raise ValueError(f"embedding dim {d}: a {bitwidth}-bit table needs a multiple of {mult} in [{mult}, {MAX_DIM}]")
    if layout == "tbd" and len(set(dims)) != 1:
        raise ValueError('layout "tbd" needs one common embedding dim')


def _table_bitwidths(bitwidth, dims: Sequence[int], layout: str):
    """``(bitwidths, bitwidth)`` of a constructor's ``bitwidth`` -- an int for every table, or one int per table as any Sequence but a
    string (a list, a tuple, a range) or an array / tensor (its ``tolist()``) -- after
    refusing what cannot be served, before anything is allocated.  ``bitwidth`` is the int of a uniform module and ``None`` of a mixed
    one; a sequence whose entries are all equal IS that int (today's module, today's launch)."""
    if isinstance(bitwidth, (str, bytes)) or not (isinstance(bitwidth, Sequence) or hasattr(bitwidth, "tolist")):
        _check_spec(bitwidth, dims, layout)
        return [int(bitwidth)] * len(dims), int(bitwidth)
    if hasattr(bitwidth, "tolist"):         # a numpy array or a tensor of per-table widths: its Python values
        bitwidth = bitwidth.tolist()
        if not isinstance(bitwidth, list):
            bitwidth = [bitwidth]
    bitwidth = list(bitwidth)               # (any Sequence: a list, a tuple, a range ..)
    if len(bitwidth) != len(dims):
        raise ValueError(f"bitwidth names {len(bitwidth)} tables, rows and dims name {len(dims)}: one entry per table (or one int)")
    for b in bitwidth:
        if isinstance(b, bool) or not isinstance(b, int) or b not in BITWIDTHS:
            raise ValueError(f"bitwidth must be 8 or 4 for every table, got {b!r} (2-bit tables are not implemented; 16 bits is a table "
                             "dtype of BatchedEmbeddingBagMI355)")
    if len(set(bitwidth)) == 1:
        _check_spec(bitwidth[0], dims, layout)
        return [int(bitwidth[0])] * len(dims), int(bitwidth[0])
    _check_spec(4, dims, layout)        # the stricter column rule (a multiple of 8), applied to every table: a lane holds eight columns
    return [int(b) for b in bitwidth], None


def _sum_only(mode, padding_idx, who: str) -> None:
    if str(getattr(mode, "name", mode)).lower() not in ("sum", "0"):
        raise ValueError(f"{who}: only sum pooling is implemented for row-quantised tables (got {mode!r})")
    if padding_idx is not None and not (isinstance(padding_idx, (list, tuple)) and all(k is None for k in padding_idx)):
        raise ValueError(f"{who}: padding_idx is not implemented for row-quantised tables")


def _check_remaps(index_remapping, rows: Sequence[int], dims: Sequence[int]):
    """``index_remapping`` of a constructor as a list of one ``None`` or 1-D tensor per table, or ``None`` for a module without a pruned
    table (``None``, or every entry ``None``) -- after refusing what cannot be served, before anything is allocated: a wrong count, an
    entry that is no 1-D int32 / int64 tensor, an empty one, ``logical_rows_t >= 2^31``, a value outside ``[-1, rows_t)`` (ONE host read
    for all tables), dims that are no multiples of 8 (the pruned lookups are the per-table-format kernels' siblings: eight columns per lane)."""
    if index_remapping is None:
        return None
    if isinstance(index_remapping, (bool, int, float, str, bytes, torch.Tensor)) or not isinstance(index_remapping, Sequence):
        raise TypeError(f"index_remapping must be None or a sequence of one None or 1-D int32 / int64 tensor per table, got "
                        f"{type(index_remapping).__name__}")
    remaps = list(index_remapping)
    if len(remaps) != len(rows):
        raise ValueError(f"index_remapping names {len(remaps)} tables, rows and dims name {len(rows)}: one entry per table (None: not pruned)")
    if all(r is None for r in remaps):
        return None
    for t, r in enumerate(remaps):
        if r is None:
            continue
        if not isinstance(r, torch.Tensor) or r.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"index_remapping[{t}] must be None or an int32 / int64 tensor, got {getattr(r, 'dtype', type(r).__name__)}")
        if r.dim() != 1 or r.numel() == 0:
            raise ValueError(f"index_remapping[{t}] must be 1-D with one entry per logical row, at least one (None: the table is not pruned); "
                             f"got shape {tuple(r.shape)}")
        if r.numel() >= 2**31:
            raise ValueError(f"index_remapping[{t}]: a table needs logical rows < 2^31, got {r.numel()}")
    if any(d % 8 for d in dims):
        raise ValueError(f"a pruned module needs every embedding dim a multiple of 8 (a lane holds eight columns), got {list(dims)}")
    pruned = [t for t, r in enumerate(remaps) if r is not None]
    lo_hi = torch.stack([torch.stack([remaps[t].min(), remaps[t].max()]).to(torch.int64).cpu() for t in pruned]).tolist()
    for t, (lo, hi) in zip(pruned, lo_hi):
        if lo < -1 or hi >= rows[t]:
            raise ValueError(f"index_remapping[{t}]: values must lie in [-1, rows[{t}]) = [-1, {rows[t]}) (-1: the row is pruned), "
                             f"got [{lo}, {hi}]")
    return remaps


def _keep_remap(keep: torch.Tensor, rows: int, t: int) -> torch.Tensor:
    """the int32 remap of a bool ``keep`` mask over a source's rows: kept rows get consecutive physical rows in order, dropped rows -1"""
    if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool or tuple(keep.shape) != (rows,):
        raise ValueError(f"keep[{t}] must be None or a bool tensor of shape ({rows},), got {getattr(keep, 'dtype', type(keep).__name__)} "
                         f"{tuple(getattr(keep, 'shape', ()))}")
    phys = torch.cumsum(keep.to(torch.int32), 0, dtype=torch.int32) - 1
    return torch.where(keep, phys, torch.full_like(phys, -1))


class _QTableSet(_TableSet):
    """:class:`_TableSet` over uint8 tables of quantised rows: ``dims`` are the LOGICAL column counts, ``dtype`` (what the request's
    ``weight_dtype`` says) is fp32 -- ``pm_embbag_fwd_qrows`` does not read it, the sanitiser reads rows, indices and offsets only."""

    def __init__(self, tables: Sequence[torch.Tensor], dims: Sequence[int], layout: str, bitwidths: Optional[Sequence[int]] = None,
                 index_rows: Optional[Sequence[int]] = None, ptrs: Optional[Sequence[int]] = None):
        t0 = tables[0]
        for t in tables:
            _require_device(t, "quantised table")
            if t.dtype != torch.uint8 or t.dim() != 2 or not t.is_contiguous() or t.data_ptr() % 4:
                raise ValueError("quantised tables must be contiguous, 4-byte aligned 2-D uint8 tensors")
            if t.shape[0] >= 2**31:
                raise ValueError("tables with >= 2^31 rows are not supported")
        self.device, self.dtype, self.layout = t0.device, torch.float32, layout
        self.rows = [int(t.shape[0]) for t in tables]
        self.dims = [int(d) for d in dims]
        self.block_bags = None
        self._blk_cache: dict = {}
        self.T = len(tables)
        self.max_dim, self.min_dim, self.total_dim = max(self.dims), min(self.dims), sum(self.dims)
        # (ptrs: where the tables begin in their slab -- a pruned module's, whose tables may have no row: torch gives an empty view no address)
        self.ptrs = [t.data_ptr() for t in tables] if ptrs is None else [int(p) for p in ptrs]
        self.d_ptrs = torch.tensor(self.ptrs, dtype=torch.int64, device=self.device)
        # the request's rows: every table's INDEX SPACE, which the sanitiser reads -- of a pruned module the logical rows (index_rows)
        self.d_rows = torch.tensor(self.rows if index_rows is None else list(index_rows), dtype=torch.int64, device=self.device)
        self.d_dims = torch.tensor(self.dims, dtype=torch.int32, device=self.device)
        # the tables' formats for the per-table-format calls (pm_embbag_fwd_qrows_mixed: table_bits), None for a uniform module
        self.d_bits = None if bitwidths is None else torch.tensor(list(bitwidths), dtype=torch.int32, device=self.device)
        col0 = [0]
        for d in self.dims[:-1]:
            col0.append(col0[-1] + d)
        self.col0 = col0
        self.d_col0 = torch.tensor(col0, dtype=torch.int64, device=self.device)
        self._tbd_cache: dict = {}
        self._req: dict = {}
        self._pool_key, self._pool_val = None, 0


class QuantizedBatchedEmbeddingBagMI355(nn.Module, _BoundsChecked):
    """T row-quantised embedding tables in one HBM slab, pooled (sum, optionally weighted) by ONE kernel launch that reads the quantised
    bytes.

    ``QuantizedBatchedEmbeddingBagMI355(rows, dims, bitwidth, device="cuda", layout="bd", output_dtype=None, bounds_check_mode="none")``:
    ``bitwidth`` 8 (``row_bytes = D + 8``) or 4 (``D / 2 + 4``); ``dims`` multiples of 4 (8-bit) / 8 (4-bit), at most 4096, and may differ
    per table with ``layout="bd"`` (lane groups are sized for the widest table).  ``bitwidth`` may also be a sequence of one 8 or 4 PER
    TABLE (a serving model keeps its big tables at 4 bits and its small or sensitive ones at 8): ``bitwidths`` is always that list,
    ``bitwidth`` the int of a uniform module and ``None`` of a mixed one; a sequence whose entries are all equal is the int (the same
    launch, plan and bits).  A mixed module needs every dim a multiple of 8; its ``lookup`` and ``lookup_sequence`` are still ONE launch
    (``pm_embbag_fwd_qrows_mixed`` / ``pm_embedding_gather_qrows_mixed``) and give, per table, the bits of a module of that table's
    format alone; ``table(t)``, ``quantize_from_``, ``dequantized_table`` and the slab layout use table ``t``'s format.
    The tables start as zero bytes: every row dequantises
    to zeros.  ``table(t)`` is the uint8 ``[rows_t, row_bytes]`` tensor -- copy prepacked bytes into it, or fill it with
    ``quantize_from_(t, fp32)`` (the ``quantize_rows`` kernel: fp32 sources, dims a multiple of 8 up to 512).  ``dequantized_table(t)`` is
    ``dequantize_rows`` of it.

    ``lookup(indices, offsets, per_sample_weights=None, out=None, bag_begin=0, bag_count=None, batch=None)`` -- and ``forward``, the same
    call -- takes the TBE request of :class:`BatchedEmbeddingBagMI355` and returns ``[B, sum D]`` (``"bd"``) or ``[T, B, D]`` (``"tbd"``) in
    ``output_dtype`` (fp32, or bf16 / fp16: the fp32 value rounded once in the kernel).  The rule is the module docstring's.
    ``plan(...)`` returns the launch geometry of the same request as a dict (``pm_embbag_qrows_plan``; nothing is launched).
    ``lookup_sequence(indices, offsets, batch=None, out=None, bag_begin=0, bag_count=None)`` is the UN-POOLED lookup of the same request:
    ``[N, D]``, one dequantised row per lookup position (one common embedding dim); ``sequence_plan(...)`` its launch geometry.
    ``bounds_check_mode``: see :class:`_BoundsChecked` -- the sanitiser reads rows, indices and offsets, never the tables.

    ``index_remapping``: ``None``, or a sequence of one entry per table, each ``None`` (the table is not pruned) or a 1-D int32 / int64
    tensor of ``logical_rows_t`` values in ``[-1, rows_t)``: the physical row of every logical row, -1 for a pruned one.  ``rows`` stays
    the PHYSICAL row count (the storage, what ``table(t)`` holds); ``logical_rows`` is every table's index space, ``index_remapping(t)``
    table ``t``'s remap (int32) or ``None``, ``pruned`` whether any table has one.  The remaps live in the buffers ``index_remap`` and
    ``index_remap_offsets``, registered only for a pruned module (``state_dict`` round-trips them; loaded values are the caller's
    responsibility).  A pruned module needs every dim a multiple of 8 and always launches ``pm_embbag_fwd_qrows_pruned`` /
    ``pm_embedding_gather_qrows_pruned`` (one launch, tables of one format included); ``plan`` / ``sequence_plan`` report that launch's
    geometry.  ``bounds_check_mode`` and ``sanitize_`` check indices against ``logical_rows``, before the remap: an index repaired to 0
    is remapped like any other.  ``from_float(source, bitwidth, keep=masks)`` builds such a module from bool masks over the source's rows.

    No gradients: the tables are a buffer (``state_dict`` round-trips the bytes), the output never requires grad.  ValueError before
    anything is allocated: ``bitwidth`` not 8 or 4, dims breaking the column rules, ``layout="blocked"``, mean pooling, ``padding_idx``.
    At call time: tensors that are not on a ROCm device raise RuntimeError (no CPU fallback), a floating-point index tensor TypeError.
    """

    def __init__(self, rows: Sequence[int], dims, bitwidth, device="cuda", layout: str = "bd", output_dtype=None,
                 bounds_check_mode="none", pooling_mode="sum", padding_idx=None, index_remapping=None):
        super().__init__()
        self._init_shared(bounds_check_mode, output_dtype)
        rows = [int(r) for r in rows]
        dims = [int(dims)] * len(rows) if isinstance(dims, int) else [int(d) for d in dims]
        if len(rows) != len(dims) or not rows:
            raise ValueError("rows and dims must name the same tables, at least one")
        bitwidths, bitwidth = _table_bitwidths(bitwidth, dims, layout)
        _sum_only(pooling_mode, padding_idx, type(self).__name__)
        if any(r < 0 or r >= 2**31 for r in rows):
            raise ValueError("every table needs 0 <= rows < 2^31")
        remaps = _check_remaps(index_remapping, rows, dims)
        self.padding_idx = None
        self.rows, self.dims, self.bitwidth, self.bitwidths, self.layout = rows, dims, bitwidth, bitwidths, layout
        self.pruned = remaps is not None
        self.logical_rows = list(rows) if remaps is None else [r if m is None else int(m.numel()) for r, m in zip(rows, remaps)]
        self._row_bytes = [quant.host_row_bytes(d, b) for d, b in zip(dims, bitwidths)]
        # table starts padded to 256 B (rows themselves are 4-byte aligned and no better)
        starts, cur = [], 0
        for r, rb in zip(rows, self._row_bytes):
            starts.append(cur)
            cur += (r * rb + 255) // 256 * 256
        if self.pruned:
            cur = max(cur, 256)     # (the un-pooled pruned lookup reads table 0's first 8 bytes for a pruned position, whatever rows[0] is)
        self._starts = starts
        self.register_buffer("weights", torch.zeros(cur, dtype=torch.uint8, device=device))
        if self.pruned:
            # the remaps, concatenated, and where each table's begins (pm_embbag_fwd_qrows_pruned: remap, remap_offsets): buffers of a
            # pruned module only -- the state_dict keys of a module without a pruned table are what they were
            ends, cat = [0], []
            for m in remaps:
                ends.append(ends[-1] + (0 if m is None else int(m.numel())))
                if m is not None:
                    cat.append(m.detach().to(device=device, dtype=torch.int32))
            self.register_buffer("index_remap", torch.cat(cat))
            self.register_buffer("index_remap_offsets", torch.tensor(ends, dtype=torch.int64, device=device))
            self._remap_ends = ends
        self._ts: Optional[_QTableSet] = None

    _TABLES = "weights"

    # -- tables ------------------------------------------------------------------------------
    def table(self, t: int) -> torch.Tensor:
        s, n = self._starts[t], self.rows[t] * self._row_bytes[t]
        return self.weights[s:s + n].view(self.rows[t], self._row_bytes[t])

    def index_remapping(self, t: int) -> Optional[torch.Tensor]:
        """table ``t``'s remap -- int32 ``[logical_rows[t]]``, a view of the ``index_remap`` buffer: the physical row of every logical
        row, -1 for a pruned one -- or ``None`` for a table that is not pruned"""
        if not self.pruned or self._remap_ends[t + 1] == self._remap_ends[t]:
            return None
        return self.index_remap[self._remap_ends[t]:self._remap_ends[t + 1]]

    def quantize_from_(self, t: int, source: torch.Tensor) -> None:
        """fill table ``t`` from the fp32 tensor ``source`` ``[rows_t, D_t]`` on the GPU with the ``quantize_rows`` kernel (its limits: fp32
        only, D a multiple of 8 up to 512; other widths: copy prepacked bytes into ``table(t)``)"""
        if source.dtype != torch.float32:
            raise TypeError(f"quantize_from_: float32 expected, got {source.dtype} (widen 16-bit tables first)")
        if tuple(source.shape) != (self.rows[t], self.dims[t]):
            raise ValueError(f"quantize_from_: table {t} is {(self.rows[t], self.dims[t])}, got {tuple(source.shape)}")
        _require_device(self.weights, f"{type(self).__name__}.weights")
        if self.rows[t]:
            quant.quantize_rows(source.detach().contiguous(), self.dims[t], self.bitwidths[t], out=self.table(t))

    def dequantized_table(self, t: int) -> torch.Tensor:
        """fp32 ``[rows_t, D_t]``: ``dequantize_rows`` of table ``t``"""
        _require_device(self.weights, f"{type(self).__name__}.weights")
        return quant.dequantize_rows(self.table(t), self.dims[t], self.bitwidths[t])

    @classmethod
    def from_float(cls, source, bitwidth, keep=None, **kw):
        """quantise a :class:`BatchedEmbeddingBagMI355` sum module (16-bit tables are widened first) or a sequence of fp32 ``[rows, D]``
        tensors; ``bitwidth``: an int, or one per table; keywords go to the constructor (``device``, ``layout`` default to the source's).
        ``keep``: ``None``, or per table ``None`` or a bool mask over the source's rows -- only the kept rows are quantised, into
        consecutive physical rows in order, and the module is a pruned one whose remap sends the dropped rows to -1."""
        if isinstance(source, BatchedEmbeddingBagMI355):
            _sum_only(source.pooling_mode, source.padding_idx, "from_float")
            tables = [source.table(t).float() for t in range(len(source.rows))]
            kw.setdefault("layout", source.layout)
        else:
            tables = list(source)
            if not tables or any(not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32 for x in tables):
                raise TypeError("from_float takes a BatchedEmbeddingBagMI355 or a sequence of 2-D float32 tensors")
        kw.setdefault("device", tables[0].device)
        if keep is not None:
            if isinstance(keep, torch.Tensor) or not isinstance(keep, Sequence) or len(keep) != len(tables):
                raise ValueError(f"keep must be None or a sequence of one None or bool mask per table ({len(tables)})")
            remaps = [None if k is None else _keep_remap(k, int(x.shape[0]), t) for t, (k, x) in enumerate(zip(keep, tables))]
            tables = [x if k is None else x[k.to(x.device)] for k, x in zip(keep, tables)]
            kw["index_remapping"] = remaps
        m = cls([int(x.shape[0]) for x in tables], [int(x.shape[1]) for x in tables], bitwidth, **kw)
        for t, x in enumerate(tables):
            m.quantize_from_(t, x.to(m.weights.device))
        return m

    def _tables(self) -> _QTableSet:
        if self.pruned:
            # a pruned module always launches the per-table-format kernels' siblings: it carries table_bits, its index space, and the
            # tables' addresses in the slab (the un-pooled lookup reads 8 bytes at tables[0] even if table 0 has no row)
            base = self.weights.data_ptr()
            if self._ts is None or self._ts.ptrs[0] != base + self._starts[0]:
                self._ts = _QTableSet([self.table(t) for t in range(len(self.rows))], self.dims, self.layout, self.bitwidths, self.logical_rows,
                                      [base + s for s in self._starts])
            return self._ts
        if self._ts is None or self._ts.ptrs[0] != self.table(0).data_ptr():
            self._ts = _QTableSet([self.table(t) for t in range(len(self.rows))], self.dims, self.layout,
                                  None if self.bitwidth is not None else self.bitwidths)
        return self._ts

    def _remap_ptrs(self):
        _require_device(self.index_remap, f"{type(self).__name__}.index_remap")
        _require_device(self.index_remap_offsets, f"{type(self).__name__}.index_remap_offsets")
        return self.index_remap.data_ptr(), self.index_remap_offsets.data_ptr()

    _batch_of = BatchedEmbeddingBagMI355._batch_of

    # -- ops ---------------------------------------------------------------------------------
    def _request(self, indices, offsets, per_sample_weights, bag_begin, bag_count, batch, sanitize: bool):
        if indices.dtype.is_floating_point or offsets.dtype.is_floating_point:
            raise TypeError(f"indices and offsets must both be int64 or both int32, got {indices.dtype} / {offsets.dtype}")
        _require_device(self.weights, f"{type(self).__name__}.weights")
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
        if self.pruned:
            remap, remap_offsets = self._remap_ptrs()
            rc = _lib.load().pm_embbag_fwd_qrows_pruned(ctypes.byref(op), ts.d_bits.data_ptr(), remap, remap_offsets, _WDTYPE[odt],
                                                        out.data_ptr(), _stream_ptr())
        elif self.bitwidth is not None:
            rc = _lib.load().pm_embbag_fwd_qrows(ctypes.byref(op), self.bitwidth, _WDTYPE[odt], out.data_ptr(), _stream_ptr())
        else:
            rc = _lib.load().pm_embbag_fwd_qrows_mixed(ctypes.byref(op), ts.d_bits.data_ptr(), _WDTYPE[odt], out.data_ptr(), _stream_ptr())
        if rc:
            _lib.check(rc)
        return out

    def forward(self, indices, offsets, per_sample_weights=None, out=None, bag_begin=0, bag_count=None, batch: Optional[int] = None):
        return self.lookup(indices, offsets, per_sample_weights, out, bag_begin, bag_count, batch)

    def plan(self, indices, offsets, per_sample_weights=None, bag_begin=0, bag_count=None, batch: Optional[int] = None) -> dict:
        """the launch geometry ``lookup`` would use for this request under the knobs as they stand (``_lib.PLAN_FIELDS`` by name;
        ``pm_embbag_qrows_plan``, or ``pm_embbag_qrows_mixed_plan`` for a module of per-table formats and for a pruned one, whose
        launch has that geometry)"""
        _, _, op = self._request(indices, offsets, per_sample_weights, bag_begin, bag_count, batch, False)
        if self.bitwidth is None or self.pruned:
            return _lib.embbag_qrows_mixed_plan(op, _WDTYPE[self.output_dtype])
        return _lib.embbag_qrows_plan(op, self.bitwidth, _WDTYPE[self.output_dtype])

    # -- un-pooled ---------------------------------------------------------------------------
    def _sequence_request(self, indices, offsets, batch, bag_begin, bag_count, sanitize: bool, out=None):
        if len(set(self.dims)) != 1:
            raise ValueError("lookup_sequence needs one common embedding dim (mixed dims are served by pm_embedding_gather_qrows, the C call)")
        if out is not None:
            _check_rows_out(out, indices.numel(), self.dims[0], self.output_dtype, self.weights.device)
        return self._request(indices, offsets, None, bag_begin, bag_count, batch, sanitize)

    def lookup_sequence(self, indices, offsets, batch: Optional[int] = None, out=None, bag_begin=0, bag_count=None):
        """The UN-POOLED forward over the module's T tables (int-nbit TBE's ``PoolingMode.NONE``): ``[N, D]`` in the module's
        ``output_dtype``, ``N = indices.numel()``, row ``j`` = row ``indices[j]`` of the table that owns lookup position ``j`` (table ``t``
        owns ``[offsets[t * B], offsets[(t + 1) * B])``), dequantised by the module docstring's rule for a bag of one -- one launch,
        ``pm_embedding_gather_qrows`` (a module of per-table formats: ``pm_embedding_gather_qrows_mixed``, every row in its table's
        format), that reads the quantised bytes.  Runs after ``bounds_check_mode``, like ``lookup``.
        ``bag_begin/bag_count`` select a batch slice: only the rows of lookups inside it are written -- a caller's ``out`` keeps every
        other row, a tensor allocated here holds zeros there.  Needs one common embedding dim; mixed dims and an ``out`` that is not a
        contiguous ``[N, D]`` tensor of ``output_dtype`` on the module's device raise ValueError, floating-point indices TypeError."""
        ts, B, op = self._sequence_request(indices, offsets, batch, bag_begin, bag_count, True, out)
        n, D, odt = indices.numel(), self.dims[0], self.output_dtype
        if out is None:
            whole = bag_begin == 0 and bag_count in (None, B)
            out = (torch.empty if whole else torch.zeros)((n, D), dtype=odt, device=ts.device)
        if n:
            if self.pruned:
                remap, remap_offsets = self._remap_ptrs()
                rc = _lib.load().pm_embedding_gather_qrows_pruned(ctypes.byref(op), ts.d_bits.data_ptr(), remap, remap_offsets, _WDTYPE[odt],
                                                                  out.data_ptr(), D, _stream_ptr())
            elif self.bitwidth is not None:
                rc = _lib.load().pm_embedding_gather_qrows(ctypes.byref(op), self.bitwidth, _WDTYPE[odt], out.data_ptr(), D, _stream_ptr())
            else:
                rc = _lib.load().pm_embedding_gather_qrows_mixed(ctypes.byref(op), ts.d_bits.data_ptr(), _WDTYPE[odt], out.data_ptr(), D,
                                                                 _stream_ptr())
            if rc:
                _lib.check(rc)
        return out

    def sequence_plan(self, indices, offsets, batch: Optional[int] = None, bag_begin=0, bag_count=None) -> dict:
        """the launch geometry ``lookup_sequence`` would use for this request under the knobs as they stand (``_lib.GATHER_PLAN_FIELDS``
        by name; ``pm_embedding_gather_qrows_plan`` -- a module of per-table formats or a pruned one:
        ``pm_embedding_gather_qrows_mixed_plan`` --, nothing is launched)"""
        _, _, op = self._sequence_request(indices, offsets, batch, bag_begin, bag_count, False)
        if self.bitwidth is None or self.pruned:
            return _lib.embedding_gather_qrows_mixed_plan(op)
        return _lib.embedding_gather_qrows_plan(op, self.bitwidth)

    def sanitize_(self, indices, offsets, batch: Optional[int] = None, mode=None) -> None:
        """The sanitiser on its own (see :class:`BatchedEmbeddingBagMI355`)."""
        _require_device(self.weights, f"{type(self).__name__}.weights")
        B = self._batch_of(offsets, indices) if batch is None else batch
        mode = bounds_check_mode_name(mode) if mode is not None else self.bounds_check_mode
        self._sanitize(self._tables(), indices, offsets, B, "warning" if mode == "none" else mode)

    def extra_repr(self) -> str:
        return (f"rows={self.rows}, dims={self.dims}, bitwidth={self.bitwidth if self.bitwidth is not None else self.bitwidths}, layout={self.layout}" +
                (f", output_dtype={self.output_dtype}" if self._out16 is not None else ""))


class QuantizedEmbeddingBagMI355(QuantizedBatchedEmbeddingBagMI355):
    """``torch.ao.nn.quantized.EmbeddingBag`` / ``nn.EmbeddingBag(mode="sum")`` over ONE row-quantised table, on the HIP kernel.

    ``QuantizedEmbeddingBagMI355(num_embeddings, embedding_dim, bitwidth=8, device="cuda", output_dtype=None, bounds_check_mode="none",
    weight=None)``; ``forward(input, offsets=None, per_sample_weights=None)`` -> ``[B, D]``: ``input`` 1-D with ``offsets`` ``[B]``
    (``include_last_offset=False``), or 2-D ``[B, L]`` with ``offsets=None`` (every row one bag of L lookups; ``per_sample_weights`` then has
    the input's shape).  ``weight``: the packed uint8 ``[num_embeddings, row_bytes]`` bytes of ``quantized::embedding_bag_{byte,4bit}_prepack``
    (what ``torch.ao.nn.quantized.EmbeddingBag`` holds): the same layout, copied as they are.  ``from_float(m)`` quantises an
    :class:`EmbeddingBagMI355` or a ``torch.nn.EmbeddingBag`` of ``mode="sum"`` without ``padding_idx`` on the GPU.  Refusals as the
    batched module's; ``mode`` other than ``"sum"`` and ``padding_idx`` raise ValueError."""

    def __init__(self, num_embeddings: int, embedding_dim: int, bitwidth: int = 8, device="cuda", output_dtype=None,
                 bounds_check_mode="none", mode="sum", padding_idx=None, weight: Optional[torch.Tensor] = None, index_remapping=None):
        if weight is not None:
            _check_spec(bitwidth, [int(embedding_dim)], "bd")
            want = (int(num_embeddings), quant.host_row_bytes(int(embedding_dim), bitwidth))
            if weight.dtype != torch.uint8 or tuple(weight.shape) != want:
                raise ValueError(f"weight must be the packed uint8 rows {want}, got {weight.dtype} {tuple(weight.shape)}")
        super().__init__([num_embeddings], [embedding_dim], bitwidth, device=device, layout="bd", output_dtype=output_dtype,
                         bounds_check_mode=bounds_check_mode, pooling_mode=mode, padding_idx=padding_idx,
                         index_remapping=None if index_remapping is None else [index_remapping])
        self.num_embeddings, self.embedding_dim = int(num_embeddings), int(embedding_dim)
        self._off2d: dict = {}
        if weight is not None:
            self.table(0).copy_(weight)

    _bags_2d = EmbeddingBagMI355._bags_2d

    @classmethod
    def from_float(cls, module, bitwidth: int = 8, keep=None, **kw):
        if not isinstance(module, (EmbeddingBagMI355, nn.EmbeddingBag)):
            raise TypeError("from_float takes an EmbeddingBagMI355 or a torch.nn.EmbeddingBag")
        _sum_only(module.mode, module.padding_idx, "from_float")
        w = module.weight.detach()
        kw.setdefault("device", w.device if w.is_cuda else "cuda")
        if keep is not None:        # a bool mask over the source's rows: only the kept rows are stored, the rest is pruned
            kw["index_remapping"] = _keep_remap(keep, int(w.shape[0]), 0)
            w = w[keep.to(w.device)]
        m = cls(int(w.shape[0]), int(w.shape[1]), bitwidth, **kw)
        m.quantize_from_(0, w.to(device=m.weights.device, dtype=torch.float32))
        return m

    def forward(self, input, offsets=None, per_sample_weights=None):
        if input.dim() == 2:
            input, offsets, per_sample_weights = self._bags_2d(input, offsets, per_sample_weights)
        elif offsets is None:
            raise ValueError("offsets has to be a 1D Tensor but got None")
        return self.lookup(input, offsets, per_sample_weights, batch=offsets.numel())

    def extra_repr(self) -> str:
        return f"{self.num_embeddings}, {self.embedding_dim}, bitwidth={self.bitwidth}" + (f", output_dtype={self.output_dtype}" if self._out16 is not None else "")


class QuantizedEmbeddingMI355(QuantizedBatchedEmbeddingBagMI355):
    """``torch.ao.nn.quantized.Embedding`` over ONE row-quantised table, on the HIP kernel: the un-pooled sibling of
    :class:`QuantizedEmbeddingBagMI355` and the quantised sibling of :class:`EmbeddingMI355`.

    ``QuantizedEmbeddingMI355(num_embeddings, embedding_dim, bitwidth=8, device="cuda", output_dtype=None, bounds_check_mode="none",
    weight=None)``; ``forward(input)`` takes an int32 / int64 tensor of any shape and returns ``[*input.shape, D]`` in ``output_dtype``:
    row ``input[...]`` of the table per lookup, dequantised by the module docstring's rule for a bag of one (bit for bit what
    ``quantized::embedding_byte`` computes), moved by ONE launch (``pm_embedding_gather_qrows``: the request is :class:`EmbeddingMI355`'s
    -- one table, one bag, ``offsets = [0]``).  An empty input returns an empty result without a launch.  ``weight``: the packed uint8
    ``[num_embeddings, row_bytes]`` bytes of ``quantized::embedding_bag_{byte,4bit}_prepack`` (what ``torch.ao.nn.quantized.Embedding``
    holds), copied as they are.  ``from_float(m, bitwidth=8)`` quantises a ``torch.nn.Embedding`` or an :class:`EmbeddingMI355` on the
    GPU (``quantize_from_``: D a multiple of 8 up to 512); its ``padding_idx`` changes nothing here (a forward returns the padding row as
    stored), ``max_norm`` raises ValueError.  ``table(0)``, ``dequantized_table(0)``, ``sanitize_(input)`` and the ``state_dict`` round
    trip are the batched module's; no parameters, the output never requires grad.  A floating-point input raises TypeError, tensors
    that are not on a ROCm device RuntimeError (no CPU fallback)."""

    def __init__(self, num_embeddings: int, embedding_dim: int, bitwidth: int = 8, device="cuda", output_dtype=None,
                 bounds_check_mode="none", weight: Optional[torch.Tensor] = None, index_remapping=None):
        if weight is not None:
            _check_spec(bitwidth, [int(embedding_dim)], "bd")
            want = (int(num_embeddings), quant.host_row_bytes(int(embedding_dim), bitwidth))
            if weight.dtype != torch.uint8 or tuple(weight.shape) != want:
                raise ValueError(f"weight must be the packed uint8 rows {want}, got {weight.dtype} {tuple(weight.shape)}")
        super().__init__([num_embeddings], [embedding_dim], bitwidth, device=device, layout="bd", output_dtype=output_dtype,
                         bounds_check_mode=bounds_check_mode, index_remapping=None if index_remapping is None else [index_remapping])
        self.num_embeddings, self.embedding_dim = int(num_embeddings), int(embedding_dim)
        self._off0: dict = {}        # the request's offsets [0], one per (dtype, device)
        if weight is not None:
            self.table(0).copy_(weight)

    _offsets0 = EmbeddingMI355._offsets0

    @classmethod
    def from_float(cls, module, bitwidth: int = 8, keep=None, **kw):
        if not isinstance(module, (EmbeddingMI355, nn.Embedding)):
            raise TypeError("from_float takes an EmbeddingMI355 or a torch.nn.Embedding")
        if getattr(module, "max_norm", None) is not None:
            raise ValueError("from_float: max_norm is not implemented (the rows would be renormalised at lookup time)")
        w = module.weight.detach()
        kw.setdefault("device", w.device if w.is_cuda else "cuda")
        if keep is not None:        # a bool mask over the source's rows: only the kept rows are stored, the rest is pruned
            kw["index_remapping"] = _keep_remap(keep, int(w.shape[0]), 0)
            w = w[keep.to(w.device)]
        m = cls(int(w.shape[0]), int(w.shape[1]), bitwidth, **kw)
        m.quantize_from_(0, w.to(device=m.weights.device, dtype=torch.float32))
        return m

    def _flat(self, input) -> torch.Tensor:
        if not isinstance(input, torch.Tensor) or input.dtype not in _IDTYPE:
            raise TypeError(f"QuantizedEmbeddingMI355: input must be an int32 or int64 tensor, got {getattr(input, 'dtype', type(input))}")
        _require_device(self.weights, "QuantizedEmbeddingMI355.weights")
        _require_device(input, "input")
        return input.reshape(-1).contiguous()

    def forward(self, input):
        indices = self._flat(input)
        if not indices.numel():
            return torch.empty((*input.shape, self.embedding_dim), dtype=self.output_dtype, device=self.weights.device)
        return self.lookup_sequence(indices, self._offsets0(indices), batch=1).view(*input.shape, self.embedding_dim)

    def sanitize_(self, input, mode=None) -> None:
        """The sanitiser on its own: repairs ``input`` in place (it must be contiguous: a copy would be repaired instead),
        stream-ordered.  ``mode``: default the module's ``bounds_check_mode``, ``"warning"`` where that is ``"none"``."""
        if not input.is_contiguous():
            raise ValueError("sanitize_ needs a contiguous input (it is repaired in place)")
        indices = self._flat(input)
        if indices.numel():
            super().sanitize_(indices, self._offsets0(indices), batch=1, mode=mode)

    def extra_repr(self) -> str:
        return f"{self.num_embeddings}, {self.embedding_dim}, bitwidth={self.bitwidth}" + (f", output_dtype={self.output_dtype}" if self._out16 is not None else "")
