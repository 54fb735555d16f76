"""Host-side (PyTorch-ROCm) mirror of the reference's EmbeddingBag operator surface.

* :class:`EmbeddingBagMI355`      -- drop-in for ``torch.nn.EmbeddingBag(n, m, mode="sum")`` as
  used at reference ``train/compute/pt/pytorch_emb.py:179,40,61`` and
  ``train/comms/pt/pytorch_dist_backend.py:923-934`` / ``dlrm.py:380``: ``forward(indices,
  offsets)``, ``.weight`` parameter, survives ``.to("cuda:0")``.
* :class:`BatchedEmbeddingBagMI355` -- the multi-table (TBE) form the reference reaches through
  ``fbgemm_gpu.SplitTableBatchedEmbeddingBagsCodegen`` (``comms_utils.py:1994-2017``,
  ``pytorch_dist_backend.py:221,845-857``, ``split_table_batched_embeddings_ops.py:279-324``):
  ``forward(indices, offsets, per_sample_weights)`` -> ``[B, sum D]``; ``backward`` applies the
  fused in-place scatter-add update (plain SGD form); ``lookup_sequence`` -> ``[N, D]``, fbgemm's un-pooled (sequence) forward.
* :class:`EmbeddingMI355`         -- drop-in for ``torch.nn.Embedding(n, m)``, the un-pooled sibling: ``forward(input)`` ->
  ``[*input.shape, m]``.

PyTorch is plumbing here (device memory, streams, autograd glue); all arithmetic runs in the
hand-written HIP kernels behind the C ABI (include/param_amd.h).  There is no CPU path: a
tensor that is not on a ROCm device raises.
"""
from __future__ import annotations

import ctypes
import math
import operator
from typing import Optional, Sequence

import torch
import torch.nn as nn

from . import _lib

_WDTYPE = {torch.float32: _lib.PM_F32, torch.bfloat16: _lib.PM_BF16, torch.float16: _lib.PM_F16}
_IDTYPE = {torch.int64: _lib.PM_I64, torch.int32: _lib.PM_I32}


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_ptr() -> int:
    """raw ``hipStream_t`` of torch's current stream on the current device (the fast accessor when torch has it)"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _require_device(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"param_amd: {what} is on '{t.device}'. The MI355X EmbeddingBag path runs only on a "
            "ROCm device (no CPU fallback); move the module and its inputs to cuda.")


def fill_random_(t: torch.Tensor, dist: str = "normal", a: float = 0.0, b: float = 1.0, seed: int = 0) -> torch.Tensor:
    """In-place counter-based fill at HBM speed (``pm_fill_random``): ``dist="normal"`` ->
    N(mean=a, std=b) (nn.EmbeddingBag's default init, pytorch_emb.py:179), ``"uniform"`` ->
    U[a, b) (dlrm table init, pytorch_dist_backend.py:923-934)."""
    _require_device(t, "tensor")
    if not t.is_contiguous():
        raise ValueError("fill_random_ needs a contiguous tensor")
    _lib.check(_lib.load().pm_fill_random(t.data_ptr(), t.numel(), _WDTYPE[t.dtype],
                                          1 if dist == "normal" else 0, float(a), float(b),
                                          int(seed) & (2**64 - 1), _stream_ptr()))
    return t


def _normalize_padding_idx(padding_idx, num_embeddings: int) -> Optional[int]:
    """torch's rule for ``padding_idx`` (``nn.EmbeddingBag.__init__``): ``None``, or an int in ``[-n, n)``; negative values count
    from the end.  Out of range raises with torch's text."""
    if padding_idx is None:
        return None
    if isinstance(padding_idx, bool):
        raise TypeError("padding_idx must be an int or None")
    k = operator.index(padding_idx)
    if not -num_embeddings <= k < num_embeddings:
        raise ValueError(f"padding_idx must be within num_embeddings (got {k} for {num_embeddings} rows)")
    return k + num_embeddings if k < 0 else k


def _pad_tensor(pads: Sequence[Optional[int]], device) -> torch.Tensor:
    """the device form of per-table padding indices: int64 ``[T]``, -1 = the table has none (include/param_amd.h)"""
    return torch.tensor([-1 if k is None else k for k in pads], dtype=torch.int64, device=device)


class _PadGuard:
    """``pm_pad_rows_guard`` around a backward call that is left as it is: ``save()`` copies every table's padding row (and its
    optimizer state) into a stash cached on the table set, ``restore()`` puts them back -- two small stream-ordered launches, no
    synchronisation.  ``tables_dev`` / ``state_dev``: device pointer arrays ``[T]`` (the weight tables or a dense gradient's
    buffers; the Adagrad state).  With ``pad=None`` both calls do nothing."""

    def __init__(self, ts: "_TableSet", pad: Optional[torch.Tensor], tables_dev: torch.Tensor, dtype: torch.dtype,
                 state_dev: Optional[torch.Tensor] = None, state_kind: int = _lib.PM_PAD_STATE_NONE):
        self.pad = pad
        if pad is None:
            return
        self.args = (ts.T, ts.max_dim, tables_dev.data_ptr(), ts.d_dims.data_ptr(), _WDTYPE[dtype], pad.data_ptr(),
                     None if state_dev is None else state_dev.data_ptr(), state_kind)
        self.stash = ts.scratch("_pad_stash", _lib.load().pm_pad_rows_guard_bytes(ts.T, ts.max_dim, _WDTYPE[dtype], state_kind))

    def _call(self, direction: int) -> None:
        if self.pad is not None:
            _lib.check(_lib.load().pm_pad_rows_guard(*self.args, self.stash.data_ptr(), self.stash.numel(), direction, _stream_ptr()))

    def save(self) -> None:
        self._call(_lib.PM_PAD_SAVE)

    def restore(self) -> None:
        self._call(_lib.PM_PAD_RESTORE)


class _TableSet:
    """Device-side description of T tables (pointer / rows / dims / output-offset arrays)."""

    def __init__(self, tables: Sequence[torch.Tensor], layout: str = "bd", block_bags: Optional[int] = None):
        assert layout in ("bd", "tbd", "blocked")
        t0 = tables[0]
        for t in tables:
            _require_device(t, "embedding table")
            if t.dtype != t0.dtype or t.dim() != 2 or not t.is_contiguous():
                raise ValueError("tables must be contiguous 2-D tensors of one dtype")
            if t.shape[0] >= 2**31:
                raise ValueError("tables with >= 2^31 rows are not supported")
        if t0.dtype not in _WDTYPE:
            raise TypeError(f"unsupported table dtype {t0.dtype}")
        self.device = t0.device
        self.dtype = t0.dtype
        self.layout = layout
        self.rows = [int(t.shape[0]) for t in tables]
        self.dims = [int(t.shape[1]) for t in tables]
        vec = 4 if t0.dtype == torch.float32 else 8
        for d in self.dims:
            if d % vec:
                raise ValueError(f"embedding dim {d} must be a multiple of {vec} for dtype {t0.dtype}")
        if layout in ("tbd", "blocked") and len(set(self.dims)) != 1:
            raise ValueError(f'layout "{layout}" needs one common embedding dim')
        # "blocked" = [W][T][block_bags][D], W = B / block_bags: the send layout of a table-wise sharded exchange whose peers each
        # get ONE contiguous chunk made of [block_bags, D] runs per table (include/param_amd.h, pm_embbag_batch, ABI v6)
        self.block_bags = None
        if layout == "blocked":
            if block_bags is None or block_bags < 1 or block_bags & (block_bags - 1):
                raise ValueError('layout "blocked" needs block_bags = a power of two (the per-rank batch)')
            self.block_bags = int(block_bags)
        self._blk_cache: dict = {}
        self.T = len(tables)
        self.max_dim = max(self.dims)
        self.min_dim = min(self.dims)
        self.total_dim = sum(self.dims)
        self.ptrs = [t.data_ptr() for t in tables]
        self.d_ptrs = torch.tensor(self.ptrs, dtype=torch.int64, device=self.device)
        self.d_rows = torch.tensor(self.rows, dtype=torch.int64, device=self.device)
        self.d_dims = torch.tensor(self.dims, dtype=torch.int32, device=self.device)
        col0 = [0]
        for d in self.dims[:-1]:
            col0.append(col0[-1] + d)
        self.col0 = col0
        self.d_col0 = torch.tensor(col0, dtype=torch.int64, device=self.device)
        self._tbd_cache: dict[int, torch.Tensor] = {}
        self._req: dict = {}         # one cached descriptor per kind of request (forward of a blocked layout / everything else)
        self._pool_key, self._pool_val = None, 0

    def scratch(self, slot: str, need: int, dtype: torch.dtype = torch.uint8) -> torch.Tensor:
        """The scratch tensor kept as attribute ``slot`` of this table set (``_ws``: the sorted backward's workspace, ``_pad_stash``,
        ``_bounds_scratch``), of at least ``need`` bytes in whole elements of ``dtype``: grown, never shrunk.  ``need`` is what a size
        query of the library returned: a negative value is its error code and raises."""
        if need < 0:
            _lib.check(int(need))
        t = self.__dict__.get(slot)
        if t is None or t.nbytes < need:
            t = torch.empty((int(need) + dtype.itemsize - 1) // dtype.itemsize, dtype=dtype, device=self.device)
            setattr(self, slot, t)
        return t

    def out_desc(self, B: int):
        """(out_offsets device tensor, out_stride, output shape) for a batch of B bags."""
        if self.layout == "bd":
            return self.d_col0, self.total_dim, (B, self.total_dim)
        D = self.dims[0]
        if self.layout == "blocked":
            # (the BACKWARD's description: T weight tables, batch B, gradient of bag b at t * Bl * D + b * D + (b >> log2 Bl) * (T - 1) * Bl * D)
            Bl = self.block_bags
            if B % Bl:
                raise ValueError(f"blocked layout: batch {B} is not a multiple of block_bags {Bl}")
            key = ("bwd", B)
            if key not in self._blk_cache:
                self._blk_cache[key] = torch.arange(self.T, dtype=torch.int64, device=self.device) * (Bl * D)
            return self._blk_cache[key], D, (B // Bl, self.T, Bl, D)
        if B not in self._tbd_cache:
            self._tbd_cache[B] = torch.arange(self.T, dtype=torch.int64, device=self.device) * (B * D)
        return self._tbd_cache[B], D, (self.T, B, D)

    def blocked_forward_arrays(self, B: int):
        """request tables of the blocked FORWARD: W = B / block_bags consecutive request tables per weight table (the
        table-major indices / offsets arrays already are that request) -> (tables, rows, dims, out_offsets) device arrays, W"""
        Bl, D, T = self.block_bags, self.dims[0], self.T
        W = B // Bl
        key = ("fwd", W)
        if key not in self._blk_cache:
            rep_ = lambda t: t.repeat_interleave(W)                                                        # noqa: E731
            w = torch.arange(W, dtype=torch.int64, device=self.device).repeat(T)
            tt = torch.arange(T, dtype=torch.int64, device=self.device).repeat_interleave(W)
            self._blk_cache[key] = (rep_(self.d_ptrs), rep_(self.d_rows), rep_(self.d_dims), w * (T * Bl * D) + tt * (Bl * D))
        return self._blk_cache[key], W

    def request(self, indices, offsets, B, psw, bag_begin, bag_count, d_ptrs=None, forward: bool = False) -> _lib.pm_embbag_batch:
        # benchmark loops call with the SAME tensors every step (pytorch_emb.py:56-66): the validated descriptor of the
        # last request is reused when pointers, sizes and dtypes are unchanged (saves ~4 us of host time per call, which
        # is what a 512-bag lookup costs on the device)
        # (the caching allocator hands freed addresses out again: everything _build_request validates is part of the key)
        key = (indices.data_ptr(), indices.numel(), indices.dtype, indices.is_contiguous(), indices.device,
               offsets.data_ptr(), offsets.numel(), offsets.dtype, offsets.is_contiguous(), offsets.device, B,
               None if psw is None else (psw.data_ptr(), psw.numel(), psw.dtype, psw.is_contiguous(), psw.device),
               bag_begin, bag_count, None if d_ptrs is None else d_ptrs.data_ptr(), forward and self.layout == "blocked")
        # (two slots: with layout="blocked" the forward descriptor -- T * W request tables -- and the backward's -- T tables with a
        # blocked gradient -- differ, and a training loop alternates between them)
        slot = bool(forward and self.layout == "blocked")
        hit = self._req.get(slot)
        if hit is not None and hit[0] == key:
            return hit[1]
        op = self._build_request(indices, offsets, B, psw, bag_begin, bag_count, d_ptrs, forward)
        self._req[slot] = (key, op)
        return op

    def fixed_pooling(self, indices, offsets, B, claim: Optional[int] = None) -> int:
        """L if every bag of the request has exactly L lookups, else 0 (``pm_embbag_batch.fixed_pooling``: lets the sorted
        backward use per-table sort segments, the XCD-affine and the two-phase apply).  ``claim``: the caller's word for it
        (no device read).  Otherwise ONE comparison on the device per new ``offsets`` tensor, remembered while the same
        tensor is passed again (benchmark loops); pass ``pooling=`` to the module methods to skip it in a training loop."""
        n, tb = indices.numel(), self.T * B
        if claim is not None:
            return int(claim) if claim > 0 and tb * int(claim) == n else 0
        if tb == 0 or n == 0 or n % tb:
            return 0
        # the verdict is a property of the tensor's CONTENTS: the key carries torch's in-place version counter, so an
        # ``offsets.copy_(...)`` into a persistent buffer (same pointer, same total, now ragged) is looked at again.  Writers
        # that bypass torch (a raw-pointer kernel) must pass ``pooling=``.
        key = (offsets.data_ptr(), offsets.numel(), offsets.dtype, offsets._version, n, B)
        if key != self._pool_key:
            L = n // tb
            ramp = torch.arange(tb, dtype=offsets.dtype, device=offsets.device) * L
            self._pool_key, self._pool_val = key, (L if bool(torch.equal(offsets[:tb], ramp)) else 0)
        return self._pool_val

    def _build_request(self, indices, offsets, B, psw, bag_begin, bag_count, d_ptrs=None, forward: bool = False) -> _lib.pm_embbag_batch:
        _require_device(indices, "indices")
        _require_device(offsets, "offsets")
        if indices.dtype != offsets.dtype or indices.dtype not in _IDTYPE:
            raise TypeError("indices and offsets must both be int64 or both int32")
        if not (indices.is_contiguous() and offsets.is_contiguous()):
            raise ValueError("indices/offsets must be contiguous")
        n_off = offsets.numel()
        if n_off not in (self.T * B, self.T * B + 1):
            raise ValueError(f"offsets has {n_off} entries, expected T*B={self.T * B} (or T*B+1)")
        if psw is not None:
            _require_device(psw, "per_sample_weights")
            if psw.dtype != torch.float32 or psw.numel() != indices.numel() or not psw.is_contiguous():
                raise ValueError("per_sample_weights must be contiguous float32 with one entry per index")
        off_t, stride, _ = self.out_desc(B)
        op = _lib.pm_embbag_batch()
        op.num_tables = self.T
        op.weight_dtype = _WDTYPE[self.dtype]
        op.index_dtype = _IDTYPE[indices.dtype]
        op.max_dim = self.max_dim
        op.min_dim = self.min_dim          # ABI v7: lets the forward pick its lane-group width per table for mixed-dim requests
        op.batch = B
        op.num_indices = indices.numel()
        op.bag_begin = bag_begin
        op.bag_count = B - bag_begin if bag_count is None else bag_count
        op.tables = (self.d_ptrs if d_ptrs is None else d_ptrs).data_ptr()
        op.rows = self.d_rows.data_ptr()
        op.dims = self.d_dims.data_ptr()
        op.out_offsets = off_t.data_ptr()
        op.out_stride = stride
        op.indices = indices.data_ptr()
        op.offsets = offsets.data_ptr()
        op.per_sample_weights = None if psw is None else psw.data_ptr()
        op.fixed_pooling = 0          # filled in by the sorted backward (fixed_pooling()); the forward does not use it
        if self.layout == "blocked":
            Bl, D = self.block_bags, self.dims[0]
            if forward:
                # the same arrays read as T * W request tables of batch Bl (include/param_amd.h, pm_embbag_batch, ABI v6)
                if bag_begin != 0 or (bag_count is not None and bag_count != B) or d_ptrs is not None:
                    raise ValueError("blocked layout: the forward takes whole-batch requests only")
                (tabs, rows_v, dims_v, offs_v), W = self.blocked_forward_arrays(B)
                op.num_tables = self.T * W
                op.batch = Bl
                op.bag_begin, op.bag_count = 0, Bl
                op.tables, op.rows, op.dims, op.out_offsets = tabs.data_ptr(), rows_v.data_ptr(), dims_v.data_ptr(), offs_v.data_ptr()
                op.table_group = W
            else:
                op.grad_block_shift = Bl.bit_length() - 1
                op.grad_block_extra = (self.T - 1) * Bl * D
                if Bl == 1 and self.T > 1:
                    raise ValueError("blocked layout: block_bags must be at least 2")
        return op


def _fwd(ts: _TableSet, indices, offsets, B, psw=None, out=None, bag_begin=0, bag_count=None, split_bags: bool = False,
         pad: Optional[torch.Tensor] = None, mean: bool = False, out16: Optional[torch.dtype] = None):
    """``split_bags``: one workgroup per bag with wave-shuffle / LDS partial reductions (``pm_embbag_fwd_split``) -- for
    few, long bags; agrees with the default kernel to fp32 rounding, not bit for bit.  ``pad``: per-table padding indices
    (device int64 ``[T]``, -1 = none): the padded forward (``pm_embbag_fwd_padded``); ``None``: the call is what it always was.
    ``mean``: mean pooling (``pm_embbag_fwd_mean``: the padded forward's kernel with the division fused; ``pad`` may be ``None``).
    ``out16``: ``torch.bfloat16`` / ``torch.float16``: the output is that dtype (``pm_embbag_fwd_out16``: the padded forward's kernel with
    one rounding fused in front of its stores -- sum, weighted sum or mean, ``pad`` may be ``None``); ``None``: fp32, the calls above."""
    if out16 is not None and (split_bags or ts.layout == "blocked"):
        raise ValueError('a 16-bit output_dtype is not supported with split_bags=True or layout="blocked"')
    if pad is not None and (split_bags or ts.layout == "blocked"):
        raise ValueError('padding_idx is not supported with split_bags=True or layout="blocked"')
    if mean and (split_bags or ts.layout == "blocked" or psw is not None):
        raise ValueError('mean pooling is not supported with split_bags=True, layout="blocked" or per_sample_weights')
    op = ts.request(indices, offsets, B, psw, bag_begin, bag_count, forward=True)
    _, _, shape = ts.out_desc(B)
    odt = torch.float32 if out16 is None else out16
    if out is None:
        out = torch.empty(shape, dtype=odt, device=ts.device)
    elif out.dtype != odt or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {str(odt).replace('torch.', '')} tensor of shape {shape}")
    L = _lib.load()
    if out16 is not None:
        rc = L.pm_embbag_fwd_out16(ctypes.byref(op), None if pad is None else pad.data_ptr(), 1 if mean else 0, _WDTYPE[out16],
                                   out.data_ptr(), _stream_ptr())
    elif mean:
        rc = L.pm_embbag_fwd_mean(ctypes.byref(op), None if pad is None else pad.data_ptr(), out.data_ptr(), _stream_ptr())
    elif pad is not None:
        rc = L.pm_embbag_fwd_padded(ctypes.byref(op), pad.data_ptr(), out.data_ptr(), _stream_ptr())
    else:
        rc = (L.pm_embbag_fwd_split if split_bags else L.pm_embbag_fwd)(ctypes.byref(op), out.data_ptr(), _stream_ptr())
    if rc:
        _lib.check(rc)
    return out


def _fwd_max(ts: _TableSet, indices, offsets, B, out=None, bag_begin=0, bag_count=None, pad: Optional[torch.Tensor] = None,
             out16: Optional[torch.dtype] = None, max_indices=False):
    """MAX pooling (``pm_embbag_fwd_max``: a sibling of the padded forward's kernel; rule in include/param_amd.h, MAX POOLING) ->
    ``(out, max_indices)``.  ``pad`` / ``out16`` / ``out`` / the batch slice: as for ``_fwd``.  ``max_indices``: ``False`` -- not
    written, ``None`` comes back (inference); ``True`` -- a fresh int32 tensor of the output's shape (-1 for the bags outside a batch
    slice); a tensor -- the caller's (contiguous int32 of the output's shape: bags outside the slice keep their bits)."""
    if ts.layout == "blocked":
        raise ValueError('max pooling is not supported with layout="blocked"')
    op = ts.request(indices, offsets, B, None, bag_begin, bag_count, forward=True)
    _, _, shape = ts.out_desc(B)
    odt = torch.float32 if out16 is None else out16
    if out is None:
        out = torch.empty(shape, dtype=odt, device=ts.device)
    elif out.dtype != odt or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {str(odt).replace('torch.', '')} tensor of shape {shape}")
    arg = None
    if max_indices is True:
        whole = bag_begin == 0 and bag_count in (None, B)
        arg = torch.empty(shape, dtype=torch.int32, device=ts.device) if whole else torch.full(shape, -1, dtype=torch.int32, device=ts.device)
    elif max_indices is not False and max_indices is not None:
        arg = max_indices
        if arg.dtype != torch.int32 or tuple(arg.shape) != tuple(shape) or not arg.is_contiguous() or arg.device != ts.device:
            raise ValueError(f"max_indices must be a contiguous int32 tensor of shape {shape} on {ts.device}")
    rc = _lib.load().pm_embbag_fwd_max(ctypes.byref(op), None if pad is None else pad.data_ptr(), _WDTYPE[odt], out.data_ptr(),
                                       None if arg is None else arg.data_ptr(), _stream_ptr())
    if rc:
        _lib.check(rc)
    return out, arg


_MAX_MIXED = "the gradient of max pooling needs one common embedding dim (it is applied by the sequence backward, which takes one)"


def _max_expand(ts: _TableSet, grad, max_indices, indices, offsets, B, bag_begin=0, bag_count=None,
                out16: Optional[torch.dtype] = None) -> torch.Tensor:
    """The gradient of a MAX-pooled forward as a sequence gradient (``pm_embbag_max_grad``): fp32 ``[N, D]`` from torch's allocator,
    row ``j`` = ``grad`` of ``j``'s bag in the columns whose arg-max is ``indices[j]`` and for which ``j`` is the bag's first such
    position, +0.0 elsewhere.  Rows of positions outside the batch slice are not written (the sequence backward of the slice reads
    none of them).  ``grad``: fp32 or the module's 16-bit output dtype ``out16``, widened exactly in the same launch; never modified.
    One launch for any number of tables.  ``N x D`` fp32: 1.34 GB for 16 tables x batch 8192 x pooling 20 x D = 128."""
    if ts.layout == "blocked":
        raise ValueError('max pooling is not supported with layout="blocked"')
    if len(set(ts.dims)) != 1:
        raise ValueError(_MAX_MIXED)
    grad = _check_grad(ts, grad, B, out16)
    if (max_indices.dtype != torch.int32 or tuple(max_indices.shape) != tuple(grad.shape) or not max_indices.is_contiguous() or
            max_indices.device != ts.device):
        raise ValueError(f"max_indices must be a contiguous int32 tensor of shape {tuple(grad.shape)} on {ts.device}")
    n, D = indices.numel(), ts.dims[0]
    op = ts.request(indices, offsets, B, None, bag_begin, bag_count)
    g_seq = torch.empty((n, D), dtype=torch.float32, device=ts.device)
    if n:
        rc = _lib.load().pm_embbag_max_grad(ctypes.byref(op), grad.data_ptr(), _WDTYPE[grad.dtype], max_indices.data_ptr(), g_seq.data_ptr(),
                                            D, _stream_ptr())
        if rc:
            _lib.check(rc)
    return g_seq


def _max_bwd(ts: _TableSet, grad, indices, offsets, B, dst_ptrs_dev, dst_dtype, alpha, pad: Optional[torch.Tensor] = None, max_indices=None,
             bag_begin=0, bag_count=None, out16: Optional[torch.dtype] = None) -> None:
    """The backward of a MAX-pooled forward: ``dst_t[max_indices(t, b)[c], c] += alpha * grad(t, b)[c]``, deterministic.  No apply
    kernel of its own: the gradient is expanded to one row per lookup position (``_max_expand``) and the sequence backward of the same
    request (``_seq_bwd``: ``pm_embseq_bwd_fused``, 1024 tables per call) applies it, so a table row accumulates its bags' contributions
    in ascending bag order.  ``max_indices=None``: recomputed by one forward launch into a scratch.  ``pad``: the padding rows of the
    destinations keep their bits (``_PadGuard``).  A looked-up row that wins no column receives additions of ``alpha * 0.0``."""
    if len(set(ts.dims)) != 1:
        raise ValueError(_MAX_MIXED)
    if max_indices is None:
        _check_grad(ts, grad, B, out16)      # (refused before the forward launch)
        _, max_indices = _fwd_max(ts, indices, offsets, B, None, bag_begin, bag_count, pad, None, True)
    g_seq = _max_expand(ts, grad, max_indices, indices, offsets, B, bag_begin, bag_count, out16)
    L, s, dt, D = _lib.load(), _stream_ptr(), _WDTYPE[dst_dtype], ts.dims[0]

    def call(fn):
        return lambda sub, gp, t0, max_rows, ws: fn(ctypes.byref(sub), gp, D, dst_ptrs_dev.data_ptr() + 8 * t0, dt, float(alpha), max_rows,
                                                    ws.data_ptr(), ws.numel(), s)
    _seq_bwd(ts, g_seq, indices, offsets, B, bag_begin, bag_count, False, call(L.pm_embseq_bwd_fused), call(L.pm_embseq_bwd_sorted),
             _PadGuard(ts, pad, dst_ptrs_dev, dst_dtype))


def _fwd_quantized(ts: _TableSet, indices, offsets, B, bitwidth: int, psw=None, out=None, bag_begin=0, bag_count=None):
    """Forward whose output is row-wise quantised (``pm_embbag_fwd_quantized``): one quantised row per pooled vector, in
    the order of the fp32 layout.  Returns a uint8 tensor ``[*shape[:-1] as rows, row_bytes]`` -- ``(B, T, rb)`` for the
    ``bd`` layout, ``(T, B, rb)`` for ``tbd``.  Requests the staged kernel does not take (ragged bags) are served by the
    fp32 forward + ``pm_rows_quantize``: same bytes, one more pass."""
    from . import quant
    if len(set(ts.dims)) != 1:
        raise ValueError("quantised output needs one common embedding dim")
    D = ts.dims[0]
    rb = quant.host_row_bytes(D, bitwidth)
    if D % 8 or D > 512:
        raise ValueError(f"quantised output needs an embedding dim that is a multiple of 8 and <= 512, got {D}")
    qshape = ((B, ts.T, rb) if ts.layout == "bd" else (ts.T, B, rb) if ts.layout == "tbd" else
              (B // ts.block_bags, ts.T, ts.block_bags, rb))
    if out is None:
        out = torch.empty(qshape, dtype=torch.uint8, device=ts.device)
    elif out.dtype != torch.uint8 or out.numel() != B * ts.T * rb or not out.is_contiguous() or out.device != ts.device:
        raise ValueError(f"out must be a contiguous uint8 tensor of {B * ts.T * rb} bytes on {ts.device}")
    op = ts.request(indices, offsets, B, psw, bag_begin, bag_count, forward=True)
    L = _lib.load()
    rc = L.pm_embbag_fwd_quantized(ctypes.byref(op), out.data_ptr(), int(bitwidth), _stream_ptr())
    if rc == _lib.PM_ERR_UNSUPPORTED and (bag_begin, bag_count) in ((0, None), (0, B)):
        full = _fwd(ts, indices, offsets, B, psw)
        quant.quantize_rows(full, D, bitwidth, out=out)
        return out
    _lib.check(rc)
    return out


def _check_rows_out(out: torch.Tensor, n: int, D: int, odt: torch.dtype, device) -> None:
    """a caller's ``out`` of the un-pooled lookup: contiguous ``[n, D]`` of ``odt`` on ``device`` (checked before anything runs)"""
    if out.dtype != odt or tuple(out.shape) != (n, D) or not out.is_contiguous() or out.device != device:
        raise ValueError(f"out must be a contiguous {str(odt).replace('torch.', '')} tensor of shape {(n, D)} on {device}")


def _gather(ts: _TableSet, indices, offsets, B, odt: torch.dtype, out=None, bag_begin=0, bag_count=None) -> torch.Tensor:
    """Un-pooled rows (``pm_embedding_gather``): ``[N, D]`` of ``odt``, row ``j`` = row ``indices[j]`` of the table that owns position
    ``j`` -- the stored bits when ``odt`` is the tables' dtype, widened exactly or rounded once otherwise.  Needs one common embedding
    dim.  With a batch slice only the rows of positions inside it are written: a caller's ``out`` keeps the others, a tensor
    allocated here holds zeros there.  No launch for an empty request."""
    D, n = ts.dims[0], indices.numel()
    op = ts.request(indices, offsets, B, None, bag_begin, bag_count)
    if out is None:
        whole = bag_begin == 0 and bag_count in (None, B)
        out = (torch.empty if whole else torch.zeros)((n, D), dtype=odt, device=ts.device)
    else:
        _check_rows_out(out, n, D, odt, ts.device)
    if n:
        rc = _lib.load().pm_embedding_gather(ctypes.byref(op), _WDTYPE[odt], out.data_ptr(), D, _stream_ptr())
        if rc:
            _lib.check(rc)
    return out


def _workspace(ts: _TableSet, op, max_rows: Optional[int] = None, query=None) -> torch.Tensor:
    """Scratch for the sort-based backward, cached on the table set (grown, never shrunk).  ``max_rows``: of the tables ``op``
    names, when it is a table range of the set's request.  ``query``: the size function (default
    ``pm_embbag_bwd_sorted_workspace``; the sparse gradient has its own)."""
    query = query or _lib.load().pm_embbag_bwd_sorted_workspace
    return ts.scratch("_ws", query(ctypes.byref(op), max(ts.rows) if max_rows is None else max_rows))


def _sort_issued(ts: _TableSet, ws: torch.Tensor) -> None:
    """a key sort (on its own, or inside a fused call) has been issued on the table set's workspace ``ws``"""
    ts._ws_sorted = ws.data_ptr()


_NOT_SORTED = {False: "pm_embbag_sort_indices has not been called for this request on this workspace (same indices / offsets pointers, "
                      "batch, bag slice and weights as the sort's)",
               True: "pm_embseq_sort_indices has not been called for this request on this workspace (same indices / offsets pointers, "
                     "batch and bag slice as the sort's)"}


def _require_sort(ts: _TableSet, ws: torch.Tensor, sequence: bool = False) -> None:
    """``presorted=True`` on a workspace this table set has not sorted on: refused here, with the library's text.  The library keeps its
    record of the last sort by the workspace's ADDRESS, and torch's caching allocator hands the address of a freed workspace out again:
    to the fresh workspace of another table set, the record of a sort of the very same request tensors that a module since freed issued
    there would pass for its own -- and the apply would read whatever the block holds now.  (A C caller owns its workspaces and the
    order of its calls; here the workspace's lifetime is this layer's.)"""
    if ts.__dict__.get("_ws_sorted") != ws.data_ptr():
        raise _lib.ParamAmdError(_lib.PM_ERR_INVALID, _NOT_SORTED[sequence])


def _check_grad(ts: _TableSet, grad, B, out16: Optional[torch.dtype] = None) -> torch.Tensor:
    """the gradient of a batch of B bags in the table set's output layout, contiguous: fp32 (always), or the module's 16-bit output
    dtype ``out16``"""
    _require_device(grad, "grad")
    _, _, shape = ts.out_desc(B)
    if (grad.dtype != torch.float32 and (out16 is None or grad.dtype != out16)) or tuple(grad.shape) != tuple(shape):
        also = "" if out16 is None else f" or {str(out16).replace('torch.', '')} (the module's output_dtype)"
        raise ValueError(f"grad must be float32{also} of shape {shape}")
    return grad.contiguous()


def _output_dtype(spec) -> torch.dtype:
    """``output_dtype`` of the two modules as a torch dtype: ``None`` / ``torch.float32`` (fp32, the default), ``torch.bfloat16``,
    ``torch.float16``, the strings ``"fp32"`` / ``"bf16"`` / ``"fp16"`` in any case, or an enum member whose ``value`` or ``name`` is one
    of those (fbgemm's ``SparseType``, read by shape).  Anything else raises ValueError.  Needs no device."""
    names = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
    if spec is None:
        return torch.float32
    if isinstance(spec, torch.dtype) and spec in names.values():
        return spec
    for key in (spec, getattr(spec, "value", None), getattr(spec, "name", None)):
        if isinstance(key, str) and key.lower() in names:
            return names[key.lower()]
    raise ValueError(f"output_dtype must be None, torch.float32, torch.bfloat16, torch.float16, one of fp32 / bf16 / fp16 (any case) or "
                     f"an enum member of that value or name (fbgemm's SparseType), got {spec!r}")


def _widen(ts: _TableSet, grad, indices, offsets, B, psw, pad: Optional[torch.Tensor], mean: bool, bag_begin=0, bag_count=None) -> torch.Tensor:
    """A bf16 / fp16 gradient as the fp32 gradient of a SUM forward (``pm_embbag_grad_widen``): a scratch of ``grad``'s shape from torch's
    allocator holding ``float(grad(t, b))`` for the bags of the slice -- with ``mean`` times ``1.0f / count(t, b)`` in the same launch,
    which is ``_mean_scale`` of the widened gradient bit for bit.  Bags outside the slice are not written (no backward reads them);
    ``grad`` itself is never modified.  One launch for any number of tables.  ``psw`` only keeps the cached request descriptor of the
    backward that follows: the call reads no weights."""
    if ts.layout == "blocked":
        raise ValueError('a 16-bit gradient is not supported with layout="blocked"')
    op = ts.request(indices, offsets, B, psw, bag_begin, bag_count)
    wide = torch.empty(grad.shape, dtype=torch.float32, device=grad.device)
    rc = _lib.load().pm_embbag_grad_widen(ctypes.byref(op), None if pad is None else pad.data_ptr(), 1 if mean else 0, _WDTYPE[grad.dtype],
                                          grad.data_ptr(), wide.data_ptr(), _stream_ptr())
    if rc:
        _lib.check(rc)
    return wide


_MEAN_WEIGHTED = "mean pooling is unweighted: per_sample_weights must be None (fbgemm's weighted mean is not implemented)"


def _mean_scale(ts: _TableSet, grad, indices, offsets, B, pad: Optional[torch.Tensor] = None, bag_begin=0, bag_count=None) -> torch.Tensor:
    """The gradient of a MEAN-pooled forward as the gradient of its sum (``pm_embbag_mean_grad``): a scratch of ``grad``'s shape from
    torch's allocator holding ``grad(t, b) * (1.0f / count(t, b))`` for the bags of the slice (+0.0 for a bag without kept lookups;
    bags outside the slice are not written -- no backward reads them).  ``grad`` itself is never modified.  One launch for any
    number of tables; every backward route then runs unchanged on the result."""
    if ts.layout == "blocked":
        raise ValueError('mean pooling is not supported with layout="blocked"')
    grad = _check_grad(ts, grad, B)
    op = ts.request(indices, offsets, B, None, bag_begin, bag_count)
    scaled = torch.empty_like(grad)
    rc = _lib.load().pm_embbag_mean_grad(ctypes.byref(op), None if pad is None else pad.data_ptr(), grad.data_ptr(), scaled.data_ptr(),
                                         _stream_ptr())
    if rc:
        _lib.check(rc)
    return scaled


def _grad_as_sum(ts: _TableSet, grad, indices, offsets, B, psw, pad, mean: bool, bag_begin=0, bag_count=None,
                 out16: Optional[torch.dtype] = None) -> torch.Tensor:
    """The gradient of the module's forward as the fp32 gradient of a SUM forward of the same request, which is what every backward
    route below takes: ``grad`` itself for sum pooling, its scaled copy (``_mean_scale``) for mean pooling -- which is unweighted.  A
    gradient in the module's 16-bit output dtype ``out16`` is widened once (``_widen``), the mean scaling fused into that launch."""
    if out16 is not None:
        grad = _check_grad(ts, grad, B, out16)      # (fp32 or out16: any other dtype is refused here, by the module's own rule)
        if grad.dtype == out16:
            if mean and psw is not None:
                raise ValueError(_MEAN_WEIGHTED)
            return _widen(ts, grad, indices, offsets, B, psw, pad, mean, bag_begin, bag_count)
    if not mean:
        return grad
    if psw is not None:
        raise ValueError(_MEAN_WEIGHTED)
    return _mean_scale(ts, grad, indices, offsets, B, pad, bag_begin, bag_count)


def _sort_indices(ts: _TableSet, indices, offsets, B, psw=None, bag_begin=0, bag_count=None, phases: int = 2,
                  pooling: Optional[int] = None) -> None:
    """Step 1+2 of the deterministic backward (keys + stable radix sort): needs only the request,
    so it can be issued early / on another stream; ``_bwd(..., presorted=True)`` consumes it.  A sort issued on its own is
    always COMPLETE (the request's index buffer may be reused once it has run); the hybrid backward, which defers part of the
    sort into the apply and reads the indices again there, is taken by the fused calls only (``_bwd`` / ``_adagrad`` without
    ``presorted``).  ``phases=2`` (scatter-add /
    SGD apply) lets the apply run in two bag phases where the request allows; the fused row-wise Adagrad needs ``phases=1``."""
    _no_presorted_split(ts, True)
    op = ts.request(indices, offsets, B, psw, bag_begin, bag_count)
    op.fixed_pooling = ts.fixed_pooling(indices, offsets, B, pooling) if _lib.needs_pooling_hint() else 0
    ws = _workspace(ts, op)
    _lib.check(_lib.load().pm_embbag_sort_indices_ex(ctypes.byref(op), max(ts.rows), phases, ws.data_ptr(), ws.numel(),
                                                     _stream_ptr()))
    _sort_issued(ts, ws)


def sort_plan(ts: _TableSet, indices, offsets, B, psw=None, bag_begin=0, bag_count=None, phases: int = 1,
              pooling: Optional[int] = None) -> str:
    """one-line description of the layout the sort would choose for this request (``pm_embbag_sort_plan``; host-only)"""
    op = ts.request(indices, offsets, B, psw, bag_begin, bag_count)
    op.fixed_pooling = 0 if pooling is None else int(pooling)
    buf = ctypes.create_string_buffer(1024)
    _lib.check(_lib.load().pm_embbag_sort_plan(ctypes.byref(op), max(ts.rows), phases, buf, 1024))
    return buf.value.decode()


def sorted_pairs(ts: _TableSet, indices, offsets, B, psw=None, bag_begin=0, bag_count=None):
    """(keys, values, tshift) of the last ``_sort_indices`` on this table set's workspace, as torch tensors copied off the
    workspace (``pm_embbag_sorted_pairs``) -- for tests and tools; synchronises."""
    op = ts.request(indices, offsets, B, psw, bag_begin, bag_count)
    ws = _workspace(ts, op)
    vp = ctypes.c_void_p
    keys, vals, cnt, kb, tsh = vp(), vp(), vp(), ctypes.c_int32(), ctypes.c_int32()
    _lib.check(_lib.load().pm_embbag_sorted_pairs(ctypes.byref(op), max(ts.rows), ws.data_ptr(), ctypes.byref(keys), ctypes.byref(vals),
                                                  ctypes.byref(cnt), ctypes.byref(kb), ctypes.byref(tsh)))
    torch.cuda.synchronize()
    base = ws.data_ptr()
    n = indices.numel()
    if cnt.value:
        n = int(ws[cnt.value - base:cnt.value - base + 4].view(torch.int32)[0].item()) & 0xffffffff
    kdt = torch.int32 if kb.value == 4 else torch.int64
    k = ws[keys.value - base:keys.value - base + n * kb.value].view(kdt).clone()
    v = ws[vals.value - base:vals.value - base + n * 4].view(torch.int32).clone()
    return k, v, tsh.value


def sort_status(ts: _TableSet, indices, offsets, B, psw=None, bag_begin=0, bag_count=None) -> dict:
    """What the last ``_sort_indices`` / backward on this table set's workspace left on the device (``pm_embbag_sort_status``;
    SYNCHRONISES): ``lookback_fallbacks`` (look-back walks that counted a predecessor's digits themselves: harmless),
    ``pairs_sorted``, ``hybrid_tables``, ``hybrid_launched``, ``lds_pairs`` / ``lds_tables`` (flagged lookups / hybrid tables finished
    inside LDS by the left-over kernel: they never reach the sort)."""
    op = ts.request(indices, offsets, B, psw, bag_begin, bag_count)
    ws = _workspace(ts, op)
    st = _lib.pm_sort_status()
    _lib.check(_lib.load().pm_embbag_sort_status(ctypes.byref(op), max(ts.rows), ws.data_ptr(), ctypes.byref(st), _stream_ptr()))
    return {"lookback_fallbacks": st.lookback_fallbacks, "pairs_sorted": st.pairs_sorted, "hybrid_tables": st.hybrid_tables,
            "hybrid_launched": st.hybrid_launched, "lds_pairs": st.lds_pairs, "lds_tables": st.lds_tables}


_SORTED_MAX_TABLES = 1024      # kSegSortMaxTables: the sorted path's limit per call; larger requests are split by tables


def _table_chunks(ts: _TableSet, op, indices, offsets, B, psw=None):
    """The request ``op`` as sub-requests of at most 1024 tables each, in table order: ``(sub, t0, t1, max_rows)`` per range
    [t0, t1).  The lookups of a table range are one contiguous stretch of the table-major index array: its offsets are rebased to
    that stretch, ``tables`` / ``rows`` / ``dims`` / ``out_offsets`` are the range's slice of the request's own device arrays, the index and
    weight pointers are advanced, ``max_dim`` / ``min_dim`` are the range's; the gradient and its addressing (stride, blocking, batch
    slice) stay the full request's.  A caller that passes its own per-table pointer arrays (destinations, optimizer state) slices
    them ``[t0:t1]`` the same way.  A request within the limit comes back as it is (no copy, no synchronisation); a larger one
    costs one small device-to-host read of the offsets at the cuts."""
    T = ts.T
    if T <= _SORTED_MAX_TABLES:
        yield op, 0, T, max(ts.rows)
        return
    cuts = list(range(0, T, _SORTED_MAX_TABLES)) + [T]
    n = indices.numel()
    if B == 0:
        starts = [0] * len(cuts)
    else:
        starts = offsets[[c * B for c in cuts[:-1]]].tolist() + [n]
    esz = {"tables": 8, "rows": 8, "dims": 4, "out_offsets": 8}
    for t0, t1, n0, n1 in zip(cuts[:-1], cuts[1:], starts[:-1], starts[1:]):
        sub = _lib.pm_embbag_batch.from_buffer_copy(op)
        sub_off = (offsets[t0 * B:t1 * B] - n0).contiguous()
        sub.num_tables = t1 - t0
        sub.max_dim, sub.min_dim = max(ts.dims[t0:t1]), min(ts.dims[t0:t1])
        sub.num_indices = n1 - n0
        for name, e in esz.items():
            setattr(sub, name, getattr(op, name) + t0 * e)
        sub.indices = indices.data_ptr() + n0 * indices.element_size()
        sub.offsets = sub_off.data_ptr()
        if psw is not None:
            sub.per_sample_weights = psw.data_ptr() + n0 * psw.element_size()
        # (sub_off is referenced until the consumer has launched this range's kernels on the current stream; the caching allocator
        # reuses its memory in stream order only)
        yield sub, t0, t1, max(ts.rows[t0:t1])
        del sub_off


def _no_presorted_split(ts, presorted: bool) -> None:
    """``sort_indices`` + ``presorted=True`` keep ONE sort in the cached workspace: refused, on the host, for requests that need several"""
    if presorted and ts.T > _SORTED_MAX_TABLES:
        raise ValueError(f"presorted=True takes requests of at most {_SORTED_MAX_TABLES} tables (this one has {ts.T}): a larger request "
                         "runs as several sorted calls that share one workspace, which cannot hold several sorts at once; call "
                         "without presorted (the sort then runs inside the call, once per 1024 tables)")


def _bwd(ts: _TableSet, grad, indices, offsets, B, dst_ptrs_dev, dst_dtype, alpha, psw=None,
         bag_begin=0, bag_count=None, method: str = "sorted", presorted: bool = False, pooling: Optional[int] = None,
         pad: Optional[torch.Tensor] = None, mean: bool = False, out16: Optional[torch.dtype] = None):
    """``method="sorted"`` (default): deterministic, bit-identical to a sequential scatter-add;
    ``method="atomic"``: hardware float atomics (order not fixed; tests / tools: the alternates build).
    ``pad``: per-table padding indices (device int64 ``[T]``): those rows of the destinations are saved before and restored
    after the call (``_PadGuard``) -- once, around all table ranges of a large request; a call refused on the host launches neither.
    ``mean``: ``grad`` is the gradient of a mean-pooled forward: scaled once (``_grad_as_sum``), then everything below as it is.
    ``out16``: the module's 16-bit output dtype: a gradient of that dtype is widened once (``_grad_as_sum``)."""
    grad = _check_grad(ts, _grad_as_sum(ts, grad, indices, offsets, B, psw, pad, mean, bag_begin, bag_count, out16), B)
    if method not in ("sorted", "atomic"):
        raise ValueError('method must be "sorted" or "atomic"')
    if method == "sorted":
        _no_presorted_split(ts, presorted)
    op = ts.request(indices, offsets, B, psw, bag_begin, bag_count)
    dst_dt, s, g = _WDTYPE[dst_dtype], _stream_ptr(), grad.data_ptr()
    guard = _PadGuard(ts, pad, dst_ptrs_dev, dst_dtype)
    guard.save()
    if method == "atomic":
        # the atomic kernel is a measured baseline and a cross-check (25 x slower): it lives in the ALTERNATES build only
        # (libparam_amd_alt.so, `make -C param_amd/csrc alt`; ImportError if that is not built)
        A = _lib.load_alternates()
        rc = A.pm_embbag_bwd(ctypes.byref(op), g, dst_ptrs_dev.data_ptr(), dst_dt, float(alpha), s)
        if rc != _lib.PM_OK:
            raise _lib.ParamAmdError(rc, A.pm_last_error().decode())
    else:
        L = _lib.load()

        def call(fn):      # the fused and the sorted call take the same arguments
            return lambda sub, t0, max_rows, ws: fn(ctypes.byref(sub), g, dst_ptrs_dev.data_ptr() + 8 * t0, dst_dt, float(alpha), max_rows,
                                                    ws.data_ptr(), ws.numel(), s)
        # (the alternative key sorts may lay out two bag phases for the scatter-add apply)
        _sorted_chunks_call(ts, op, indices, offsets, B, psw, presorted, pooling, 2, call(L.pm_embbag_bwd_fused), call(L.pm_embbag_bwd_sorted))
    guard.restore()


def _sorted_chunks_call(ts: _TableSet, op, indices, offsets, B, psw, presorted: bool, pooling, phases: int, fused, sorted_) -> None:
    """The sorted backward of the request ``op``, one call per range of at most 1024 tables, in table order on this stream, sharing
    the cached workspace.  ``fused(sub, t0, max_rows, ws)`` issues the fused call (sort + apply) of a range, ``sorted_`` the apply
    of a sorted one; both return the library's code.  ``phases``: what a sort issued here may lay out (2: scatter-add, 1: Adagrad)."""
    L, s = _lib.load(), _stream_ptr()
    for sub, t0, t1, max_rows in _table_chunks(ts, op, indices, offsets, B, psw):
        ws = _workspace(ts, sub, max_rows)
        if not presorted and not _lib.needs_pooling_hint():
            # sort + apply sequenced by the library itself: the one form in which it may defer part of the sort into the apply
            # (hybrid backward: rows looked up once skip the sort)
            sub.fixed_pooling = 0  # (the cached descriptor may carry a hint from an alternates-build run: the segmented sort takes none)
            _lib.check(fused(sub, t0, max_rows, ws))
            _sort_issued(ts, ws)
            continue
        if not presorted:      # the alternative key sorts (sort_impl 1 / 2) read a pooling hint and may lay out two bag phases
            sub.fixed_pooling = ts.fixed_pooling(indices, offsets, B, pooling) if sub is op else 0
            _lib.check(L.pm_embbag_sort_indices_ex(ctypes.byref(sub), max_rows, phases, ws.data_ptr(), ws.numel(), s))
            _sort_issued(ts, ws)
        else:
            _require_sort(ts, ws)
        _lib.check(sorted_(sub, t0, max_rows, ws))


def _seq_sort_indices(ts: _TableSet, indices, offsets, B, bag_begin=0, bag_count=None) -> None:
    """The key sort of a SEQUENCE request (``pm_embseq_sort_indices``): every table's keys from the index array, the value the lookup's
    position.  Needs only the request; ``_seq_bwd(..., presorted=True)`` consumes it.  One sort per cached workspace: at most 1024
    tables."""
    _no_presorted_split(ts, True)
    if not indices.numel():
        return
    op = ts.request(indices, offsets, B, None, bag_begin, bag_count)
    op.fixed_pooling = 0
    ws = _workspace(ts, op)
    _lib.check(_lib.load().pm_embseq_sort_indices(ctypes.byref(op), max(ts.rows), ws.data_ptr(), ws.numel(), _stream_ptr()))
    _sort_issued(ts, ws)


def _seq_bwd(ts: _TableSet, grad, indices, offsets, B, bag_begin, bag_count, presorted: bool, fused, sorted_, guard: _PadGuard) -> None:
    """The sequence backward of the request, one call per range of at most 1024 tables, in table order on this stream, sharing the
    cached workspace.  ``grad``: contiguous fp32 ``[N, D]``, row ``j`` the gradient of lookup position ``j``; a table range's positions
    start at its first lookup ``n0`` (``_table_chunks`` rebases its offsets and advances its index pointer), so its gradient pointer is
    advanced by ``n0 * D`` elements.  ``fused(sub, g, t0, max_rows, ws)`` issues sort + apply of a range with the gradient at ``g``,
    ``sorted_`` the apply of a sorted one; both return the library's code.  ``guard`` goes around all ranges."""
    _no_presorted_split(ts, presorted)
    if not indices.numel():
        return
    op = ts.request(indices, offsets, B, None, bag_begin, bag_count)
    op.fixed_pooling = 0
    D, base, esz = ts.dims[0], indices.data_ptr(), indices.element_size()
    if presorted:      # (at most 1024 tables: one range, the whole request's workspace; refused before the guard launches anything)
        _require_sort(ts, _workspace(ts, op), True)
    guard.save()
    for sub, t0, _, max_rows in _table_chunks(ts, op, indices, offsets, B):
        ws = _workspace(ts, sub, max_rows)
        n0 = ((sub.indices or 0) - base) // esz
        _lib.check((sorted_ if presorted else fused)(sub, grad.data_ptr() + n0 * D * 4, t0, max_rows, ws))
        if not presorted:
            _sort_issued(ts, ws)
    guard.restore()


def check_request(ts: _TableSet, indices, offsets, B, psw=None) -> None:
    """Raise IndexError / ValueError like torch does on the CPU path for out-of-range
    indices or non-monotone offsets (synchronises: not for timed loops)."""
    op = ts.request(indices, offsets, B, psw, 0, None)
    err = torch.zeros(1, dtype=torch.int32, device=ts.device)
    _lib.check(_lib.load().pm_embbag_check(ctypes.byref(op), err.data_ptr(), _stream_ptr()))
    n = int(err.item())
    if n:
        raise IndexError(f"param_amd: {n} out-of-range indices / invalid offsets in EmbeddingBag request")


_BOUNDS_MODES = {"fatal": _lib.PM_BOUNDS_FATAL, "warning": _lib.PM_BOUNDS_WARNING, "ignore": _lib.PM_BOUNDS_IGNORE, "none": 0}
_FBGEMM_BOUNDS_INTS = {0: "fatal", 1: "warning", 2: "ignore", 3: "none"}      # fbgemm_gpu's BoundsCheckMode values


def _mode_name(mode, ints: dict, names, what: str) -> str:
    """an fbgemm-style enum argument as one of ``names``: such a name in any case, an enum member (read by its ``name``) or its int
    (``ints``: int -> name); anything else raises ValueError(``what``, got ...)"""
    name = getattr(mode, "name", None)
    if isinstance(name, str):
        key = name.lower()
    elif isinstance(mode, str):
        key = mode.lower()
    elif isinstance(mode, int) and not isinstance(mode, bool):
        key = ints.get(mode)
    else:
        key = None
    if key not in names:
        raise ValueError(f"{what}, got {mode!r}")
    return key


def bounds_check_mode_name(mode) -> str:
    """``"fatal" | "warning" | "ignore" | "none"`` from what a caller of fbgemm's TBE module passes as ``bounds_check_mode``: one of
    those names in any case, a ``BoundsCheckMode`` member (read by its name) or its int (FATAL 0, WARNING 1, IGNORE 2, NONE 3);
    ``None`` is ``"none"``.  Anything else raises ValueError."""
    if mode is None:
        return "none"
    return _mode_name(mode, _FBGEMM_BOUNDS_INTS, _BOUNDS_MODES, "bounds_check_mode must be one of fatal / warning / ignore / none "
                      "(any case, fbgemm's BoundsCheckMode members or their ints 0 .. 3)")


_FBGEMM_POOLING_INTS = {0: "sum", 1: "mean", 2: "none"}      # fbgemm_gpu's PoolingMode values


def pooling_mode_name(mode) -> str:
    """``"sum" | "mean"`` from what a caller of fbgemm's TBE module passes as ``pooling_mode``: one of those names in any case, a
    ``PoolingMode`` member (read by its name) or its int (SUM 0, MEAN 1).  ``NONE`` / 2 (no pooling: one output row per lookup) and
    anything else raise ValueError (max pooling, which fbgemm's enum does not have, is :class:`MaxBatchedEmbeddingBagMI355`).  Needs no
    device."""
    return _mode_name(mode, _FBGEMM_POOLING_INTS, ("sum", "mean"), "pooling_mode must be sum or mean (any case, fbgemm's "
                      "PoolingMode.SUM / MEAN or their ints 0 / 1; PoolingMode.NONE is not implemented)")


def _bounds_report_dict(report: torch.Tensor) -> dict:
    """the device report of ``pm_embbag_bounds_check`` as a dict (synchronises); PM_BOUNDS_NONE -> None"""
    bi, bo, fi, fo = report.tolist()
    none = _lib.PM_BOUNDS_NONE
    return {"bad_indices": bi, "bad_offsets": bo, "first_bad_index": None if fi == none else fi,
            "first_bad_offset": None if fo == none else fo}


def _bounds_check(ts: _TableSet, indices, offsets, B, mode: str, report: Optional[torch.Tensor], psw=None, bag_begin=0,
                  bag_count=None) -> None:
    """``pm_embbag_bounds_check`` on the whole request (the plain descriptor: T tables, batch B -- also for ``layout="blocked"``),
    stream-ordered, no synchronisation.  ``psw`` / ``bag_begin`` / ``bag_count`` only keep the cached descriptor of the lookup that
    follows; the call reads none of them.  ``report``: int64[4] on the device (``"ignore"``: not used).  Memory the call repairs is
    written behind torch's back: the caller drops what it remembers about the request's contents (``_contents_changed``)."""
    op = ts.request(indices, offsets, B, psw, bag_begin, bag_count)
    L = _lib.load()
    scratch = ts.scratch("_bounds_scratch", L.pm_embbag_bounds_check_scratch(ctypes.byref(op)), torch.int64)
    flags = _BOUNDS_MODES[mode] | (_lib.PM_BOUNDS_LAST_OFFSET if offsets.numel() == ts.T * B + 1 else 0)
    if report is not None and ts.T * B == 0:
        report.copy_(torch.tensor([0, 0, _lib.PM_BOUNDS_NONE, _lib.PM_BOUNDS_NONE], dtype=torch.int64))     # nothing is launched for no bags
    rc = L.pm_embbag_bounds_check(ctypes.byref(op), flags, None if report is None or mode == "ignore" else report.data_ptr(),
                                  scratch.data_ptr(), scratch.numel() * 8, _stream_ptr())
    if rc:
        _lib.check(rc)


class _BoundsChecked:
    """What the two modules share: ``bounds_check_mode``, described below, and the plumbing of ``padding_idx`` (``_pad_dev``).

    ``bounds_check_mode`` of the two modules (fbgemm TBE's constructor argument): with a mode other than ``"none"`` every
    ``forward`` / ``lookup`` first runs the device-side sanitiser (``pm_embbag_bounds_check``; rule in include/param_amd.h) on the
    caller's ``indices`` / ``offsets``, so that the lookup and -- through the tensors autograd saved -- the backward see the repaired
    request.  The other standalone entry points (``scatter_add_``, ``adagrad_step_``, ``dense_grad``, ``sparse_grad``,
    ``per_sample_weights_grad``, ``sort_indices``, ``lookup_quantized``) do NOT call it: run ``sanitize_`` in front of them.

    * ``"none"`` (default): no launch, no byte touched.
    * ``"ignore"``: repair in place.
    * ``"warning"``: repair in place and keep the report on the device; ``bounds_report()`` synchronises and returns the last call's.
    * ``"fatal"``: dry run, ONE synchronisation, then ``IndexError`` naming counts and first positions; the caller's tensors are
      untouched and no lookup kernel is issued.
    """

    _TABLES = "weight"      # the nn.Parameter that holds the tables: where they live is where the pad array goes

    def _init_shared(self, bounds_check_mode, output_dtype=None) -> None:
        self.bounds_check_mode = bounds_check_mode_name(bounds_check_mode)
        self.output_dtype = _output_dtype(output_dtype)
        self._out16 = None if self.output_dtype == torch.float32 else self.output_dtype      # what the host layer is handed
        self._bounds_report: Optional[torch.Tensor] = None
        self._bounds_reported = False
        self._seen: dict = {}      # what the module remembers about the CONTENTS of request tensors (dropped by _contents_changed)
        self._pad_t: Optional[torch.Tensor] = None

    def _pad_dev(self) -> Optional[torch.Tensor]:
        """``padding_idx`` as the kernels take it (device int64 ``[T]``, -1 = the table has none), or None"""
        pads = self.padding_idx
        if pads is None:
            return None
        dev = self._parameters[self._TABLES].device
        if self._pad_t is None or self._pad_t.device != dev:
            self._pad_t = _pad_tensor(pads if isinstance(pads, list) else [pads], dev)
        return self._pad_t

    def _contents_changed(self, ts: _TableSet) -> None:
        """the request's bytes were rewritten behind torch's back (no version counter moved): every memo about them goes -- the
        table set's fixed-pooling verdict and whatever the module keeps in ``_seen``"""
        ts._pool_key = None
        self._seen.clear()

    def _sanitize(self, ts: _TableSet, indices, offsets, B, mode: str, psw=None, bag_begin=0, bag_count=None) -> None:
        rep = None
        if mode != "ignore":
            rep = self._bounds_report
            if rep is None or rep.device != ts.device:
                rep = self._bounds_report = torch.empty(4, dtype=torch.int64, device=ts.device)
        _bounds_check(ts, indices, offsets, B, mode, rep, psw, bag_begin, bag_count)
        self._bounds_reported = rep is not None
        if mode != "fatal":
            self._contents_changed(ts)
            return
        r = _bounds_report_dict(rep)
        if r["bad_indices"] or r["bad_offsets"]:
            raise IndexError(f"param_amd: bounds_check_mode=fatal: {r['bad_indices']} out-of-range indices (first at position "
                             f"{r['first_bad_index']}), {r['bad_offsets']} invalid offsets (first at position {r['first_bad_offset']}) "
                             "in EmbeddingBag request")

    def bounds_report(self) -> Optional[dict]:
        """What the last sanitiser call of this module found (``"warning"`` and ``"fatal"`` calls; synchronises):
        ``{"bad_indices", "bad_offsets", "first_bad_index", "first_bad_offset"}``, the positions ``None`` without a finding.
        ``None`` when the last call kept no report (``"ignore"``) or none has run."""
        if not self._bounds_reported or self._bounds_report is None:
            return None
        return _bounds_report_dict(self._bounds_report)


_WD_MODES = {None: _lib.PM_WD_NONE, "none": _lib.PM_WD_NONE, 0: _lib.PM_WD_NONE, "l2": _lib.PM_WD_L2, 1: _lib.PM_WD_L2,
             "decouple": _lib.PM_WD_DECOUPLE, "decoupled": _lib.PM_WD_DECOUPLE, 2: _lib.PM_WD_DECOUPLE}


def _adagrad(ts: _TableSet, grad, indices, offsets, B, mom_ptrs_dev, lr: float, eps: float, psw=None,
             presorted: bool = False, weight_decay: float = 0.0, weight_decay_mode=None, stochastic_rounding: bool = False,
             seed: int = 0, pooling: Optional[int] = None, elementwise: bool = False, pad: Optional[torch.Tensor] = None,
             mean: bool = False, out16: Optional[torch.dtype] = None):
    """Fused backward + exact row-wise Adagrad on the tables of ``ts`` (``pm_embbag_bwd_sorted_adagrad_ex``), or, with
    ``elementwise``, exact element-wise Adagrad (``pm_embbag_bwd_sorted_adagrad_elem``: ``mom_ptrs_dev`` then points at one
    fp32 ``[rows_t, dims_t]`` state buffer per table).  ``pad``: per-table padding indices (device int64 ``[T]``): those rows
    and their state are saved before and restored after the step (``_PadGuard``); a step refused on the host launches neither.
    ``mean``: ``grad`` is the gradient of a mean-pooled forward: scaled once (``_grad_as_sum``), then everything below as it is.
    ``out16``: the module's 16-bit output dtype: a gradient of that dtype is widened once (``_grad_as_sum``)."""
    grad = _grad_as_sum(ts, grad, indices, offsets, B, psw, pad, mean, out16=out16)
    if weight_decay_mode not in _WD_MODES:
        raise ValueError(f"weight_decay_mode must be one of none / l2 / decouple, got {weight_decay_mode!r}")
    grad = _check_grad(ts, grad, B)
    _no_presorted_split(ts, presorted)
    op = ts.request(indices, offsets, B, psw, 0, None)
    L = _lib.load()
    wdt, s = _WDTYPE[ts.dtype], _stream_ptr()
    fused_call = L.pm_embbag_bwd_fused_adagrad_elem if elementwise else L.pm_embbag_bwd_fused_adagrad
    sorted_call = L.pm_embbag_bwd_sorted_adagrad_elem if elementwise else L.pm_embbag_bwd_sorted_adagrad_ex
    # (more than 1024 tables: one call per table range, as in _bwd.  A stochastic-rounding draw is keyed by the seed, the table's
    # number INSIDE its call, the row and the column pair: every range gets a seed of its own -- the first one the caller's -- so
    # that table t and table t + 1024 do not share their draws)
    def call(fn):
        def issue(sub, t0, max_rows, ws):
            opt = _lib.pm_rowwise_adagrad(float(lr), float(eps), float(weight_decay), _WD_MODES[weight_decay_mode],
                                          1 if stochastic_rounding else 0, 0, (int(seed) + (t0 << 32)) & (2**64 - 1))
            return fn(ctypes.byref(sub), grad.data_ptr(), ts.d_ptrs.data_ptr() + 8 * t0, wdt, mom_ptrs_dev.data_ptr() + 8 * t0,
                      ctypes.byref(opt), max_rows, ws.data_ptr(), ws.numel(), s)
        return issue
    guard = _PadGuard(ts, pad, ts.d_ptrs, ts.dtype, mom_ptrs_dev, _lib.PM_PAD_STATE_ELEM if elementwise else _lib.PM_PAD_STATE_ROW)
    guard.save()
    _sorted_chunks_call(ts, op, indices, offsets, B, psw, presorted, pooling, 1, call(fused_call), call(sorted_call))
    guard.restore()


def _sparse_grad_call(ts: _TableSet, op, grad, max_rows: int, dims: Sequence[int], pads=None):
    """sort + count + (one synchronisation) + exact allocation + relabelled apply of ONE request of at most 1024 tables.
    ``pads``: the tables' padding indices (host ints / None): those rows are taken out of the result (one more synchronisation)."""
    L = _lib.load()
    ws = _workspace(ts, op, max_rows, L.pm_embbag_sparse_grad_workspace)
    s = _stream_ptr()
    _lib.check(L.pm_embbag_sort_indices(ctypes.byref(op), max_rows, ws.data_ptr(), ws.numel(), s))
    _sort_issued(ts, ws)
    counts = torch.empty(len(dims), dtype=torch.int64, device=ts.device)
    _lib.check(L.pm_embbag_sparse_grad_count(ctypes.byref(op), max_rows, ws.data_ptr(), ws.numel(), counts.data_ptr(), s))
    U = counts.tolist()                                   # the call's one host synchronisation
    rows = [torch.empty(u, dtype=torch.int64, device=ts.device) for u in U]
    vals = [torch.empty((u, d), dtype=torch.float32, device=ts.device) for u, d in zip(U, dims)]
    r_ptrs = torch.tensor([r.data_ptr() for r in rows], dtype=torch.int64, device=ts.device)
    v_ptrs = torch.tensor([v.data_ptr() for v in vals], dtype=torch.int64, device=ts.device)
    _lib.check(L.pm_embbag_sparse_grad(ctypes.byref(op), grad.data_ptr(), max_rows, ws.data_ptr(), ws.numel(), r_ptrs.data_ptr(),
                                       v_ptrs.data_ptr(), s))
    if pads is not None:
        rows, vals = _drop_padding_rows(rows, vals, pads)
    return list(zip(rows, vals))


def _drop_padding_rows(rows, vals, pads):
    """the padding row out of every table's coalesced ``(rows_t, values_t)``: rows_t is ascending, so the row's slot is one
    ``searchsorted``; the slots of all padded tables come back in ONE device-to-host read (-1: the row was not looked up)"""
    at = [(t, k) for t, k in enumerate(pads) if k is not None and rows[t].numel()]
    if not at:
        return rows, vals
    found = []
    for t, k in at:
        key = torch.tensor([k], dtype=torch.int64, device=rows[t].device)
        pos = torch.searchsorted(rows[t], key).clamp_(max=rows[t].numel() - 1)
        found.append(torch.where(rows[t][pos] == key, pos, torch.full_like(pos, -1)))
    rows, vals = list(rows), list(vals)
    for (t, _), pos in zip(at, torch.cat(found).tolist()):
        if pos >= 0:
            rows[t] = torch.cat((rows[t][:pos], rows[t][pos + 1:]))
            vals[t] = torch.cat((vals[t][:pos], vals[t][pos + 1:]))
    return rows, vals


def _sparse_grad(ts: _TableSet, grad, indices, offsets, B, psw=None, bag_begin=0, bag_count=None, pads=None,
                 mean: bool = False, pad: Optional[torch.Tensor] = None, out16: Optional[torch.dtype] = None):
    """Coalesced sparse gradient (``pm_embbag_sparse_grad*``): a list of T ``(rows_t, values_t)`` -- rows_t the distinct rows table t's
    lookups hit (ascending int64), values_t ``[U_t, D_t]`` fp32, ``values_t[k] = sum_{j: idx_j = rows_t[k]} w_j * grad[t, bag(j)]`` in
    the sorted backward's order.  Synchronises once per request of at most 1024 tables (to size the outputs).  ``mean``: ``grad`` is
    the gradient of a mean-pooled forward: scaled once (``_grad_as_sum``; ``pad`` = the device form of ``pads``).  ``out16``: the module's
    16-bit output dtype: a gradient of that dtype is widened once (``_grad_as_sum``)."""
    grad = _check_grad(ts, _grad_as_sum(ts, grad, indices, offsets, B, psw, pad, mean, bag_begin, bag_count, out16), B)
    op = ts.request(indices, offsets, B, psw, bag_begin, bag_count)
    op.fixed_pooling = 0
    # more tables than one sorted call takes: independent requests of at most 1024 tables (_table_chunks)
    res = []
    for sub, t0, t1, max_rows in _table_chunks(ts, op, indices, offsets, B, psw):
        res += _sparse_grad_call(ts, sub, grad, max_rows, ts.dims[t0:t1], None if pads is None else pads[t0:t1])
    return res


def _psw_grad(ts: _TableSet, grad, indices, offsets, B, psw=None, out=None, bag_begin=0, bag_count=None,
              pad: Optional[torch.Tensor] = None, out16: Optional[torch.dtype] = None):
    """Gradient of ``per_sample_weights`` (``pm_embbag_psw_grad``): fp32 ``[N]``, ``out[j] = <grad[t, bag(j)], table_t[indices[j]]>``
    for the lookups of the bag slice, with the arithmetic fixed in include/param_amd.h.  ``psw`` only keeps the cached request
    descriptor of the backward that follows: the value does not depend on it.  ``pad``: per-table padding indices (device int64
    ``[T]``): the entries of padded lookups are then overwritten with +0.0 (``pm_embbag_pad_mask``, one more launch).  ``out16``: the
    module's 16-bit output dtype: a gradient of that dtype is widened first (``_grad_as_sum``)."""
    grad = _check_grad(ts, _grad_as_sum(ts, grad, indices, offsets, B, psw, None, False, bag_begin, bag_count, out16), B)
    op = ts.request(indices, offsets, B, psw, bag_begin, bag_count)
    n = indices.numel()
    if out is None:
        out = torch.zeros(n, dtype=torch.float32, device=ts.device)      # lookups outside the slice (or outside every bag): zero
    elif out.dtype != torch.float32 or out.numel() != n or not out.is_contiguous() or out.device != ts.device:
        raise ValueError(f"out must be a contiguous float32 tensor of {n} entries on {ts.device}")
    rc = _lib.load().pm_embbag_psw_grad(ctypes.byref(op), grad.data_ptr(), out.data_ptr(), _stream_ptr())
    if rc:
        _lib.check(rc)
    if pad is not None:
        _lib.check(_lib.load().pm_embbag_pad_mask(ctypes.byref(op), pad.data_ptr(), out.data_ptr(), _stream_ptr()))
    return out


def _psw_shared_grad(ctx, ts: _TableSet, grad_out, indices, offsets, psw, B=None) -> torch.Tensor:
    """``grad_out`` of an autograd backward that also owes the ``per_sample_weights`` gradient: a 16-bit one is widened here, once, for
    both consumers (weighted requests are sum-pooled: no scaling); every other gradient comes back as it is"""
    out16 = ctx.module._out16
    if out16 is None or grad_out.dtype != out16 or not (ctx.has_psw and ctx.needs_input_grad[4]):
        return grad_out
    return _grad_as_sum(ts, grad_out, indices, offsets, ctx.B if B is None else B, psw, None, False, out16=out16)


class _DenseGradFn(torch.autograd.Function):
    """forward = batched lookup; backward = scatter-add into a dense fp32 weight.grad
    (torch ``sparse=False`` semantics, aten::_embedding_bag_dense_backward), and -- for ``per_sample_weights`` that require it --
    their gradient (aten::_embedding_bag_per_sample_weights_backward)."""

    @staticmethod
    def forward(ctx, weight, module, indices, offsets, psw):
        ts = module._tables()
        B = offsets.numel()
        ctx.module, ctx.B = module, B
        ctx.save_for_backward(indices, offsets, psw if psw is not None else torch.empty(0))
        ctx.has_psw = psw is not None
        return _fwd(ts, indices, offsets, B, psw, pad=module._pad_dev(), mean=module.mode == "mean", out16=module._out16)

    @staticmethod
    def backward(ctx, grad_out):
        indices, offsets, psw = ctx.saved_tensors
        m = ctx.module
        ts = m._tables()
        dW = torch.zeros(m.weight.shape, dtype=torch.float32, device=grad_out.device)
        d_ptr = torch.tensor([dW.data_ptr()], dtype=torch.int64, device=grad_out.device)
        grad_out = _psw_shared_grad(ctx, ts, grad_out.contiguous(), indices, offsets, psw)
        pad = m._pad_dev()
        # (mean: grad_out is left as it is -- the scaled copy is a scratch of _bwd's)
        _bwd(ts, grad_out, indices, offsets, ctx.B, d_ptr, torch.float32, 1.0, psw if ctx.has_psw else None, pad=pad, mean=m.mode == "mean",
             out16=m._out16)
        d_psw = _psw_grad(ts, grad_out, indices, offsets, ctx.B, psw, pad=pad) if ctx.has_psw and ctx.needs_input_grad[4] else None
        return dW.to(m.weight.dtype), None, None, None, d_psw


class _SparseGradFn(_DenseGradFn):
    """the same forward; backward = the coalesced sparse gradient (``pm_embbag_sparse_grad``): ``weight.grad`` is a coalesced
    sparse COO tensor of the U distinct rows looked up, torch ``sparse=True`` semantics (values in the weight's dtype)."""

    @staticmethod
    def backward(ctx, grad_out):
        indices, offsets, psw = ctx.saved_tensors
        m = ctx.module
        w = m.weight
        grad_out = _psw_shared_grad(ctx, m._tables(), grad_out.contiguous(), indices, offsets, psw)
        ((rows, vals),) = _sparse_grad(m._tables(), grad_out, indices, offsets, ctx.B, psw if ctx.has_psw else None,
                                       pads=None if m.padding_idx is None else [m.padding_idx], mean=m.mode == "mean", pad=m._pad_dev(),
                                       out16=m._out16)
        d_psw = (_psw_grad(m._tables(), grad_out, indices, offsets, ctx.B, psw, pad=m._pad_dev())
                 if ctx.has_psw and ctx.needs_input_grad[4] else None)
        g = torch.sparse_coo_tensor(rows[None], vals.to(w.dtype), tuple(w.shape), is_coalesced=True)
        # autograd's accumulation into .grad keeps these very index / value tensors but drops the coalesced flag: the module's
        # post-accumulate hook sets it again when .grad still holds them (an accumulated sum of two steps is torch's own result)
        m._sparse_mark = (g._values().data_ptr(), g._indices().data_ptr())
        return g, None, None, None, d_psw


class _MaxGradFn(torch.autograd.Function):
    """``mode="max"``: forward = the max lookup, which also writes ``max_indices`` (saved); backward = ``grad_out[b, c]`` into row
    ``max_indices[b, c]`` of a zeroed dense fp32 ``weight.grad`` (``_max_bwd``: aten::_embedding_bag_dense_backward's max branch)."""

    @staticmethod
    def forward(ctx, weight, module, indices, offsets):
        ts = module._tables()
        B = offsets.numel()
        ctx.module, ctx.B = module, B
        out, arg = _fwd_max(ts, indices, offsets, B, pad=module._pad_dev(), out16=module._out16, max_indices=True)
        ctx.save_for_backward(indices, offsets, arg)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        indices, offsets, arg = ctx.saved_tensors
        m = ctx.module
        dW = torch.zeros(m.weight.shape, dtype=torch.float32, device=grad_out.device)
        d_ptr = torch.tensor([dW.data_ptr()], dtype=torch.int64, device=grad_out.device)
        _max_bwd(m._tables(), grad_out.contiguous(), indices, offsets, ctx.B, d_ptr, torch.float32, 1.0, m._pad_dev(), arg, out16=m._out16)
        return dW.to(m.weight.dtype), None, None, None


class EmbeddingBagMI355(nn.Module, _BoundsChecked):
    """``torch.nn.EmbeddingBag(num_embeddings, embedding_dim, mode="sum" | "mean")`` on MI355X HIP kernels.

    Same call contract as the module the reference builds at pytorch_emb.py:179 and
    pytorch_dist_backend.py:924: ``forward(indices[N], offsets[B]) -> float32[B, D]``,
    ``include_last_offset=False``; ``.weight`` is an ``nn.Parameter`` (N(0,1) init like torch).
    ``sparse=True``: ``weight.grad`` is a sparse COO tensor, as torch's, but coalesced -- one row per distinct index looked up
    (``U x D`` values, not torch's ``N x D``); torch's sparse-capable optimizers (``SparseAdam``, ``SGD``, ``Adagrad``) take it.
    The backward then synchronises once (to size the gradient), as ``coalesce()`` does.
    ``bounds_check_mode`` (default ``"none"``): see :class:`_BoundsChecked` -- ``forward`` repairs / refuses a bad request first.
    ``padding_idx`` (default ``None``; torch's argument): an int in ``[-n, n)``, negative values count from the end.  Lookups of that
    row contribute nothing to the output, the row gets no gradient (dense: its gradient row is zero; ``sparse=True``: it is absent
    from the COO rows) and their ``per_sample_weights`` gradient is +0.0; the row is never read into a sum, so what it holds (NaN)
    reaches no output.  A module that creates its own weights zero-fills the row; a caller's ``_weight`` is left alone.  ``None``
    adds no launch.  The sanitiser runs first: a bad index it repairs to 0 is padding when ``padding_idx == 0``.
    2-D input: ``forward(input[B, L])`` (``offsets`` must be ``None``) treats every row as one bag of L lookups, as torch does;
    ``per_sample_weights`` then has the input's shape, and so has its gradient.
    ``mode="mean"``: ``out = sum / (float)count``, ``count`` = the bag's lookups that are not ``padding_idx`` (after the sanitiser's
    repairs): the sum forward's additions, then one correctly rounded fp32 division per element; an empty or all-padding bag gives
    +0.0.  Every lookup receives ``grad * (1.0f / (float)count)`` -- the reciprocal rounded to fp32 first, then one multiplication --
    summed as the sum backward sums, dense and ``sparse=True``.  On fp32 tables that is torch's CPU module bit for bit (forward always;
    gradients where no row is looked up twice, otherwise up to the order of the additions).  16-bit tables keep this package's
    convention (rows widened, fp32 sums and output); torch's own 16-bit module rounds the sum to 16 bits before it divides.
    ``per_sample_weights`` with ``mode="mean"`` raises ``NotImplementedError``, as torch does; this constructor refuses ``mode="max"``
    as it always did: max pooling is :class:`MaxEmbeddingBagMI355`.
    ``output_dtype`` (default ``None`` = fp32; fbgemm TBE's argument): ``torch.bfloat16`` / ``torch.float16``, ``"bf16"`` / ``"fp16"`` in
    any case or an enum member of that value or name (``SparseType``): ``forward`` returns that dtype -- the fp32 result of the same
    request rounded once, to nearest even, in the lookup kernel (``pm_embbag_fwd_out16``) -- and the backward receives it: the gradient
    is widened exactly (``pm_embbag_grad_widen``, the mean scaling fused) and then treated as the fp32 gradient it stands for.
    """

    _MODES = ("sum", "mean")      # what this constructor takes as ``mode`` (:class:`MaxEmbeddingBagMI355`: ``"max"``)

    def __init__(self, num_embeddings: int, embedding_dim: int, mode: str = "sum", sparse: bool = False,
                 dtype: torch.dtype = torch.float32, device=None, _weight: Optional[torch.Tensor] = None,
                 bounds_check_mode="none", padding_idx: Optional[int] = None, output_dtype=None):
        super().__init__()
        if mode not in self._MODES:
            raise NotImplementedError('only mode="sum" (the reference hot path, pytorch_emb.py:179) and mode="mean" are implemented'
                                      if "sum" in self._MODES else f'{type(self).__name__} is mode="max" only')
        if mode == "max" and sparse:
            raise ValueError("max mode does not support sparse weights")
        self._init_shared(bounds_check_mode, output_dtype)      # (validated before anything is allocated)
        self.padding_idx = _normalize_padding_idx(padding_idx, num_embeddings if _weight is None else int(_weight.shape[0]))
        self._off2d: dict = {}
        self.num_embeddings, self.embedding_dim, self.mode, self.sparse = num_embeddings, embedding_dim, mode, sparse
        if _weight is None:
            w = torch.empty(num_embeddings, embedding_dim, dtype=dtype, device=device)
            if w.is_cuda:
                fill_random_(w, "normal", 0.0, 1.0, seed=torch.initial_seed())
            else:
                nn.init.normal_(w)  # host staging only; forward refuses non-ROCm tensors
            if self.padding_idx is not None:
                w[self.padding_idx].zero_()      # torch: the padding row of module-made weights starts as zeros
        else:
            w = _weight
        self.weight = nn.Parameter(w)
        self._ts: Optional[_TableSet] = None
        self._sparse_mark = None
        if sparse:
            self.weight.register_post_accumulate_grad_hook(self._mark_coalesced)

    def _mark_coalesced(self, p: torch.Tensor) -> None:
        g, mark = p.grad, self._sparse_mark
        self._sparse_mark = None
        if g is not None and g.is_sparse and mark == (g._values().data_ptr(), g._indices().data_ptr()):
            g._coalesced_(True)

    def _tables(self) -> _TableSet:
        w = self.weight.data
        if self._ts is None or self._ts.ptrs[0] != w.data_ptr():
            self._ts = _TableSet([w], "bd")
        return self._ts

    def _bags_2d(self, input, offsets, per_sample_weights):
        """a ``[B, L]`` input as the 1-D request of B bags of L lookups: ``offsets = arange(B) * L`` is built on the device once
        per (B, L, dtype) and reused"""
        if offsets is not None:
            raise ValueError(f"if input is 2D, then offsets has to be None, as input is treated is a mini-batch of fixed length "
                             f"sequences. However, found offsets of type {type(offsets)}")
        B, L = int(input.shape[0]), int(input.shape[1])
        if per_sample_weights is not None:
            if tuple(per_sample_weights.shape) != tuple(input.shape):
                raise ValueError(f"embedding_bag: If per_sample_weights ({tuple(per_sample_weights.shape)}) is not None, then it must "
                                 f"have the same shape as the input ({tuple(input.shape)})")
            per_sample_weights = per_sample_weights.reshape(-1)
        key = (B, L, input.dtype, input.device)
        off = self._off2d.get(key)
        if off is None:
            if len(self._off2d) >= 8:
                self._off2d.clear()
            off = self._off2d[key] = torch.arange(B, dtype=input.dtype, device=input.device) * L
        return input.reshape(-1), off, per_sample_weights

    def forward(self, indices, offsets=None, per_sample_weights=None):
        # (the reference's benchmark loop calls this once per step, pytorch_emb.py:56-66: below batch ~2048 the step IS the host
        # time of this call, so the parameter is fetched once -- nn.Module.__getattr__ per access otherwise -- and the table set
        # is revalidated by pointer only)
        if indices.dim() == 2:
            indices, offsets, per_sample_weights = self._bags_2d(indices, offsets, per_sample_weights)
        elif offsets is None:
            raise ValueError("offsets has to be a 1D Tensor but got None")
        if per_sample_weights is not None and self.mode != "sum":
            raise NotImplementedError("embedding_bag: per_sample_weights was not None. per_sample_weights is only supported for "
                                      f"mode='sum' (got mode='{self.mode}'). Please open a feature request on GitHub.")
        w = self._parameters["weight"]
        if not w.is_cuda:
            _require_device(w, "EmbeddingBagMI355.weight")
        if self.bounds_check_mode != "none":
            self._sanitize(self._tables(), indices, offsets, offsets.numel(), self.bounds_check_mode, per_sample_weights)
        if self.mode == "max":
            if w.requires_grad and torch.is_grad_enabled():
                return _MaxGradFn.apply(w, self, indices, offsets)
            return _fwd_max(self._tables(), indices, offsets, offsets.numel(), pad=self._pad_dev(), out16=self._out16)[0]
        if w.requires_grad and torch.is_grad_enabled():
            return (_SparseGradFn if self.sparse else _DenseGradFn).apply(w, self, indices, offsets, per_sample_weights)
        ts = self._ts
        if ts is None or ts.ptrs[0] != w.data_ptr():
            ts = self._tables()
        return _fwd(ts, indices, offsets, offsets.numel(), per_sample_weights, pad=self._pad_dev(), mean=self.mode == "mean",
                    out16=self._out16)

    def sanitize_(self, indices, offsets, mode=None) -> None:
        """The sanitiser on its own (``offsets`` is ``[B]``, as ``forward`` takes it): in place, stream-ordered.  ``mode``: default
        the module's ``bounds_check_mode``, ``"warning"`` where that is ``"none"``."""
        _require_device(self.weight, "EmbeddingBagMI355.weight")
        mode = bounds_check_mode_name(mode) if mode is not None else self.bounds_check_mode
        self._sanitize(self._tables(), indices, offsets, offsets.numel(), "warning" if mode == "none" else mode)

    def extra_repr(self) -> str:
        return (f"{self.num_embeddings}, {self.embedding_dim}, mode={self.mode}, dtype={self.weight.dtype}" + (", sparse=True" if self.sparse else "") +
                (f", padding_idx={self.padding_idx}" if self.padding_idx is not None else "") +
                (f", output_dtype={self.output_dtype}" if self._out16 is not None else ""))


class MaxEmbeddingBagMI355(EmbeddingBagMI355):
    """``torch.nn.EmbeddingBag(num_embeddings, embedding_dim, mode="max")`` on MI355X HIP kernels: :class:`EmbeddingBagMI355`'s surface
    (1-D and 2-D input, ``padding_idx``, ``output_dtype``, ``bounds_check_mode``) with max pooling.  A class of its own because
    ``EmbeddingBagMI355(mode="max")`` keeps raising ``NotImplementedError``, as it always did; ``mode``, if given, must be ``"max"``.

    Per column the maximum over the bag's lookups that are not ``padding_idx``, by torch's rule -- the first kept lookup sets the value
    whatever it holds, a later one replaces it iff it is greater (ordered, strict): a NaN in the first kept lookup stays, a later NaN
    never enters, of equal values the first wins; an empty or all-padding bag gives +0.0.  torch's CPU module bit for bit on fp32,
    bf16 and fp16 tables (fp32 output of a 16-bit table: torch's widened).  The backward sends ``grad[b, c]`` to the row that supplied
    the maximum, once; ``weight.grad`` is dense and equals torch's CPU autograd bit for bit wherever a row has at most 256 lookups in
    the request.  ``per_sample_weights`` raises ``NotImplementedError`` and ``sparse=True`` ``ValueError`` (at construction), with
    torch's texts."""

    _MODES = ("max",)

    def __init__(self, num_embeddings: int, embedding_dim: int, mode: str = "max", **kw):
        super().__init__(num_embeddings, embedding_dim, mode=mode, **kw)


class _EmbeddingGradFn(torch.autograd.Function):
    """forward = the un-pooled lookup (``pm_embedding_gather``); backward = the SUM backward of the derived request "one bag per
    lookup" -- ``offsets' = arange(N)``, ``B' = N``, gradient ``grad_out.reshape(N, D)`` -- dense (``_bwd`` into a zeroed fp32 buffer,
    aten::embedding_dense_backward) or, with ``sparse=True``, coalesced COO (``_sparse_grad``).  No backward kernel of its own."""

    @staticmethod
    def forward(ctx, weight, module, indices, shape):
        ctx.module = module
        ctx.save_for_backward(indices)
        ts = module._tables()
        return _gather(ts, indices, module._offsets0(indices), 1, module.output_dtype).view(*shape, module.embedding_dim)

    @staticmethod
    def backward(ctx, grad_out):
        (indices,) = ctx.saved_tensors
        m = ctx.module
        w = m.weight
        ts = m._tables()
        n = indices.numel()
        grad = grad_out.reshape(n, m.embedding_dim).contiguous()
        offsets = m._offsets_arange(indices)
        if not m.sparse:
            dW = torch.zeros(w.shape, dtype=torch.float32, device=grad.device)
            if n:
                d_ptr = torch.tensor([dW.data_ptr()], dtype=torch.int64, device=grad.device)
                _bwd(ts, grad, indices, offsets, n, d_ptr, torch.float32, 1.0, pad=m._pad_dev(), out16=m._out16)
            return dW.to(w.dtype), None, None, None
        if n:
            ((rows, vals),) = _sparse_grad(ts, grad, indices, offsets, n, pads=None if m.padding_idx is None else [m.padding_idx],
                                           pad=m._pad_dev(), out16=m._out16)
        else:
            rows = torch.empty(0, dtype=torch.int64, device=grad.device)
            vals = torch.empty((0, m.embedding_dim), dtype=torch.float32, device=grad.device)
        g = torch.sparse_coo_tensor(rows[None], vals.to(w.dtype), tuple(w.shape), is_coalesced=True)
        m._sparse_mark = (g._values().data_ptr(), g._indices().data_ptr())      # (see _SparseGradFn)
        return g, None, None, None


class EmbeddingMI355(nn.Module, _BoundsChecked):
    """``torch.nn.Embedding(num_embeddings, embedding_dim)`` on an MI355X HIP kernel: the un-pooled sibling of
    :class:`EmbeddingBagMI355` (fbgemm TBE's sequence embeddings, ``PoolingMode.NONE``, for one table).

    ``forward(input)`` takes an int32 / int64 tensor of any shape and returns ``[*input.shape, D]``: row ``input[...]`` of ``.weight``
    per lookup, moved by ONE launch (``pm_embedding_gather``: the request is one table, one bag, ``offsets = [0]``).  An empty input
    returns an empty output without a launch.  A floating-point input raises ``TypeError``.
    ``output_dtype`` (default ``None`` = fp32, this package's convention: 16-bit rows are widened exactly): ``torch.float32`` /
    ``torch.bfloat16`` / ``torch.float16`` or the spellings the bag modules take.  With the table's own dtype the stored bits come
    back as they are -- ``-0.0``, NaN payloads and subnormals included, which is what torch's module returns; an fp32 table with a
    16-bit ``output_dtype``, and bf16 <-> fp16, are rounded once to nearest even (the rule of the bag modules' ``output_dtype``).
    ``padding_idx`` (default ``None``) follows ``nn.Embedding``: an int in ``[-n, n)``, negative values count from the end; the forward
    still returns the row as stored (a NaN kept there comes out); the row receives no gradient (dense: its gradient row is zero;
    ``sparse=True``: it is absent from the COO rows); a module that creates its own weights zero-fills it.
    Autograd: the sum backward of the request "one bag per lookup" (``offsets = arange(N)``), so ``weight.grad`` is what
    :class:`EmbeddingBagMI355` gives for bags of one -- dense fp32 accumulation in lookup order, or with ``sparse=True`` a coalesced
    sparse COO tensor of the distinct rows looked up (one synchronisation, as there).  A gradient in a 16-bit ``output_dtype`` is
    widened exactly first.  ``N >= 2^32`` lookups raise ``ValueError``.
    ``bounds_check_mode`` (default ``"none"``): see :class:`_BoundsChecked` -- ``forward`` repairs / refuses bad indices first;
    ``sanitize_`` is the call on its own.  ``max_norm`` and ``scale_grad_by_freq`` are not implemented (no such parameters).
    """

    def __init__(self, num_embeddings: int, embedding_dim: int, padding_idx: Optional[int] = None, sparse: bool = False,
                 dtype: torch.dtype = torch.float32, device=None, _weight: Optional[torch.Tensor] = None,
                 bounds_check_mode="none", output_dtype=None):
        super().__init__()
        self._init_shared(bounds_check_mode, output_dtype)      # (validated before anything is allocated)
        self.padding_idx = _normalize_padding_idx(padding_idx, num_embeddings if _weight is None else int(_weight.shape[0]))
        self.num_embeddings, self.embedding_dim, self.sparse = num_embeddings, embedding_dim, sparse
        if _weight is None:
            w = torch.empty(num_embeddings, embedding_dim, dtype=dtype, device=device)
            if w.is_cuda:
                fill_random_(w, "normal", 0.0, 1.0, seed=torch.initial_seed())
            else:
                nn.init.normal_(w)  # host staging only; forward refuses non-ROCm tensors
            if self.padding_idx is not None:
                w[self.padding_idx].zero_()      # torch: the padding row of module-made weights starts as zeros
        else:
            w = _weight
        self.weight = nn.Parameter(w)
        self._ts: Optional[_TableSet] = None
        self._off0: dict = {}        # the forward's offsets [0], one per (dtype, device)
        self._offn: dict = {}        # the backward's offsets arange(N), per (N, dtype, device)
        self._sparse_mark = None
        if sparse:
            self.weight.register_post_accumulate_grad_hook(self._mark_coalesced)

    @classmethod
    def from_pretrained(cls, embeddings: torch.Tensor, freeze: bool = True, padding_idx: Optional[int] = None, sparse: bool = False, **kw):
        """``nn.Embedding.from_pretrained``: the module around a caller's 2-D ``embeddings`` (left as they are, the padding row
        included); ``freeze=True`` (default) turns the weight's gradient off.  ``kw``: ``bounds_check_mode``, ``output_dtype``."""
        if embeddings.dim() != 2:
            raise ValueError("Embeddings parameter is expected to be 2-dimensional")
        m = cls(int(embeddings.shape[0]), int(embeddings.shape[1]), padding_idx=padding_idx, sparse=sparse, _weight=embeddings, **kw)
        m.weight.requires_grad = not freeze
        return m

    _mark_coalesced = EmbeddingBagMI355._mark_coalesced
    _tables = EmbeddingBagMI355._tables

    def _offsets0(self, indices) -> torch.Tensor:
        key = (indices.dtype, indices.device)
        off = self._off0.get(key)
        if off is None:
            off = self._off0[key] = torch.zeros(1, dtype=indices.dtype, device=indices.device)
        return off

    def _offsets_arange(self, indices) -> torch.Tensor:
        """``arange(N)`` in the indices' dtype, built on the device once per (N, dtype, device) and reused (like ``_off2d``)"""
        key = (indices.numel(), indices.dtype, indices.device)
        off = self._offn.get(key)
        if off is None:
            if len(self._offn) >= 8:
                self._offn.clear()
            off = self._offn[key] = torch.arange(key[0], dtype=indices.dtype, device=indices.device)
        return off

    def _flat(self, input) -> torch.Tensor:
        if not isinstance(input, torch.Tensor) or input.dtype not in _IDTYPE:
            raise TypeError(f"EmbeddingMI355: input must be an int32 or int64 tensor, got {getattr(input, 'dtype', type(input))}")
        if input.numel() >= 2**32:
            raise ValueError("EmbeddingMI355: the backward carries lookup positions in 32 bits: fewer than 2^32 lookups per call")
        w = self._parameters["weight"]
        if not w.is_cuda:
            _require_device(w, "EmbeddingMI355.weight")
        _require_device(input, "input")
        return input.reshape(-1).contiguous()

    def forward(self, input):
        indices = self._flat(input)
        w = self._parameters["weight"]
        if self.bounds_check_mode != "none" and indices.numel():
            self._sanitize(self._tables(), indices, self._offsets0(indices), 1, self.bounds_check_mode)
        if w.requires_grad and torch.is_grad_enabled():
            return _EmbeddingGradFn.apply(w, self, indices, tuple(input.shape))
        out = _gather(self._tables(), indices, self._offsets0(indices), 1, self.output_dtype)
        return out.view(*input.shape, self.embedding_dim)

    def sanitize_(self, input, mode=None) -> None:
        """The sanitiser on its own: repairs ``input`` in place (it must be contiguous: a copy would be repaired instead),
        stream-ordered.  ``mode``: default the module's ``bounds_check_mode``, ``"warning"`` where that is ``"none"``."""
        if not input.is_contiguous():
            raise ValueError("sanitize_ needs a contiguous input (it is repaired in place)")
        indices = self._flat(input)
        mode = bounds_check_mode_name(mode) if mode is not None else self.bounds_check_mode
        if indices.numel():
            self._sanitize(self._tables(), indices, self._offsets0(indices), 1, "warning" if mode == "none" else mode)

    def extra_repr(self) -> str:
        return (f"{self.num_embeddings}, {self.embedding_dim}, dtype={self.weight.dtype}" + (", sparse=True" if self.sparse else "") +
                (f", padding_idx={self.padding_idx}" if self.padding_idx is not None else "") +
                (f", output_dtype={self.output_dtype}" if self._out16 is not None else ""))


class _FusedUpdateFn(torch.autograd.Function):
    """TBE-style: backward applies ``W[idx] += -lr * grad`` in place (no weight.grad); ``per_sample_weights`` that require grad get
    theirs (fbgemm's ``indice_weights`` gradient), computed from the tables as the forward read them."""

    @staticmethod
    def forward(ctx, anchor, module, indices, offsets, psw):
        ctx.module = module
        ctx.save_for_backward(indices, offsets, psw if psw is not None else torch.empty(0))
        ctx.has_psw = psw is not None
        return module.lookup(indices, offsets, psw)

    @staticmethod
    def backward(ctx, grad_out):
        indices, offsets, psw = ctx.saved_tensors
        m = ctx.module
        d_psw = None
        if ctx.has_psw and ctx.needs_input_grad[4]:
            # before the in-place update, on the same stream: the gradient belongs to the weights the forward read
            B = m._batch_of(offsets, indices)
            grad_out = _psw_shared_grad(ctx, m._tables(), grad_out.contiguous(), indices, offsets, psw, B)
            d_psw = _psw_grad(m._tables(), grad_out, indices, offsets, B, psw, pad=m._pad_dev())
        m.optimizer_step_(grad_out, indices, offsets, per_sample_weights=psw if ctx.has_psw else None)
        return None, None, None, None, d_psw


class _FusedSequenceFn(torch.autograd.Function):
    """the sequence sibling of ``_FusedUpdateFn``: forward = ``lookup_sequence``; backward applies the module's optimizer to the ``[N, D]``
    gradient rows in place (``sequence_optimizer_step_``; no weight.grad)"""

    @staticmethod
    def forward(ctx, anchor, module, indices, offsets, batch):
        ctx.module, ctx.batch = module, batch
        ctx.save_for_backward(indices, offsets)
        return module.lookup_sequence(indices, offsets, batch)

    @staticmethod
    def backward(ctx, grad_out):
        indices, offsets = ctx.saved_tensors
        ctx.module.sequence_optimizer_step_(grad_out, indices, offsets, batch=ctx.batch)
        return None, None, None, None, None


_MAX_WEIGHTED = "max pooling is unweighted: per_sample_weights must be None"
_MAX_FUSED = ("a fused optimizer would apply weight decay and state updates to looked-up rows whose gradient is zero (a row that wins no "
              "column); use dense_grad or scatter_add_")


class _FusedMaxRefusedFn(torch.autograd.Function):
    """what ``forward`` of a ``pooling_mode="max"`` module with ``fused_update`` returns under autograd: the lookup's result, whose
    ``.backward()`` is refused with the reason (there is no fused update for max pooling)"""

    @staticmethod
    def forward(ctx, anchor, out):
        return out.view_as(out)

    @staticmethod
    def backward(ctx, grad_out):
        raise ValueError('the fused .backward() does not take pooling_mode="max": ' + _MAX_FUSED)


class BatchedEmbeddingBagMI355(nn.Module, _BoundsChecked):
    """T embedding tables in one HBM slab, looked up by ONE kernel launch.

    ``forward(indices, offsets, per_sample_weights=None)`` uses the TBE request layout
    (indices concatenated table-major, offsets ``[T*B+1]``) and returns ``[B, sum D]``
    (``layout="bd"``) or ``[T, B, D]`` (``layout="tbd"``, dlrm.py's ``torch.stack`` shape) or ``[B / block_bags, T, block_bags, D]``
    (``layout="blocked"``: the send layout of a table-wise sharded exchange -- every peer's chunk contiguous, made of ``[block_bags, D]``
    runs per table; forward whole-batch requests only).

    ``bounds_check_mode`` (default ``"none"``; fbgemm TBE's argument of that name): see :class:`_BoundsChecked` -- ``forward`` and
    ``lookup`` repair / refuse a bad request first, ``sanitize_`` is the call on its own.  With ONE table and a mode other than
    ``"none"`` pass ``batch=``: whether a ``[B + 1]`` or a ``[B]`` offsets tensor was meant is otherwise guessed from ``offsets[-1]``,
    which may be the corrupt entry.

    ``padding_idx`` (default ``None``): ``None``, one int applied to every table, or a sequence of ``int | None`` per table; each
    int in ``[-rows_t, rows_t)``, negative values count from the end.  The attribute ``padding_idx`` holds the normalised per-table
    list (``None`` when no table has a padding row).  A lookup of its table's padding row contributes nothing to ``forward`` /
    ``lookup`` (the row is never read into a sum); ``scatter_add_``, ``adagrad_step_``, ``optimizer_step_``, ``dense_grad`` and the
    fused ``backward`` leave the row -- and its optimizer state -- bit for bit as it was; ``sparse_grad`` leaves it out;
    ``per_sample_weights_grad`` gives +0.0 there.  ``reset_parameters`` zero-fills the padding rows.  ``lookup_quantized``,
    ``lookup(split_bags=True)`` and ``layout="blocked"`` do not take padding (ValueError).  The sanitiser runs first: a bad index
    it repairs to 0 is padding in a table whose ``padding_idx`` is 0.

    ``pooling_mode`` (default ``"sum"``; fbgemm TBE's argument of that name): ``"sum"`` / ``"mean"`` in any case, a ``PoolingMode``
    member or its int (0 / 1); ``NONE`` / 2 raises ValueError.  With ``"mean"``, ``forward`` / ``lookup`` (``out=`` and batch slices
    included) give ``sum / (float)count`` -- ``count`` = the bag's lookups that are not its table's padding index, after the
    sanitiser's repairs; the sum forward's additions, then one correctly rounded fp32 division; +0.0 for a bag without kept lookups
    -- and ``scatter_add_``, ``adagrad_step_``, ``optimizer_step_``, ``dense_grad``, ``sparse_grad`` and the fused ``backward`` take
    ``grad`` as the gradient of THAT forward: every lookup receives ``grad * (1.0f / (float)count)`` (one more launch and a scratch
    of ``grad``'s shape; ``grad`` is not modified), then each is exactly what it is for a sum module.  A stated difference to
    fbgemm, which allows weighted mean: ``per_sample_weights`` with ``"mean"`` raises ValueError, and so do
    ``per_sample_weights_grad``, ``lookup(split_bags=True)``, ``lookup_quantized`` and ``layout="blocked"``.  ``"sum"`` adds no launch.

    Max pooling (which fbgemm's enum does not have; ``pooling_mode="max"`` stays a ValueError here) is
    :class:`MaxBatchedEmbeddingBagMI355`; sum and mean modules reach none of its code.

    ``output_dtype`` (default ``None`` = fp32; fbgemm TBE's argument of that name): ``torch.float32`` / ``torch.bfloat16`` /
    ``torch.float16``, ``"fp32"`` / ``"bf16"`` / ``"fp16"`` in any case, or an enum member whose value or name is one of those
    (``SparseType``); anything else raises ValueError.  With a 16-bit dtype ``forward`` / ``lookup`` (``out=`` and batch slices
    included) return it: the fp32 result of the same request -- sum, weighted sum or mean, with or without padding -- rounded once per
    element, to nearest even, in the lookup kernel (``pm_embbag_fwd_out16``).  ``scatter_add_``, ``adagrad_step_``, ``optimizer_step_``,
    ``dense_grad``, ``sparse_grad``, ``per_sample_weights_grad`` and the fused ``backward`` then take ``grad`` in fp32 (always) or in
    that dtype: a 16-bit gradient is widened exactly into an fp32 scratch (one more launch, ``pm_embbag_grad_widen``, which also does
    the mean scaling; ``grad`` is not modified) and each is exactly what it is for that fp32 gradient.  ``layout="blocked"``,
    ``lookup(split_bags=True)`` and ``lookup_quantized`` do not take a 16-bit ``output_dtype`` (ValueError).  The default adds no launch.
    """

    _POOLING = None      # a subclass's fixed pooling mode (:class:`MaxBatchedEmbeddingBagMI355`: ``"max"``); None: the ``pooling_mode`` argument

    def __init__(self, rows: Sequence[int], dims, dtype: torch.dtype = torch.float32, device="cuda",
                 layout: str = "bd", init: Optional[str] = "uniform_dlrm", seed: int = 0,
                 learning_rate: float = 0.01, fused_update: bool = True, optimizer: str = "sgd", eps: float = 1.0e-8,
                 weight_decay: float = 0.0, weight_decay_mode=None, stochastic_rounding: bool = False,
                 block_bags: Optional[int] = None, bounds_check_mode="none", padding_idx=None, pooling_mode="sum", output_dtype=None):
        super().__init__()
        self._init_shared(bounds_check_mode, output_dtype)      # (validated, like the optimizer below, before anything is allocated)
        if self._out16 is not None and layout == "blocked":
            raise ValueError('a 16-bit output_dtype is not supported with layout="blocked"')
        self.pooling_mode = self._POOLING or pooling_mode_name(pooling_mode)
        self._mean = self.pooling_mode == "mean"
        self._max = self.pooling_mode == "max"
        if (self._mean or self._max) and layout == "blocked":
            raise ValueError(f'pooling_mode="{self.pooling_mode}" is not supported with layout="blocked"')
        rows = [int(r) for r in rows]
        dims = [int(dims)] * len(rows) if isinstance(dims, int) else [int(d) for d in dims]
        assert len(rows) == len(dims) and len(rows) >= 1
        try:
            pads = [padding_idx if padding_idx is None or isinstance(padding_idx, bool) else operator.index(padding_idx)] * len(rows)
        except TypeError:      # not one integer (of any integer type) for every table: one entry per table
            pads = list(padding_idx)
            if len(pads) != len(rows):
                raise ValueError(f"padding_idx has {len(pads)} entries for {len(rows)} tables (None, one int, or one int | None per table)")
        pads = [_normalize_padding_idx(k, r) for k, r in zip(pads, rows)]
        self.padding_idx = pads if any(k is not None for k in pads) else None
        if self.padding_idx is not None and layout == "blocked":
            raise ValueError('padding_idx is not supported with layout="blocked"')
        self.rows, self.dims, self.layout = rows, dims, layout
        self.block_bags = block_bags      # layout="blocked": [B / block_bags, T, block_bags, D] (the per-rank batch of a sharded exchange)
        self.learning_rate, self.fused_update = learning_rate, fused_update
        if optimizer not in ("sgd", "rowwise_adagrad", "adagrad"):
            raise ValueError('optimizer must be "sgd", "rowwise_adagrad" or "adagrad"')
        self.optimizer, self.eps = optimizer, eps
        if weight_decay_mode not in _WD_MODES:
            raise ValueError(f"weight_decay_mode must be one of none / l2 / decouple, got {weight_decay_mode!r}")
        # Adagrad options (row-wise and element-wise) of the reference's TBE operator (split_table_batched_embeddings_ops.py:289-300)
        self.weight_decay, self.weight_decay_mode = weight_decay, weight_decay_mode
        self.stochastic_rounding = stochastic_rounding      # 16-bit tables only; fp32 tables ignore it
        self._sr_step = 0
        self._mom_ptrs: Optional[torch.Tensor] = None
        self._mom_base = None
        sizes = [r * d for r, d in zip(rows, dims)]
        esize = torch.empty(0, dtype=dtype).element_size()
        # table starts padded to 256 B so every row stays 16-byte aligned
        starts, cur = [], 0
        for s in sizes:
            starts.append(cur)
            cur += (s * esize + 255) // 256 * 256 // esize
        self.weights = nn.Parameter(torch.empty(cur, dtype=dtype, device=device), requires_grad=False)
        self._starts, self._sizes = starts, sizes
        self._anchor = nn.Parameter(torch.zeros((), device=device))  # lets autograd reach backward()
        # Adagrad state -- row-wise: one fp32 per row; element-wise ("adagrad"): one fp32 per weight, sum(rows_t * dims_t) values --
        # a buffer (follows .to() / state_dict), allocated on first use
        self.register_buffer("momentum", None)
        self._ts: Optional[_TableSet] = None
        if init is not None:
            self.reset_parameters(init, seed)

    # -- tables ------------------------------------------------------------------------------
    @property
    def embedding_specs(self):
        """``(rows, dim, location, compute device)`` per table -- the attribute of fbgemm's TBE module that callers of the
        reference's operator read back (train/compute/python/test/test_split_table_batched_embeddings_ops.py:29-30)"""
        dev = self.weights.device
        return [(int(r), int(d), "device" if dev.type == "cuda" else "host", dev.type) for r, d in zip(self.rows, self.dims)]

    def table(self, t: int) -> torch.Tensor:
        s = self._starts[t]
        return self.weights.data[s:s + self._sizes[t]].view(self.rows[t], self.dims[t])

    def reset_parameters(self, init: str = "uniform_dlrm", seed: int = 0) -> None:
        for t in range(len(self.rows)):
            w = self.table(t)
            if init == "normal":
                fill_random_(w, "normal", 0.0, 1.0, seed=seed * 1000003 + t)
            else:  # U(-1/sqrt(n), 1/sqrt(n)): pytorch_dist_backend.py:923-934
                lim = math.sqrt(1.0 / self.rows[t])
                fill_random_(w, "uniform", -lim, lim, seed=seed * 1000003 + t)
            if self.padding_idx is not None and self.padding_idx[t] is not None:
                w[self.padding_idx[t]].zero_()      # torch: a padding row starts as zeros

    def _tables(self) -> _TableSet:
        if self._ts is None or self._ts.ptrs[0] != self.table(0).data_ptr():
            self._ts = _TableSet([self.table(t) for t in range(len(self.rows))], self.layout, self.block_bags)
        return self._ts

    _TABLES = "weights"

    def _batch_of(self, offsets, indices=None) -> int:
        # TBE convention first: offsets has T*B+1 entries (split_table_batched_embeddings_ops.py:
        # 121-128); a T*B-entry tensor is accepted too (pass batch= to disambiguate T == 1).
        T = len(self.rows)
        n = offsets.numel()
        if T == 1 and n >= 1:
            # both readings fit every length.  TBE's [B+1] form ends with the number of indices; an nn.EmbeddingBag-style
            # [B] tensor does not (its last bag would silently be dropped): look once per request (one small D2H read,
            # remembered for the tensors of a benchmark loop); pass batch= to skip the question altogether.
            key = (offsets.data_ptr(), offsets._version, n, None if indices is None else indices.numel())
            if self._seen.get("b1_key") != key:
                closed = indices is not None and int(offsets[-1]) == indices.numel()
                self._seen.update(b1_key=key, b1_val=n - 1 if closed else n)
            return self._seen["b1_val"]
        if n >= 1 and (n - 1) % T == 0:
            return (n - 1) // T
        if n % T == 0:
            return n // T
        raise ValueError(f"offsets has {n} entries: neither T*B+1 nor T*B for T={T}")

    def _batch(self, offsets, indices, batch: Optional[int]) -> int:
        return self._batch_of(offsets, indices) if batch is None else batch

    # -- ops ---------------------------------------------------------------------------------
    def _max_refuses(self, what: str, why: str = "") -> None:
        """a call that a ``pooling_mode="max"`` module does not take: ValueError naming it (and the reason, where there is one)"""
        if self._max:
            raise ValueError(f'{what} does not take pooling_mode="max"' + (f": {why}" if why else ""))

    def lookup(self, indices, offsets, per_sample_weights=None, out=None, bag_begin=0, bag_count=None,
               batch: Optional[int] = None, split_bags: bool = False, return_max_indices: bool = False, max_indices=None):
        """Forward without autograd glue; ``bag_begin/bag_count`` select a batch slice.  ``split_bags=True`` selects the
        one-workgroup-per-bag kernel for few, long bags (deterministic, fp32-rounding-close to the default, not bit-equal).
        ``pooling_mode="max"`` only: ``return_max_indices=True`` returns ``(out, max_indices)`` -- int32 of the output's shape, the row
        that supplied each maximum, -1 for a bag without kept lookups; ``max_indices=`` is a caller's tensor for it (bags outside a
        batch slice keep their bits) and implies the pair."""
        if self._max:
            if split_bags or per_sample_weights is not None:
                raise ValueError('pooling_mode="max" does not take split_bags=True' if split_bags else _MAX_WEIGHTED)
            _require_device(self.weights, "BatchedEmbeddingBagMI355.weights")
            B = self._batch_of(offsets, indices) if batch is None else batch
            if self.bounds_check_mode != "none":
                self._sanitize(self._tables(), indices, offsets, B, self.bounds_check_mode, None, bag_begin, bag_count)
            want = return_max_indices or max_indices is not None
            res = _fwd_max(self._tables(), indices, offsets, B, out, bag_begin, bag_count, self._pad_dev(), self._out16,
                           (True if max_indices is None else max_indices) if want else False)
            return res if want else res[0]
        if return_max_indices or max_indices is not None:
            raise ValueError('return_max_indices / max_indices need max pooling (MaxBatchedEmbeddingBagMI355)')
        if split_bags and self.padding_idx is not None:
            raise ValueError("lookup(split_bags=True) does not take padding_idx")
        if self._mean and (split_bags or per_sample_weights is not None):
            raise ValueError('pooling_mode="mean" does not take split_bags=True' if split_bags else _MEAN_WEIGHTED)
        if split_bags and self._out16 is not None:
            raise ValueError("lookup(split_bags=True) does not take a 16-bit output_dtype")
        _require_device(self.weights, "BatchedEmbeddingBagMI355.weights")
        B = self._batch_of(offsets, indices) if batch is None else batch
        if self.bounds_check_mode != "none":
            self._sanitize(self._tables(), indices, offsets, B, self.bounds_check_mode, per_sample_weights, bag_begin, bag_count)
        return _fwd(self._tables(), indices, offsets, B, per_sample_weights, out, bag_begin, bag_count, split_bags,
                    pad=self._pad_dev(), mean=self._mean, out16=self._out16)

    def lookup_sequence(self, indices, offsets, batch: Optional[int] = None, out=None, bag_begin=0, bag_count=None):
        """The UN-POOLED forward over the module's T tables (fbgemm TBE's sequence embeddings, ``PoolingMode.NONE``): ``[N, D]`` in the
        module's ``output_dtype``, ``N = indices.numel()``, row ``j`` = row ``indices[j]`` of the table that owns lookup position ``j``
        (table ``t`` owns ``[offsets[t * B], offsets[(t + 1) * B])``) -- one launch, ``pm_embedding_gather``.  With the tables' own dtype
        as ``output_dtype`` the stored bits come back; fp32 (the default) widens 16-bit rows exactly; anything else is rounded once.
        Runs after ``bounds_check_mode``, like ``lookup``.  ``bag_begin/bag_count`` select a batch slice: only the rows of lookups
        inside it are written -- a caller's ``out`` keeps every other row, a tensor allocated here holds zeros there.
        ``padding_idx`` does not affect it (``nn.Embedding``'s forward rule: the padding row comes back as stored).  Needs one common
        embedding dim; ``layout="blocked"``, mixed dims, ``pooling_mode="mean"`` (a mean module has no un-pooled form) and an ``out``
        that is not a contiguous ``[N, D]`` tensor of ``output_dtype`` on the module's device raise ValueError.  The gradient of
        sequence rows: ``sequence_scatter_add_`` / ``sequence_optimizer_step_`` / ``sequence_dense_grad``, or ``forward_sequence`` for
        autograd (see README, "Un-pooled lookups")."""
        if self.layout == "blocked":
            raise ValueError('lookup_sequence does not take layout="blocked"')
        if len(set(self.dims)) != 1:
            raise ValueError("lookup_sequence needs one common embedding dim")
        if self._mean:
            raise ValueError('lookup_sequence does not take pooling_mode="mean": a mean module has no un-pooled form')
        self._max_refuses("lookup_sequence", "a max module has no un-pooled form")
        if out is not None:
            _check_rows_out(out, indices.numel(), self.dims[0], self.output_dtype, self.weights.device)
        _require_device(self.weights, "BatchedEmbeddingBagMI355.weights")
        B = self._batch_of(offsets, indices) if batch is None else batch
        if self.bounds_check_mode != "none":
            self._sanitize(self._tables(), indices, offsets, B, self.bounds_check_mode, None, bag_begin, bag_count)
        return _gather(self._tables(), indices, offsets, B, self.output_dtype, out, bag_begin, bag_count)

    def sanitize_(self, indices, offsets, batch: Optional[int] = None, mode=None) -> None:
        """The sanitiser on its own, in front of any entry point that does not run it (everything but ``forward`` / ``lookup``):
        repairs ``indices`` / ``offsets`` in place on the current stream, without a synchronisation (``"fatal"``: one, and nothing
        is written).  ``mode``: default the module's ``bounds_check_mode``, ``"warning"`` where that is ``"none"``;
        ``bounds_report()`` reads what it found.  One table: pass ``batch=`` (see the class)."""
        _require_device(self.weights, "BatchedEmbeddingBagMI355.weights")
        B = self._batch(offsets, indices, batch)
        mode = bounds_check_mode_name(mode) if mode is not None else self.bounds_check_mode
        self._sanitize(self._tables(), indices, offsets, B, "warning" if mode == "none" else mode)

    def lookup_quantized(self, indices, offsets, bitwidth: int, per_sample_weights=None, out=None, bag_begin=0,
                         bag_count=None, batch: Optional[int] = None):
        """Forward with a row-wise quantised output (``bitwidth`` 16 / 8 / 4 / 2): one quantised row per pooled vector,
        uint8 ``(B, T, row_bytes)`` (``(T, B, row_bytes)`` for the ``tbd`` layout) -- the payload of a quantised
        all-to-all (the reference's ``--bitwidth``), written by the lookup kernel itself.  ``param_amd.quant.
        dequantize_rows`` restores fp32; the bytes equal ``quantize_rows(lookup(...))``.  Whole-batch requests the staged
        kernel does not take (ragged bags) run as lookup + quantiser; a batch SLICE of such a request raises (PM_ERR_UNSUPPORTED)."""
        if self.padding_idx is not None:
            raise ValueError("lookup_quantized does not take padding_idx")
        if self._mean:
            raise ValueError('lookup_quantized does not take pooling_mode="mean"')
        self._max_refuses("lookup_quantized")
        if self._out16 is not None:
            raise ValueError("lookup_quantized does not take a 16-bit output_dtype (its fp16 rows are a payload format of its own)")
        _require_device(self.weights, "BatchedEmbeddingBagMI355.weights")
        B = self._batch_of(offsets, indices) if batch is None else batch
        return _fwd_quantized(self._tables(), indices, offsets, B, bitwidth, per_sample_weights, out, bag_begin, bag_count)

    def forward(self, indices, offsets, per_sample_weights=None, return_max_indices: bool = False):
        if self._max:
            # (no fused update for max: the result carries a backward node only to refuse ``.backward()`` with the reason)
            res = self.lookup(indices, offsets, per_sample_weights, return_max_indices=return_max_indices)
            if not (self.fused_update and torch.is_grad_enabled()):
                return res
            out = _FusedMaxRefusedFn.apply(self._anchor, res[0] if return_max_indices else res)
            return (out, res[1]) if return_max_indices else out
        if return_max_indices:
            raise ValueError('return_max_indices needs max pooling (MaxBatchedEmbeddingBagMI355)')
        if self.fused_update and torch.is_grad_enabled():
            return _FusedUpdateFn.apply(self._anchor, self, indices, offsets, per_sample_weights)
        return self.lookup(indices, offsets, per_sample_weights)

    def sort_indices(self, indices, offsets, per_sample_weights=None, batch: Optional[int] = None,
                     for_adagrad: Optional[bool] = None, pooling: Optional[int] = None) -> None:
        """Pre-sort the request for the deterministic backward (can overlap the forward).  ``for_adagrad`` (default: what
        the module's optimizer is): the fused row-wise Adagrad needs a one-phase sort, the scatter-add apply may use two."""
        B = self._batch(offsets, indices, batch)
        if for_adagrad is None:
            for_adagrad = self.optimizer in ("rowwise_adagrad", "adagrad")
        _sort_indices(self._tables(), indices, offsets, B, per_sample_weights, phases=1 if for_adagrad else 2, pooling=pooling)

    def _max_grad_args(self, what: str, per_sample_weights, method: str = "sorted", presorted: bool = False) -> None:
        """what the two gradient calls of a max module refuse, on the host and before anything is launched"""
        if per_sample_weights is not None:
            raise ValueError(_MAX_WEIGHTED)
        if method != "sorted" or presorted:
            raise ValueError(f'{what} with pooling_mode="max" runs the sequence backward on the expanded gradient: method="atomic" and '
                             "presorted=True are not taken")
        if len(set(self.dims)) != 1:
            raise ValueError(_MAX_MIXED)

    def scatter_add_(self, grad, indices, offsets, alpha: float, per_sample_weights=None,
                     batch: Optional[int] = None, bag_begin=0, bag_count=None, method: str = "sorted",
                     presorted: bool = False, pooling: Optional[int] = None, max_indices=None):
        """In place ``W_t[idx[j]] += alpha * psw[j] * grad(t, bag(j))`` (alpha = -lr: SGD step).  ``pooling``: the
        caller's word that every bag has exactly that many lookups (saves the one-off device check of a new request).
        ``pooling_mode="max"``: in place ``W_t[max_indices(t, b)[c], c] += alpha * grad(t, b)[c]`` (``_max_bwd``); ``max_indices``: what
        ``lookup(..., return_max_indices=True)`` returned for the request, or ``None`` to recompute it with one forward launch.  A
        looked-up row that wins no column receives ``alpha * 0.0``: with a positive ``alpha`` a stored -0.0 there becomes +0.0."""
        if self._max:
            self._max_grad_args("scatter_add_", per_sample_weights, method, presorted)
        elif max_indices is not None:
            raise ValueError('max_indices needs max pooling (MaxBatchedEmbeddingBagMI355)')
        ts = self._tables()
        B = self._batch(offsets, indices, batch)
        if self._max:
            _max_bwd(ts, grad, indices, offsets, B, ts.d_ptrs, self.weights.dtype, alpha, self._pad_dev(), max_indices, bag_begin, bag_count,
                     self._out16)
            return
        _bwd(ts, grad, indices, offsets, B, ts.d_ptrs, self.weights.dtype, alpha, per_sample_weights,
             bag_begin, bag_count, method, presorted, pooling, pad=self._pad_dev(), mean=self._mean, out16=self._out16)

    def sort_status(self, indices, offsets, per_sample_weights=None, batch: Optional[int] = None, bag_begin=0, bag_count=None) -> dict:
        """status of the last key sort on this module's workspace (synchronises)"""
        B = self._batch(offsets, indices, batch)
        return sort_status(self._tables(), indices, offsets, B, per_sample_weights, bag_begin, bag_count)

    def momentum_table(self, t: int) -> torch.Tensor:
        """Adagrad state of table t (allocated zero on first use): ``[rows_t]`` for ``optimizer="rowwise_adagrad"``,
        ``[rows_t, dims_t]`` for the element-wise ``optimizer="adagrad"``"""
        elem = self.optimizer == "adagrad"
        per_row = self.dims if elem else [1] * len(self.rows)      # state values per table row
        if self.momentum is None:
            self.momentum = torch.zeros(sum(r * w for r, w in zip(self.rows, per_row)), dtype=torch.float32, device=self.weights.device)
        if self._mom_base != (self.momentum.data_ptr(), self.momentum.device):     # first use, or moved by .to()
            starts = [0]
            for r, w in zip(self.rows[:-1], per_row[:-1]):
                starts.append(starts[-1] + r * w)
            self._mom_starts = starts
            self._mom_ptrs = torch.tensor([self.momentum.data_ptr() + 4 * s for s in starts], dtype=torch.int64,
                                          device=self.momentum.device)
            self._mom_base = (self.momentum.data_ptr(), self.momentum.device)
        s = self._mom_starts[t]
        if elem:
            return self.momentum[s:s + self.rows[t] * self.dims[t]].view(self.rows[t], self.dims[t])
        return self.momentum[s:s + self.rows[t]]

    def adagrad_step_(self, grad, indices, offsets, per_sample_weights=None, batch: Optional[int] = None,
                      presorted: bool = False, pooling: Optional[int] = None):
        """Fused backward + exact row-wise Adagrad (TBE ``EXACT_ROWWISE_ADAGRAD``, the optimizer the reference
        configures at comms_utils.py:2014): ``m[r] += mean_d(G[r,d]^2); W[r] -= lr / (sqrt(m[r]) + eps) * G[r]``,
        with the module's ``weight_decay`` / ``weight_decay_mode`` (l2 | decouple) and, for 16-bit tables,
        ``stochastic_rounding``.  With ``optimizer="adagrad"``: exact ELEMENT-wise Adagrad (TBE ``EXACT_ADAGRAD``,
        ``torch.optim.Adagrad``'s arithmetic), one state value per weight: ``s[r,d] += G[r,d]^2;
        W[r,d] -= lr * G[r,d] / (sqrt(s[r,d]) + eps)``, same options (l2 adds ``wd * W`` to ``G`` first).  (Called on a module of
        any other optimizer, the step is the row-wise one, as before.)"""
        self._max_refuses("adagrad_step_", _MAX_FUSED)
        self.momentum_table(0)
        B = self._batch(offsets, indices, batch)
        self._sr_step += 1          # a fresh stochastic-rounding stream every step, reproducible run to run
        _adagrad(self._tables(), grad, indices, offsets, B, self._mom_ptrs, self.learning_rate, self.eps,
                 per_sample_weights, presorted, self.weight_decay, self.weight_decay_mode, self.stochastic_rounding,
                 seed=0x5EED0000 + self._sr_step, pooling=pooling, elementwise=self.optimizer == "adagrad", pad=self._pad_dev(),
                 mean=self._mean, out16=self._out16)

    def optimizer_step_(self, grad, indices, offsets, per_sample_weights=None, batch: Optional[int] = None,
                        presorted: bool = False):
        """what ``.backward()`` applies when ``fused_update`` is on"""
        self._max_refuses("optimizer_step_", _MAX_FUSED)
        if self.optimizer in ("rowwise_adagrad", "adagrad"):
            self.adagrad_step_(grad, indices, offsets, per_sample_weights, batch, presorted)
        else:
            self.scatter_add_(grad, indices, offsets, alpha=-self.learning_rate, per_sample_weights=per_sample_weights,
                              batch=batch, presorted=presorted)

    def _dense_grad_buffers(self, ts: _TableSet, out):
        """the destinations of a dense gradient -- fresh zeros, or a caller's ``out`` checked -- and their device pointer array"""
        if out is None:
            outs = [torch.zeros(r, d, dtype=torch.float32, device=ts.device) for r, d in zip(self.rows, self.dims)]
        else:
            outs = list(out)
            if len(outs) != len(self.rows) or any(o.dtype != torch.float32 or tuple(o.shape) != (r, d) or not o.is_contiguous() or
                                                  o.device != ts.device for o, r, d in zip(outs, self.rows, self.dims)):
                raise ValueError("out must hold one contiguous float32 [rows_t, dims_t] tensor per table on the module's device")
        return outs, torch.tensor([o.data_ptr() for o in outs], dtype=torch.int64, device=ts.device)

    def dense_grad(self, grad, indices, offsets, per_sample_weights=None, batch: Optional[int] = None,
                   method: str = "sorted", out: Optional[Sequence[torch.Tensor]] = None, max_indices=None):
        """fp32 dense gradients (list, one per table) -- small tables / parity tests only.  ``out``: one contiguous fp32
        ``[rows_t, dims_t]`` buffer per table to ADD the gradient to (default: fresh zeros); a padding row of such a buffer is
        exactly what it was before the call.  ``pooling_mode="max"``: ``grad(t, b)[c]`` lands in row ``max_indices(t, b)[c]``
        (``max_indices``: as for ``scatter_add_``)."""
        if self._max:
            self._max_grad_args("dense_grad", per_sample_weights, method)
        elif max_indices is not None:
            raise ValueError('max_indices needs max pooling (MaxBatchedEmbeddingBagMI355)')
        ts = self._tables()
        B = self._batch(offsets, indices, batch)
        outs, d_ptrs = self._dense_grad_buffers(ts, out)
        if self._max:
            _max_bwd(ts, grad, indices, offsets, B, d_ptrs, torch.float32, 1.0, self._pad_dev(), max_indices, out16=self._out16)
            return outs
        _bwd(ts, grad, indices, offsets, B, d_ptrs, torch.float32, 1.0, per_sample_weights, method=method, pad=self._pad_dev(),
             mean=self._mean, out16=self._out16)
        return outs

    def sparse_grad(self, grad, indices, offsets, per_sample_weights=None, batch: Optional[int] = None, bag_begin=0,
                    bag_count=None):
        """Coalesced sparse gradients of the tables, without a dense buffer: a list of T ``(rows_t, values_t)`` pairs -- ``rows_t``
        the distinct rows table t's lookups (of the bag slice) hit, ascending int64; ``values_t`` fp32 ``[U_t, D_t]``,
        ``values_t[k] = sum_{j: idx_j = rows_t[k]} psw[j] * grad[t, bag(j)]`` summed in the sorted backward's order (bit-identical
        to ``sort_indices`` + ``scatter_add_(alpha=1, presorted=True)`` into zeroed fp32 tables, read at ``rows_t``).  A table with
        no lookups gives empty tensors.  ``grad`` has the shape ``scatter_add_`` takes for the module's layout.  The call
        synchronises once (to read the U_t and allocate exactly), as torch's ``coalesce()`` does -- once per 1024 tables for larger
        requests, which are split into independent calls.  The gradient with respect to ``per_sample_weights`` is a call of its
        own: ``per_sample_weights_grad``."""
        self._max_refuses("sparse_grad", "the max gradient is dense (torch's max mode does not support sparse weights)")
        B = self._batch(offsets, indices, batch)
        return _sparse_grad(self._tables(), grad, indices, offsets, B, per_sample_weights, bag_begin, bag_count,
                            pads=self.padding_idx, mean=self._mean, pad=self._pad_dev(), out16=self._out16)

    def per_sample_weights_grad(self, grad, indices, offsets, batch: Optional[int] = None, out=None, bag_begin=0, bag_count=None):
        """Gradient of ``per_sample_weights``: fp32 ``[N]``, ``out[j] = sum_c grad[t, bag(j)][c] * table_t[indices[j], c]`` -- what
        ``torch.nn.functional.embedding_bag(..., mode="sum", per_sample_weights=w)`` returns as ``w.grad`` and fbgemm's TBE as the
        ``indice_weights`` gradient.  One gather kernel over the rows the forward read (``pm_embbag_psw_grad``), deterministic:
        products and adds rounded to fp32 one by one in a fixed order (include/param_amd.h), the same bits for every launch shape.
        ``grad`` has the shape ``scatter_add_`` takes for the module's layout.  ``bag_begin/bag_count`` select a batch slice:
        entries of lookups outside it are zero in a tensor the method allocates and untouched in a caller's ``out``.  Any number
        of tables (no sort, no workspace).  Call it BEFORE an in-place update of the tables."""
        if self._mean:
            raise ValueError('per_sample_weights_grad: pooling_mode="mean" is unweighted')
        self._max_refuses("per_sample_weights_grad", "max pooling is unweighted")
        _require_device(self.weights, "BatchedEmbeddingBagMI355.weights")
        B = self._batch(offsets, indices, batch)
        return _psw_grad(self._tables(), grad, indices, offsets, B, None, out, bag_begin, bag_count, pad=self._pad_dev(), out16=self._out16)

    # -- sequence (un-pooled) gradients ----------------------------------------------------------
    def _seq_request(self, what: str, indices, offsets, batch, grad=None):
        """What the sequence calls share, refusals first and on the host: ``(table set, B, fp32 gradient or None)``.  ``grad`` is ``[N, D]``
        in fp32 or the module's 16-bit ``output_dtype``; a 16-bit one is widened exactly, once, into an fp32 scratch (a torch cast:
        exact, and ``[N, D]`` has no bag structure for ``pm_embbag_grad_widen``); the caller's tensor is never modified."""
        if self.layout == "blocked":
            raise ValueError(f'{what} does not take layout="blocked"')
        if len(set(self.dims)) != 1:
            raise ValueError(f"{what} needs one common embedding dim")
        if self._mean:
            raise ValueError(f'{what} does not take pooling_mode="mean": a mean module has no un-pooled form')
        self._max_refuses(what, "a max module has no un-pooled form")
        if grad is not None:
            shape = (indices.numel(), self.dims[0])
            if (grad.dtype != torch.float32 and grad.dtype != self._out16) or tuple(grad.shape) != shape:
                also = "" if self._out16 is None else f" or {str(self._out16).replace('torch.', '')} (the module's output_dtype)"
                raise ValueError(f"{what}: grad must be float32{also} of shape {shape}, one row per lookup position")
            _require_device(grad, "grad")
            grad = grad.contiguous()
            if grad.dtype != torch.float32:
                grad = grad.float()
        _require_device(self.weights, "BatchedEmbeddingBagMI355.weights")
        return self._tables(), self._batch(offsets, indices, batch), grad

    def sequence_sort_indices(self, indices, offsets, batch: Optional[int] = None, bag_begin=0, bag_count=None) -> None:
        """Pre-sort a sequence request (``pm_embseq_sort_indices``; can overlap the forward): keys ``(table, row)``, values the lookup
        positions.  ``sequence_scatter_add_`` / ``sequence_optimizer_step_`` with ``presorted=True`` consume it; the pooled calls refuse
        a workspace that holds a sequence sort, and the other way round.  At most 1024 tables."""
        ts, B, _ = self._seq_request("sequence_sort_indices", indices, offsets, batch)
        _seq_sort_indices(ts, indices, offsets, B, bag_begin, bag_count)

    def sequence_scatter_add_(self, grad, indices, offsets, alpha: float, batch: Optional[int] = None, bag_begin=0, bag_count=None,
                              presorted: bool = False) -> None:
        """The batched backward of ``lookup_sequence``: in place ``W_t[indices[j]] += alpha * grad[j]`` for every lookup position ``j`` of
        the bag slice, ``t`` the table that owns ``j`` -- per row in ascending position order, deterministic, no atomics; one sort and one
        apply for all T tables (``pm_embseq_bwd_fused``; 1024 tables per call).  ``grad``: ``[N, D]`` fp32 or the module's 16-bit
        ``output_dtype``; rows of positions outside the slice are never read.  Padding rows keep their bits.  Does not run
        ``bounds_check_mode`` (``sanitize_`` is the call on its own)."""
        ts, B, g = self._seq_request("sequence_scatter_add_", indices, offsets, batch, grad)
        self._seq_scatter(ts, g, indices, offsets, B, ts.d_ptrs, self.weights.dtype, alpha, bag_begin, bag_count, presorted)

    def _seq_scatter(self, ts, g, indices, offsets, B, dst_ptrs_dev, dst_dtype, alpha, bag_begin=0, bag_count=None, presorted=False) -> None:
        L, s, dt, D = _lib.load(), _stream_ptr(), _WDTYPE[dst_dtype], ts.dims[0]

        def call(fn):
            return lambda sub, gp, t0, max_rows, ws: fn(ctypes.byref(sub), gp, D, dst_ptrs_dev.data_ptr() + 8 * t0, dt, float(alpha), max_rows,
                                                        ws.data_ptr(), ws.numel(), s)
        _seq_bwd(ts, g, indices, offsets, B, bag_begin, bag_count, presorted, call(L.pm_embseq_bwd_fused), call(L.pm_embseq_bwd_sorted),
                 _PadGuard(ts, self._pad_dev(), dst_ptrs_dev, dst_dtype))

    def sequence_optimizer_step_(self, grad, indices, offsets, batch: Optional[int] = None, presorted: bool = False) -> None:
        """The module's optimizer on sequence gradient rows (what ``forward_sequence(...).backward()`` applies with ``fused_update``): SGD
        (``sequence_scatter_add_`` with ``alpha = -learning_rate``), exact row-wise Adagrad or exact element-wise Adagrad, with the
        module's weight decay and stochastic rounding -- the arithmetic of ``optimizer_step_`` on the one-table request "one bag per
        lookup", for all T tables in one sort and one apply (``pm_embseq_bwd_fused_adagrad``).  Stochastic rounding draws from the same
        ``_sr_step`` seed stream as ``adagrad_step_``."""
        ts, B, g = self._seq_request("sequence_optimizer_step_", indices, offsets, batch, grad)
        if self.optimizer not in ("rowwise_adagrad", "adagrad"):
            self._seq_scatter(ts, g, indices, offsets, B, ts.d_ptrs, self.weights.dtype, -self.learning_rate, presorted=presorted)
            return
        self.momentum_table(0)
        self._sr_step += 1          # a fresh stochastic-rounding stream every step, reproducible run to run
        L, s, wdt, D, elem = _lib.load(), _stream_ptr(), _WDTYPE[ts.dtype], ts.dims[0], self.optimizer == "adagrad"
        seed, mom = 0x5EED0000 + self._sr_step, self._mom_ptrs

        def call(fn):      # (every table range gets a seed of its own, as in _adagrad)
            def issue(sub, gp, t0, max_rows, ws):
                opt = _lib.pm_rowwise_adagrad(float(self.learning_rate), float(self.eps), float(self.weight_decay),
                                              _WD_MODES[self.weight_decay_mode], 1 if self.stochastic_rounding else 0, 0,
                                              (seed + (t0 << 32)) & (2**64 - 1))
                return fn(ctypes.byref(sub), gp, D, ts.d_ptrs.data_ptr() + 8 * t0, wdt, mom.data_ptr() + 8 * t0, ctypes.byref(opt),
                          1 if elem else 0, max_rows, ws.data_ptr(), ws.numel(), s)
            return issue
        guard = _PadGuard(ts, self._pad_dev(), ts.d_ptrs, ts.dtype, mom, _lib.PM_PAD_STATE_ELEM if elem else _lib.PM_PAD_STATE_ROW)
        _seq_bwd(ts, g, indices, offsets, B, 0, None, presorted, call(L.pm_embseq_bwd_fused_adagrad), call(L.pm_embseq_bwd_sorted_adagrad),
                 guard)

    def sequence_dense_grad(self, grad, indices, offsets, batch: Optional[int] = None, out: Optional[Sequence[torch.Tensor]] = None):
        """fp32 dense gradients of sequence rows (list, one ``[rows_t, D]`` per table): ``out_t[r] += sum of grad[j]`` over table t's
        lookups of row r in position order -- ``aten::embedding_dense_backward`` per table, in one sort and one apply.  ``out``: as for
        ``dense_grad`` (buffers to ADD to; default fresh zeros; a padding row is exactly what it was before the call)."""
        ts, B, g = self._seq_request("sequence_dense_grad", indices, offsets, batch, grad)
        outs, d_ptrs = self._dense_grad_buffers(ts, out)
        self._seq_scatter(ts, g, indices, offsets, B, d_ptrs, torch.float32, 1.0)
        return outs

    def forward_sequence(self, indices, offsets, batch: Optional[int] = None):
        """``lookup_sequence`` with autograd glue: with ``fused_update`` and grad enabled, ``.backward(g)`` on the ``[N, D]`` result applies
        ``sequence_optimizer_step_(g, ...)`` in place (no weight.grad), as ``forward`` does for pooled lookups."""
        if self.fused_update and torch.is_grad_enabled():
            return _FusedSequenceFn.apply(self._anchor, self, indices, offsets, batch)
        return self.lookup_sequence(indices, offsets, batch)

    def extra_repr(self) -> str:
        return f"output_dtype={self.output_dtype}" if self._out16 is not None else ""

    def check(self, indices, offsets, per_sample_weights=None, batch: Optional[int] = None) -> None:
        B = self._batch(offsets, indices, batch)
        check_request(self._tables(), indices, offsets, B, per_sample_weights)


class MaxBatchedEmbeddingBagMI355(BatchedEmbeddingBagMI355):
    """:class:`BatchedEmbeddingBagMI355` with MAX pooling: T tables in one slab, max-pooled by one launch.  A class of its own because
    fbgemm's ``PoolingMode`` has no such member and ``BatchedEmbeddingBagMI355(pooling_mode="max")`` keeps raising ValueError, as it
    always did.  The constructor's arguments are the parent's; ``pooling_mode``, if given, must be the string ``"max"`` (any case).
    The attribute ``pooling_mode`` is ``"max"``.

    ``forward`` / ``lookup`` (``out=``, batch slices, ``bd`` / ``tbd``, ``padding_idx``, ``output_dtype`` and ``bounds_check_mode``
    included) give, per column, the maximum over the bag's kept lookups by torch's ``mode="max"`` rule (include/param_amd.h, MAX
    POOLING); ``return_max_indices=True`` also returns the int32 rows that supplied the maxima (-1 for a bag without kept lookups).
    ``dense_grad`` and ``scatter_add_`` take ``max_indices=`` (``None``: recomputed by one forward launch) and send ``grad(t, b)[c]`` to
    that row, once: the gradient is expanded to an fp32 ``[N, D]`` scratch (one more launch) and applied by the sequence backward, 1024
    tables per call; they need one common embedding dim.  ``per_sample_weights``, ``optimizer_step_``, ``adagrad_step_``, the fused
    ``.backward()``, ``sparse_grad``, ``per_sample_weights_grad``, ``lookup_sequence`` / ``sequence_*``, ``lookup(split_bags=True)``,
    ``lookup_quantized`` and ``layout="blocked"`` raise ValueError."""

    _POOLING = "max"

    def __init__(self, rows: Sequence[int], dims, *args, pooling_mode="max", **kw):
        if not (isinstance(pooling_mode, str) and pooling_mode.lower() == "max"):
            raise ValueError(f'MaxBatchedEmbeddingBagMI355 pools with max: pooling_mode must be the string "max", got {pooling_mode!r}')
        super().__init__(rows, dims, *args, **kw)
