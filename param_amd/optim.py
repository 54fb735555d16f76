"""Lazy Adam over the coalesced sparse gradients this package produces (``pm_sparse_rows_adam``, csrc/sparse_rows_adam.hip).

* :func:`sparse_adam_rows_` -- one launch updates T tables in place from the ``(rows_t, values_t)`` list that
  ``BatchedEmbeddingBagMI355.sparse_grad`` returns.
* :class:`SparseAdamMI355`  -- a ``torch.optim.Optimizer`` with ``torch.optim.SparseAdam``'s arguments, checks and state keys (a
  ``state_dict`` moves between the two) and one addition, decoupled ``weight_decay`` on the touched rows.  It consumes the sparse
  ``.grad`` of ``EmbeddingBagMI355(sparse=True)`` / ``EmbeddingMI355(sparse=True)``.

The rule is fixed in include/param_amd.h (SPARSE-ROW ADAM) and restated in numpy by tests/sparse_adam_rules.py; the host computes the
step's five scalars in double precision and rounds each once to fp32.  There is no CPU path: a tensor that is not on a ROCm device raises.
"""
from __future__ import annotations

import ctypes
import math
from typing import Sequence, Tuple

import torch

from . import _lib
from .embedding_bag import _WDTYPE, _require_device, _stream_ptr

_MAX_DIM = 4096
_NONTEMPORAL = True      # cache policy of SparseAdamMI355's launches (tools/sparse_adam_probe.py measures both): a speed matter only


def _step_scalars(step: int, lr: float, betas: Tuple[float, float], eps: float, weight_decay: float, maximize: bool,
                  nontemporal: bool) -> _lib.pm_sparse_adam:
    """one step's scalars, in double precision; ctypes rounds each once to fp32 (round to nearest even)"""
    beta1, beta2 = float(betas[0]), float(betas[1])
    step_size = float(lr) * math.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step)
    return _lib.pm_sparse_adam(1.0 - beta1, 1.0 - beta2, float(eps), step_size, 1.0 - float(lr) * float(weight_decay),
                               1 if maximize else 0, 1 if nontemporal else 0, 0)


def sparse_adam_rows_(tables: Sequence[torch.Tensor], grads: Sequence[Tuple[torch.Tensor, torch.Tensor]],
                      exp_avg: Sequence[torch.Tensor], exp_avg_sq: Sequence[torch.Tensor], step: int, lr: float,
                      betas: Tuple[float, float], eps: float, weight_decay: float = 0.0, maximize: bool = False,
                      nontemporal: bool = True) -> None:
    """One lazy Adam / AdamW step of T tables, in place, in ONE launch.  ``grads[t] = (rows_t, values_t)``: int64 ``[U_t]`` distinct
    row ids and fp32 ``[U_t, D_t]`` values (``BatchedEmbeddingBagMI355.sparse_grad``'s result).  ``tables[t]``: ``[rows_t, D_t]`` of one
    dtype (fp32 / bf16 / fp16); ``exp_avg[t]`` / ``exp_avg_sq[t]``: fp32 of the table's shape.  ``step`` counts from 1.  Rows that are not
    listed, and their state, are untouched; a table with ``U_t == 0`` costs nothing.  ``nontemporal``: cache policy of the gradient and
    state accesses (a speed matter only).  Stream-ordered: the pointer and prefix arrays go to the device in one small copy."""
    T = len(tables)
    if not (len(grads) == len(exp_avg) == len(exp_avg_sq) == T):
        raise ValueError("tables, grads, exp_avg and exp_avg_sq must have one entry per table")
    if step < 1:
        raise ValueError(f"step counts from 1 (got {step})")
    for t in range(T):
        for x, what in ((tables[t], "table"), (grads[t][0], "row ids"), (grads[t][1], "gradient values"), (exp_avg[t], "exp_avg"),
                        (exp_avg_sq[t], "exp_avg_sq")):
            _require_device(x, what)
    live = []
    for t in range(T):
        w, (r, g), m, v = tables[t], grads[t], exp_avg[t], exp_avg_sq[t]
        if w.dtype not in _WDTYPE or w.dtype != tables[0].dtype or w.dim() != 2 or not w.is_contiguous():
            raise ValueError("tables must be contiguous 2-D fp32 / bf16 / fp16 tensors of one dtype")
        D = w.shape[1]
        if D % 4 != 0 or not 4 <= D <= _MAX_DIM:
            raise ValueError(f"table {t}: dim must be a multiple of 4 in [4, {_MAX_DIM}] (got {D})")
        for s, what in ((m, "exp_avg"), (v, "exp_avg_sq")):
            if s.dtype != torch.float32 or s.shape != w.shape or not s.is_contiguous():
                raise ValueError(f"table {t}: {what} must be a contiguous float32 tensor of the table's shape")
        if r.dtype != torch.int64 or r.dim() != 1 or not r.is_contiguous():
            raise ValueError(f"table {t}: row ids must be a contiguous 1-D int64 tensor")
        if g.dtype != torch.float32 or tuple(g.shape) != (r.numel(), D) or not g.is_contiguous() or g.data_ptr() % 16 != 0:
            raise ValueError(f"table {t}: gradient values must be a contiguous, 16-byte aligned float32 [{r.numel()}, {D}] tensor")
        if len({x.device for x in (w, r, g, m, v, tables[0])}) != 1:
            raise ValueError("every tensor of a call must be on one device")
        if r.numel():
            live.append((w, r, g, m, v))
    if not live:
        return
    n = len(live)
    prefix = [0]
    for _, r, _, _, _ in live:
        prefix.append(prefix[-1] + r.numel())
    # one host array, one copy: five pointer arrays [n], the prefix [n + 1], then the dims as int32
    host = torch.empty(6 * n + 1 + (n + 1) // 2, dtype=torch.int64)
    host[:6 * n + 1] = torch.tensor([x.data_ptr() for k in range(5) for x in (e[k] for e in live)] + prefix, dtype=torch.int64)
    host[6 * n + 1:].view(torch.int32)[:n] = torch.tensor([e[0].shape[1] for e in live], dtype=torch.int32)
    dev = live[0][0].device
    with torch.cuda.device(dev):
        args = host.to(dev)
        base = args.data_ptr()
        opt = _step_scalars(step, lr, betas, eps, weight_decay, maximize, nontemporal)
        _lib.check(_lib.load().pm_sparse_rows_adam(n, prefix[-1], max(e[0].shape[1] for e in live), base, _WDTYPE[live[0][0].dtype],
                                                   base + 8 * n, base + 16 * n, base + 24 * n, base + 32 * n, base + 8 * (6 * n + 1),
                                                   base + 40 * n, ctypes.byref(opt), _stream_ptr()))


class SparseAdamMI355(torch.optim.Optimizer):
    """``torch.optim.SparseAdam`` on the HIP path: lazy, bias-corrected Adam over sparse COO gradients (no amsgrad), plus decoupled
    ``weight_decay`` (AdamW's, applied to the touched rows only).  Parameters are 2-D tables in fp32, bf16 or fp16 on a ROCm device;
    the state (``step``, ``exp_avg``, ``exp_avg_sq`` -- torch's keys) is always fp32.  ``step()`` coalesces a gradient that is not
    coalesced, skips parameters without one, and sends all parameters of a group that share a dtype (and a step count) through ONE
    ``pm_sparse_rows_adam`` launch."""

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, maximize: bool = False,
                 weight_decay: float = 0.0):
        if not 0.0 < lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 < eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, {"lr": lr, "betas": betas, "eps": eps, "maximize": maximize, "weight_decay": weight_decay})
        sparse_params, complex_params = [], []
        for index, group in enumerate(self.param_groups):
            for d_index, p in enumerate(group["params"]):
                if p.is_sparse:
                    sparse_params.append([index, d_index])
                if p.is_complex():
                    complex_params.append([index, d_index])
        if sparse_params:
            raise ValueError(f"Sparse params at indices {sparse_params}: SparseAdam requires dense parameter tensors")
        if complex_params:
            raise ValueError(f"Complex params at indices {complex_params}: SparseAdam does not support complex parameters")
        for index, group in enumerate(self.param_groups):
            for d_index, p in enumerate(group["params"]):
                if p.dim() != 2 or p.dtype not in _WDTYPE:
                    raise ValueError(f"SparseAdamMI355: parameter {d_index} of group {index} must be a 2-D fp32 / bf16 / fp16 table")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            buckets = {}                                  # (dtype, step, device) -> the five lists of one launch
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.grad.is_sparse:
                    raise RuntimeError("SparseAdam does not support dense gradients, please consider Adam instead")
                _require_device(p, "parameter")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
                for key in ("exp_avg", "exp_avg_sq"):     # a state_dict loaded from torch.optim.SparseAdam holds the parameter's dtype
                    if state[key].dtype != torch.float32:
                        state[key] = state[key].float()
                state["step"] = int(state["step"]) + 1
                g = p.grad if p.grad.is_coalesced() else p.grad.coalesce()
                b = buckets.setdefault((p.dtype, state["step"], p.device), ([], [], [], []))
                b[0].append(p.data)
                b[1].append((g._indices()[0].contiguous(), g._values().float().contiguous()))
                b[2].append(state["exp_avg"])
                b[3].append(state["exp_avg_sq"])
            for (_, step, _), (tables, grads, m, v) in buckets.items():
                sparse_adam_rows_(tables, grads, m, v, step, float(group["lr"]), group["betas"], group["eps"],
                                  group.get("weight_decay", 0.0), group.get("maximize", False), _NONTEMPORAL)
        return loss
