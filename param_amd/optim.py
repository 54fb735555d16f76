"""Optimizers over the coalesced sparse gradients this package produces: lazy Adam (``pm_sparse_rows_adam``, csrc/sparse_rows_adam.hip),
Adagrad, row-wise Adagrad and SGD (``pm_sparse_rows_adagrad`` / ``pm_sparse_rows_sgd``, csrc/sparse_rows_step.hip).

* :func:`sparse_adam_rows_` -- one launch updates T tables in place from the ``(rows_t, values_t)`` list that
  ``BatchedEmbeddingBagMI355.sparse_grad`` returns.
* :class:`SparseAdamMI355`  -- a ``torch.optim.Optimizer`` with ``torch.optim.SparseAdam``'s arguments, checks and state keys (a
  ``state_dict`` moves between the two) and one addition, decoupled ``weight_decay`` on the touched rows.  It consumes the sparse
  ``.grad`` of ``EmbeddingBagMI355(sparse=True)`` / ``EmbeddingMI355(sparse=True)``.
* :func:`sparse_adagrad_rows_` / :class:`SparseAdagradMI355` -- ``torch.optim.Adagrad`` on sparse gradients, element-wise or
  (``rowwise=True``) with one state value per row; :func:`sparse_sgd_rows_` / :class:`SparseSGDMI355` -- ``torch.optim.SGD`` without
  momentum and weight decay.

The rules are fixed in include/param_amd.h (SPARSE-ROW ADAM; SPARSE-ROW ADAGRAD AND SGD) and restated in numpy by
tests/sparse_adam_rules.py and tests/sparse_step_rules.py; the host computes a step's scalars in double precision and rounds each once to fp32.  There is no CPU path: a tensor that is not on a ROCm device raises.
"""
from __future__ import annotations

import ctypes
import math
from typing import Sequence, Tuple

import torch

from . import _lib
from .embedding_bag import _WDTYPE, _require_device, _stream_ptr

_MAX_DIM = 4096
_NONTEMPORAL = True      # cache policy of the optimizers' launches (tools/sparse_adam_probe.py, sparse_step_probe.py measure both): a speed matter only


def _step_scalars(step: int, lr: float, betas: Tuple[float, float], eps: float, weight_decay: float, maximize: bool,
                  nontemporal: bool) -> _lib.pm_sparse_adam:
    """one step's scalars, in double precision; ctypes rounds each once to fp32 (round to nearest even)"""
    beta1, beta2 = float(betas[0]), float(betas[1])
    step_size = float(lr) * math.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step)
    return _lib.pm_sparse_adam(1.0 - beta1, 1.0 - beta2, float(eps), step_size, 1.0 - float(lr) * float(weight_decay),
                               1 if maximize else 0, 1 if nontemporal else 0, 0)


def _launch_rows(entry, tables: Sequence[torch.Tensor], grads: Sequence[Tuple[torch.Tensor, torch.Tensor]], states, step, tail) -> None:
    """The checks and the one small copy every sparse-row step shares.  ``states``: ``(name, per-table tensors, per_row)`` -- fp32 of
    the table's shape, or ``[rows_t]`` when ``per_row``; ``step``: the step count, or None where the rule has none.  Tables with
    ``U_t == 0`` are dropped; with none left nothing is launched.
    ``entry(n, U, max_dim, tables, dtype, row_ids, values, *state arrays, dims, prefix, *tail, stream)`` is the C call."""
    T = len(tables)
    if len(grads) != T or any(len(xs) != T for _, xs, _ in states):
        names = ["tables", "grads"] + [name for name, _, _ in states]
        raise ValueError(", ".join(names[:-1]) + " and " + names[-1] + " must have one entry per table")
    if step is not None and step < 1:
        raise ValueError(f"step counts from 1 (got {step})")
    for t in range(T):
        for x, what in [(tables[t], "table"), (grads[t][0], "row ids"), (grads[t][1], "gradient values")] + [(xs[t], name) for name, xs, _ in states]:
            _require_device(x, what)
    live = []
    for t in range(T):
        w, (r, g) = tables[t], grads[t]
        if w.dtype not in _WDTYPE or w.dtype != tables[0].dtype or w.dim() != 2 or not w.is_contiguous():
            raise ValueError("tables must be contiguous 2-D fp32 / bf16 / fp16 tensors of one dtype")
        D = w.shape[1]
        if D % 4 != 0 or not 4 <= D <= _MAX_DIM:
            raise ValueError(f"table {t}: dim must be a multiple of 4 in [4, {_MAX_DIM}] (got {D})")
        for name, xs, per_row in states:
            s = xs[t]
            if s.dtype != torch.float32 or s.shape != (w.shape[:1] if per_row else w.shape) or not s.is_contiguous():
                raise ValueError(f"table {t}: {name} must be a contiguous float32 tensor of "
                                 + ("one value per table row" if per_row else "the table's shape"))
        if r.dtype != torch.int64 or r.dim() != 1 or not r.is_contiguous():
            raise ValueError(f"table {t}: row ids must be a contiguous 1-D int64 tensor")
        if g.dtype != torch.float32 or tuple(g.shape) != (r.numel(), D) or not g.is_contiguous() or g.data_ptr() % 16 != 0:
            raise ValueError(f"table {t}: gradient values must be a contiguous, 16-byte aligned float32 [{r.numel()}, {D}] tensor")
        entry_t = (w, r, g) + tuple(xs[t] for _, xs, _ in states)
        if len({x.device for x in entry_t + (tables[0],)}) != 1:
            raise ValueError("every tensor of a call must be on one device")
        if r.numel():
            live.append(entry_t)
    if not live:
        return
    n, k = len(live), 3 + len(states)
    prefix = [0]
    for e in live:
        prefix.append(prefix[-1] + e[1].numel())
    # one host array, one copy: k pointer arrays [n], the prefix [n + 1], then the dims as int32
    words = (k + 1) * n + 1
    host = torch.empty(words + (n + 1) // 2, dtype=torch.int64)
    host[:words] = torch.tensor([x.data_ptr() for i in range(k) for x in (e[i] for e in live)] + prefix, dtype=torch.int64)
    host[words:].view(torch.int32)[:n] = torch.tensor([e[0].shape[1] for e in live], dtype=torch.int32)
    dev = live[0][0].device
    with torch.cuda.device(dev):
        args = host.to(dev)
        base = args.data_ptr()
        _lib.check(entry(n, prefix[-1], max(e[0].shape[1] for e in live), base, _WDTYPE[live[0][0].dtype],
                         *[base + 8 * i * n for i in range(1, k)], base + 8 * words, base + 8 * k * n, *tail, _stream_ptr()))


def sparse_adam_rows_(tables: Sequence[torch.Tensor], grads: Sequence[Tuple[torch.Tensor, torch.Tensor]],
                      exp_avg: Sequence[torch.Tensor], exp_avg_sq: Sequence[torch.Tensor], step: int, lr: float,
                      betas: Tuple[float, float], eps: float, weight_decay: float = 0.0, maximize: bool = False,
                      nontemporal: bool = True) -> None:
    """One lazy Adam / AdamW step of T tables, in place, in ONE launch.  ``grads[t] = (rows_t, values_t)``: int64 ``[U_t]`` distinct
    row ids and fp32 ``[U_t, D_t]`` values (``BatchedEmbeddingBagMI355.sparse_grad``'s result).  ``tables[t]``: ``[rows_t, D_t]`` of one
    dtype (fp32 / bf16 / fp16); ``exp_avg[t]`` / ``exp_avg_sq[t]``: fp32 of the table's shape.  ``step`` counts from 1.  Rows that are not
    listed, and their state, are untouched; a table with ``U_t == 0`` costs nothing.  ``nontemporal``: cache policy of the gradient and
    state accesses (a speed matter only).  Stream-ordered: the pointer and prefix arrays go to the device in one small copy."""
    opt = _step_scalars(max(step, 1), lr, betas, eps, weight_decay, maximize, nontemporal)      # (step < 1: refused below)
    _launch_rows(_lib.load().pm_sparse_rows_adam, tables, grads, (("exp_avg", exp_avg, False), ("exp_avg_sq", exp_avg_sq, False)), step,
                 (ctypes.byref(opt),))


def sparse_adagrad_rows_(tables: Sequence[torch.Tensor], grads: Sequence[Tuple[torch.Tensor, torch.Tensor]],
                         state_sum: Sequence[torch.Tensor], step: int, lr: float, lr_decay: float, eps: float, maximize: bool = False,
                         rowwise: bool = False, nontemporal: bool = True) -> None:
    """One Adagrad step of T tables, in place, in ONE launch; ``tables`` and ``grads`` as for :func:`sparse_adam_rows_`.
    ``state_sum[t]``: fp32 of the table's shape (``torch.optim.Adagrad``'s rule on a sparse gradient), or, with ``rowwise``, fp32
    ``[rows_t]`` holding one mean square per row (fbgemm's exact row-wise Adagrad).  ``step`` counts from 1 and enters through
    ``lr / (1 + (step - 1) * lr_decay)`` only.  Rows that are not listed, and their state, are untouched."""
    # alpha in double precision; ctypes rounds it and eps once to fp32 (step < 1: refused below)
    opt = _lib.pm_sparse_adagrad(-(float(lr) / (1.0 + (max(step, 1) - 1) * float(lr_decay))), float(eps), 1 if rowwise else 0,
                                 1 if maximize else 0, 1 if nontemporal else 0, 0)
    _launch_rows(_lib.load().pm_sparse_rows_adagrad, tables, grads, (("state_sum", state_sum, bool(rowwise)),), step,
                 (ctypes.byref(opt),))


def sparse_sgd_rows_(tables: Sequence[torch.Tensor], grads: Sequence[Tuple[torch.Tensor, torch.Tensor]], lr: float,
                     maximize: bool = False, nontemporal: bool = True) -> None:
    """One SGD step (no momentum, no weight decay) of T tables, in place, in ONE launch: ``w[rows] -= lr * values`` with one rounding
    per element; ``tables`` and ``grads`` as for :func:`sparse_adam_rows_`."""
    _launch_rows(_lib.load().pm_sparse_rows_sgd, tables, grads, (), None,
                 (ctypes.c_float(-float(lr)), 1 if maximize else 0, 1 if nontemporal else 0))


def _check_tables(self: torch.optim.Optimizer, name: str) -> None:
    """the constructor checks of the sparse-row optimizers (torch.optim.SparseAdam's, under `name`): dense, real, 2-D fp32 / bf16 / fp16"""
    sparse_params, complex_params = [], []
    for index, group in enumerate(self.param_groups):
        for d_index, p in enumerate(group["params"]):
            if p.is_sparse:
                sparse_params.append([index, d_index])
            if p.is_complex():
                complex_params.append([index, d_index])
    if sparse_params:
        raise ValueError(f"Sparse params at indices {sparse_params}: {name} requires dense parameter tensors")
    if complex_params:
        raise ValueError(f"Complex params at indices {complex_params}: {name} does not support complex parameters")
    for index, group in enumerate(self.param_groups):
        for d_index, p in enumerate(group["params"]):
            if p.dim() != 2 or p.dtype not in _WDTYPE:
                raise ValueError(f"{type(self).__name__}: parameter {d_index} of group {index} must be a 2-D fp32 / bf16 / fp16 table")


def _require_sparse_grad(p: torch.Tensor, name: str, dense_name: str) -> None:
    """a dense ``.grad`` raises torch.optim.SparseAdam's error under `name`; the parameter must be on a ROCm device"""
    if not p.grad.is_sparse:
        raise RuntimeError(f"{name} does not support dense gradients, please consider {dense_name} instead")
    _require_device(p, "parameter")


def _rows_and_values(p: torch.Tensor):
    """(row ids, fp32 values) of p's sparse ``.grad``, coalesced if it is not"""
    g = p.grad if p.grad.is_coalesced() else p.grad.coalesce()
    return g._indices()[0].contiguous(), g._values().float().contiguous()


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
        _check_tables(self, "SparseAdam")

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
                _require_sparse_grad(p, "SparseAdam", "Adam")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
                for key in ("exp_avg", "exp_avg_sq"):     # a state_dict loaded from torch.optim.SparseAdam holds the parameter's dtype
                    if state[key].dtype != torch.float32:
                        state[key] = state[key].float()
                state["step"] = int(state["step"]) + 1
                b = buckets.setdefault((p.dtype, state["step"], p.device), ([], [], [], []))
                b[0].append(p.data)
                b[1].append(_rows_and_values(p))
                b[2].append(state["exp_avg"])
                b[3].append(state["exp_avg_sq"])
            for (_, step, _), (tables, grads, m, v) in buckets.items():
                sparse_adam_rows_(tables, grads, m, v, step, float(group["lr"]), group["betas"], group["eps"],
                                  group.get("weight_decay", 0.0), group.get("maximize", False), _NONTEMPORAL)
        return loss


class SparseAdagradMI355(torch.optim.Optimizer):
    """``torch.optim.Adagrad`` for sparse COO gradients on the HIP path (its arguments and checks, minus ``weight_decay``, which torch
    refuses with sparse gradients), and with ``rowwise=True`` exact row-wise Adagrad: one fp32 mean square per table row.  Parameters
    are 2-D tables in fp32, bf16 or fp16 on a ROCm device.  The state has torch's keys, ``step`` and ``sum``, created with the optimizer
    as torch creates it; ``sum`` is always fp32 (a loaded ``sum`` of another dtype is widened), of the parameter's shape or ``[rows]``
    when row-wise.  ``step()`` coalesces a gradient that is not coalesced, skips parameters without one, and sends all parameters of a
    group that share a dtype (and a step count) through ONE ``pm_sparse_rows_adagrad`` launch."""

    def __init__(self, params, lr: float = 1e-2, lr_decay: float = 0.0, eps: float = 1e-10, initial_accumulator_value: float = 0.0,
                 maximize: bool = False, rowwise: bool = False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= lr_decay:
            raise ValueError(f"Invalid lr_decay value: {lr_decay}")
        if not 0.0 <= initial_accumulator_value:
            raise ValueError(f"Invalid initial_accumulator_value value: {initial_accumulator_value}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        # weight_decay = 0: torch.optim.Adagrad reads the key after loading this optimizer's state_dict
        super().__init__(params, {"lr": lr, "lr_decay": lr_decay, "eps": eps, "initial_accumulator_value": initial_accumulator_value,
                                  "weight_decay": 0, "maximize": maximize, "rowwise": bool(rowwise)})
        _check_tables(self, "SparseAdagradMI355")
        for group in self.param_groups:
            for p in group["params"]:
                shape = p.shape[:1] if group["rowwise"] else p.shape
                self.state[p] = {"step": torch.tensor(0.0), "sum": torch.full(shape, float(group["initial_accumulator_value"]),
                                                                              dtype=torch.float32, device=p.device)}

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:                   # groups loaded from torch.optim.Adagrad's state_dict lack `rowwise`
            group.setdefault("rowwise", False)
            group.setdefault("maximize", False)
            group.setdefault("weight_decay", 0)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            if group["weight_decay"] != 0:                # (torch's own refusal, of a loaded group's value)
                raise RuntimeError("weight_decay option is not compatible with sparse gradients")
            with_grad = [p for p in group["params"] if p.grad is not None]
            for p in with_grad:                           # every refusal before any state changes
                _require_sparse_grad(p, "SparseAdagradMI355", "torch.optim.Adagrad")
            buckets = {}                                  # (dtype, step, device) -> the three lists of one launch
            for p in with_grad:
                grad = _rows_and_values(p)
                state = self.state[p]
                if state["sum"].dtype != torch.float32:   # a state_dict loaded from torch.optim.Adagrad holds the parameter's dtype
                    state["sum"] = state["sum"].float()
                state["step"] += 1
                b = buckets.setdefault((p.dtype, int(state["step"]), p.device), ([], [], []))
                b[0].append(p.data)
                b[1].append(grad)
                b[2].append(state["sum"])
            for (_, step, _), (tables, grads, sums) in buckets.items():
                sparse_adagrad_rows_(tables, grads, sums, step, float(group["lr"]), float(group["lr_decay"]), float(group["eps"]),
                                     group["maximize"], group["rowwise"], _NONTEMPORAL)
        return loss


class SparseSGDMI355(torch.optim.Optimizer):
    """``torch.optim.SGD`` with ``momentum = 0`` and ``weight_decay = 0`` for sparse COO gradients on the HIP path: no state; all
    parameters of a group that share a dtype go through ONE ``pm_sparse_rows_sgd`` launch."""

    def __init__(self, params, lr: float, maximize: bool = False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        # the zero options: torch.optim.SGD reads these keys after loading this optimizer's state_dict
        super().__init__(params, {"lr": lr, "momentum": 0, "dampening": 0, "weight_decay": 0, "nesterov": False, "maximize": maximize})
        _check_tables(self, "SparseSGDMI355")

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("maximize", False)
            for key in ("momentum", "weight_decay"):
                group.setdefault(key, 0)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            if group["momentum"] != 0 or group["weight_decay"] != 0:
                raise RuntimeError("SparseSGDMI355: momentum and weight_decay are not supported (a loaded group asks for one)")
            buckets = {}                                  # (dtype, device) -> the two lists of one launch
            for p in group["params"]:
                if p.grad is None:
                    continue
                _require_sparse_grad(p, "SparseSGDMI355", "torch.optim.SGD")
                b = buckets.setdefault((p.dtype, p.device), ([], []))
                b[0].append(p.data)
                b[1].append(_rows_and_values(p))
            for tables, grads in buckets.values():
                sparse_sgd_rows_(tables, grads, float(group["lr"]), group["maximize"], _NONTEMPORAL)
        return loss
