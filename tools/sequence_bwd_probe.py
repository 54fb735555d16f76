#!/usr/bin/env python3
"""What the batched sequence backward costs, measured in ONE process with the variants taking turns window by window.

Shape (the probes' usual request): 16 tables of 10 M x 128, batch 8192, pooling 20 -> 2.6 M lookups, hence 2.6 M gradient rows of 128
fp32; uniform and Zipf (alpha 1.05) indices; fp32 and bf16 tables; SGD and row-wise Adagrad.  Every variant is fed --rotate different
requests in turn, so that no call finds the rows of the call before in a cache.  Device events around windows of at least 100 ms (the
iteration count is sized from a pilot window), after warm-up; medians over --windows windows (at least 5), spread = (max - min) / median.

Per (dtype, distribution, optimizer), us per call:
  sequence_us    sequence_optimizer_step_ on the [N, D] gradient: one sort + one apply for all T tables (pm_embseq_bwd_fused*)
  per_table_us   (a) the only route the package had before: T one-table modules over the same weights, each stepped with the existing
                 optimizer_step_ on offsets = arange(n_t), batch = n_t and its table's gradient rows -- T sorts, T applies
  pooled_us      (b) for context: the pooled fused step of the SAME request (gradient [B, T * D]: 20 x fewer gradient rows, and the
                 hybrid route where it is offered)
  copy_us        (b) a device-to-device copy of the gradient's size
  expectation: sequence_us is not above per_table_us by more than that route's spread ("sequence_not_slower").
Nothing here is a gate.  One JSON document to stdout and to --out (default profiles/sequence_bwd_probe.json)."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import param_amd  # noqa: E402
from param_amd.indices import tbe_request  # noqa: E402


def window_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def take_turns(fns, windows, warmup, min_window_ms):
    """{name: [us per call, one per window]}: the variants take turns, every window at least min_window_ms long"""
    iters = {}
    for name, fn in fns.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        pilot = window_us(fn, 5)
        iters[name] = max(5, math.ceil(min_window_ms * 1e3 / pilot))
    res = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            res[name].append(window_us(fn, iters[name]))
    return res, iters


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


class Rotating:
    """calls ``fn(request k)`` for k = 0, 1, .., rotate - 1, 0, .. -- one request per call"""

    def __init__(self, fn, requests):
        self.fn, self.requests, self.k = fn, requests, 0

    def __call__(self):
        self.fn(*self.requests[self.k])
        self.k = (self.k + 1) % len(self.requests)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=16)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pooling", type=int, default=20)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-window-ms", type=float, default=110.0)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--optimizers", default="sgd,rowwise_adagrad")
    ap.add_argument("--out", default=os.path.join("profiles", "sequence_bwd_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert a.windows >= 5, "medians of at least 5 windows"
    dev = "cuda:0"
    T, B, L, D = a.tables, a.batch, a.pooling, a.dim
    rows = [a.rows] * T
    n = B * L                      # lookups per table
    N = T * n
    med = statistics.median
    seq_grad = torch.randn(N, D, device=dev) * 1e-3
    pooled_grad = torch.randn(B, T * D, device=dev) * 1e-3
    spare = torch.empty_like(seq_grad)
    one = torch.arange(n, dtype=torch.int64, device=dev)       # the per-table route's offsets (fixed pooling: every table has n lookups)
    lines = []
    for name in a.dtypes.split(","):
        dt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[name]
        for opt in a.optimizers.split(","):
            m = param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=dt, device=dev, init="normal", seed=1, fused_update=False, optimizer=opt,
                                                   learning_rate=1e-3)
            # (a): T one-table modules OVER THE SAME WEIGHTS (views of m's slab; their own Adagrad state)
            ones = []
            for t in range(T):
                o = param_amd.BatchedEmbeddingBagMI355([a.rows], D, dtype=dt, device=dev, init=None, fused_update=False, optimizer=opt,
                                                       learning_rate=1e-3)
                o.weights = torch.nn.Parameter(m.table(t).reshape(-1), requires_grad=False)
                o._starts, o._ts = [0], None
                ones.append(o)
            for dist, alpha in (("uniform", 0.0), ("zipf", 1.05)):
                reqs = [tbe_request(rows, B, L, alpha=alpha, device=dev, seed=10 + k) for k in range(a.rotate)]

                def sequence(idx, off):
                    m.sequence_optimizer_step_(seq_grad, idx, off, batch=B)

                def per_table(idx, off):
                    for t, o in enumerate(ones):
                        o.optimizer_step_(seq_grad[t * n:(t + 1) * n], idx[t * n:(t + 1) * n], one, batch=n)

                def pooled(idx, off):
                    m.optimizer_step_(pooled_grad, idx, off, batch=B)

                fns = {"sequence": Rotating(sequence, reqs), "per_table": Rotating(per_table, reqs), "pooled": Rotating(pooled, reqs),
                       "copy": lambda: spare.copy_(seq_grad)}
                t_us, iters = take_turns(fns, a.windows, a.warmup, a.min_window_ms)
                s, p, po, cp = (med(t_us[k]) for k in ("sequence", "per_table", "pooled", "copy"))
                sp_p = spread(t_us["per_table"])
                rec = {"exp": "sequence_bwd_probe", "tables": T, "rows": a.rows, "dim": D, "batch": B, "pooling": L, "lookups": N,
                       "table_dtype": name, "optimizer": opt, "indices": dist, "rotate": a.rotate, "windows": a.windows,
                       "sequence_us": round(s, 2), "per_table_us": round(p, 2), "pooled_us": round(po, 2), "copy_us": round(cp, 2),
                       "sequence_over_per_table": round(s / p, 4), "sequence_over_pooled": round(s / po, 4),
                       "sequence_spread": round(spread(t_us["sequence"]), 4), "per_table_spread": round(sp_p, 4),
                       "pooled_spread": round(spread(t_us["pooled"]), 4), "copy_spread": round(spread(t_us["copy"]), 4),
                       "sequence_not_slower": bool(s <= p * (1 + sp_p)),
                       "windows_us": {k: [round(x, 2) for x in v] for k, v in t_us.items()}, "iters": iters,
                       "device": torch.cuda.get_device_name(0)}
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                del reqs
            del m, ones
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"exp": "sequence_bwd_probe", "records": lines}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
