#!/usr/bin/env python3
"""What max pooling costs next to sum pooling, measured in ONE process with the routes taking turns window by window.

Shape: 16 tables of 10 M x 128, fp32 and bf16, batch 8192, fixed pooling 20, uniform and Zipf 1.05 indices.  Every route walks three
requests in rotation (three index sets of the same distribution).  Device events around windows of at least 110 ms (the iteration
count is sized from a pilot window), after warm-up; medians over --windows windows (at least 5), the spread (max - min) / median reported.

Forward, us per call:
  fwd_sum_us        the sum forward of the request (pm_embbag_fwd: code this change does not touch)
  fwd_max_us        pm_embbag_fwd_max without max_indices        (a) expectation: fwd_sum_us within the run's spread -- the same bytes move
  fwd_max_arg_us    pm_embbag_fwd_max writing max_indices        (b)
Backward, us per call, as scatter_add_ into the tables themselves (dense_grad runs the very same calls with fp32 [rows, D] buffers as
the destination; for this shape those buffers would be another 82 GB):
  bwd_sum_us        the sum module's step: pm_embbag_bwd_fused on the [B, T * D] gradient
  bwd_max_us        the max module's step with saved max_indices: pm_embbag_max_grad into the [N, D] fp32 scratch, then pm_embseq_bwd_fused
  expand_us         pm_embbag_max_grad alone                      (c) expectation: bwd_max is about the sequence backward of the request
                                                                   (1.3 - 1.5 x the pooled step) plus one [N, D] write
Nothing here is a gate and nothing is tuned.  One JSON document to stdout and to --out (default profiles/max_probe.json)."""
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
from param_amd import embedding_bag as eb  # noqa: E402
from param_amd.indices import tbe_request  # noqa: E402


def window_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def take_turns(fns, windows, warmup, min_window_ms):
    """{name: [us per call, one per window]}: the routes take turns, every window at least min_window_ms long; fn(i) is call number i"""
    iters = {}
    for name, fn in fns.items():
        for i in range(warmup):
            fn(i)
        torch.cuda.synchronize()
        pilot = window_us(fn, 6)
        iters[name] = max(6, math.ceil(min_window_ms * 1e3 / pilot))
    res = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            res[name].append(window_us(fn, iters[name]))
    return res, iters


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=16)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pooling", type=int, default=20)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--alphas", default="0,1.05", help="Zipf exponents; 0 = uniform")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--min-window-ms", type=float, default=110.0)
    ap.add_argument("--out", default=os.path.join("profiles", "max_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert a.windows >= 5, "medians of at least 5 windows"
    dev = "cuda:0"
    T, B, L, D = a.tables, a.batch, a.pooling, a.dim
    rows = [a.rows] * T
    lr = 1.0e-3
    med = statistics.median
    lines = []
    for dname in a.dtypes.split(","):
        dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[dname]
        # ONE slab serves both modules' calls: the sum and the max routes are host functions over the same table set
        m = param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=dtype, device=dev, init="normal", seed=1, fused_update=False)
        ts = m._tables()
        out = torch.empty(B, T * D, device=dev)
        arg = torch.empty(B, T * D, dtype=torch.int32, device=dev)
        grad = torch.randn(B, T * D, device=dev)
        for alpha in [float(x) for x in a.alphas.split(",")]:
            reqs = [tbe_request(rows, B, L, alpha=alpha, device=dev, seed=10 + k) for k in range(3)]
            args = []
            for idx, off in reqs:      # the saved max_indices of each request, as a training step holds them
                args.append(eb._fwd_max(ts, idx, off, B, max_indices=True)[1])
            torch.cuda.synchronize()
            n = int(reqs[0][0].numel())
            rq = lambda i: reqs[i % 3]                                                                            # noqa: E731
            fns = {
                "fwd_sum": lambda i: eb._fwd(ts, *rq(i), B, out=out),
                "fwd_max": lambda i: eb._fwd_max(ts, *rq(i), B, out=out),
                "fwd_max_arg": lambda i: eb._fwd_max(ts, *rq(i), B, out=out, max_indices=arg),
                "bwd_sum": lambda i: eb._bwd(ts, grad, *rq(i), B, ts.d_ptrs, dtype, -lr),
                "bwd_max": lambda i: eb._max_bwd(ts, grad, *rq(i), B, ts.d_ptrs, dtype, -lr, None, args[i % 3]),
                "expand": lambda i: eb._max_expand(ts, grad, args[i % 3], *rq(i), B),
            }
            r, iters = take_turns(fns, a.windows, a.warmup, a.min_window_ms)
            v = {k: med(x) for k, x in r.items()}
            sp = {k: spread(x) for k, x in r.items()}
            f_sp = max(sp["fwd_sum"], sp["fwd_max"])
            rec = {"exp": "max_probe", "tables": T, "rows": a.rows, "dim": D, "batch": B, "pooling": L, "table_dtype": dname,
                   "zipf_alpha": alpha, "lookups": n, "windows": a.windows, "requests_in_rotation": 3,
                   "g_seq_bytes": n * D * 4, "grad_bytes": int(grad.numel() * 4)}
            rec.update({k + "_us": round(x, 2) for k, x in v.items()})
            rec.update({k + "_spread": round(x, 4) for k, x in sp.items()})
            rec.update({"fwd_max_over_sum": round(v["fwd_max"] / v["fwd_sum"], 4),
                        "fwd_max_arg_over_sum": round(v["fwd_max_arg"] / v["fwd_sum"], 4),
                        "fwd_max_equals_sum_within_spread": bool(abs(v["fwd_max"] - v["fwd_sum"]) <= f_sp * v["fwd_sum"]),
                        "bwd_max_over_sum": round(v["bwd_max"] / v["bwd_sum"], 4),
                        "bwd_max_minus_expand_over_sum": round((v["bwd_max"] - v["expand"]) / v["bwd_sum"], 4),
                        "expand_gbps": round(n * D * 4 / v["expand"] / 1e3, 1),
                        "windows_us": {k: [round(x, 2) for x in xs] for k, xs in r.items()}, "iters": iters,
                        "device": torch.cuda.get_device_name(0)})
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del reqs, args
        del m, ts, out, arg, grad
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"exp": "max_probe", "records": lines}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
