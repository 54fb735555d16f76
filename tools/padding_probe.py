#!/usr/bin/env python3
"""What padding_idx costs and saves, measured in ONE process with the variants taking turns window by window.

Shape: 16 fp32 tables of 10 M x 128, batch 8192, fixed pooling 20, uniform indices, with 0 %, 25 % and 50 % of the lookups replaced by
the padding index (row 0 of every table).  Device events around windows of at least 100 ms (the iteration count is sized from a pilot
window), after warm-up; medians over --windows windows.

Forward, us per call:
  a  fwd_padded_us     the padded kernel (pm_embbag_fwd_padded) on the padded request
  b  fwd_filtered_us   the product forward (pm_embbag_fwd) on the same request with the padded lookups removed beforehand: the floor, the
                       same useful bytes
  c  fwd_ignored_us    the product forward on the padded request, padding ignored (it loads the padding row like any other)
  a/b, a/c and the spread of b over its windows, (max - min) / median.  The one condition: a must not be slower than c at 25 % and 50 %
  by more than that spread ("a_not_slower_than_c").
Backward, us per call:
  bwd_guarded_us       the fused SGD step (pm_embbag_bwd_fused) with the guard (pm_pad_rows_guard before and after) on the padded request
  bwd_filtered_us      the same step, no guard, on the filtered request
  their difference is the cost of the guard PLUS the padded lookups that are still sorted and accumulated into a row that is put back.
One JSON document to stdout and to --out (default profiles/padding_probe.json)."""
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
        pilot = window_us(fn, 10)
        iters[name] = max(10, math.ceil(min_window_ms * 1e3 / pilot))
    res = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            res[name].append(window_us(fn, iters[name]))
    return res, iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=16)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pooling", type=int, default=20)
    ap.add_argument("--shares", default="0,0.25,0.5")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--min-window-ms", type=float, default=110.0)
    ap.add_argument("--out", default=os.path.join("profiles", "padding_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    dev = "cuda:0"
    T, B, L, D = a.tables, a.batch, a.pooling, a.dim
    rows = [a.rows] * T
    m = param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=torch.float32, device=dev, init="normal", seed=1, fused_update=False,
                                           padding_idx=0, learning_rate=0.01)
    ts, pad = m._tables(), m._pad_dev()
    out = torch.empty(B, T * D, device=dev)
    grad = torch.randn(B, T * D, device=dev)
    clean_idx, off = tbe_request(rows, B, L, alpha=0.0, device=dev, seed=2)
    tab = torch.arange(T, device=dev).repeat_interleave(B * L)
    gen = torch.Generator(device=dev).manual_seed(3)
    lines = []
    for share in [float(x) for x in a.shares.split(",")]:
        idx = clean_idx.clone()
        idx[torch.rand(idx.numel(), device=dev, generator=gen) < share] = 0
        keep = idx != pad[tab]
        f_idx = idx[keep].contiguous()
        f_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(keep, 0)])[off].contiguous()
        fwd = {"a": lambda: eb._fwd(ts, idx, off, B, out=out, pad=pad),
               "b": lambda: eb._fwd(ts, f_idx, f_off, B, out=out),
               "c": lambda: eb._fwd(ts, idx, off, B, out=out)}
        f, f_iters = take_turns(fwd, a.windows, a.warmup, a.min_window_ms)
        bwd = {"guarded": lambda: eb._bwd(ts, grad, idx, off, B, ts.d_ptrs, torch.float32, -0.01, pad=pad),
               "filtered": lambda: eb._bwd(ts, grad, f_idx, f_off, B, ts.d_ptrs, torch.float32, -0.01)}
        g, g_iters = take_turns(bwd, a.windows, a.warmup, a.min_window_ms)
        med = statistics.median
        fa, fb, fc = med(f["a"]), med(f["b"]), med(f["c"])
        spread_b = (max(f["b"]) - min(f["b"])) / fb
        rec = {"exp": "padding_probe", "tables": T, "rows": a.rows, "dim": D, "batch": B, "pooling": L, "padded_share": share,
               "padded_lookups": int(idx.numel() - f_idx.numel()), "lookups": int(idx.numel()), "windows": a.windows,
               "fwd_padded_us": round(fa, 2), "fwd_filtered_us": round(fb, 2), "fwd_ignored_us": round(fc, 2),
               "a_over_b": round(fa / fb, 4), "a_over_c": round(fa / fc, 4), "spread_b": round(spread_b, 4),
               "a_not_slower_than_c": bool(fa <= fc * (1.0 + spread_b)),
               "fwd_windows_us": {k: [round(x, 2) for x in v] for k, v in f.items()}, "fwd_iters": f_iters,
               "bwd_guarded_us": round(med(g["guarded"]), 2), "bwd_filtered_us": round(med(g["filtered"]), 2),
               "bwd_guard_and_wasted_lookups_us": round(med(g["guarded"]) - med(g["filtered"]), 2),
               "bwd_windows_us": {k: [round(x, 2) for x in v] for k, v in g.items()}, "bwd_iters": g_iters,
               "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del idx, keep, f_idx, f_off
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"exp": "padding_probe", "records": lines}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
