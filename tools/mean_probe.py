#!/usr/bin/env python3
"""What mean pooling costs over sum pooling, measured in ONE process with the variants taking turns window by window.

Shape (the padding probe's): 16 fp32 tables of 10 M x 128, batch 8192, fixed pooling 20, uniform indices, with 0 % and 25 % of the
lookups replaced by the padding index (row 0 of every table).  Device events around windows of at least 100 ms (the iteration count
is sized from a pilot window), after warm-up; medians over --windows windows (at least 5).

Forward, us per call:
  fwd_mean_us     pm_embbag_fwd_mean (no pad array at 0 %, the pad array at 25 %)
  fwd_sum_us      the sum forward of the same request: pm_embbag_fwd at 0 %, pm_embbag_fwd_padded at 25 %
  expectation: equal within the windows' spread ("fwd_equal_within_spread").
Backward, us per call, for SGD (pm_embbag_bwd_fused) and row-wise Adagrad (pm_embbag_bwd_fused_adagrad), guard included at 25 %:
  step_mean_us    the step of a mean module: pm_embbag_mean_grad into a scratch, then the sum step on it
  step_sum_us     the sum step on the gradient itself
  scale_us        pm_embbag_mean_grad alone
  copy_us         a plain device copy of the gradient buffer (B x sum D floats): the yardstick for the scaling pass
  expectation: step_mean - step_sum is about one read + write of the gradient (~3 % of the step at pooling 20); a mean step that
  costs more than step_sum + copy + spread is recorded as a finding ("step_surprise").
Nothing here is a gate.  One JSON document to stdout and to --out (default profiles/mean_probe.json)."""
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


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=16)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pooling", type=int, default=20)
    ap.add_argument("--shares", default="0,0.25")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--min-window-ms", type=float, default=110.0)
    ap.add_argument("--out", default=os.path.join("profiles", "mean_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert a.windows >= 5, "medians of at least 5 windows"
    dev = "cuda:0"
    T, B, L, D = a.tables, a.batch, a.pooling, a.dim
    rows = [a.rows] * T
    lr, eps = 0.01, 1.0e-8
    m = param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=torch.float32, device=dev, init="normal", seed=1, fused_update=False,
                                           padding_idx=0, learning_rate=lr, optimizer="rowwise_adagrad", eps=eps)
    m.momentum_table(0)
    ts, mom = m._tables(), m._mom_ptrs
    out = torch.empty(B, T * D, device=dev)
    grad = torch.randn(B, T * D, device=dev)
    scratch = torch.empty_like(grad)
    clean_idx, off = tbe_request(rows, B, L, alpha=0.0, device=dev, seed=2)
    gen = torch.Generator(device=dev).manual_seed(3)
    med = statistics.median
    lines = []
    for share in [float(x) for x in a.shares.split(",")]:
        idx = clean_idx.clone()
        pad = None
        if share > 0:
            idx[torch.rand(idx.numel(), device=dev, generator=gen) < share] = 0
            pad = m._pad_dev()
        fwd = {"mean": lambda: eb._fwd(ts, idx, off, B, out=out, pad=pad, mean=True),
               "sum": lambda: eb._fwd(ts, idx, off, B, out=out, pad=pad)}
        f, f_iters = take_turns(fwd, a.windows, a.warmup, a.min_window_ms)
        bwd = {"sgd_mean": lambda: eb._bwd(ts, grad, idx, off, B, ts.d_ptrs, torch.float32, -lr, pad=pad, mean=True),
               "sgd_sum": lambda: eb._bwd(ts, grad, idx, off, B, ts.d_ptrs, torch.float32, -lr, pad=pad),
               "adagrad_mean": lambda: eb._adagrad(ts, grad, idx, off, B, mom, lr, eps, pad=pad, mean=True),
               "adagrad_sum": lambda: eb._adagrad(ts, grad, idx, off, B, mom, lr, eps, pad=pad),
               "scale": lambda: eb._mean_scale(ts, grad, idx, off, B, pad),
               "copy": lambda: scratch.copy_(grad)}
        g, g_iters = take_turns(bwd, a.windows, a.warmup, a.min_window_ms)
        fm, fs = med(f["mean"]), med(f["sum"])
        f_spread = max(spread(f["mean"]), spread(f["sum"]))
        rec = {"exp": "mean_probe", "tables": T, "rows": a.rows, "dim": D, "batch": B, "pooling": L, "padded_share": share,
               "lookups": int(idx.numel()), "windows": a.windows,
               "fwd_sum_kernel": "pm_embbag_fwd_padded" if pad is not None else "pm_embbag_fwd",
               "fwd_mean_us": round(fm, 2), "fwd_sum_us": round(fs, 2), "fwd_mean_over_sum": round(fm / fs, 4),
               "fwd_spread": round(f_spread, 4), "fwd_equal_within_spread": bool(abs(fm - fs) <= f_spread * fs),
               "fwd_windows_us": {k: [round(x, 2) for x in v] for k, v in f.items()}, "fwd_iters": f_iters,
               "scale_us": round(med(g["scale"]), 2), "copy_us": round(med(g["copy"]), 2),
               "grad_bytes": int(grad.numel() * 4)}
        for opt in ("sgd", "adagrad"):
            sm, ss = med(g[opt + "_mean"]), med(g[opt + "_sum"])
            sp = max(spread(g[opt + "_mean"]), spread(g[opt + "_sum"]))
            rec.update({f"{opt}_step_mean_us": round(sm, 2), f"{opt}_step_sum_us": round(ss, 2),
                        f"{opt}_mean_minus_sum_us": round(sm - ss, 2), f"{opt}_mean_over_sum": round(sm / ss, 4),
                        f"{opt}_spread": round(sp, 4),
                        f"{opt}_step_surprise": bool(sm > ss + med(g["copy"]) + sp * ss)})
        rec.update({"bwd_windows_us": {k: [round(x, 2) for x in v] for k, v in g.items()}, "bwd_iters": g_iters,
                    "device": torch.cuda.get_device_name(0)})
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del idx
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"exp": "mean_probe", "records": lines}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
