#!/usr/bin/env python3
"""What a bf16 output and a bf16 gradient cost against fp32 ones, measured in ONE process with the variants taking turns window by window.

Shape (the mean probe's): 16 fp32 tables of 10 M x 128, batch 8192, fixed pooling 20, uniform indices, sum and mean pooling, no padding.
Device events around windows of at least 100 ms (the iteration count is sized from a pilot window), after warm-up; medians over
--windows windows (at least 5).

Forward, us per call, per pooling:
  fwd_out16_us    pm_embbag_fwd_out16 writing bf16
  fwd_fp32_us     the fp32-output forward of the same request: pm_embbag_fwd (sum), pm_embbag_fwd_mean (mean)
  expectation: the 16-bit forward is no slower ("fwd_out16_not_slower": within the windows' spread).
Backward, us per call, per pooling, for SGD (pm_embbag_bwd_fused) and row-wise Adagrad (pm_embbag_bwd_fused_adagrad):
  step_g16_us     the step fed the bf16 gradient: pm_embbag_grad_widen into a scratch (mean: the scaling fused), then the step on it
  step_g32_us     the same step fed the fp32 gradient (mean: pm_embbag_mean_grad into a scratch first)
  widen_us        pm_embbag_grad_widen alone;  scale_us: pm_embbag_mean_grad alone (mean);  copy_us: a plain device copy of the fp32
                  gradient buffer, the yardstick
  expectation: the widening costs about what the mean scaling costs (28-36 us at this shape).
Nothing here is a gate.  One JSON document to stdout and to --out (default profiles/out16_probe.json)."""
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
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--min-window-ms", type=float, default=110.0)
    ap.add_argument("--out", default=os.path.join("profiles", "out16_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert a.windows >= 5, "medians of at least 5 windows"
    dev = "cuda:0"
    T, B, L, D = a.tables, a.batch, a.pooling, a.dim
    rows = [a.rows] * T
    lr, eps = 0.01, 1.0e-8
    bf16 = torch.bfloat16
    m = param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=torch.float32, device=dev, init="normal", seed=1, fused_update=False,
                                           learning_rate=lr, optimizer="rowwise_adagrad", eps=eps)
    m.momentum_table(0)
    ts, mom = m._tables(), m._mom_ptrs
    out32 = torch.empty(B, T * D, device=dev)
    out16 = torch.empty(B, T * D, device=dev, dtype=bf16)
    grad32 = torch.randn(B, T * D, device=dev)
    grad16 = grad32.to(bf16)
    scratch = torch.empty_like(grad32)
    idx, off = tbe_request(rows, B, L, alpha=0.0, device=dev, seed=2)
    med = statistics.median
    lines = []
    for mean in (False, True):
        fwd = {"out16": lambda: eb._fwd(ts, idx, off, B, out=out16, mean=mean, out16=bf16),
               "fp32": lambda: eb._fwd(ts, idx, off, B, out=out32, mean=mean)}
        f, f_iters = take_turns(fwd, a.windows, a.warmup, a.min_window_ms)
        bwd = {"sgd_g16": lambda: eb._bwd(ts, grad16, idx, off, B, ts.d_ptrs, torch.float32, -lr, mean=mean, out16=bf16),
               "sgd_g32": lambda: eb._bwd(ts, grad32, idx, off, B, ts.d_ptrs, torch.float32, -lr, mean=mean),
               "adagrad_g16": lambda: eb._adagrad(ts, grad16, idx, off, B, mom, lr, eps, mean=mean, out16=bf16),
               "adagrad_g32": lambda: eb._adagrad(ts, grad32, idx, off, B, mom, lr, eps, mean=mean),
               "widen": lambda: eb._widen(ts, grad16, idx, off, B, None, None, mean),
               "copy": lambda: scratch.copy_(grad32)}
        if mean:
            bwd["scale"] = lambda: eb._mean_scale(ts, grad32, idx, off, B, None)
        g, g_iters = take_turns(bwd, a.windows, a.warmup, a.min_window_ms)
        f16, f32 = med(f["out16"]), med(f["fp32"])
        f_spread = max(spread(f["out16"]), spread(f["fp32"]))
        rec = {"exp": "out16_probe", "tables": T, "rows": a.rows, "dim": D, "batch": B, "pooling": L, "mode": "mean" if mean else "sum",
               "out_dtype": "bf16", "lookups": int(idx.numel()), "windows": a.windows,
               "fwd_fp32_kernel": "pm_embbag_fwd_mean" if mean else "pm_embbag_fwd",
               "fwd_out16_us": round(f16, 2), "fwd_fp32_us": round(f32, 2), "fwd_out16_over_fp32": round(f16 / f32, 4),
               "fwd_spread": round(f_spread, 4), "fwd_out16_not_slower": bool(f16 <= f32 * (1 + f_spread)),
               "fwd_windows_us": {k: [round(x, 2) for x in v] for k, v in f.items()}, "fwd_iters": f_iters,
               "widen_us": round(med(g["widen"]), 2), "copy_us": round(med(g["copy"]), 2),
               "grad16_bytes": int(grad16.numel() * 2), "grad32_bytes": int(grad32.numel() * 4)}
        if mean:
            rec["scale_us"] = round(med(g["scale"]), 2)
        for opt in ("sgd", "adagrad"):
            s16, s32 = med(g[opt + "_g16"]), med(g[opt + "_g32"])
            sp = max(spread(g[opt + "_g16"]), spread(g[opt + "_g32"]))
            rec.update({f"{opt}_step_g16_us": round(s16, 2), f"{opt}_step_g32_us": round(s32, 2),
                        f"{opt}_g16_minus_g32_us": round(s16 - s32, 2), f"{opt}_g16_over_g32": round(s16 / s32, 4),
                        f"{opt}_spread": round(sp, 4)})
        rec.update({"bwd_windows_us": {k: [round(x, 2) for x in v] for k, v in g.items()}, "bwd_iters": g_iters,
                    "device": torch.cuda.get_device_name(0)})
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"exp": "out16_probe", "records": lines}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
