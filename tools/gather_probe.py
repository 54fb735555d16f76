#!/usr/bin/env python3
"""What the un-pooled lookup costs, measured in ONE process with the variants taking turns window by window.

Shape (the probes' usual request): 16 tables of 10 M x 128, batch 8192, pooling 20 -> 2.6 M lookups; uniform and Zipf (alpha 1.05)
indices; fp32 tables with fp32 output, and bf16 tables with bf16 output.  Every variant is fed --rotate different requests in turn, so
that no call finds the rows of the call before in a cache.  Device events around windows of at least 100 ms (the iteration count is
sized from a pilot window), after warm-up; medians over --windows windows (at least 5), spread = (max - min) / median.

Per (dtype, distribution), us per call:
  gather_u{1,2,4,8}_us  lookup_sequence (pm_embedding_gather) with that many rows in flight per lane group (pm_set_tuning's unroll);
                        gather_us is the default's (launch_plan.h: kGatherUnroll)
  bag_of_one_us         the same rows through the pooled lookup as bags of one -- offsets = arange(N), output [N / T, T * D]: the only
                        route without the new entry point, unchanged code, the yardstick (bf16: the 16-bit-output forward)
  copy_us               a device-to-device copy of the output's size: the write floor
  bytes_per_lookup      algorithmic: the index, D * e_in read, D * e_out written;  *_frac_of_8TBs = bytes / time / 8e12
  expectation: the gather is not slower than the bag-of-one route by more than that route's spread ("gather_not_slower").
Nothing here is a gate.  One JSON document to stdout and to --out (default profiles/gather_probe.json)."""
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

PEAK = 8.0e12      # bytes / s: the HBM peak the project's fractions are stated against


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
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--min-window-ms", type=float, default=110.0)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--out", default=os.path.join("profiles", "gather_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert a.windows >= 5, "medians of at least 5 windows"
    dev = "cuda:0"
    T, B, L, D = a.tables, a.batch, a.pooling, a.dim
    rows = [a.rows] * T
    n = B * L                      # lookups per table
    N = T * n
    med = statistics.median
    lines = []
    for name in a.dtypes.split(","):
        dt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[name]
        m = param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=dt, device=dev, init="normal", seed=1, fused_update=False,
                                               output_dtype=None if dt == torch.float32 else dt)
        e = dt.itemsize
        seq_out = torch.empty(N, D, dtype=dt, device=dev)
        bag_out = torch.empty(n, T * D, dtype=dt, device=dev)
        spare = torch.empty_like(seq_out)
        one = torch.arange(N + 1, dtype=torch.int64, device=dev)           # the bag-of-one route's offsets: part of its cost
        for dist, alpha in (("uniform", 0.0), ("zipf", 1.05)):
            reqs = [tbe_request(rows, B, L, alpha=alpha, device=dev, seed=10 + k) for k in range(a.rotate)]

            def gather(u):
                def call(idx, off):
                    param_amd.set_tuning(unroll=u)
                    m.lookup_sequence(idx, off, batch=B, out=seq_out)
                return Rotating(call, reqs)

            def bag_of_one(idx, off):
                param_amd.set_tuning(unroll=0)
                m.lookup(idx, one, batch=n, out=bag_out)

            fns = {"gather": gather(0), "bag_of_one": Rotating(bag_of_one, reqs), "copy": lambda: spare.copy_(seq_out)}
            fns.update({f"gather_u{u}": gather(u) for u in (1, 2, 4, 8)})
            t, iters = take_turns(fns, a.windows, a.warmup, a.min_window_ms)
            param_amd.set_tuning()
            # same rows, either route (fp32: bit for bit unless a stored -0.0 was looked up; 16-bit: the stored bits)
            idx, off = reqs[0]
            m.lookup_sequence(idx, off, batch=B, out=seq_out)
            m.lookup(idx, one, batch=n, out=bag_out)
            agree = bool(torch.equal(seq_out.view(T, n, D).permute(1, 0, 2).reshape(n, T * D), bag_out))
            bytes_per = 8 + D * e + D * e
            g, b1, cp = med(t["gather"]), med(t["bag_of_one"]), med(t["copy"])
            sp_b1 = spread(t["bag_of_one"])
            rec = {"exp": "gather_probe", "tables": T, "rows": a.rows, "dim": D, "batch": B, "pooling": L, "lookups": N, "table_dtype": name,
                   "out_dtype": name, "indices": dist, "rotate": a.rotate, "windows": a.windows, "bytes_per_lookup": bytes_per,
                   "gather_us": round(g, 2), "bag_of_one_us": round(b1, 2), "copy_us": round(cp, 2),
                   "gather_over_bag_of_one": round(g / b1, 4), "bag_of_one_spread": round(sp_b1, 4), "gather_spread": round(spread(t["gather"]), 4),
                   "gather_not_slower": bool(g <= b1 * (1 + sp_b1)),
                   "gather_frac_of_8TBs": round(N * bytes_per / (g * 1e-6) / PEAK, 4),
                   "bag_of_one_frac_of_8TBs": round(N * bytes_per / (b1 * 1e-6) / PEAK, 4),
                   "copy_frac_of_8TBs": round(2 * N * D * e / (cp * 1e-6) / PEAK, 4),
                   "unroll_sweep_us": {str(u): round(med(t[f"gather_u{u}"]), 2) for u in (1, 2, 4, 8)},
                   "unroll_sweep_spread": {str(u): round(spread(t[f"gather_u{u}"]), 4) for u in (1, 2, 4, 8)},
                   "routes_agree": agree, "windows_us": {k: [round(x, 2) for x in v] for k, v in t.items()}, "iters": iters,
                   "device": torch.cuda.get_device_name(0)}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del reqs
        del m, seq_out, bag_out, spare
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"exp": "gather_probe", "records": lines}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
