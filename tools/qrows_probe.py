#!/usr/bin/env python3
"""What pooling from row-quantised tables costs, measured in ONE process with the variants taking turns window by window.

Shape (the probes' usual request): 16 tables of 10 M x 128, batch 8192, pooling 20 -> 2.6 M lookups; uniform and Zipf (alpha 1.05)
indices.  Every variant is fed --rotate different requests in turn, so that no call finds the rows of the call before in a cache.
Device events around windows of at least 100 ms (the iteration count is sized from a pilot window), after warm-up; medians over
--windows windows (at least 5), spread = (max - min) / median.

Variants, per distribution, us per call:
  fp32 / bf16               BatchedEmbeddingBagMI355.lookup over fp32 / bf16 tables, fp32 output -- unchanged code: the yardsticks
  q8_f32 / q8_f16           QuantizedBatchedEmbeddingBagMI355.lookup over 8-bit tables, fp32 / fp16 output (pm_embbag_fwd_qrows)
  q4_f32 / q4_f16           the same over 4-bit tables
  q8_f32_u2 / _u4, q4_..    the rows-in-flight sweep (pm_set_tuning's unroll; the default is launch_plan.h's kQrowsUnroll)
Per variant: algorithmic bytes = (row_bytes + 8) per lookup + (D * e_out + 8) per bag, and bytes / time as a fraction of 8 TB/s.
The quantised tables are quantize_rows of the fp32 tables (the existing kernel).  "expectation": q8_f32 faster than bf16, q4_f32 faster
than q8_f32 -- reported, never a gate.  ``lib`` names the library the process loaded (PARAM_AMD_LIB: an experiment build of the kernel,
e.g. -DPM_QROWS_WIDE, is measured by a second run of this tool).  One JSON document to stdout and to --out
(default profiles/qrows_probe.json)."""
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
from param_amd import quant  # noqa: E402
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
    ap.add_argument("--no-sweep", action="store_true", help="leave the rows-in-flight sweep out")
    ap.add_argument("--out", default=os.path.join("profiles", "qrows_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert a.windows >= 5, "medians of at least 5 windows"
    dev = "cuda:0"
    T, B, L, D = a.tables, a.batch, a.pooling, a.dim
    rows = [a.rows] * T
    N = T * B * L
    med = statistics.median

    m32 = param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=torch.float32, device=dev, init="normal", seed=1, fused_update=False)
    m16 = param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=torch.bfloat16, device=dev, init=None, fused_update=False)
    q = {}
    for bits in (8, 4):
        for odt in (torch.float32, torch.float16):
            q[bits, odt] = param_amd.QuantizedBatchedEmbeddingBagMI355(rows, D, bits, device=dev, output_dtype=odt)
    for t in range(T):
        src = m32.table(t)
        m16.table(t).copy_(src)
        for bits in (8, 4):
            q[bits, torch.float32].quantize_from_(t, src)
        for bits in (8, 4):
            q[bits, torch.float16].table(t).copy_(q[bits, torch.float32].table(t))
    out32 = torch.empty(B, T * D, dtype=torch.float32, device=dev)
    out16 = torch.empty(B, T * D, dtype=torch.float16, device=dev)

    def variant(module, out, unroll=0):
        def call(idx, off):
            param_amd.set_tuning(unroll=unroll)
            module.lookup(idx, off, out=out, batch=B)
        return call

    # name: (call, bytes of one table row, bytes of one output element)
    variants = {"fp32": (variant(m32, out32), 4 * D, 4), "bf16": (variant(m16, out32), 2 * D, 4)}
    for bits in (8, 4):
        rb = quant.host_row_bytes(D, bits)
        variants[f"q{bits}_f32"] = (variant(q[bits, torch.float32], out32), rb, 4)
        variants[f"q{bits}_f16"] = (variant(q[bits, torch.float16], out16), rb, 2)
        if not a.no_sweep:
            for u in (2, 4):
                variants[f"q{bits}_f32_u{u}"] = (variant(q[bits, torch.float32], out32, u), rb, 4)

    lines = []
    for dist, alpha in (("uniform", 0.0), ("zipf", 1.05)):
        reqs = [tbe_request(rows, B, L, alpha=alpha, device=dev, seed=10 + k) for k in range(a.rotate)]
        fns = {name: Rotating(v[0], reqs) for name, v in variants.items()}
        t, iters = take_turns(fns, a.windows, a.warmup, a.min_window_ms)
        param_amd.set_tuning()
        # the quantised lookups against the fp32 lookup over the dequantised rows of the same request: closeness, not bits (README)
        idx, off = reqs[0]
        ref = m32.lookup(idx, off, batch=B).double()
        scale = float(ref.abs().max())
        close = {f"q{bits}": float((q[bits, torch.float32].lookup(idx, off, batch=B).double() - ref).abs().max()) / scale for bits in (8, 4)}
        rec = {"exp": "qrows_probe", "tables": T, "rows": a.rows, "dim": D, "batch": B, "pooling": L, "lookups": N, "indices": dist,
               "rotate": a.rotate, "windows": a.windows, "lib": os.path.basename(param_amd.LIB_PATH),
               "plan": {f"q{bits}_{'f32' if odt == torch.float32 else 'f16'}": q[bits, odt].plan(idx, off, batch=B) for bits, odt in q},
               "max_abs_diff_to_fp32_tables_over_max_abs": close, "variants": {}}
        for name, (_, row_b, e_out) in variants.items():
            us = med(t[name])
            nbytes = N * (row_b + 8) + T * B * (D * e_out + 8)
            rec["variants"][name] = {"us": round(us, 2), "spread": round(spread(t[name]), 4), "bytes": nbytes,
                                     "frac_of_8TBs": round(nbytes / (us * 1e-6) / PEAK, 4), "lookups_per_s_G": round(N / us * 1e-3, 3),
                                     "windows_us": [round(x, 2) for x in t[name]], "iters": iters[name]}
        v = rec["variants"]
        rec["expectation"] = {"q8_f32_faster_than_bf16": bool(v["q8_f32"]["us"] < v["bf16"]["us"]),
                              "q4_f32_faster_than_q8_f32": bool(v["q4_f32"]["us"] < v["q8_f32"]["us"])}
        rec["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del reqs
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"exp": "qrows_probe", "records": lines}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
