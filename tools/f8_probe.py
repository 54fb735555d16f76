#!/usr/bin/env python3
"""What pooling and gathering from FP8 tables costs, measured in ONE process with the routes taking turns window by window
(the pattern of tools/qrows_probe.py).

Shape: 16 tables of 10 M x 128, batch 8192, pooling 20 -> 2.6 M lookups; uniform and Zipf (alpha 1.05) indices.  Every route is fed
--rotate different requests in turn, so that no call finds the rows of the call before in a cache.  Device events around windows of at
least 110 ms (the iteration count is sized from a pilot window), after warm-up; medians over --windows windows (at least 5), spread =
(max - min) / median.

Pooled routes, us per call:
  f8_f32 / f8_f16           Float8BatchedEmbeddingBagMI355.lookup over e4m3 tables, fp32 / fp16 output (pm_embbag_fwd_f8)
  f8_f32_u2 / _u4 / _u8     the rows-in-flight sweep (pm_set_tuning's unroll; the default is launch_plan.h's kF8Unroll)
  bf16                      BatchedEmbeddingBagMI355.lookup over bf16 tables, fp32 output   -- unchanged code: a yardstick
  q8_f32                    QuantizedBatchedEmbeddingBagMI355.lookup over 8-bit row-quantised tables -- unchanged code: a yardstick
Un-pooled routes (``lookup_sequence``, fp32 output [N, D]):
  f8_seq / bf16_seq / q8_seq   the three table formats;   copy: a device copy of the output's size
Algorithmic bytes = (row_bytes + 8) per lookup + the output (pooled: (D * e_out + 8) per bag; un-pooled: D * e_out per lookup; the copy:
read + write of the output), and bytes / time as a fraction of 8 TB/s.  The FP8 tables hold random finite codes (no cast of torch's is
involved); the 8-bit tables are quantize_rows of the bf16 tables widened.
--other-dims: the pooled f8_f32 and bf16 routes at D = 64 (10 M rows) and D = 512 (2.5 M rows), uniform indices, one setting each.
"expectation": f8_f32 faster than bf16 and than q8_f32 beyond the run's spread, pooled, uniform -- reported, never a gate.
One JSON document to stdout and to --out (default profiles/f8_probe.json)."""
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
    """{name: [us per call, one per window]}: the routes take turns, every window at least min_window_ms long"""
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


def random_codes_(f8):
    """fill an FP8 module's tables with random finite e4m3 codes, a table at a time"""
    for t in range(len(f8.rows)):
        c = torch.randint(0, 256, (f8.rows[t], f8.dims[t]), dtype=torch.uint8, device=f8.weights.device)
        c[(c & 0x7f) == 0x7f] = 0x3f
        f8.copy_from_(t, c)
        del c


def summarise(t, iters, nbytes, lookups):
    us = statistics.median(t)
    return {"us": round(us, 2), "spread": round(spread(t), 4), "bytes": nbytes, "frac_of_8TBs": round(nbytes / (us * 1e-6) / PEAK, 4),
            "lookups_per_s_G": round(lookups / us * 1e-3, 3), "windows_us": [round(x, 2) for x in t], "iters": iters}


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
    ap.add_argument("--other-dims", action="store_true", help="also D = 64 and D = 512, pooled, uniform, one setting each")
    ap.add_argument("--out", default=os.path.join("profiles", "f8_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert a.windows >= 5, "medians of at least 5 windows"
    dev = "cuda:0"
    T, B, L, D = a.tables, a.batch, a.pooling, a.dim
    rows = [a.rows] * T
    N = T * B * L
    f32, f16 = torch.float32, torch.float16

    m16 = param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=torch.bfloat16, device=dev, init="normal", seed=1, fused_update=False)
    q8 = param_amd.QuantizedBatchedEmbeddingBagMI355(rows, D, 8, device=dev)
    for t in range(T):
        q8.quantize_from_(t, m16.table(t).float())
    f8 = {odt: param_amd.Float8BatchedEmbeddingBagMI355(rows, D, "e4m3", device=dev, output_dtype=odt) for odt in (f32, f16)}
    random_codes_(f8[f32])
    f8[f16].weights.copy_(f8[f32].weights)
    out32 = torch.empty(B, T * D, dtype=f32, device=dev)
    out16 = torch.empty(B, T * D, dtype=f16, device=dev)
    seq = torch.empty(N, D, dtype=f32, device=dev)
    seq2 = torch.empty_like(seq)

    def pooled(module, out, unroll=0):
        def call(idx, off):
            param_amd.set_tuning(unroll=unroll)
            module.lookup(idx, off, out=out, batch=B)
        return call

    def unpooled(module):
        def call(idx, off):
            param_amd.set_tuning()
            module.lookup_sequence(idx, off, batch=B, out=seq)
        return call

    # name: (call, bytes of one table row, bytes per output element)
    pooled_routes = {"f8_f32": (pooled(f8[f32], out32), D, 4), "f8_f16": (pooled(f8[f16], out16), D, 2),
                     "bf16": (pooled(m16, out32), 2 * D, 4), "q8_f32": (pooled(q8, out32), quant.host_row_bytes(D, 8), 4)}
    for u in (2, 4, 8):
        pooled_routes[f"f8_f32_u{u}"] = (pooled(f8[f32], out32, u), D, 4)
    seq_routes = {"f8_seq": (unpooled(f8[f32]), D), "bf16_seq": (unpooled(m16), 2 * D), "q8_seq": (unpooled(q8), quant.host_row_bytes(D, 8)),
                  "copy": (lambda idx, off: seq2.copy_(seq), None)}

    lines = []
    for dist, alpha in (("uniform", 0.0), ("zipf", 1.05)):
        reqs = [tbe_request(rows, B, L, alpha=alpha, device=dev, seed=10 + k) for k in range(a.rotate)]
        fns = {name: Rotating(v[0], reqs) for name, v in {**pooled_routes, **seq_routes}.items()}
        t, iters = take_turns(fns, a.windows, a.warmup, a.min_window_ms)
        param_amd.set_tuning()
        idx, off = reqs[0]
        rec = {"exp": "f8_probe", "tables": T, "rows": a.rows, "dim": D, "batch": B, "pooling": L, "lookups": N, "indices": dist,
               "rotate": a.rotate, "windows": a.windows, "lib": os.path.basename(param_amd.LIB_PATH),
               "plan": {"f8_f32": f8[f32].plan(idx, off, batch=B), "f8_f16": f8[f16].plan(idx, off, batch=B),
                        "f8_seq": f8[f32].sequence_plan(idx, off, batch=B)},
               "pooled": {}, "unpooled": {}}
        for name, (_, row_b, e_out) in pooled_routes.items():
            rec["pooled"][name] = summarise(t[name], iters[name], N * (row_b + 8) + T * B * (D * e_out + 8), N)
        for name, (_, row_b) in seq_routes.items():
            nbytes = 2 * N * D * 4 if row_b is None else N * (row_b + 8) + N * D * 4
            rec["unpooled"][name] = summarise(t[name], iters[name], nbytes, N)
        p = rec["pooled"]
        noise = max(p[k]["spread"] for k in ("f8_f32", "bf16", "q8_f32"))
        rec["expectation"] = {"f8_f32_faster_than_bf16_beyond_spread": bool(p["f8_f32"]["us"] < p["bf16"]["us"] * (1 - noise)),
                              "f8_f32_faster_than_q8_f32_beyond_spread": bool(p["f8_f32"]["us"] < p["q8_f32"]["us"] * (1 - noise)),
                              "spread_used": noise}
        rec["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del reqs

    if a.other_dims:
        del m16, q8, f8, out32, out16, seq, seq2, pooled_routes, seq_routes, fns
        torch.cuda.empty_cache()
        for D2, rows2 in ((64, a.rows), (512, a.rows // 4)):
            rws = [rows2] * T
            b16 = param_amd.BatchedEmbeddingBagMI355(rws, D2, dtype=torch.bfloat16, device=dev, init="normal", seed=1, fused_update=False)
            g8 = param_amd.Float8BatchedEmbeddingBagMI355(rws, D2, "e4m3", device=dev)
            random_codes_(g8)
            out = torch.empty(B, T * D2, dtype=f32, device=dev)

            def call_of(module):
                return lambda idx, off: module.lookup(idx, off, out=out, batch=B)

            reqs = [tbe_request(rws, B, L, alpha=0.0, device=dev, seed=10 + k) for k in range(a.rotate)]
            fns = {"f8_f32": Rotating(call_of(g8), reqs), "bf16": Rotating(call_of(b16), reqs)}
            t, iters = take_turns(fns, a.windows, a.warmup, a.min_window_ms)
            rec = {"exp": "f8_probe_other_dim", "tables": T, "rows": rows2, "dim": D2, "batch": B, "pooling": L, "lookups": N, "indices": "uniform",
                   "plan": {"f8_f32": g8.plan(*reqs[0], batch=B)}, "pooled": {}}
            for name, row_b in (("f8_f32", D2), ("bf16", 2 * D2)):
                rec["pooled"][name] = summarise(t[name], iters[name], N * (row_b + 8) + T * B * (D2 * 4 + 8), N)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del b16, g8, out, reqs, fns
            torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"exp": "f8_probe", "records": lines}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
