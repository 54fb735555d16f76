#!/usr/bin/env python3
"""What MXFP4 TABLES cost next to the formats the package already serves, measured in ONE process with the routes taking turns window by
window (tools/f8_probe.py's pattern and helpers).

Shape: 16 tables of 10 M x 128, batch 8192, pooling 20 -> 2.6 M lookups; uniform and Zipf (alpha 1.05) indices; every route is fed
--rotate different requests in turn; device events around windows of at least 110 ms; medians over --windows windows (at least 5),
spread = (max - min) / median.

Pooled routes, us per call, fp32 output:
  mx4         MX4BatchedEmbeddingBagMI355.lookup           (pm_embbag_fwd_mx4; 72-byte rows, rows in flight: the plan's default)
  mx4_u4      the same with pm_set_tuning(unroll=4)
  q4          QuantizedBatchedEmbeddingBagMI355.lookup over 4-bit row-quantised tables (68-byte rows) -- unchanged code
  f8s_row     Float8BatchedEmbeddingBagMI355.lookup, e4m3, scale="row" -- unchanged code
  f8          the same, scale=None -- unchanged code
Un-pooled: mx4_seq (``lookup_sequence``, fp32 output [N, D]) against copy, a device copy of the output's size.
Quantiser (one table, fp32 source [rows, 128]): ``quantize_from_`` against a device copy of the source's size.
Error table: 4096 x 128 rows of the uniform init of 10 M / 100 k / 1 k rows, relative L1 error of MXFP4, e4m3fn with scale="row" and
4-bit row-quantised rows, each through its own HIP quantiser.
"expectation": the pooled MX4 lookup is not slower than the 4-bit row-quantised lookup -- reported, never a gate.
One JSON document to stdout and to --out (default profiles/mx4_probe.json)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import param_amd  # noqa: E402
from f8_probe import Rotating, spread, summarise, take_turns  # noqa: E402
from param_amd import _lib, mx4_bag, quant  # noqa: E402
from param_amd.indices import tbe_request  # noqa: E402


def error_table(dev):
    recs = []
    for n in (10_000_000, 100_000, 1_000):
        x = torch.empty(4096, 128, device=dev).uniform_(-1.0 / n ** 0.5, 1.0 / n ** 0.5)
        mx = param_amd.MX4BatchedEmbeddingBagMI355.from_float([x])
        f8 = param_amd.Float8BatchedEmbeddingBagMI355.from_float([x], "e4m3", scale="row")
        q4 = param_amd.QuantizedBatchedEmbeddingBagMI355([4096], 128, 4, device=dev)
        q4.quantize_from_(0, x)
        rel = lambda m: round(float((m.dequantized_table(0) - x).abs().sum() / x.abs().sum()), 5)      # noqa: E731
        recs.append({"init_rows": n, "mx4": rel(mx), "e4m3_row": rel(f8), "q4_rows": rel(q4)})
    return recs


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
    ap.add_argument("--out", default=os.path.join("profiles", "mx4_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert a.windows >= 5, "medians of at least 5 windows"
    dev = "cuda:0"
    T, B, L, D = a.tables, a.batch, a.pooling, a.dim
    rows = [a.rows] * T
    N = T * B * L
    lines = [{"exp": "mx4_probe_error_table", "shape": [4096, 128], "relative_l1": error_table(dev)}]
    print(json.dumps(lines[0]), flush=True)

    mx = param_amd.MX4BatchedEmbeddingBagMI355(rows, D, device=dev)
    q4 = param_amd.QuantizedBatchedEmbeddingBagMI355(rows, D, 4, device=dev)
    f8 = param_amd.Float8BatchedEmbeddingBagMI355(rows, D, "e4m3", device=dev)
    f8r = param_amd.Float8BatchedEmbeddingBagMI355(rows, D, "e4m3", device=dev, scale="row")
    for t in range(T):
        x = torch.randn(rows[t], D, device=dev)
        mx.quantize_from_(t, x)
        q4.quantize_from_(t, x)
        f8r.quantize_from_(t, x)
        f8.copy_from_(t, f8r.table(t))
        del x
    out32 = torch.empty(B, T * D, dtype=torch.float32, device=dev)
    seq = torch.empty(N, D, dtype=torch.float32, device=dev)
    seq2 = torch.empty_like(seq)

    def pooled(module, unroll=0):
        def call(idx, off):
            if unroll:
                _lib.set_tuning(unroll=unroll)
            r = module.lookup(idx, off, out=out32, batch=B)
            if unroll:
                _lib.set_tuning()
            return r
        return call

    # name: (call, bytes read per lookup)
    pooled_routes = {"mx4": (pooled(mx), mx4_bag.row_bytes(D)), "mx4_u4": (pooled(mx, 4), mx4_bag.row_bytes(D)),
                     "q4": (pooled(q4), quant.host_row_bytes(D, 4)), "f8s_row": (pooled(f8r), D + 1), "f8": (pooled(f8), D)}
    seq_routes = {"mx4_seq": (lambda idx, off: mx.lookup_sequence(idx, off, batch=B, out=seq), mx4_bag.row_bytes(D)),
                  "copy": (lambda idx, off: seq2.copy_(seq), None)}
    for dist, alpha in (("uniform", 0.0), ("zipf", 1.05)):
        reqs = [tbe_request(rows, B, L, alpha=alpha, device=dev, seed=10 + k) for k in range(a.rotate)]
        fns = {name: Rotating(v[0], reqs) for name, v in {**pooled_routes, **seq_routes}.items()}
        t, iters = take_turns(fns, a.windows, a.warmup, a.min_window_ms)
        idx, off = reqs[0]
        rec = {"exp": "mx4_probe", "tables": T, "rows": a.rows, "dim": D, "batch": B, "pooling": L, "lookups": N, "indices": dist,
               "rotate": a.rotate, "windows": a.windows, "lib": os.path.basename(param_amd.LIB_PATH),
               "plan": {"mx4": mx.plan(idx, off, batch=B), "mx4_seq": mx.sequence_plan(idx, off, batch=B)}, "pooled": {}, "unpooled": {}}
        for name, (_, row_b) in pooled_routes.items():
            rec["pooled"][name] = summarise(t[name], iters[name], N * (row_b + 8) + T * B * (D * 4 + 8), N)
        for name, (_, row_b) in seq_routes.items():
            rec["unpooled"][name] = summarise(t[name], iters[name], 2 * N * D * 4 if row_b is None else N * (row_b + 8) + N * D * 4, N)
        p = rec["pooled"]
        rec["ratio_mx4_to"] = {k: round(p["mx4"]["us"] / p[k]["us"], 4) for k in ("mx4_u4", "q4", "f8s_row", "f8")}
        rec["expectation"] = {"mx4_not_slower_than_q4": bool(p["mx4"]["us"] <= p["q4"]["us"] * (1 + max(p["mx4"]["spread"], p["q4"]["spread"]))),
                              "spread_used": max(p["mx4"]["spread"], p["q4"]["spread"])}
        rec["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del reqs, fns

    # the quantiser: one table's fp32 source, against a device copy of the source's size
    del q4, f8, f8r, seq, seq2
    torch.cuda.empty_cache()
    src = torch.empty(a.rows, D, dtype=torch.float32, device=dev).uniform_(-1.0 / a.rows ** 0.5, 1.0 / a.rows ** 0.5)
    dst = torch.empty_like(src)
    qfns = {"quantize_mx4": lambda: mx.quantize_from_(0, src), "copy_of_source": lambda: dst.copy_(src)}
    t, iters = take_turns(qfns, a.windows, 2, a.min_window_ms)
    rec = {"exp": "mx4_probe_quantiser", "rows": a.rows, "dim": D, "source": "fp32", "source_bytes": src.numel() * 4, "routes": {}}
    for name in qfns:
        rec["routes"][name] = {"us": round(statistics.median(t[name]), 1), "spread": round(spread(t[name]), 4), "iters": iters[name],
                               "windows_us": [round(x, 1) for x in t[name]]}
    rec["ratio_to_copy"] = round(rec["routes"]["quantize_mx4"]["us"] / rec["routes"]["copy_of_source"]["us"], 3)
    print(json.dumps(rec), flush=True)
    lines.append(rec)

    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"exp": "mx4_probe", "records": lines}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
