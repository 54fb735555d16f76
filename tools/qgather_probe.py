#!/usr/bin/env python3
"""What the un-pooled lookup over row-quantised tables costs, measured in ONE process with the variants taking turns window by window.

Shape (the probes' usual request): 16 tables of 10 M x 128, batch 8192, pooling 20 -> 2.6 M lookups; uniform and Zipf (alpha 1.05)
indices.  Every variant is fed --rotate different requests in turn, so that no call finds the rows of the call before in a cache.
Device events around windows of at least 100 ms (the iteration count is sized from a pilot window), after warm-up; medians over
--windows windows (at least 5), spread = (max - min) / median.

Per case (8- and 4-bit tables x fp32 and fp16 output x distribution), us per call:
  qgather_us              lookup_sequence (pm_embedding_gather_qrows) under the default rows in flight (launch_plan.h: kQgatherUnroll)
  qgather_u{1,2,4,8}_us   ... with that many rows in flight per lane group (pm_set_tuning's unroll)
  bag_of_one_us           the same rows through the pooled lookup (pm_embbag_fwd_qrows) as bags of one -- offsets = arange(N), output
                          [N / T, T * D]: the only route without the new entry point, unchanged code, the yardstick
  bf16_sequence_us        context: the bf16-table lookup_sequence (pm_embedding_gather) into the same output dtype
  copy_us                 context: a device-to-device copy of the output's size
  bytes_per_lookup        algorithmic: row_bytes read, the 8-byte index, D * e_out written;  *_frac_of_8TBs = bytes / time / 8e12, and which
                          side -- the rows read or the output written -- is the larger share of those bytes ("bound_by")
  expectation: the new call is not slower than the bag-of-one route by more than the larger of the two spreads ("qgather_not_slower").
--wide-dim D (default 512; 0: none) adds the rows-in-flight sweep for 8- and 4-bit tables of that width (lane groups of 64 / 32 lanes,
whose instances hold the most registers), fp32 output, uniform indices: --wide-rows rows per table, pooling 5.
Nothing here is a gate.  One JSON document to stdout and to --out (default profiles/qgather_probe.json)."""
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
from param_amd.embedding_bag import _gather  # noqa: E402
from param_amd.indices import tbe_request  # noqa: E402

PEAK = 8.0e12      # bytes / s: the HBM peak the project's fractions are stated against
UNROLLS = (1, 2, 4, 8)
ODT = {"fp32": torch.float32, "fp16": torch.float16}


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


def sequence(m, reqs, B, out, unroll):
    def call(idx, off):
        param_amd.set_tuning(unroll=unroll)
        m.lookup_sequence(idx, off, batch=B, out=out)
    return Rotating(call, reqs)


def sweep_fields(t, med):
    return {"unroll_sweep_us": {str(u): round(med(t[f"qgather_u{u}"]), 2) for u in UNROLLS},
            "unroll_sweep_spread": {str(u): round(spread(t[f"qgather_u{u}"]), 4) for u in UNROLLS}}


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
    ap.add_argument("--wide-dim", type=int, default=512)
    ap.add_argument("--wide-rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join("profiles", "qgather_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert a.windows >= 5, "medians of at least 5 windows"
    dev = "cuda:0"
    T, B, L, D = a.tables, a.batch, a.pooling, a.dim
    rows = [a.rows] * T
    n = B * L                      # lookups per table
    N = T * n
    med = statistics.median
    name = torch.cuda.get_device_name(0)
    lines = []

    # the bf16 tables are the source: the quantised tables are quantize_rows of them, widened (the existing kernel)
    m16 = param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=torch.bfloat16, device=dev, init="normal", seed=1, fused_update=False)
    q = {(bits, o): param_amd.QuantizedBatchedEmbeddingBagMI355(rows, D, bits, device=dev, output_dtype=ODT[o]) for bits in (8, 4) for o in ODT}
    for t in range(T):
        src = m16.table(t).float()
        for bits in (8, 4):
            q[bits, "fp32"].quantize_from_(t, src)
            q[bits, "fp16"].table(t).copy_(q[bits, "fp32"].table(t))
        del src
    one = torch.arange(N + 1, dtype=torch.int64, device=dev)           # the bag-of-one route's offsets: part of its cost
    for dist, alpha in (("uniform", 0.0), ("zipf", 1.05)):
        reqs = [tbe_request(rows, B, L, alpha=alpha, device=dev, seed=10 + k) for k in range(a.rotate)]
        for o, odt in ODT.items():
            e = odt.itemsize
            seq_out = torch.empty(N, D, dtype=odt, device=dev)
            bag_out = torch.empty(n, T * D, dtype=odt, device=dev)
            spare = torch.empty_like(seq_out)
            for bits in (8, 4):
                m = q[bits, o]

                def bag_of_one(idx, off, m=m):
                    param_amd.set_tuning(unroll=0)
                    m.lookup(idx, one, batch=n, out=bag_out)

                def bf16_sequence(idx, off):
                    param_amd.set_tuning(unroll=0)
                    _gather(m16._tables(), idx, off, B, odt, seq_out)

                fns = {"qgather": sequence(m, reqs, B, seq_out, 0), "bag_of_one": Rotating(bag_of_one, reqs),
                       "bf16_sequence": Rotating(bf16_sequence, reqs), "copy": lambda: spare.copy_(seq_out)}
                fns.update({f"qgather_u{u}": sequence(m, reqs, B, seq_out, u) for u in UNROLLS})
                t, iters = take_turns(fns, a.windows, a.warmup, a.min_window_ms)
                param_amd.set_tuning()
                idx, off = reqs[0]                                    # same rows, either route: bit for bit
                m.lookup_sequence(idx, off, batch=B, out=seq_out)
                m.lookup(idx, one, batch=n, out=bag_out)
                agree = bool(torch.equal(seq_out.view(T, n, D).permute(1, 0, 2).reshape(n, T * D), bag_out))
                rb = quant.host_row_bytes(D, bits)
                bytes_per = rb + 8 + D * e
                g, b1 = med(t["qgather"]), med(t["bag_of_one"])
                margin = max(spread(t["qgather"]), spread(t["bag_of_one"]))
                rec = {"exp": "qgather_probe", "tables": T, "rows": a.rows, "dim": D, "batch": B, "pooling": L, "lookups": N, "bits": bits,
                       "out_dtype": o, "indices": dist, "rotate": a.rotate, "windows": a.windows, "bytes_per_lookup": bytes_per,
                       "bound_by": "stores" if D * e >= rb + 8 else "loads", "default_unroll": m.sequence_plan(idx, off, batch=B)["unroll"],
                       "qgather_us": round(g, 2), "bag_of_one_us": round(b1, 2), "bf16_sequence_us": round(med(t["bf16_sequence"]), 2),
                       "copy_us": round(med(t["copy"]), 2), "qgather_over_bag_of_one": round(g / b1, 4),
                       "qgather_spread": round(spread(t["qgather"]), 4), "bag_of_one_spread": round(spread(t["bag_of_one"]), 4),
                       "qgather_not_slower": bool(g <= b1 * (1 + margin)),
                       "qgather_frac_of_8TBs": round(N * bytes_per / (g * 1e-6) / PEAK, 4),
                       "bag_of_one_frac_of_8TBs": round(N * bytes_per / (b1 * 1e-6) / PEAK, 4),
                       "copy_frac_of_8TBs": round(2 * N * D * e / (med(t["copy"]) * 1e-6) / PEAK, 4),
                       **sweep_fields(t, med), "routes_agree": agree,
                       "windows_us": {k: [round(x, 2) for x in v] for k, v in t.items()}, "iters": iters, "device": name}
                print(json.dumps(rec), flush=True)
                lines.append(rec)
            del seq_out, bag_out, spare
        del reqs
    del m16, q, one
    torch.cuda.empty_cache()

    if a.wide_dim:
        W, Lw = a.wide_dim, 5
        wrows = [a.wide_rows] * T
        Nw = T * B * Lw
        src = torch.randn(a.wide_rows, W, device=dev)
        out = torch.empty(Nw, W, dtype=torch.float32, device=dev)
        reqs = [tbe_request(wrows, B, Lw, alpha=0.0, device=dev, seed=20 + k) for k in range(a.rotate)]
        for bits in (8, 4):
            m = param_amd.QuantizedBatchedEmbeddingBagMI355(wrows, W, bits, device=dev)
            m.quantize_from_(0, src)
            for t in range(1, T):
                m.table(t).copy_(m.table(0))
            fns = {f"qgather_u{u}": sequence(m, reqs, B, out, u) for u in UNROLLS}
            t, iters = take_turns(fns, a.windows, a.warmup, a.min_window_ms)
            param_amd.set_tuning()
            rec = {"exp": "qgather_probe_wide", "tables": T, "rows": a.wide_rows, "dim": W, "batch": B, "pooling": Lw, "lookups": Nw, "bits": bits,
                   "out_dtype": "fp32", "indices": "uniform", "group_lanes": m.sequence_plan(*reqs[0], batch=B)["group_lanes"],
                   **sweep_fields(t, med), "windows_us": {k: [round(x, 2) for x in v] for k, v in t.items()}, "iters": iters, "device": name}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del m
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"exp": "qgather_probe", "records": lines}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
