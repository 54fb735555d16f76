#!/usr/bin/env python3
"""The per_sample_weights gradient (pm_embbag_psw_grad) against its yardstick: the WEIGHTED FORWARD of the same request, in the
same process, the two taking turns window by window.  Both gather the same rows; the forward writes [B, sum D] fp32 and reads one
weight per lookup, the gradient kernel reads [B, sum D] fp32 and writes one value per lookup.

Shapes: the benchmark's 48 x 10 M x 128 fp32 tables, batch 8192, pooling 20, under uniform and Zipf(1.05) indices, and the Criteo
tables with mixed dims (dataset.criteo_v2_mixed_dims; multi-hot pooling 1 .. 100), uniform and Zipf(1.05).  Four requests of every
kind rotate, so that no call finds the rows of the call before it in the caches.  Per shape: --windows windows (at least three) of --iters
calls each per kernel, device events around a window, medians over the windows; one JSON line per shape to stdout and to --out
(default profiles/psw_grad_probe.jsonl):
  psw_grad_us / fwd_weighted_us   median window time per call
  ratio                           psw_grad_us / fwd_weighted_us
  *_alg_frac                      algorithmic bytes / time over 8 TB/s.  Gradient kernel: D e row bytes + the index + 4 bytes out per lookup,
                                  T B D 4 gradient bytes and the offsets per call; forward: the same rows and index + 4 bytes of
                                  weight per lookup, T B D 4 output bytes and the offsets per call.
Run it under rocprofv3 --kernel-trace --stats in a run of its own (--windows 3 --iters 5) for kernel times."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import param_amd  # noqa: E402
from param_amd.compute.pt import dataset as ds  # noqa: E402
from param_amd.indices import tbe_request  # noqa: E402


def window_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bench,criteo")
    ap.add_argument("--tables", type=int, default=48)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pooling", type=int, default=20)
    ap.add_argument("--alphas", default="0,1.05")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join("profiles", "psw_grad_probe.jsonl"))
    a = ap.parse_args()
    if a.windows < 3:
        ap.error("--windows must be at least 3")
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    dev = "cuda:0"
    B = a.batch
    lines = []
    for shape in a.shapes.split(","):
        if shape == "bench":
            rows, dims, pools = [a.rows] * a.tables, [a.dim] * a.tables, a.pooling
            per_table = [a.pooling] * a.tables
        elif shape == "criteo":
            rows = list(ds.criteo_v2_rows)
            dims, per_table = ds.criteo_v2_mixed_dims(rows), list(ds.criteo_v2_multi_hot)
            pools = per_table
        else:
            ap.error(f"unknown shape {shape}")
        T = len(rows)
        m = param_amd.BatchedEmbeddingBagMI355(rows, dims, dtype=torch.float32, device=dev, init="normal", seed=1, fused_update=False)
        grad = torch.randn(B, sum(dims), device=dev)
        fwd_out = torch.empty(B, sum(dims), device=dev)
        n = B * sum(per_table)
        rows_bytes = sum(B * L * (D * 4 + 8) for L, D in zip(per_table, dims))
        dense_bytes = B * sum(dims) * 4 + T * B * 8
        alg = rows_bytes + 4 * n + dense_bytes                  # the same count for both kernels: 4 B per lookup out / in, [B, sum D] in / out
        for alpha in [float(x) for x in a.alphas.split(",")]:
            reqs = [tbe_request(rows, B, pools, alpha=alpha, device=dev, seed=2 + 1000 * k) for k in range(4)]
            psw = torch.rand(n, device=dev) + 0.5
            pg_out = torch.empty(n, device=dev)
            k = [0, 0]

            def grad_call():
                i, o = reqs[k[0] % 4]
                k[0] += 1
                m.per_sample_weights_grad(grad, i, o, batch=B, out=pg_out)

            def fwd_call():
                i, o = reqs[k[1] % 4]
                k[1] += 1
                m.lookup(i, o, psw, out=fwd_out, batch=B)

            for _ in range(a.warmup):
                grad_call()
                fwd_call()
            torch.cuda.synchronize()
            g_us, f_us = [], []
            for _ in range(a.windows):                          # the two kernels take turns
                g_us.append(window_us(grad_call, a.iters))
                f_us.append(window_us(fwd_call, a.iters))
            g, f = statistics.median(g_us), statistics.median(f_us)
            rec = {"exp": "psw_grad_probe", "shape": shape, "tables": T, "batch": B, "lookups": n, "alpha": alpha, "dtype": "fp32",
                   "dims": dims[0] if len(set(dims)) == 1 else "mixed", "windows": a.windows, "iters": a.iters,
                   "psw_grad_us": round(g, 2), "fwd_weighted_us": round(f, 2), "ratio": round(g / f, 4),
                   "psw_grad_windows_us": [round(x, 2) for x in g_us], "fwd_weighted_windows_us": [round(x, 2) for x in f_us],
                   "alg_MB": round(alg / 1e6, 1), "psw_grad_alg_frac": round(alg / (g * 1e-6) / 8e12, 4),
                   "fwd_weighted_alg_frac": round(alg / (f * 1e-6) / 8e12, 4), "device": torch.cuda.get_device_name(0)}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del reqs, psw, pg_out
        del m, grad, fwd_out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
