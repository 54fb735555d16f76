#!/usr/bin/env python3
"""The device-side bounds check (pm_embbag_bounds_check) against its yardstick: the FORWARD of the same request, in the same process,
the two taking turns window by window.  What bounds_check_mode="warning" / "ignore" adds in front of every lookup.

Shape: the benchmark's 48 x 10 M x 128 fp32 tables, batch 8192, pooling 20, uniform indices, int64 (and int32 with --index-dtypes);
CLEAN requests -- what a training loop sees step after step: the sanitiser reads everything and writes nothing -- and, with --bad,
requests in which that share of the indices is out of range, restored from a pristine copy before every window (the repair makes
them clean).  Four requests rotate.  Per line: --windows windows (at least three) of --iters calls each per kernel, device events
around a window, medians over the windows; one JSON line per shape to stdout and to --out (default profiles/bounds_check_probe.jsonl):
  bounds_us / fwd_us     median window time per call (the four launches of the sanitiser together)
  ratio                  bounds_us / fwd_us
  bounds_read_frac       (N + T B + 1) index-sized bytes / time over the 6.29 TB/s measured streaming-copy rate
Run it under rocprofv3 --kernel-trace --stats in a run of its own (--windows 3 --iters 5) for the four kernels' own times."""
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
    ap.add_argument("--tables", type=int, default=48)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pooling", type=int, default=20)
    ap.add_argument("--index-dtypes", default="int64")
    ap.add_argument("--modes", default="warning,ignore")
    ap.add_argument("--bad", default="0", help="shares of out-of-range indices, comma separated (0 = clean requests)")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join("profiles", "bounds_check_probe.jsonl"))
    a = ap.parse_args()
    if a.windows < 3:
        ap.error("--windows must be at least 3")
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    dev = "cuda:0"
    T, B, L = a.tables, a.batch, a.pooling
    rows = [a.rows] * T
    m = param_amd.BatchedEmbeddingBagMI355(rows, a.dim, dtype=torch.float32, device=dev, init="normal", seed=1, fused_update=False)
    fwd_out = torch.empty(B, T * a.dim, device=dev)
    n = T * B * L
    lines = []
    for idt in a.index_dtypes.split(","):
        tdt = getattr(torch, idt)
        esz = 8 if idt == "int64" else 4
        clean = [tuple(t.to(tdt) for t in tbe_request(rows, B, L, alpha=0.0, device=dev, seed=2 + 1000 * k)) for k in range(4)]
        for share in [float(x) for x in a.bad.split(",")]:
            reqs = [(i.clone(), o.clone()) for i, o in clean]
            n_bad = int(share * n)
            if n_bad:
                g = torch.Generator(device=dev).manual_seed(5)
                for i, _ in reqs:
                    i[torch.randint(0, n, (n_bad,), device=dev, generator=g)] = a.rows + 7
            pristine = [i.clone() for i, _ in reqs] if n_bad else None
            for i, o in reqs:                                   # the yardstick looks up what the sanitiser leaves: repair once, check
                m.sanitize_(i, o, batch=B, mode="ignore")
                m.check(i, o, batch=B)
            for mode in a.modes.split(","):
                k = [0, 0]

                def bounds_call():
                    i, o = (bad_reqs if n_bad else reqs)[k[0] % 4]
                    k[0] += 1
                    m.sanitize_(i, o, batch=B, mode=mode)

                def fwd_call():
                    i, o = reqs[k[1] % 4]
                    k[1] += 1
                    m.lookup(i, o, out=fwd_out, batch=B)

                bad_reqs = [(p.clone(), o) for p, (_, o) in zip(pristine, reqs)] if n_bad else None
                for _ in range(a.warmup):
                    bounds_call()
                    fwd_call()
                torch.cuda.synchronize()
                b_us, f_us = [], []
                for _ in range(a.windows):                      # the two take turns
                    if n_bad:                                   # a repaired request is clean: every window starts from the bad one
                        for (bi, _), p in zip(bad_reqs, pristine):          # (only its first pass over a request repairs)
                            bi.copy_(p)
                        torch.cuda.synchronize()
                    b_us.append(window_us(bounds_call, a.iters))
                    f_us.append(window_us(fwd_call, a.iters))
                bu, fu = statistics.median(b_us), statistics.median(f_us)
                read = (n + T * B + 1) * esz
                rec = {"exp": "bounds_check_probe", "tables": T, "batch": B, "pooling": L, "lookups": n, "index_dtype": idt, "mode": mode,
                       "bad_share": share, "windows": a.windows, "iters": a.iters, "bounds_us": round(bu, 2), "fwd_us": round(fu, 2),
                       "ratio": round(bu / fu, 4), "bounds_windows_us": [round(x, 2) for x in b_us],
                       "fwd_windows_us": [round(x, 2) for x in f_us], "read_MB": round(read / 1e6, 1),
                       "bounds_read_frac": round(read / (bu * 1e-6) / 6.29e12, 4), "report": m.bounds_report(),
                       "device": torch.cuda.get_device_name(0)}
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                del bad_reqs
            del reqs, pristine
        del clean
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
