#!/usr/bin/env python3
"""What the direct backward of max pooling costs next to the expansion route and the sum step, measured in ONE process with the routes
taking turns window by window (tools/max_probe.py's harness: device events around windows of at least 110 ms sized from a pilot window,
after warm-up; medians over --windows windows, at least 5; the spread (max - min) / median reported).

Shape: 16 tables of 10 M x 128, fp32 and bf16, batch 8192, fixed pooling 20, uniform and Zipf 1.05 indices; every route walks three
requests in rotation.  All three are scatter_add_ steps into the tables themselves, us per call:
  bwd_sum_us          the sum module's step: pm_embbag_bwd_fused on the [B, T * D] gradient
  bwd_max_sorted_us   the max module's expansion route with saved max_indices: pm_embbag_max_grad into the [N, D] fp32 scratch, then
                      pm_embseq_bwd_fused
  bwd_max_direct_us   the max module's direct route with saved max_indices: pm_embbag_max_bwd (key sort + apply through max_indices)
The expectation to report against: direct is not slower than the expansion route measured in the same run.  Not a gate, nothing is tuned.
One JSON document to stdout and to --out (default profiles/max_direct_probe.json)."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import param_amd  # noqa: E402
from max_probe import spread, take_turns  # noqa: E402
from param_amd import _lib  # noqa: E402
from param_amd import embedding_bag as eb  # noqa: E402
from param_amd.indices import tbe_request  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=16)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pooling", type=int, default=20)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--alphas", default="0,1.05", help="Zipf exponents; 0 = uniform")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--min-window-ms", type=float, default=110.0)
    ap.add_argument("--out", default=os.path.join("profiles", "max_direct_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert a.windows >= 5, "medians of at least 5 windows"
    dev = "cuda:0"
    T, B, L, D = a.tables, a.batch, a.pooling, a.dim
    rows = [a.rows] * T
    lr = 1.0e-3
    lines = []
    for dname in a.dtypes.split(","):
        dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[dname]
        # ONE slab serves every route: the sum and the max steps are host functions over the same table set
        m = param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=dtype, device=dev, init="normal", seed=1, fused_update=False)
        ts = m._tables()
        grad = torch.randn(B, T * D, device=dev)
        for alpha in [float(x) for x in a.alphas.split(",")]:
            reqs = [tbe_request(rows, B, L, alpha=alpha, device=dev, seed=10 + k) for k in range(3)]
            args = [eb._fwd_max(ts, idx, off, B, max_indices=True)[1] for idx, off in reqs]      # saved, as a training step holds them
            torch.cuda.synchronize()
            n = int(reqs[0][0].numel())
            op = ts.request(*reqs[0], B, None, 0, None)
            ws_sorted = int(_lib.load().pm_embbag_bwd_sorted_workspace(ctypes.byref(op), a.rows))
            ws_direct = int(_lib.load().pm_embbag_max_bwd_workspace(ctypes.byref(op), a.rows))
            rq = lambda i: reqs[i % 3]                                                                            # noqa: E731
            fns = {
                "bwd_sum": lambda i: eb._bwd(ts, grad, *rq(i), B, ts.d_ptrs, dtype, -lr),
                "bwd_max_sorted": lambda i: eb._max_bwd(ts, grad, *rq(i), B, ts.d_ptrs, dtype, -lr, None, args[i % 3]),
                "bwd_max_direct": lambda i: eb._max_bwd_direct(ts, grad, *rq(i), B, ts.d_ptrs, dtype, -lr, None, args[i % 3]),
            }
            r, iters = take_turns(fns, a.windows, a.warmup, a.min_window_ms)
            v = {k: statistics.median(x) for k, x in r.items()}
            rec = {"exp": "max_direct_probe", "tables": T, "rows": a.rows, "dim": D, "batch": B, "pooling": L, "table_dtype": dname,
                   "zipf_alpha": alpha, "lookups": n, "windows": a.windows, "requests_in_rotation": 3, "g_seq_bytes": n * D * 4,
                   "direct_extra_workspace_bytes": ws_direct - ws_sorted}
            rec.update({k + "_us": round(x, 2) for k, x in v.items()})
            rec.update({k + "_spread": round(spread(x), 4) for k, x in r.items()})
            rec.update({"sorted_over_sum": round(v["bwd_max_sorted"] / v["bwd_sum"], 4),
                        "direct_over_sum": round(v["bwd_max_direct"] / v["bwd_sum"], 4),
                        "direct_over_sorted": round(v["bwd_max_direct"] / v["bwd_max_sorted"], 4),
                        "direct_not_slower_than_sorted": bool(v["bwd_max_direct"] <= v["bwd_max_sorted"]),
                        "windows_us": {k: [round(x, 2) for x in xs] for k, xs in r.items()}, "iters": iters,
                        "device": torch.cuda.get_device_name(0)})
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del reqs, args
        del m, ts, grad
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"exp": "max_direct_probe", "records": lines}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
