#!/usr/bin/env python3
"""What the fused lazy Adam step of AdamBatchedEmbeddingBagMI355 costs next to the composition it replaces, measured in ONE process with
the routes taking turns window by window (tools/max_probe.py's harness: device events around windows of at least 110 ms sized from a pilot
window, after warm-up; medians over --windows windows, at least 5; the spread (max - min) / median reported).

Shape: 16 tables of 10 M x 128, fp32 and bf16, batch 8192, fixed pooling 20, uniform and Zipf 1.05 indices; every route walks three
requests in rotation.  All routes step the SAME slab and the same state (only time is measured).  us per call:
  fused_us        optimizer_step_: pm_embbag_bwd_adam (key sort, counter clear, adam_bwd_kernel, adam_bwd_combine_kernel)
  composed_us     sparse_grad (sort, relabel, apply into a compact [U, D] gradient; one host synchronisation, T allocations) followed by
                  sparse_adam_rows_ over it -- the only route to an Adam step before this module
  rowwise_us      the parent's fused row-wise Adagrad step on the same tables, for context (given the fixed-pooling hint, which the
                  other two routes do not take: not like for like)
The row count is lowered to what the device's free memory holds (recorded as "rows").  The expectation to report against: fused is not
slower than composed in the same run.  Not a gate, nothing is tuned.  One JSON document to stdout and to --out (default
profiles/adam_bag_probe.json)."""
from __future__ import annotations

import argparse
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
    ap.add_argument("--out", default=os.path.join("profiles", "adam_bag_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert a.windows >= 5, "medians of at least 5 windows"
    dev = "cuda:0"
    T, B, L, D = a.tables, a.batch, a.pooling, a.dim
    lr, betas, eps = 1.0e-3, (0.9, 0.999), 1.0e-8
    lines = []
    for dname in a.dtypes.split(","):
        dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[dname]
        ew = 4 if dname == "fp32" else 2
        per_row = D * (ew + 8) + 4      # the table, exp_avg and exp_avg_sq in fp32, one row-wise Adagrad value
        n_rows = min(a.rows, int(0.88 * torch.cuda.mem_get_info()[0] / (T * per_row)))
        rows = [n_rows] * T
        m = param_amd.AdamBatchedEmbeddingBagMI355(rows, D, dtype=dtype, device=dev, init="normal", seed=1, learning_rate=lr, betas=betas, eps=eps)
        ts = m._tables()
        tabs, ms, vs = ([f(t) for t in range(T)] for f in (m.table, m.exp_avg_table, m.exp_avg_sq_table))
        mom = torch.zeros(T * n_rows, device=dev)
        mom_ptrs = torch.tensor([mom.data_ptr() + 4 * t * n_rows for t in range(T)], dtype=torch.int64, device=dev)
        grad = torch.randn(B, T * D, device=dev)
        for alpha in [float(x) for x in a.alphas.split(",")]:
            reqs = [tbe_request(rows, B, L, alpha=alpha, device=dev, seed=10 + k) for k in range(3)]
            U = int(statistics.mean(sum(int(r.numel()) for r, _ in m.sparse_grad(grad, idx, off)) for idx, off in reqs))
            torch.cuda.synchronize()

            def composed(i):
                idx, off = reqs[i % 3]
                param_amd.sparse_adam_rows_(tabs, m.sparse_grad(grad, idx, off), ms, vs, i + 1, lr, betas, eps)

            fns = {
                "fused": lambda i: m.optimizer_step_(grad, *reqs[i % 3], batch=B),
                "composed": composed,
                "rowwise": lambda i: eb._adagrad(ts, grad, *reqs[i % 3], B, mom_ptrs, lr, eps, pooling=L),
            }
            r, iters = take_turns(fns, a.windows, a.warmup, a.min_window_ms)
            v = {k: statistics.median(x) for k, x in r.items()}
            step_bytes = U * (16 + 2 * ew) * D + B * T * D * 4      # m and v read + written (fp32), w read + written; grad read once
            rec = {"exp": "adam_bag_probe", "tables": T, "rows": n_rows, "dim": D, "batch": B, "pooling": L, "table_dtype": dname,
                   "zipf_alpha": alpha, "lookups": int(reqs[0][0].numel()), "distinct_rows": U, "windows": a.windows,
                   "requests_in_rotation": 3, "algorithmic_bytes": step_bytes}
            rec.update({k + "_us": round(x, 2) for k, x in v.items()})
            rec.update({k + "_spread": round(spread(x), 4) for k, x in r.items()})
            rec.update({"fused_gbps": round(step_bytes / v["fused"] / 1e3, 1), "fused_over_composed": round(v["fused"] / v["composed"], 4),
                        "fused_not_slower_than_composed": bool(v["fused"] <= v["composed"]),
                        "windows_us": {k: [round(x, 2) for x in xs] for k, xs in r.items()}, "iters": iters,
                        "device": torch.cuda.get_device_name(0)})
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as fh:                  # (after every line: a later configuration that does not fit loses nothing)
                json.dump({"exp": "adam_bag_probe", "records": lines}, fh, indent=1)
                fh.write("\n")
            del reqs
        del m, ts, tabs, ms, vs, mom, mom_ptrs, grad
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
