#!/usr/bin/env python3
"""What an SGD, Adagrad or row-wise Adagrad step over coalesced sparse gradients costs on the HIP path next to torch.optim.SGD /
torch.optim.Adagrad, measured in ONE process with the routes taking turns window by window (tools/max_probe.py's harness: device events
around windows of at least 110 ms sized from a pilot window, after warm-up; medians over --windows windows, at least 5; the spread
(max - min) / median reported).  tools/sparse_adam_probe.py's shape and gradients:

16 tables of 10 M x 128, fp32 and bf16, batch 8192, fixed pooling 20, uniform and Zipf 1.05 indices; every route walks three requests in
rotation.  The sparse gradients are the package's own (BatchedEmbeddingBagMI355.sparse_grad), wrapped as coalesced COO tensors; every
route call first hangs request i's gradients on the parameters, then steps.  Per rule R in sgd, adagrad, rowwise, us per call:
  R_mi355_us        the optimizer class's step(): one launch for the 16 tables (non-temporal gradient / state accesses)
  R_mi355_plain_us  the same launch with plain accesses
  R_torch_us        torch.optim.SGD / torch.optim.Adagrad .step() on the same parameters and gradients (rowwise: torch has none; the
                    element-wise torch.optim.Adagrad figure is repeated for context)
  R_copy_us         a device copy that moves the step's algorithmic bytes, for context
Algorithmic bytes per distinct row, e_w the table's element size: sgd (4 + 2 e_w) D + 8, adagrad (12 + 2 e_w) D + 8, rowwise
(4 + 2 e_w) D + 16.  For fp32 tables the element-wise optimizers step the same `sum` tensors in turn (only time is measured).  torch
keeps the state of a bf16 table in bf16, so the bf16 lines hold two state sets; the row count is lowered to what the device's free
memory holds (recorded as "rows").  The expectation to report against: R_mi355 is not slower than R_torch in the same run.  Not a gate,
nothing is tuned.  One JSON document to stdout and to --out (default profiles/sparse_step_probe.json)."""
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
from param_amd import optim  # noqa: E402
from param_amd.indices import tbe_request  # noqa: E402

RULES = ("sgd", "adagrad", "rowwise")


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
    ap.add_argument("--out", default=os.path.join("profiles", "sparse_step_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert a.windows >= 5, "medians of at least 5 windows"
    dev = "cuda:0"
    T, B, L, D = a.tables, a.batch, a.pooling, a.dim
    lines = []
    for dname in a.dtypes.split(","):
        dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[dname]
        ew = 4 if dname == "fp32" else 2
        # bytes per table row resident: the table, our fp32 sum and torch's own sum (fp32 tables share one afterwards: the second is transient)
        per_row = D * (ew + 4 + ew) + 4
        free = torch.cuda.mem_get_info()[0]
        n_rows = min(a.rows, int(0.88 * free / (T * per_row)))
        rows = [n_rows] * T
        m = param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=dtype, device=dev, init="normal", seed=1, fused_update=False)
        params = [torch.nn.Parameter(m.table(t)) for t in range(T)]
        ours = {"sgd": param_amd.SparseSGDMI355(params, lr=1e-2), "adagrad": param_amd.SparseAdagradMI355(params, lr=1e-2),
                "rowwise": param_amd.SparseAdagradMI355(params, lr=1e-2, rowwise=True)}
        ref = {"sgd": torch.optim.SGD(params, lr=1e-2), "adagrad": torch.optim.Adagrad(params, lr=1e-2)}
        if ew == 4:
            for p in params:
                ref["adagrad"].state[p]["sum"] = ours["adagrad"].state[p]["sum"]
            torch.cuda.empty_cache()
        grad = torch.randn(B, T * D, device=dev)
        for alpha in [float(x) for x in a.alphas.split(",")]:
            reqs = [tbe_request(rows, B, L, alpha=alpha, device=dev, seed=10 + k) for k in range(3)]
            sets = [[torch.sparse_coo_tensor(r[None], v.to(dtype), tuple(p.shape), is_coalesced=True)
                     for p, (r, v) in zip(params, m.sparse_grad(grad, idx, off))] for idx, off in reqs]
            U = int(statistics.mean(sum(int(g._values().shape[0]) for g in gs) for gs in sets))
            step_bytes = {"sgd": U * ((4 + 2 * ew) * D + 8), "adagrad": U * ((12 + 2 * ew) * D + 8), "rowwise": U * ((4 + 2 * ew) * D + 16)}
            src = {r: torch.empty(step_bytes[r] // 8, device=dev) for r in RULES}       # a copy reads and writes each float: 8 bytes
            dst = {r: torch.empty_like(src[r]) for r in RULES}
            torch.cuda.synchronize()

            def hang(i):
                for p, g in zip(params, sets[i % 3]):
                    p.grad = g

            def mi355(rule, i, nontemporal):
                hang(i)
                optim._NONTEMPORAL = nontemporal
                ours[rule].step()

            fns = {}
            for r in RULES:
                fns[r + "_mi355"] = lambda i, r=r: mi355(r, i, True)
                fns[r + "_mi355_plain"] = lambda i, r=r: mi355(r, i, False)
                if r in ref:
                    fns[r + "_torch"] = lambda i, r=r: (hang(i), ref[r].step())
                fns[r + "_copy"] = lambda i, r=r: dst[r].copy_(src[r])
            res, iters = take_turns(fns, a.windows, a.warmup, a.min_window_ms)
            optim._NONTEMPORAL = True
            res["rowwise_torch"] = res["adagrad_torch"]
            v = {k: statistics.median(x) for k, x in res.items()}
            rec = {"exp": "sparse_step_probe", "tables": T, "rows": n_rows, "dim": D, "batch": B, "pooling": L, "table_dtype": dname,
                   "zipf_alpha": alpha, "lookups": int(reqs[0][0].numel()), "distinct_rows": U, "windows": a.windows,
                   "requests_in_rotation": 3, "algorithmic_bytes": step_bytes}
            rec.update({k + "_us": round(x, 2) for k, x in v.items()})
            rec.update({k + "_spread": round(spread(x), 4) for k, x in res.items()})
            for r in RULES:
                rec.update({r + "_mi355_gbps": round(step_bytes[r] / v[r + "_mi355"] / 1e3, 1),
                            r + "_mi355_plain_gbps": round(step_bytes[r] / v[r + "_mi355_plain"] / 1e3, 1),
                            r + "_copy_gbps": round(src[r].numel() * 8 / v[r + "_copy"] / 1e3, 1),
                            r + "_mi355_over_torch": round(v[r + "_mi355"] / v[r + "_torch"], 4),
                            r + "_mi355_not_slower_than_torch": bool(v[r + "_mi355"] <= v[r + "_torch"])})
            rec.update({"windows_us": {k: [round(x, 2) for x in xs] for k, xs in res.items()}, "iters": iters,
                        "device": torch.cuda.get_device_name(0)})
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as fh:                  # (after every line: a later configuration that does not fit loses nothing)
                json.dump({"exp": "sparse_step_probe", "records": lines}, fh, indent=1)
                fh.write("\n")
            del reqs, sets, src, dst
        for p in params:
            p.grad = None
        del m, params, ours, ref, grad
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
