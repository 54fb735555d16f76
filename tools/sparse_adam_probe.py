#!/usr/bin/env python3
"""What a lazy Adam step over coalesced sparse gradients costs on the HIP path next to torch.optim.SparseAdam, measured in ONE process with
the routes taking turns window by window (tools/max_probe.py's harness: device events around windows of at least 110 ms sized from a pilot
window, after warm-up; medians over --windows windows, at least 5; the spread (max - min) / median reported).

Shape: 16 tables of 10 M x 128, fp32 and bf16, batch 8192, fixed pooling 20, uniform and Zipf 1.05 indices; every route walks three
requests in rotation.  The sparse gradients are the package's own (BatchedEmbeddingBagMI355.sparse_grad), wrapped as coalesced COO
tensors; every route call first hangs request i's gradients on the parameters, then steps.  us per call:
  adam_mi355_us        SparseAdamMI355.step(): one pm_sparse_rows_adam launch for the 16 tables (non-temporal gradient / state accesses)
  adam_mi355_plain_us  the same launch with plain accesses (pm_sparse_adam.nontemporal = 0)
  adam_torch_us        torch.optim.SparseAdam.step() on the same parameters and gradients
  copy_us              a device copy that moves what an fp32 step moves, 7 U D floats read + written, for context
For fp32 tables the two optimizers step the same state tensors in turn (only time is measured: three table-sized arrays are 246 GB).
torch keeps the state of a bf16 table in bf16, so the bf16 lines hold two state sets, and the row count is lowered to what the device's
free memory holds (recorded as "rows").  The expectation to report against: adam_mi355 is not slower than adam_torch in the same run.
Not a gate, nothing is tuned.  One JSON document to stdout and to --out (default profiles/sparse_adam_probe.json)."""
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
    ap.add_argument("--out", default=os.path.join("profiles", "sparse_adam_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert a.windows >= 5, "medians of at least 5 windows"
    dev = "cuda:0"
    T, B, L, D = a.tables, a.batch, a.pooling, a.dim
    lines = []
    for dname in a.dtypes.split(","):
        dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[dname]
        ew = 4 if dname == "fp32" else 2
        # bytes per table row resident: the table, our fp32 state, and torch's own state where it cannot share ours (16-bit tables)
        per_row = D * (ew + 8 + (0 if ew == 4 else 2 * ew))
        free = torch.cuda.mem_get_info()[0]
        n_rows = min(a.rows, int(0.88 * free / (T * per_row)))
        rows = [n_rows] * T
        m = param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=dtype, device=dev, init="normal", seed=1, fused_update=False)
        params = [torch.nn.Parameter(m.table(t)) for t in range(T)]
        ours = param_amd.SparseAdamMI355(params, lr=1e-3)
        ref = torch.optim.SparseAdam(params, lr=1e-3)
        for p in params:
            state = {"step": 0, "exp_avg": torch.zeros(p.shape, device=dev), "exp_avg_sq": torch.zeros(p.shape, device=dev)}
            ours.state[p].update(state)
            ref.state[p].update(state if ew == 4 else {"step": 0, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)})
        grad = torch.randn(B, T * D, device=dev)
        for alpha in [float(x) for x in a.alphas.split(",")]:
            reqs = [tbe_request(rows, B, L, alpha=alpha, device=dev, seed=10 + k) for k in range(3)]
            sets = [[torch.sparse_coo_tensor(r[None], v.to(dtype), tuple(p.shape), is_coalesced=True)
                     for p, (r, v) in zip(params, m.sparse_grad(grad, idx, off))] for idx, off in reqs]
            U = int(statistics.mean(sum(int(g._values().shape[0]) for g in gs) for gs in sets))
            src = torch.empty(7 * U * D // 2, device=dev)
            dst = torch.empty_like(src)
            torch.cuda.synchronize()

            def hang(i):
                for p, g in zip(params, sets[i % 3]):
                    p.grad = g

            def mi355(i, nontemporal):
                hang(i)
                optim._NONTEMPORAL = nontemporal
                ours.step()

            fns = {
                "adam_mi355": lambda i: mi355(i, True),
                "adam_mi355_plain": lambda i: mi355(i, False),
                "adam_torch": lambda i: (hang(i), ref.step()),
                "copy": lambda i: dst.copy_(src),
            }
            r, iters = take_turns(fns, a.windows, a.warmup, a.min_window_ms)
            optim._NONTEMPORAL = True
            v = {k: statistics.median(x) for k, x in r.items()}
            step_bytes = U * ((20 + 2 * ew) * D + 8)      # g read, m and v read + written (fp32), w read + written, the row id
            rec = {"exp": "sparse_adam_probe", "tables": T, "rows": n_rows, "dim": D, "batch": B, "pooling": L, "table_dtype": dname,
                   "zipf_alpha": alpha, "lookups": int(reqs[0][0].numel()), "distinct_rows": U, "windows": a.windows,
                   "requests_in_rotation": 3, "algorithmic_bytes": step_bytes}
            rec.update({k + "_us": round(x, 2) for k, x in v.items()})
            rec.update({k + "_spread": round(spread(x), 4) for k, x in r.items()})
            rec.update({"mi355_gbps": round(step_bytes / v["adam_mi355"] / 1e3, 1),
                        "mi355_plain_gbps": round(step_bytes / v["adam_mi355_plain"] / 1e3, 1),
                        "copy_gbps": round(src.numel() * 8 / v["copy"] / 1e3, 1),
                        "mi355_over_torch": round(v["adam_mi355"] / v["adam_torch"], 4),
                        "mi355_not_slower_than_torch": bool(v["adam_mi355"] <= v["adam_torch"]),
                        "windows_us": {k: [round(x, 2) for x in xs] for k, xs in r.items()}, "iters": iters,
                        "device": torch.cuda.get_device_name(0)})
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as fh:                  # (after every line: a later configuration that does not fit loses nothing)
                json.dump({"exp": "sparse_adam_probe", "records": lines}, fh, indent=1)
                fh.write("\n")
            del reqs, sets, src, dst
        for p in params:
            p.grad = None
        del m, params, ours, ref, grad, state
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
