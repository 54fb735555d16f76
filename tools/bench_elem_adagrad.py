#!/usr/bin/env python3
"""Step time of the fused element-wise Adagrad backward against the fused row-wise Adagrad and SGD steps, same tables, same
process, same requests.

    python tools/bench_elem_adagrad.py [--tables 16 --rows 10000000 --dim 128 --batch 8192 --pooling 20]
                                       [--dtypes fp32,bf16] [--alphas 0,1.05] [--out profiles/elem_adagrad_step.json]

Every (dtype, index distribution) case runs in a child process of its own under its own time limit; the parent stops at the first
case that fails or runs out of time and starts nothing after it.  A case: warm-up, then HIP-event windows of at least 100 ms over
four rotating requests, median of three windows per step kind.  Algorithmic bytes of a step, N lookups, U distinct (table, row)
pairs (counted from the requests), e the table element size:
    row-wise      4 D N + U (2 D e + 8)
    element-wise  4 D N + U (2 D e + 8 D)
Condition reported per case: element-wise time <= row-wise time x bytes ratio x 1.10.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8.0e12


def _time_windows(fn_of_request, n_req, min_ms=100.0, windows=3, warmup=3):
    """median over `windows` HIP-event windows of >= min_ms each of the time per call, the calls rotating over n_req requests"""
    import torch

    for w in range(warmup * n_req):
        fn_of_request(w % n_req)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(rounds):
        a.record()
        for r in range(rounds * n_req):
            fn_of_request(r % n_req)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    rounds, ms = 2, window(2)
    while ms < min_ms:
        rounds = max(rounds + 1, int(rounds * 1.3 * min_ms / max(ms, 1e-3)))
        ms = window(rounds)
    per_call = [window(rounds) / (rounds * n_req) for _ in range(windows)]
    return statistics.median(per_call), per_call, rounds * n_req


def run_case(a):
    import torch

    import param_amd
    from param_amd.indices import tbe_request

    dev = "cuda:0"
    dtype = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[a.case_dtype]
    rows, D, B, L, n_req = [a.rows] * a.tables, a.dim, a.batch, a.pooling, 4
    m = param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=dtype, device=dev, init="uniform_dlrm", seed=0, learning_rate=0.01,
                                           fused_update=False, optimizer="adagrad", eps=1e-8)
    reqs = [tbe_request(rows, B, L, alpha=a.case_alpha, device=dev, seed=100 + r) for r in range(n_req)]
    grads = [torch.randn(B, a.tables * D, device=dev, generator=torch.Generator(device=dev).manual_seed(r)) for r in range(n_req)]
    N = reqs[0][0].numel()
    U = []
    for idx, _ in reqs:
        U.append(sum(int(torch.unique(idx[t * B * L:(t + 1) * B * L]).numel()) for t in range(a.tables)))
    U = sum(U) / len(U)
    e = m.weights.element_size()
    bytes_row = 4 * D * N + U * (2 * D * e + 8)
    bytes_elem = 4 * D * N + U * (2 * D * e + 8 * D)
    out = {"dtype": a.case_dtype, "alpha": a.case_alpha, "tables": a.tables, "rows": a.rows, "dim": D, "batch": B, "pooling": L,
           "lookups": N, "distinct_pairs": U, "bytes_rowwise": bytes_row, "bytes_elementwise": bytes_elem,
           "bytes_ratio": bytes_elem / bytes_row, "device": torch.cuda.get_device_name(0)}

    def step(r):
        m.adagrad_step_(grads[r], reqs[r][0], reqs[r][1], batch=B)

    ms, per, calls = _time_windows(step, n_req)
    out["elementwise_ms"], out["elementwise_windows_ms"], out["calls_per_window"] = ms, per, calls
    out["sort_status_elementwise"] = m.sort_status(reqs[0][0], reqs[0][1], batch=B)
    out["state_bytes_elementwise"] = m.momentum.numel() * 4
    # the row-wise step on the same tables: the state buffer is shaped by the optimizer, so it is dropped and made anew
    m.optimizer, m.momentum, m._mom_base = "rowwise_adagrad", None, None
    torch.cuda.empty_cache()
    ms, per, _ = _time_windows(step, n_req)
    out["rowwise_ms"], out["rowwise_windows_ms"] = ms, per
    out["sort_status_rowwise"] = m.sort_status(reqs[0][0], reqs[0][1], batch=B)
    ms, per, _ = _time_windows(lambda r: m.scatter_add_(grads[r], reqs[r][0], reqs[r][1], alpha=-0.01, batch=B), n_req)
    out["sgd_ms"], out["sgd_windows_ms"] = ms, per
    out["elementwise_fraction_of_8TBps"] = bytes_elem / (out["elementwise_ms"] * 1e-3) / HBM_BYTES_PER_S
    out["rowwise_fraction_of_8TBps"] = bytes_row / (out["rowwise_ms"] * 1e-3) / HBM_BYTES_PER_S
    out["limit_ms"] = out["rowwise_ms"] * out["bytes_ratio"] * 1.10
    out["condition_met"] = out["elementwise_ms"] <= out["limit_ms"]
    print("CASE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tables", type=int, default=16)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pooling", type=int, default=20)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--alphas", default="0,1.05", help="0 = uniform indices, > 0 = Zipf(alpha)")
    ap.add_argument("--case-timeout", type=int, default=240, help="seconds per (dtype, alpha) child process")
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    ap.add_argument("--case-dtype", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--case-alpha", type=float, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case_dtype is not None:
        run_case(a)
        return 0
    results, rc = [], 0
    for dt in a.dtypes.split(","):
        for alpha in a.alphas.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--tables", str(a.tables), "--rows", str(a.rows), "--dim", str(a.dim),
                   "--batch", str(a.batch), "--pooling", str(a.pooling), "--case-dtype", dt, "--case-alpha", alpha]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.case_timeout)
            except subprocess.TimeoutExpired:
                print(f"case {dt} alpha={alpha}: no result within {a.case_timeout} s -- stopping here", file=sys.stderr)
                rc = 124
                break
            if r.returncode != 0:
                print(f"case {dt} alpha={alpha}: exit status {r.returncode} -- stopping here\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
                rc = r.returncode
                break
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("CASE ")][-1]
            res = json.loads(line[5:])
            results.append(res)
            print(f"{dt:5s} alpha={alpha:5s}: element-wise {res['elementwise_ms']:.3f} ms  row-wise {res['rowwise_ms']:.3f} ms  sgd {res['sgd_ms']:.3f} ms  "
                  f"bytes ratio {res['bytes_ratio']:.3f}  limit {res['limit_ms']:.3f} ms  {'met' if res['condition_met'] else 'MISSED'}", flush=True)
        if rc:
            break
    if a.out and results:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_elem_adagrad.py", "cases": results}, f, indent=1)
            f.write("\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
