"""Coalesced sparse gradient (ABI v8) against the dense backward paths and torch's sparse backward, at the benchmark's fp32 shape
(48 tables x 10 M x 128, batch 8192, pooling 20) under uniform and Zipf indices.  One JSON line per measurement to stdout and to
--out (default profiles/sparse_grad.jsonl).

Per index distribution, median over --iters after --warmup:
  count_us      pm_embbag_sparse_grad_count alone (device time between events; a fresh sort before every repetition)
  apply_us      pm_embbag_sparse_grad alone (row ids, zero fill, sorted apply into the compact rows)
  call_us       BatchedEmbeddingBagMI355.sparse_grad end to end (sort + count + the synchronisation + allocation + apply; host time)
  sort_us       pm_embbag_sort_indices alone
  fused_us      the product's own backward scatter_add_ (pm_embbag_bwd_fused: may take the hybrid path)
  nonfused_us   sort_indices + scatter_add_(presorted=True): the same sort and apply into the tables
  U             distinct rows per table (min / mean / max)
  GB/s          algorithmic bytes / call time: 8 B per lookup, D*4 + 8 per bag, D*4 + 8 per unique row written
and, on ONE table of that shape, torch-ROCm's nn.EmbeddingBag(sparse=True) backward + .coalesce() (the reference's own path, K5).

Run it under rocprofv3 --kernel-trace --stats in a separate run (with --iters 3) for the per-kernel split."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import param_amd  # noqa: E402
from param_amd import _lib, embedding_bag as eb  # noqa: E402
from param_amd.indices import tbe_request  # noqa: E402


def med_events(fn, iters, warmup, pre=None):
    """median device time of fn() in us; pre() runs before each repetition, outside the timed window"""
    out = []
    for k in range(warmup + iters):
        if pre is not None:
            pre()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def med_host(fn, iters, warmup):
    out = []
    for k in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=48)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pooling", type=int, default=20)
    ap.add_argument("--alphas", default="0,1.05")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "sparse_grad.jsonl"))
    a = ap.parse_args()
    dev = "cuda:0"
    T, R, D, B, L = a.tables, a.rows, a.dim, a.batch, a.pooling
    rows = [R] * T
    lines = []

    def emit(rec):
        for k, v in {"tables": T, "rows": R, "dim": D, "batch": B, "pooling": L, "dtype": "fp32", "device": torch.cuda.get_device_name(0)}.items():
            rec.setdefault(k, v)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    m = param_amd.BatchedEmbeddingBagMI355(rows, D, device=dev, init="normal", seed=1, fused_update=False)
    grad = torch.randn(B, T * D, device=dev, generator=torch.Generator(dev).manual_seed(5)) * 1e-6
    Lib = _lib.load()
    for alpha in [float(x) for x in a.alphas.split(",")]:
        idx, off = tbe_request(rows, B, L, alpha=alpha, device=dev, seed=3)
        ts = m._tables()
        got = m.sparse_grad(grad, idx, off, batch=B)            # sizes the workspace, warms the allocator
        U = [r.numel() for r, _ in got]
        del got
        op = ts.request(idx, off, B, None, 0, None)
        mr = max(rows)
        ws = ts._ws
        s = eb._stream_ptr
        counts = torch.empty(T, dtype=torch.int64, device=dev)
        sort = lambda: _lib.check(Lib.pm_embbag_sort_indices(ctypes.byref(op), mr, ws.data_ptr(), ws.numel(), s()))      # noqa: E731
        count = lambda: _lib.check(Lib.pm_embbag_sparse_grad_count(ctypes.byref(op), mr, ws.data_ptr(), ws.numel(),      # noqa: E731
                                                                   counts.data_ptr(), s()))
        sort_us = med_events(sort, a.iters, a.warmup)
        count_us = med_events(count, a.iters, a.warmup, pre=sort)
        vals = [torch.empty(u, D, device=dev) for u in U]
        rids = [torch.empty(u, dtype=torch.int64, device=dev) for u in U]
        vp = torch.tensor([v.data_ptr() for v in vals], dtype=torch.int64, device=dev)
        rp = torch.tensor([r.data_ptr() for r in rids], dtype=torch.int64, device=dev)
        sort()
        count()
        apply_us = med_events(lambda: _lib.check(Lib.pm_embbag_sparse_grad(ctypes.byref(op), grad.data_ptr(), mr, ws.data_ptr(), ws.numel(),
                                                                           rp.data_ptr(), vp.data_ptr(), s())), a.iters, a.warmup)
        del vals, rids
        call_us = med_host(lambda: m.sparse_grad(grad, idx, off, batch=B), a.iters, a.warmup)
        fused_us = med_events(lambda: m.scatter_add_(grad, idx, off, alpha=1.0, batch=B), a.iters, a.warmup)

        def nonfused():
            m.sort_indices(idx, off, batch=B, for_adagrad=True)
            m.scatter_add_(grad, idx, off, alpha=1.0, batch=B, presorted=True)
        nonfused_us = med_events(nonfused, a.iters, a.warmup)
        n, u = T * B * L, sum(U)
        algo = 8 * n + (D * 4 + 8) * T * B + (D * 4 + 8) * u
        emit({"exp": "sparse_grad", "alpha": alpha, "sort_us": round(sort_us, 1), "count_us": round(count_us, 1),
              "apply_us": round(apply_us, 1), "call_us": round(call_us, 1), "fused_us": round(fused_us, 1),
              "nonfused_us": round(nonfused_us, 1), "U_min": min(U), "U_mean": round(u / T, 1), "U_max": max(U),
              "algo_bytes": algo, "call_GBps": round(algo / call_us / 1e3, 1), "device_GBps": round(algo / (sort_us + count_us + apply_us) / 1e3, 1)})

    if not a.no_torch:
        # the reference's K5 path on ONE table of that shape: torch-ROCm nn.EmbeddingBag(sparse=True) backward + coalesce()
        del m
        torch.cuda.empty_cache()
        emb = torch.nn.EmbeddingBag(R, D, mode="sum", sparse=True).to(dev)
        g1 = torch.randn(B, D, device=dev)
        for alpha in [float(x) for x in a.alphas.split(",")]:
            idx, off = tbe_request([R], B, L, alpha=alpha, device=dev, seed=3)
            off = off[:B].contiguous()
            out = emb(idx, off)

            def torch_bwd():
                emb.weight.grad = None
                torch.autograd.grad(out, emb.weight, g1, retain_graph=True)[0].coalesce()
            us = med_host(torch_bwd, a.iters, a.warmup)
            m1 = param_amd.BatchedEmbeddingBagMI355([R], D, device=dev, init="normal", seed=1, fused_update=False)
            ours = med_host(lambda: m1.sparse_grad(g1, idx, off, batch=B), a.iters, a.warmup)
            del m1
            torch.cuda.empty_cache()
            emit({"exp": "sparse_grad_one_table", "alpha": alpha, "tables": 1, "torch_sparse_bwd_coalesce_us": round(us, 1),
                  "sparse_grad_call_us": round(ours, 1)})
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
