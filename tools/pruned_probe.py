#!/usr/bin/env python3
"""What the index remapping of PRUNED tables costs fused into the lookup against the only route there was before it, measured in ONE
process with the routes taking turns window by window.

Shapes (half of every table's logical rows are kept; tables t = 0, 2, .. are 8-bit, t = 1, 3, .. are 4-bit):
  bench     16 tables of 10 M logical rows x 128, batch 8192, pooling 20 (2.6 M lookups); uniform and Zipf (alpha 1.05) indices; fp32 output
  serving   64 tables of 1 M logical rows x 64, batch 256, pooling 10 (164 K lookups); uniform and Zipf indices; fp32 output
Every route is fed --rotate different requests in turn, so that no call finds the rows of the call before in a cache.  Device events
around windows of at least --min-window-ms (the iteration count is sized from a pilot window), after warm-up; medians over --windows
windows (at least 5), spread = (max - min) / median.  The times are per CALL as a Python caller sees them on the stream.

Per case, pooled (lookup -> [B, T * D]) and un-pooled (lookup_sequence -> [N, D]), us per call:
  pruned_us    (a) the new call: a pruned module, one launch (pm_embbag_fwd_qrows_pruned / pm_embedding_gather_qrows_pruned), int64 request
  gather_us    (b) the only route of the parent commit: ONE torch gather of the request through the concatenated remap -- the per-lookup
               base offsets are precomputed outside the timed region and added to the indices in it; -1 is redirected to an all-zero
               sentinel row behind every table's last row (baked into the route's copy of the remap) -- into an N-sized int32 temporary,
               then the per-table-format lookup over tables that carry that extra row (int32 request: the remap's type)
  plain_us     (c) context only: the per-table-format lookup of a request with the same number of lookups over the physical tables,
               no remapping at all: what the extra dependent load is charged against
  expectation: (a) is not slower than (b) by more than the larger of the two spreads ("pruned_not_slower_than_gather"); (a) / (c) is
  reported.  routes_agree: (a) and (b) give the same bits (unweighted requests: the sentinel route is not the weighted rule).
--unroll U runs every route under pm_set_tuning(unroll=U) (profiles/pruned_probe_unroll2.json, _unroll4.json: --shapes bench --kinds
unpooled); "plan" names the rows in flight of the launch.
Nothing here is a gate.  One JSON document to stdout and to --out (default profiles/pruned_probe.json)."""
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
from param_amd.indices import tbe_request  # noqa: E402

SHAPES = {"bench": dict(tables=16, rows=10_000_000, dim=128, batch=8192, pooling=20),
          "serving": dict(tables=64, rows=1_000_000, dim=64, batch=256, pooling=10)}


def window_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def take_turns(fns, windows, warmup, min_window_ms):
    """{name: [us per call, one per window]}: the routes take turns, every window at least min_window_ms long"""
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
        self.fn(self.requests[self.k])
        self.k = (self.k + 1) % len(self.requests)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bench,serving")
    ap.add_argument("--kinds", default="pooled,unpooled")
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--min-window-ms", type=float, default=110.0)
    ap.add_argument("--out", default=os.path.join("profiles", "pruned_probe.json"))
    ap.add_argument("--unroll", type=int, default=0, help="pm_set_tuning's unroll for every route (rows in flight; 0: the default)")
    a = ap.parse_args()
    if a.unroll:
        from param_amd import _lib
        _lib.set_tuning(unroll=a.unroll)
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert a.windows >= 5, "medians of at least 5 windows"
    dev = "cuda:0"
    med = statistics.median
    name = torch.cuda.get_device_name(0)
    lines = []
    QB = param_amd.QuantizedBatchedEmbeddingBagMI355

    for shape in a.shapes.split(","):
        s = SHAPES[shape]
        T, R, D, B, L = s["tables"], s["rows"], s["dim"], s["batch"], s["pooling"]
        n = B * L                      # lookups per table
        N = T * n
        bits = [8, 4] * (T // 2)
        # one keep mask (half of the rows) for every table; every table has a copy of the remap of its own in the concatenated array
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        keep = torch.rand(R, device=dev, generator=g) < 0.5
        Rp = int(keep.sum())
        remap = torch.where(keep, torch.cumsum(keep.to(torch.int32), 0, dtype=torch.int32) - 1, torch.full((R,), -1, dtype=torch.int32, device=dev))
        pruned = QB([Rp] * T, D, bits, device=dev, index_remapping=[remap] * T)
        plain = QB([Rp + 1] * T, D, bits, device=dev)          # (b), (c): the physical tables plus a sentinel row of zero bytes each
        assert pruned.pruned and plain.bitwidth is None and pruned.logical_rows == [R] * T
        src = torch.randn(Rp, D, device=dev) * (torch.rand(Rp, 1, device=dev) * 4 + 0.05)
        pruned.quantize_from_(0, src)
        pruned.quantize_from_(1, src)
        del src
        for t in range(T):
            if t >= 2:
                pruned.table(t).copy_(pruned.table(t % 2))
            plain.table(t)[:Rp].copy_(pruned.table(t % 2))     # (the last row stays zero bytes: it dequantises to zeros)
        # route (b)'s copy of the concatenated remap: -1 -> the table's sentinel row; and the per-lookup base offsets of a fixed-pooling request
        remap_b = torch.where(pruned.index_remap < 0, torch.full_like(pruned.index_remap, Rp), pruned.index_remap)
        base = (torch.arange(T, device=dev, dtype=torch.int64) * R).repeat_interleave(n)
        del keep, remap
        for dist, alpha in (("uniform", 0.0), ("zipf", 1.05)):
            reqs = []
            for k in range(a.rotate):
                idx, off = tbe_request([R] * T, B, L, alpha=alpha, device=dev, seed=10 + k)
                cidx, coff = tbe_request([Rp] * T, B, L, alpha=alpha, device=dev, seed=20 + k)
                reqs.append((idx, off, off.to(torch.int32), cidx, coff))
            share = float((pruned.index_remap[reqs[0][0] + base] < 0).float().mean())
            out_a, out_b = torch.empty(B, T * D, device=dev), torch.empty(B, T * D, device=dev)
            seq_a, seq_b = torch.empty(N, D, device=dev), torch.empty(N, D, device=dev)
            tmp, phys = torch.empty(N, dtype=torch.int64, device=dev), torch.empty(N, dtype=torch.int32, device=dev)

            def remap_request(r):
                torch.add(r[0], base, out=tmp)
                torch.index_select(remap_b, 0, tmp, out=phys)

            def pooled_pruned(r):
                pruned.lookup(r[0], r[1], out=out_a, batch=B)

            def pooled_gather(r):
                remap_request(r)
                plain.lookup(phys, r[2], out=out_b, batch=B)

            def pooled_plain(r):
                plain.lookup(r[3], r[4], out=out_b, batch=B)

            def seq_pruned(r):
                pruned.lookup_sequence(r[0], r[1], batch=B, out=seq_a)

            def seq_gather(r):
                remap_request(r)
                plain.lookup_sequence(phys, r[2], batch=B, out=seq_b)

            def seq_plain(r):
                plain.lookup_sequence(r[3], r[4], batch=B, out=seq_b)

            for kind, fa, fb, fc, ra, rb in (("pooled", pooled_pruned, pooled_gather, pooled_plain, out_a, out_b),
                                             ("unpooled", seq_pruned, seq_gather, seq_plain, seq_a, seq_b)):
                if kind not in a.kinds.split(","):
                    continue
                fns = {"pruned": Rotating(fa, reqs), "gather": Rotating(fb, reqs), "plain": Rotating(fc, reqs)}
                t, iters = take_turns(fns, a.windows, a.warmup, a.min_window_ms)
                fa(reqs[0])
                fb(reqs[0])
                torch.cuda.synchronize()
                agree = bool(torch.equal(ra.view(torch.int32), rb.view(torch.int32)))
                ma, mb, mc = med(t["pruned"]), med(t["gather"]), med(t["plain"])
                margin = max(spread(t["pruned"]), spread(t["gather"]))
                plan = (pruned.plan(reqs[0][0], reqs[0][1], batch=B) if kind == "pooled" else pruned.sequence_plan(reqs[0][0], reqs[0][1], batch=B))
                rec = {"exp": "pruned_probe", "shape": shape, "kind": kind, "tables": T, "logical_rows": R, "physical_rows": Rp, "dim": D,
                       "batch": B, "pooling": L, "lookups": N, "pruned_share_of_lookups": round(share, 4), "bits": "8,4 alternating",
                       "out_dtype": "fp32", "indices": dist, "rotate": a.rotate, "windows": a.windows,
                       "pruned_us": round(ma, 2), "gather_us": round(mb, 2), "plain_us": round(mc, 2),
                       "pruned_over_gather": round(ma / mb, 4), "pruned_over_plain": round(ma / mc, 4),
                       "pruned_spread": round(spread(t["pruned"]), 4), "gather_spread": round(spread(t["gather"]), 4),
                       "plain_spread": round(spread(t["plain"]), 4), "pruned_not_slower_than_gather": bool(ma <= mb * (1 + margin)),
                       "routes_agree": agree, "plan": plan, "windows_us": {k: [round(x, 2) for x in v] for k, v in t.items()},
                       "iters": iters, "device": name, "library": os.path.basename(param_amd.LIB_PATH)}
                print(json.dumps(rec), flush=True)
                lines.append(rec)
            del reqs, out_a, out_b, seq_a, seq_b, tmp, phys
        del pruned, plain, remap_b, base
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"exp": "pruned_probe", "records": lines}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
