#!/usr/bin/env python3
"""What ONE launch over tables of per-table format (8- and 4-bit, alternating) costs against the only route there was before it,
measured in ONE process with the routes taking turns window by window.

Shapes:
  bench     16 tables of 10 M x 128, batch 8192, pooling 20 (2.6 M lookups); uniform and Zipf (alpha 1.05) indices; fp32 and fp16 output
  serving   64 tables of 1 M x 64, batch 256, pooling 10 (164 K lookups); uniform and Zipf indices; fp32 output
Tables t = 0, 2, .. are 8-bit, t = 1, 3, .. are 4-bit.  Every route is fed --rotate different requests in turn, so that no call finds the
rows of the call before in a cache.  Device events around windows of at least --min-window-ms (the iteration count is sized from a pilot
window), after warm-up; medians over --windows windows (at least 5), spread = (max - min) / median.  The times are per CALL as a Python
caller sees them on the stream: at the serving shape the host's share of a call is part of every route.

Per case, pooled (lookup -> [B, T * D]) and un-pooled (lookup_sequence -> [N, D]), us per call:
  mixed_us     (a) the new call: one module, one launch (pm_embbag_fwd_qrows_mixed / pm_embedding_gather_qrows_mixed)
  two_copy_us  (b) the only route of the parent commit, unchanged code: two single-format modules over the same bytes (the 8-bit tables in
               one, the 4-bit tables in the other, each with its own pre-split request), two launches, plus the two strided copies that
               put their results into the mixed module's [B, T * D] / [N, D] order
  two_us       (c) the two single-format launches alone, without that copy: what choosing the format at run time is charged against
  expectation: (a) is not slower than (b) by more than the larger of the two spreads ("mixed_not_slower_than_two_copy"); (a) / (c) is
  reported.  routes_agree: (a) and (b) give the same bits.
The lane layout: the same probe under PARAM_AMD_LIB=<a build with -DPM_QMIXED_4BIT_DWORDS=2> (csrc/Makefile) measures the pooled kernel with
two dwords per lane for both formats (--kinds pooled; --out profiles/qmixed_probe_lane_dwords2.json); "library" names the build.
Nothing here is a gate.  One JSON document to stdout and to --out (default profiles/qmixed_probe.json)."""
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

ODT = {"fp32": torch.float32, "fp16": torch.float16}
SHAPES = {"bench": dict(tables=16, rows=10_000_000, dim=128, batch=8192, pooling=20, outs=("fp32", "fp16")),
          "serving": dict(tables=64, rows=1_000_000, dim=64, batch=256, pooling=10, outs=("fp32",))}


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


def set_out(m, odt):
    """the module's output dtype for the case (a plain attribute the constructor sets and the calls read)"""
    m.output_dtype = odt
    m._out16 = None if odt == torch.float32 else odt


def split_request(idx, off, T, B, L, parity):
    """the part of a fixed-pooling request that belongs to the tables t = parity, parity + 2, ..: (indices, offsets [T / 2 * B + 1])"""
    n = B * L
    part = idx.view(T, n)[parity::2].contiguous().view(-1)
    return part, torch.arange(T // 2 * B + 1, dtype=off.dtype, device=off.device) * L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bench,serving")
    ap.add_argument("--kinds", default="pooled,unpooled")
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--min-window-ms", type=float, default=110.0)
    ap.add_argument("--out", default=os.path.join("profiles", "qmixed_probe.json"))
    a = ap.parse_args()
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
        assert T % 2 == 0
        n = B * L                      # lookups per table
        N = T * n
        bits = [8, 4] * (T // 2)
        mixed = QB([R] * T, D, bits, device=dev)
        m8, m4 = QB([R] * (T // 2), D, 8, device=dev), QB([R] * (T // 2), D, 4, device=dev)
        assert mixed.bitwidth is None and (m8.bitwidth, m4.bitwidth) == (8, 4)
        # one fp32 source, quantised once per format by the existing kernel; every table of a format holds those bytes
        src = torch.randn(R, D, device=dev) * (torch.rand(R, 1, device=dev) * 4 + 0.05)
        mixed.quantize_from_(0, src)
        mixed.quantize_from_(1, src)
        del src
        for t in range(2, T):
            mixed.table(t).copy_(mixed.table(t % 2))
        for k in range(T // 2):        # the same bytes in the two single-format modules
            m8.table(k).copy_(mixed.table(0))
            m4.table(k).copy_(mixed.table(1))
        for dist, alpha in (("uniform", 0.0), ("zipf", 1.05)):
            whole = [tbe_request([R] * T, B, L, alpha=alpha, device=dev, seed=10 + k) for k in range(a.rotate)]
            reqs = [(idx, off, split_request(idx, off, T, B, L, 0), split_request(idx, off, T, B, L, 1)) for idx, off in whole]
            for o in s["outs"]:
                odt = ODT[o]
                for m in (mixed, m8, m4):
                    set_out(m, odt)
                # pooled: [B, T * D]; un-pooled: [N, D] (table t owns the positions [t * n, (t + 1) * n))
                out_a, out_b = torch.empty(B, T * D, dtype=odt, device=dev), torch.empty(B, T * D, dtype=odt, device=dev)
                o8, o4 = torch.empty(B, T // 2 * D, dtype=odt, device=dev), torch.empty(B, T // 2 * D, dtype=odt, device=dev)
                seq_a, seq_b = torch.empty(N, D, dtype=odt, device=dev), torch.empty(N, D, dtype=odt, device=dev)
                s8, s4 = torch.empty(N // 2, D, dtype=odt, device=dev), torch.empty(N // 2, D, dtype=odt, device=dev)
                pooled_b, seq_bv = out_b.view(B, T // 2, 2, D), seq_b.view(T // 2, 2, n, D)

                def pooled_mixed(r):
                    mixed.lookup(r[0], r[1], out=out_a, batch=B)

                def pooled_two(r):
                    m8.lookup(r[2][0], r[2][1], out=o8, batch=B)
                    m4.lookup(r[3][0], r[3][1], out=o4, batch=B)

                def pooled_two_copy(r):
                    pooled_two(r)
                    pooled_b[:, :, 0].copy_(o8.view(B, T // 2, D))
                    pooled_b[:, :, 1].copy_(o4.view(B, T // 2, D))

                def seq_mixed(r):
                    mixed.lookup_sequence(r[0], r[1], batch=B, out=seq_a)

                def seq_two(r):
                    m8.lookup_sequence(r[2][0], r[2][1], batch=B, out=s8)
                    m4.lookup_sequence(r[3][0], r[3][1], batch=B, out=s4)

                def seq_two_copy(r):
                    seq_two(r)
                    seq_bv[:, 0].copy_(s8.view(T // 2, n, D))
                    seq_bv[:, 1].copy_(s4.view(T // 2, n, D))

                for kind, fa, fb, fc, ra, rb in (("pooled", pooled_mixed, pooled_two_copy, pooled_two, out_a, out_b),
                                                 ("unpooled", seq_mixed, seq_two_copy, seq_two, seq_a, seq_b)):
                    if kind not in a.kinds.split(","):
                        continue
                    fns = {"mixed": Rotating(fa, reqs), "two_copy": Rotating(fb, reqs), "two": Rotating(fc, reqs)}
                    t, iters = take_turns(fns, a.windows, a.warmup, a.min_window_ms)
                    fa(reqs[0])
                    fb(reqs[0])
                    torch.cuda.synchronize()
                    agree = bool(torch.equal(ra.view(torch.int32 if odt == torch.float32 else torch.int16),
                                             rb.view(torch.int32 if odt == torch.float32 else torch.int16)))
                    ma, mb, mc = med(t["mixed"]), med(t["two_copy"]), med(t["two"])
                    margin = max(spread(t["mixed"]), spread(t["two_copy"]))
                    plan = (mixed.plan(reqs[0][0], reqs[0][1], batch=B) if kind == "pooled" else mixed.sequence_plan(reqs[0][0], reqs[0][1], batch=B))
                    rec = {"exp": "qmixed_probe", "shape": shape, "kind": kind, "tables": T, "rows": R, "dim": D, "batch": B, "pooling": L,
                           "lookups": N, "bits": "8,4 alternating", "out_dtype": o, "indices": dist, "rotate": a.rotate, "windows": a.windows,
                           "mixed_us": round(ma, 2), "two_copy_us": round(mb, 2), "two_us": round(mc, 2),
                           "mixed_over_two_copy": round(ma / mb, 4), "mixed_over_two": round(ma / mc, 4),
                           "mixed_spread": round(spread(t["mixed"]), 4), "two_copy_spread": round(spread(t["two_copy"]), 4),
                           "two_spread": round(spread(t["two"]), 4), "mixed_not_slower_than_two_copy": bool(ma <= mb * (1 + margin)),
                           "routes_agree": agree, "plan": plan, "windows_us": {k: [round(x, 2) for x in v] for k, v in t.items()},
                           "iters": iters, "device": name, "library": os.path.basename(param_amd.LIB_PATH)}
                    print(json.dumps(rec), flush=True)
                    lines.append(rec)
                del out_a, out_b, o8, o4, seq_a, seq_b, s8, s4, pooled_b, seq_bv
            del reqs, whole
        del mixed, m8, m4
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"exp": "qmixed_probe", "records": lines}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
