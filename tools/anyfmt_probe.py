#!/usr/bin/env python3
"""What ONE launch over tables of mixed format (fp16, FP8 e4m3 with a table exponent, int8, int4, cycling) costs against the only route
there was before it, measured in ONE process with the routes taking turns window by window.

Shapes:
  bench     16 tables of 10 M x 128, batch 8192, pooling 20 (2.6 M lookups); uniform and Zipf (alpha 1.05) indices; fp32 and fp16 output
  serving   64 tables of 1 M x 64, batch 256, pooling 10 (164 K lookups); uniform and Zipf indices; fp32 output
Table t has format (fp16, fp8_e4m3, int8, int4)[t % 4].  Every route is fed --rotate different requests in turn, so that no call finds
the rows of the call before in a cache.  Device events around windows of at least --min-window-ms (the iteration count is sized from a
pilot window), after warm-up; medians over --windows windows (at least 5), spread = (max - min) / median.  The times are per CALL as a
Python caller sees them on the stream: at the serving shape the host's share of a call is part of every route.

Per case, pooled (lookup -> [B, T * D]) and un-pooled (lookup_sequence -> [N, D]), us per call:
  mixed_us       (a) the new call: one module, one launch (pm_embbag_fwd_anyfmt / pm_embedding_gather_anyfmt)
  three_copy_us  (b) the only route of the parent commit, unchanged code: one existing module per format family over the same bytes (the
                 fp16 tables in a BatchedEmbeddingBagMI355, the FP8 tables in a Float8BatchedEmbeddingBagMI355 with scale="table", the
                 int8 / int4 tables in a QuantizedBatchedEmbeddingBagMI355 of per-table format), each with its own pre-split request,
                 three launches, plus the three strided copies that put their results into the mixed module's [B, T * D] / [N, D] order
  three_us       (c) the three launches alone, without the copies: what the run-time branch and registers sized for the widest format
                 are charged against
  expectation: (a) is not slower than (b) by more than the larger of the two spreads ("mixed_not_slower_than_three_copy"); (a) / (c)
  is reported.  routes_agree: (a) and (b) give the same bits.
Per family (--families, on by default): the family's tables alone through a mixed-format module ("<family>_anyfmt_us") and through the
family's own module ("<family>_own_us"), same bytes, same request: which format loses against its own kernel, if any.
Nothing here is a gate.  One JSON document to stdout and to --out (default profiles/anyfmt_probe.json)."""
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
          "serving": dict(tables=64, rows=1_000_000, dim=64, batch=256, pooling=10, outs=("fp32",)),
          "tiny": dict(tables=8, rows=1000, dim=64, batch=16, pooling=4, outs=("fp32", "fp16"))}      # a rehearsal of the script, not a measurement
CYCLE = ("fp16", "fp8_e4m3", "int8", "int4")
FAMILIES = {"float": (0, 1), "fp8": (1, 2), "quant": (2, 4)}      # positions of the cycle a family's module holds


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


def split_request(idx, off, T, B, L, lo, hi):
    """the part of a fixed-pooling request that belongs to the tables whose position in the cycle of four is in [lo, hi):
    (indices, offsets [T / 4 * (hi - lo) * B + 1])"""
    n = B * L
    part = idx.view(T // 4, 4, n)[:, lo:hi].contiguous().view(-1)
    return part, torch.arange(T // 4 * (hi - lo) * B + 1, dtype=off.dtype, device=off.device) * L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bench,serving")
    ap.add_argument("--kinds", default="pooled,unpooled")
    ap.add_argument("--families", type=int, default=1)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--min-window-ms", type=float, default=110.0)
    ap.add_argument("--out", default=os.path.join("profiles", "anyfmt_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert a.windows >= 5, "medians of at least 5 windows"
    dev = "cuda:0"
    med = statistics.median
    name = torch.cuda.get_device_name(0)
    lines = []
    MB, FB = param_amd.MixedBatchedEmbeddingBagMI355, param_amd.BatchedEmbeddingBagMI355
    QB, F8B = param_amd.QuantizedBatchedEmbeddingBagMI355, param_amd.Float8BatchedEmbeddingBagMI355

    for shape in a.shapes.split(","):
        s = SHAPES[shape]
        T, R, D, B, L = s["tables"], s["rows"], s["dim"], s["batch"], s["pooling"]
        assert T % 4 == 0
        Q = T // 4                     # tables per position of the cycle
        n = B * L                      # lookups per table
        N = T * n
        mixed = MB([R] * T, D, [CYCLE[t % 4] for t in range(T)], device=dev)
        # one source, quantised once per format by that format's own quantiser; every table of a format holds those bytes.  The values
        # are those of the benchmark's uniform init (|x| <= 1 / sqrt(rows)): without its table exponent the FP8 table would be all zeros
        src = (torch.rand(R, D, device=dev) * 2 - 1) * (1.0 / math.sqrt(R))
        for t in range(4):
            mixed.quantize_from_(t, src)
        del src
        for t in range(4, T):
            mixed._bytes(t).copy_(mixed._bytes(t % 4))
        mixed.table_exponents.copy_(mixed.table_exponents[:4].repeat(Q))
        e8 = int(mixed.table_exponents[1])
        own = {"float": FB([R] * Q, D, dtype=torch.float16, device=dev, init=None, fused_update=False),
               "fp8": F8B([R] * Q, D, torch.float8_e4m3fn, device=dev, scale="table"),
               "quant": QB([R] * (2 * Q), D, [8, 4] * Q, device=dev)}
        for k in range(Q):             # the same bytes in the three family modules
            own["float"].table(k).copy_(mixed.table(0))
            own["fp8"].copy_from_(k, mixed.table(1), exponents=e8)
            own["quant"].table(2 * k).copy_(mixed.table(2))
            own["quant"].table(2 * k + 1).copy_(mixed.table(3))
        alone = {}
        if a.families:                 # a family's tables alone in a mixed-format module
            for fam in FAMILIES:
                alone[fam] = MB.from_modules([own[fam]])
        for dist, alpha in (("uniform", 0.0), ("zipf", 1.05)):
            whole = [tbe_request([R] * T, B, L, alpha=alpha, device=dev, seed=10 + k) for k in range(a.rotate)]
            reqs = [dict(all=(idx, off), **{fam: split_request(idx, off, T, B, L, lo, hi) for fam, (lo, hi) in FAMILIES.items()}) for idx, off in whole]
            for o in s["outs"]:
                odt = ODT[o]
                for m in [mixed] + list(own.values()) + list(alone.values()):
                    set_out(m, odt)
                width = {fam: (hi - lo) * Q for fam, (lo, hi) in FAMILIES.items()}      # tables of a family
                # pooled: [B, T * D]; un-pooled: [N, D] (table t owns the positions [t * n, (t + 1) * n))
                out_a, out_b = torch.empty(B, T * D, dtype=odt, device=dev), torch.empty(B, T * D, dtype=odt, device=dev)
                seq_a, seq_b = torch.empty(N, D, dtype=odt, device=dev), torch.empty(N, D, dtype=odt, device=dev)
                po = {fam: torch.empty(B, w * D, dtype=odt, device=dev) for fam, w in width.items()}
                so = {fam: torch.empty(w * n, D, dtype=odt, device=dev) for fam, w in width.items()}
                po2 = {fam: torch.empty_like(x) for fam, x in po.items()}
                so2 = {fam: torch.empty_like(x) for fam, x in so.items()}
                pooled_b, seq_bv = out_b.view(B, Q, 4, D), seq_b.view(Q, 4, n, D)

                def pooled_mixed(r):
                    mixed.lookup(r["all"][0], r["all"][1], out=out_a, batch=B)

                def pooled_three(r):
                    for fam, m in own.items():
                        m.lookup(r[fam][0], r[fam][1], out=po[fam], batch=B)

                def pooled_three_copy(r):
                    pooled_three(r)
                    for fam, (lo, hi) in FAMILIES.items():
                        pooled_b[:, :, lo:hi].copy_(po[fam].view(B, Q, hi - lo, D))

                def seq_mixed(r):
                    mixed.lookup_sequence(r["all"][0], r["all"][1], batch=B, out=seq_a)

                def seq_three(r):
                    for fam, m in own.items():
                        m.lookup_sequence(r[fam][0], r[fam][1], batch=B, out=so[fam])

                def seq_three_copy(r):
                    seq_three(r)
                    for fam, (lo, hi) in FAMILIES.items():
                        seq_bv[:, lo:hi].copy_(so[fam].view(Q, hi - lo, n, D))

                def family_fn(m, fam, pooled, outs):
                    if pooled:
                        return lambda r: m.lookup(r[fam][0], r[fam][1], out=outs[fam], batch=B)
                    return lambda r: m.lookup_sequence(r[fam][0], r[fam][1], batch=B, out=outs[fam])

                for kind, fa, fb, fc, ra, rb in (("pooled", pooled_mixed, pooled_three_copy, pooled_three, out_a, out_b),
                                                 ("unpooled", seq_mixed, seq_three_copy, seq_three, seq_a, seq_b)):
                    if kind not in a.kinds.split(","):
                        continue
                    fns = {"mixed": Rotating(fa, reqs), "three_copy": Rotating(fb, reqs), "three": Rotating(fc, reqs)}
                    for fam in alone:
                        fns[fam + "_anyfmt"] = Rotating(family_fn(alone[fam], fam, kind == "pooled", po2 if kind == "pooled" else so2), reqs)
                        fns[fam + "_own"] = Rotating(family_fn(own[fam], fam, kind == "pooled", po if kind == "pooled" else so), reqs)
                    t, iters = take_turns(fns, a.windows, a.warmup, a.min_window_ms)
                    fa(reqs[0])
                    fb(reqs[0])
                    for fam in alone:
                        fns[fam + "_anyfmt"].fn(reqs[0])
                        fns[fam + "_own"].fn(reqs[0])
                    torch.cuda.synchronize()
                    raw = torch.int32 if odt == torch.float32 else torch.int16
                    agree = bool(torch.equal(ra.view(raw), rb.view(raw)))
                    fam_agree = {fam: bool(torch.equal((po2 if kind == "pooled" else so2)[fam].view(raw), (po if kind == "pooled" else so)[fam].view(raw)))
                                 for fam in alone}
                    ma, mb, mc = med(t["mixed"]), med(t["three_copy"]), med(t["three"])
                    margin = max(spread(t["mixed"]), spread(t["three_copy"]))
                    plan = (mixed.plan(reqs[0]["all"][0], reqs[0]["all"][1], batch=B) if kind == "pooled"
                            else mixed.sequence_plan(reqs[0]["all"][0], reqs[0]["all"][1], batch=B))
                    rec = {"exp": "anyfmt_probe", "shape": shape, "kind": kind, "tables": T, "rows": R, "dim": D, "batch": B, "pooling": L,
                           "lookups": N, "formats": ",".join(CYCLE) + " cycling", "fp8_table_exponent": e8, "out_dtype": o, "indices": dist,
                           "rotate": a.rotate, "windows": a.windows,
                           "mixed_us": round(ma, 2), "three_copy_us": round(mb, 2), "three_us": round(mc, 2),
                           "mixed_over_three_copy": round(ma / mb, 4), "mixed_over_three": round(ma / mc, 4),
                           "mixed_spread": round(spread(t["mixed"]), 4), "three_copy_spread": round(spread(t["three_copy"]), 4),
                           "three_spread": round(spread(t["three"]), 4), "mixed_not_slower_than_three_copy": bool(ma <= mb * (1 + margin)),
                           "routes_agree": agree,
                           "families": {fam: {"anyfmt_us": round(med(t[fam + "_anyfmt"]), 2), "own_us": round(med(t[fam + "_own"]), 2),
                                              "anyfmt_over_own": round(med(t[fam + "_anyfmt"]) / med(t[fam + "_own"]), 4),
                                              "anyfmt_spread": round(spread(t[fam + "_anyfmt"]), 4), "own_spread": round(spread(t[fam + "_own"]), 4),
                                              "routes_agree": fam_agree[fam]} for fam in alone},
                           "plan": plan, "windows_us": {k: [round(x, 2) for x in v] for k, v in t.items()},
                           "iters": iters, "device": name, "library": os.path.basename(param_amd.LIB_PATH)}
                    print(json.dumps(rec), flush=True)
                    lines.append(rec)
                del out_a, out_b, seq_a, seq_b, po, so, po2, so2, pooled_b, seq_bv
            del reqs, whole
        del mixed, own, alone
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"exp": "anyfmt_probe", "records": lines}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
