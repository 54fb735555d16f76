#!/usr/bin/env python3
"""What the power-of-two scales of SCALED FP8 TABLES cost, measured in ONE process with the routes taking turns window by window
(tools/f8_probe.py's pattern and helpers).

Shape: 16 tables of 10 M x 128 e4m3, batch 8192, pooling 20 -> 2.6 M lookups; uniform and Zipf (alpha 1.05) indices; every route is fed
--rotate different requests in turn; device events around windows of at least 110 ms; medians over --windows windows (at least 5),
spread = (max - min) / median.

Pooled routes, us per call, fp32 and fp16 output (``_f32`` / ``_f16``):
  f8          Float8BatchedEmbeddingBagMI355.lookup, scale=None   (pm_embbag_fwd_f8: the unchanged kernel)
  f8s_table   scale="table"  (pm_embbag_fwd_f8_scaled, one exponent per table: no more memory traffic than f8)
  f8s_row     scale="row"    (one exponent byte gathered per lookup, from another line)
  q8_f32      QuantizedBatchedEmbeddingBagMI355.lookup over 8-bit row-quantised tables -- unchanged code: a yardstick
Un-pooled routes (``lookup_sequence``, fp32 output [N, D]): f8_seq / f8s_table_seq / f8s_row_seq; copy: a device copy of the output's size.
The three FP8 modules hold the same random finite codes; row exponents are drawn from [-30, 10], the tables' exponent is -10.
Quantiser (one table, fp32 source [rows, 128]): ``quantize_from_`` of a scale="row" and of a scale="table" module against a device copy
of the source's size.
"expectation": f8s_table within the run's spread of f8 (it adds a multiply per element and no traffic) -- reported, never a gate; what
the row exponents cost is reported next to q8_f32 and fixed nowhere.
One JSON document to stdout and to --out (default profiles/f8s_probe.json)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import param_amd  # noqa: E402
from f8_probe import Rotating, spread, summarise, take_turns  # noqa: E402
from param_amd import quant  # noqa: E402
from param_amd.indices import tbe_request  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=16)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pooling", type=int, default=20)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--min-window-ms", type=float, default=110.0)
    ap.add_argument("--out", default=os.path.join("profiles", "f8s_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert a.windows >= 5, "medians of at least 5 windows"
    dev = "cuda:0"
    T, B, L, D = a.tables, a.batch, a.pooling, a.dim
    rows = [a.rows] * T
    N = T * B * L
    f32, f16 = torch.float32, torch.float16

    def f8_module(scale, odt, like=None):
        m = param_amd.Float8BatchedEmbeddingBagMI355(rows, D, "e4m3", device=dev, output_dtype=odt, scale=scale)
        if like is not None:                      # the fp16-output twin reads the fp32-output module's buffers
            m.weights = like.weights
            if scale == "table":
                m.table_exponents = like.table_exponents
            elif scale == "row":
                m.row_exponents = like.row_exponents
        return m

    mods = {(s, f32): f8_module(s, f32) for s in (None, "table", "row")}
    for t in range(T):
        c = torch.randint(0, 256, (rows[t], D), dtype=torch.uint8, device=dev)
        c[(c & 0x7f) == 0x7f] = 0x3f
        for s in (None, "table", "row"):
            mods[(s, f32)].copy_from_(t, c)
        del c
    mods[("table", f32)].table_exponents.fill_(-10)
    mods[("row", f32)].row_exponents.copy_(torch.randint(-30, 11, (sum(rows),), dtype=torch.int8, device=dev))
    for s in (None, "table", "row"):
        mods[(s, f16)] = f8_module(s, f16, like=mods[(s, f32)])
    q8 = param_amd.QuantizedBatchedEmbeddingBagMI355(rows, D, 8, device=dev)
    for t in range(T):
        q8.quantize_from_(t, torch.randn(rows[t], D, device=dev))
    out32 = torch.empty(B, T * D, dtype=f32, device=dev)
    out16 = torch.empty(B, T * D, dtype=f16, device=dev)
    seq = torch.empty(N, D, dtype=f32, device=dev)
    seq2 = torch.empty_like(seq)

    def pooled(module, out):
        return lambda idx, off: module.lookup(idx, off, out=out, batch=B)

    def unpooled(module):
        return lambda idx, off: module.lookup_sequence(idx, off, batch=B, out=seq)

    names = {None: "f8", "table": "f8s_table", "row": "f8s_row"}
    # name: (call, bytes read per lookup, bytes per output element)
    pooled_routes, seq_routes = {}, {}
    for s, name in names.items():
        extra = 1 if s == "row" else 0
        pooled_routes[name + "_f32"] = (pooled(mods[(s, f32)], out32), D + extra, 4)
        pooled_routes[name + "_f16"] = (pooled(mods[(s, f16)], out16), D + extra, 2)
        seq_routes[name + "_seq"] = (unpooled(mods[(s, f32)]), D + extra)
    pooled_routes["q8_f32"] = (pooled(q8, out32), quant.host_row_bytes(D, 8), 4)
    seq_routes["copy"] = (lambda idx, off: seq2.copy_(seq), None)

    lines = []
    for dist, alpha in (("uniform", 0.0), ("zipf", 1.05)):
        reqs = [tbe_request(rows, B, L, alpha=alpha, device=dev, seed=10 + k) for k in range(a.rotate)]
        fns = {name: Rotating(v[0], reqs) for name, v in {**pooled_routes, **seq_routes}.items()}
        t, iters = take_turns(fns, a.windows, a.warmup, a.min_window_ms)
        idx, off = reqs[0]
        rec = {"exp": "f8s_probe", "tables": T, "rows": a.rows, "dim": D, "batch": B, "pooling": L, "lookups": N, "indices": dist,
               "rotate": a.rotate, "windows": a.windows, "lib": os.path.basename(param_amd.LIB_PATH),
               "plan": {names[s] + "_f32": mods[(s, f32)].plan(idx, off, batch=B) for s in names}, "pooled": {}, "unpooled": {}}
        for name, (_, row_b, e_out) in pooled_routes.items():
            rec["pooled"][name] = summarise(t[name], iters[name], N * (row_b + 8) + T * B * (D * e_out + 8), N)
        for name, (_, row_b) in seq_routes.items():
            nbytes = 2 * N * D * 4 if row_b is None else N * (row_b + 8) + N * D * 4
            rec["unpooled"][name] = summarise(t[name], iters[name], nbytes, N)
        p, u = rec["pooled"], rec["unpooled"]
        rec["ratio_to_f8"] = {k + o: round(p[k + o]["us"] / p["f8" + o]["us"], 4) for k in ("f8s_table", "f8s_row") for o in ("_f32", "_f16")}
        rec["ratio_to_f8"].update({k + "_seq": round(u[k + "_seq"]["us"] / u["f8_seq"]["us"], 4) for k in ("f8s_table", "f8s_row")})
        rec["f8s_row_f32_to_q8_f32"] = round(p["f8s_row_f32"]["us"] / p["q8_f32"]["us"], 4)
        noise = {o: max(p["f8" + o]["spread"], p["f8s_table" + o]["spread"]) for o in ("_f32", "_f16")}
        rec["expectation"] = {"f8s_table" + o + "_within_spread_of_f8": bool(abs(p["f8s_table" + o]["us"] / p["f8" + o]["us"] - 1) <= noise[o])
                              for o in ("_f32", "_f16")}
        rec["expectation"]["spread_used"] = noise
        rec["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del reqs, fns

    # the quantiser: one table's fp32 source, against a device copy of the source's size
    del q8, seq, seq2
    torch.cuda.empty_cache()
    src = torch.empty(a.rows, D, dtype=f32, device=dev).uniform_(-1.0 / a.rows ** 0.5, 1.0 / a.rows ** 0.5)
    dst = torch.empty_like(src)
    qfns = {"quantize_row": lambda: mods[("row", f32)].quantize_from_(0, src), "quantize_table": lambda: mods[("table", f32)].quantize_from_(0, src),
            "copy_of_source": lambda: dst.copy_(src)}
    t, iters = take_turns(qfns, a.windows, 2, a.min_window_ms)
    rec = {"exp": "f8s_probe_quantiser", "rows": a.rows, "dim": D, "source": "fp32", "source_bytes": src.numel() * 4, "routes": {}}
    for name in qfns:
        us = statistics.median(t[name])
        rec["routes"][name] = {"us": round(us, 1), "spread": round(spread(t[name]), 4), "iters": iters[name], "windows_us": [round(x, 1) for x in t[name]]}
    rec["ratio_to_copy"] = {k: round(rec["routes"][k]["us"] / rec["routes"]["copy_of_source"]["us"], 3) for k in ("quantize_row", "quantize_table")}
    print(json.dumps(rec), flush=True)
    lines.append(rec)

    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"exp": "f8s_probe", "records": lines}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
