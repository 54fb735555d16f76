#!/usr/bin/env python3
"""The rounds of the forward's headline launch inside an XCD, measured: a timeline of one launch's workgroups, and the split last round
in a same-process A/B with the switch taking turns.

Needs an EXPERIMENT build (the switches are read once per process in the product; the experiment build reads them on every call and
stamps every workgroup of embbag_fwd_kernel with its start, end, XCD and table):
    make -C param_amd/csrc EXTRA=-DPM_EXPERIMENTS OBJDIR=$PWD/build/csrc_exp OUT=$PWD/build/libparam_amd_exp.so
    PARAM_AMD_LIB=build/libparam_amd_exp.so python tools/fwd_round_timeline.py --out profiles/fwd_round_timeline.json

Shape: the benchmark's -- T tables of 10 M x 128, batch 8192, pooling 20 (fp32: T = 48, [T, B, D]).  --rotate requests take turns so that
no call finds the rows of the call before in a cache.

timeline (one launch per setting and distribution, after warm-up), per XCD then averaged over the 8:
  wgs, resident_max     workgroups the XCD ran; most resident at one time (start <= t < end)
  tile_life_us          median life of a workgroup that pools a whole tile
  tables_resident       fractions of the launch's time with workgroups of 1, 2, 3+ tables resident
  drain_us              from the last moment the XCD had resident_max * 0.9 workgroups resident to its last workgroup's end
  span_us               first start to last end
A/B (device events around windows of at least --min-window-ms, medians of --windows windows, spread = (max - min) / median):
  us per call of every setting, and its gain over `off` -- to be read against the spreads.  Nothing here is a gate."""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import param_amd  # noqa: E402
from param_amd import _lib  # noqa: E402
from param_amd.indices import tbe_request  # noqa: E402

SWITCHES = ("PARAM_AMD_FWD_DRAIN_SPLIT", "PARAM_AMD_FWD_ROUND_WGS")
SETTINGS = {"off": (0,), "split4": (4,), "split2": (2,)}
SLOTS, WGS = 8, 1 << 15
XCDS = 8


def use(setting, forced_r):
    for k, v in zip(SWITCHES, SETTINGS[setting] + (forced_r,)):
        os.environ[k] = str(v)


def window_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def timeline(L_, call):
    """per-XCD figures of one launch from the experiment build's stamps: slot 0 start, 1 end (100 MHz ticks), 2 = xcd << 32 | table"""
    for _ in range(3):
        call()
    assert L_.pm_experiment_trace_fwd(None, 0, 1) == 0
    call()
    buf = np.zeros(WGS * SLOTS, dtype=np.uint64)
    assert L_.pm_experiment_trace_fwd(buf.ctypes.data, buf.size, 0) == 0
    tr = buf.reshape(WGS, SLOTS)
    live = np.nonzero((tr[:, 0] > 0) & (tr[:, 1] > 0))[0]
    start, end = tr[live, 0].astype(np.int64), tr[live, 1].astype(np.int64)
    xcd, table = (tr[live, 2] >> np.uint64(32)).astype(np.int64), (tr[live, 2] & np.uint64(0xffffffff)).astype(np.int64)
    t0 = start.min()
    start, end = (start - t0) * 0.01, (end - t0) * 0.01            # us
    per = []
    for x in sorted(set(xcd.tolist())):
        s, e, tb, bid = start[xcd == x], end[xcd == x], table[xcd == x], live[xcd == x]
        ts = np.unique(np.concatenate([s, e]))                     # the residency changes only at these times
        mid = (ts[:-1] + ts[1:]) / 2
        dur = ts[1:] - ts[:-1]
        res = np.array([int(((s <= t) & (t < e)).sum()) for t in mid])
        ntab = np.array([len(set(tb[(s <= t) & (t < e)].tolist())) for t in mid])
        rmax = int(res.max())
        full = np.nonzero(res >= 0.9 * rmax)[0]
        life = e - s
        # a whole tile's life: the blocks of the first half of the XCD's dispatch order (none of them split)
        first_half = bid < np.median(bid)
        per.append({"xcd": int(x), "wgs": int(s.size), "tables": sorted(set(tb.tolist())), "blocks_on_their_xcd": float((bid % XCDS == x).mean()),
                    "resident_max": rmax, "tile_life_us": round(float(np.median(life[first_half])), 2),
                    "span_us": round(float(e.max() - s.min()), 2), "drain_us": round(float(e.max() - ts[full[-1] + 1]), 2),
                    "tables_resident": {k: round(float(dur[sel].sum() / dur.sum()), 4)
                                        for k, sel in (("1", ntab == 1), ("2", ntab == 2), ("3+", ntab >= 3))}})
    avg = lambda f: round(float(np.mean([f(p) for p in per])), 3)                              # noqa: E731
    return {"launch_wgs": int(live.size), "span_us": round(float(end.max()), 2),
            "mean": {"resident_max": avg(lambda p: p["resident_max"]), "tile_life_us": avg(lambda p: p["tile_life_us"]),
                     "drain_us": avg(lambda p: p["drain_us"]), "span_us": avg(lambda p: p["span_us"]),
                     "one_table_resident": avg(lambda p: p["tables_resident"]["1"]),
                     "two_tables_resident": avg(lambda p: p["tables_resident"]["2"]),
                     "blocks_on_their_xcd": avg(lambda p: p["blocks_on_their_xcd"])},
            "per_xcd": per}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=48)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pooling", type=int, default=20)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--layout", default="tbd")
    ap.add_argument("--alphas", default="1.05,0")
    ap.add_argument("--settings", default="off,split4,split2")
    ap.add_argument("--timeline-settings", default="off,split4")
    ap.add_argument("--forced-r", type=int, default=0, help="resident workgroups per XCD instead of the device's answer")
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--min-window-ms", type=float, default=110.0)
    ap.add_argument("--out", default=os.path.join("profiles", "fwd_round_timeline.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert a.windows >= 5, "medians of at least 5 windows"
    L_ = _lib.load()
    assert hasattr(L_, "pm_experiment_trace_fwd"), "run with PARAM_AMD_LIB=build/libparam_amd_exp.so (an experiment build)"
    L_.pm_experiment_trace_fwd.restype = ctypes.c_int
    L_.pm_experiment_trace_fwd.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    dev = "cuda:0"
    T, B, L, D = a.tables, a.batch, a.pooling, a.dim
    rows = [a.rows] * T
    dt = {"fp32": torch.float32, "bf16": torch.bfloat16}[a.dtype]
    m = param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=dt, device=dev, layout=a.layout, init="normal", seed=1, fused_update=False)
    out = torch.empty((T, B, D) if a.layout == "tbd" else (B, T * D), dtype=torch.float32, device=dev)
    settings = a.settings.split(",")
    records = []
    for alpha in map(float, a.alphas.split(",")):
        reqs = [tbe_request(rows, B, L, alpha=alpha, device=dev, seed=10 + k) for k in range(a.rotate)]
        state = {"k": 0}

        def call():
            idx, off = reqs[state["k"]]
            state["k"] = (state["k"] + 1) % len(reqs)
            m.lookup(idx, off, out=out, batch=B)

        rec = {"exp": "fwd_round_timeline", "tables": T, "rows": a.rows, "dim": D, "batch": B, "pooling": L, "dtype": a.dtype,
               "layout": a.layout, "alpha": alpha, "forced_r": a.forced_r, "rotate": a.rotate, "windows": a.windows,
               "device": torch.cuda.get_device_name(0)}
        # same bytes under every setting
        use("off", a.forced_r)
        state["k"] = 0
        call()
        want = out.clone()
        same = {}
        for s in settings:
            use(s, a.forced_r)
            state["k"] = 0
            out.fill_(float("nan"))
            call()
            same[s] = bool(torch.equal(out, want))
        rec["same_bytes_as_off"] = same
        rec["timeline"] = {}
        for s in a.timeline_settings.split(",") if a.timeline_settings else []:
            use(s, a.forced_r)
            rec["timeline"][s] = timeline(L_, call)
        iters, res = {}, {s: [] for s in settings}
        for s in settings:
            use(s, a.forced_r)
            for _ in range(a.warmup):
                call()
            torch.cuda.synchronize()
            iters[s] = max(10, math.ceil(a.min_window_ms * 1e3 / window_us(call, 10)))
        for _ in range(a.windows):
            for s in settings:
                use(s, a.forced_r)
                res[s].append(window_us(call, iters[s]))
        med = {s: statistics.median(v) for s, v in res.items()}
        rec["us"] = {s: round(med[s], 2) for s in settings}
        rec["spread"] = {s: round(spread(res[s]), 4) for s in settings}
        rec["gain_over_off"] = {s: round(1 - med[s] / med["off"], 4) for s in settings if "off" in med}
        rec["windows_us"] = {s: [round(x, 2) for x in v] for s, v in res.items()}
        rec["iters"] = iters
        print(json.dumps({k: v for k, v in rec.items() if k != "timeline"}), flush=True)
        for s, tl in rec["timeline"].items():
            print(json.dumps({"alpha": alpha, "timeline": s, "launch_wgs": tl["launch_wgs"], "span_us": tl["span_us"], **tl["mean"]}), flush=True)
        records.append(rec)
        del reqs
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"exp": "fwd_round_timeline", "records": records}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
