#!/usr/bin/env python3
"""Summarise rocprofv3 output directories of `bench.py --only-headline --full` runs for the forward's headline kernel.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python bench.py --gpus 1 --only-headline --full ...
    rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --output-format csv -d DIR -o run -- python bench.py ...      (a run of its own)
    python tools/fwd_headline_profile.py LABEL=DIR [LABEL=DIR ...] > profiles/....json

Per directory: from *kernel_stats.csv the calls and average / min / max us of every embbag_fwd kernel; from *counter_collection.csv the
counters summed over the XCDs' channels per dispatch of the kernel with the most dispatches (the timed launch), median over its
dispatches, and hit rate = TCC_HIT_sum / (TCC_HIT_sum + TCC_MISS_sum)."""
import csv
import glob
import json
import os
import re
import statistics
import sys
from collections import defaultdict


def short(name):
    m = re.search(r"(embbag_fwd\w*kernel)<([^>]*)>", name)
    return f"{m.group(1)}<{m.group(2)}>" if m else name[:100]


def summarise(d):
    rec = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "embbag_fwd" in r["Name"]:
                rec.setdefault("kernel_stats", []).append({"kernel": short(r["Name"]), "calls": int(r["Calls"]),
                                                           "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                                           "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)})
    per = defaultdict(lambda: defaultdict(float))      # (kernel, dispatch) -> counter -> value
    for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "embbag_fwd" in r["Kernel_Name"]:
                per[(short(r["Kernel_Name"]), int(r["Dispatch_Id"]))][r["Counter_Name"]] += float(r["Counter_Value"])
    if per:
        count = defaultdict(int)
        for k, _ in per:
            count[k] += 1
        top = max(count, key=count.get)
        rows = [v for (k, _), v in sorted(per.items()) if k == top]
        hit = statistics.median(v.get("TCC_HIT_sum", 0.0) for v in rows)
        miss = statistics.median(v.get("TCC_MISS_sum", 0.0) for v in rows)
        rec["counters"] = {"kernel": top, "dispatches": len(rows), "TCC_HIT_sum": hit, "TCC_MISS_sum": miss,
                           "hit_rate": round(hit / (hit + miss), 4) if hit + miss else None,
                           "miss_min_max": [min(v.get("TCC_MISS_sum", 0.0) for v in rows), max(v.get("TCC_MISS_sum", 0.0) for v in rows)]}
    return rec


def main():
    out = {}
    for arg in sys.argv[1:]:
        label, d = arg.split("=", 1)
        out[label] = summarise(d)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
