#!/usr/bin/env python3
"""Condense the rocprofv3 passes of tools/ab_two_trees.sh: per tree the kernel-stats rows of the uniform Jacobi kernels,
their kernel time per bench step, the SQ counters per step (summed over every launch of these kernels) and the split of
the waves' resident cycles into issuing / waiting to issue / parked (MI355X_MICROARCH.md, SQ counters).

usage: tools/summarize_two_trees.py <out dir of ab_two_trees.sh>/prof [summary.json]   -> profiles/r05_packed_rows_counters.json"""
import collections
import csv
import glob
import json
import re
import sys

TRACED_STEPS = 5 + 2  # bench.py --steps 5 --warmup 2 under the trace
COUNTED_STEPS = 2 + 1  # --steps 2 --warmup 1 under each counter group


def short(name):
    m = re.search(r"Jacobi5Uniform<(\w+), (\w+)>, false, (\d+),", name)
    return f"Jacobi5Uniform<{m.group(1)}, {m.group(2)}> T={m.group(3)}" if m else None


def one(base, tag):
    o = {"kernel_stats": [], "steps_traced": TRACED_STEPS}
    with open(glob.glob(f"{base}/{tag}_stats/*/*kernel_stats.csv")[0]) as f:
        for r in csv.DictReader(f):
            if short(r["Name"]):
                o["kernel_stats"].append({
                    "kernel": short(r["Name"]), "calls": int(r["Calls"]), "total_ms": round(int(r["TotalDurationNs"]) / 1e6, 3),
                    "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(int(r["MinNs"]) / 1e3, 2),
                    "max_us": round(int(r["MaxNs"]) / 1e3, 2), "percent": float(r["Percentage"])})
    o["kernel_ms_per_step"] = round(sum(k["total_ms"] for k in o["kernel_stats"]) / TRACED_STEPS, 3)
    for group in ("sq", "sqwait"):
        sums = collections.defaultdict(lambda: collections.defaultdict(float))
        launches, seen = collections.Counter(), set()
        with open(glob.glob(f"{base}/{tag}_{group}/*/*counter_collection.csv")[0]) as f:
            for r in csv.DictReader(f):
                kernel = short(r["Kernel_Name"])
                if not kernel:
                    continue
                for key in (kernel, "all uniform kernels"):
                    sums[key][r["Counter_Name"]] += float(r["Counter_Value"])
                if r["Dispatch_Id"] not in seen:
                    seen.add(r["Dispatch_Id"])
                    launches[kernel] += 1
                    launches["all uniform kernels"] += 1
        o[group] = {"steps": COUNTED_STEPS,
                    "per_step": {k: dict({c: v / COUNTED_STEPS for c, v in d.items()}, launches=launches[k] / COUNTED_STEPS)
                                 for k, d in sums.items()}}
    w = o["sqwait"]["per_step"]["all uniform kernels"]
    cycles = w["SQ_WAVE_CYCLES"]
    o["split"] = {"parked_at_waitcnt_or_barrier": round(w["SQ_WAIT_ANY"] / cycles, 4),
                  "issue_stalled": round(w["SQ_WAIT_INST_ANY"] / cycles, 4),
                  "issuing": round(w["SQ_ACTIVE_INST_ANY"] / cycles, 4),
                  "issuing_valu": round(w["SQ_ACTIVE_INST_VALU"] / cycles, 4)}
    return o


def main():
    base = sys.argv[1]
    out = {tag: one(base, tag) for tag in ("other", "this")}
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)
    for tag, o in out.items():
        print(tag, "kernel ms per step", o["kernel_ms_per_step"], "split", o["split"])
        for k in o["kernel_stats"]:
            print("  ", k)
        for group in ("sq", "sqwait"):
            print("  ", group, {k: f"{v:.4g}" for k, v in o[group]["per_step"]["all uniform kernels"].items()})


if __name__ == "__main__":
    main()
