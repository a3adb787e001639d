#!/usr/bin/env python3
"""Per-kernel per-launch averages of a rocprofv3 counter_collection.csv.  usage: pmc_summary.py FILE.csv [--by-position]
--by-position: a kernel launched several times per batch is listed once per position ("k_shade<...> #0" is the first shade launch of every batch; a batch
starts at a k_generate_first, dispatches in Dispatch_Id order)."""
import collections
import csv
import sys

by_position = "--by-position" in sys.argv[2:]
rows = list(csv.DictReader(open(sys.argv[1])))
if by_position:
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
acc = collections.defaultdict(lambda: collections.defaultdict(float))
n = collections.defaultdict(int)
seen, at = {}, {}                # per batch: launches of a kernel so far; the position of a dispatch
for r in rows:
    k = r["Kernel_Name"].split("(")[0][:60]
    if by_position:
        if k.startswith("k_generate_first") and r["Dispatch_Id"] not in at:
            seen = {}
        if r["Dispatch_Id"] not in at:           # (one row per counter and dispatch)
            at[r["Dispatch_Id"]] = seen.get(k, 0)
            seen[k] = seen.get(k, 0) + 1
        k = f"{k} #{at[r['Dispatch_Id']]}"
    acc[k][r["Counter_Name"]] += float(r["Counter_Value"])
    n[(k, r["Counter_Name"])] += 1
for k in acc:
    print(k, {c: round(v / n[(k, c)], 1) for c, v in acc[k].items()}, "launches", max(n[(k, c)] for c in acc[k]))
