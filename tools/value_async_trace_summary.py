#!/usr/bin/env python3
"""dev: a rocprofv3 kernel trace of the plain benchmark (tools/value_async_trace.sh) reduced to what DESIGN_EXPERIMENTS.md section R quotes.
usage: value_async_trace_summary.py <rocprofv3 output directory> <prefix of the files to write>
Writes <prefix>_trace_summary.json and <prefix>_kernel_trace.csv.
  summary  "kernels_ms": per kernel name (template arguments dropped) the launches from the start of the fifth-last mgScanKernel on -- the five
           timed steps of `bench.py --steps 5` -- with their mean, shortest and longest duration; "scan_to_scan_ms": the distance between the
           starts of consecutive timed scans; "writers": EVERY mgValueWriteKernel launch of the trace, the warm-up steps' included (so two more
           than timed steps), with its duration, whether it lies inside or overlaps a scan, and how long after it the next scan started.
  csv      name, start, end in ns relative to the first timed scan's start, for every launch from 2 ms before that scan on (the last warm-up
           step's merge kernel and writer are in it: one writer fewer than the summary lists)."""
import csv, glob, sys, collections, json
src, prefix = sys.argv[1], sys.argv[2]
rows = []
for f in glob.glob(src + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        rows.append((r["Kernel_Name"].split("(")[0].replace("void ", ""), int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
rows.sort(key=lambda x: x[1])
short = lambda n: n.split("<")[0]
scans = [(a, b) for n, a, b in rows if short(n) == "mgScanKernel"]
t0 = scans[-5][0]
per = collections.defaultdict(list)
for n, a, b in rows:
    if a >= t0:
        per[short(n)].append((b - a) / 1e6)
out = {"kernels_ms": {k: {"n": len(v), "mean": round(sum(v) / len(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in sorted(per.items())}}
out["writers"] = []
for a, b in [(a, b) for n, a, b in rows if short(n) == "mgValueWriteKernel"]:
    nxt = [x for x, y in scans if x > a]
    out["writers"].append({"writer_ms": round((b - a) / 1e6, 4), "inside_a_scan": any(x <= a and b <= y for x, y in scans),
                           "overlaps_scan": any(x <= b and y >= a for x, y in scans),
                           "scan_start_minus_writer_start_us": round((min(nxt) - a) / 1e3, 1) if nxt else None})
out["scan_to_scan_ms"] = [round((scans[i + 1][0] - scans[i][0]) / 1e6, 3) for i in range(len(scans) - 5, len(scans) - 1)]
json.dump(out, open(prefix + "_trace_summary.json", "w"), indent=1)
with open(prefix + "_kernel_trace.csv", "w") as f:
    f.write("kernel,start_ns,end_ns\n")
    for n, a, b in rows:
        if a >= t0 - 2_000_000:
            f.write("%s,%d,%d\n" % (n[:60], a - t0, b - t0))
