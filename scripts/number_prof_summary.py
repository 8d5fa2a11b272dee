#!/usr/bin/env python3
"""Per-kernel summary of rocprofv3 CSVs under a directory (kernel traces: count / mean / total time; counter
collection: mean value per dispatch), for the number kernels and the span kernels of scripts/number_rate.py runs."""
import csv
import glob
import os
import sys
from collections import defaultdict


def main(root):
    for path in sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)):
        agg = defaultdict(list)
        for row in csv.DictReader(open(path)):
            agg[row["Kernel_Name"]].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
        print(f"# {os.path.relpath(path, root)}: kernel, dispatches, mean us, min us")
        for k, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
            print(f"{k[:110]:110s} {len(v):6d} {sum(v) / len(v) / 1e3:10.1f} {min(v) / 1e3:10.1f}")
    for path in sorted(glob.glob(os.path.join(root, "**", "*counter_collection.csv"), recursive=True)):
        agg = defaultdict(list)
        for row in csv.DictReader(open(path)):
            agg[(row["Kernel_Name"], row["Counter_Name"])].append(float(row["Counter_Value"]))
        print(f"# {os.path.relpath(path, root)}: kernel, counter, dispatches, mean per dispatch")
        for (k, c), v in sorted(agg.items()):
            print(f"{k[:100]:100s} {c:12s} {len(v):6d} {sum(v) / len(v):16.0f}")


if __name__ == "__main__":
    main(sys.argv[1])
