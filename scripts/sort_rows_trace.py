#!/usr/bin/env python3
"""Where msj_sort_rows_device spends its time, per kernel: the workload of a kernel-trace run of its own, and the summary of
that run.
    rocprofv3 --kernel-trace --stats -d OUT -o sort -- python scripts/sort_rows_trace.py
    python scripts/sort_rows_trace.py --summarize OUT/sort_results.db
The workload: 14.9 M hand-made records per column -- ints of seven digits, doubles with three decimals, nanosecond timestamps of
one day of 2024 -- sorted four times in full and four times with limit 10, each order checked against torch.sort(stable=True).
The summary (default profiles/sort_rows/sort_rows_kernel_trace.json): for the third call of each group, the launches and the
microseconds of every kernel of the call."""
import argparse
import collections
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 14_913_080
COLUMNS = ("ints", "doubles", "ns")
LIMITS = (0, 10)
CALLS = 4


def workload():
    import numpy as np
    import torch

    from mojo_simdjson_amd import _lib
    from mojo_simdjson_amd.device import Stage1Device

    dev = Stage1Device(0)
    g = torch.Generator(device=dev.device).manual_seed(1)

    def records(bits, tag):
        out = torch.empty((N, 2), dtype=torch.int64, device=dev.device)
        out[:, 0] = bits
        out[:, 1] = ord(tag) << 32      # (token 0, the tag, no flags, code 0)
        return out

    ints = torch.randint(1_000_000, 10_000_000, (N,), generator=g, device=dev.device, dtype=torch.int64)
    dbl = torch.randint(100_000, 1_000_000, (N,), generator=g, device=dev.device, dtype=torch.int64).to(torch.float64) / 1000.0
    ns = 1714521600000000000 + torch.randint(0, 86_400_000, (N,), generator=g, device=dev.device, dtype=torch.int64) * 1_000_000
    sel = torch.from_numpy(np.frombuffer(bytes(_lib.MsjSelectDocumentsResult(0, 0, N, 1, N, 0, 0)), dtype=np.uint8).copy()).to(dev.device)
    d_order = torch.empty(N, dtype=torch.int32, device=dev.device)
    for name, col, values in zip(COLUMNS, (records(ints, "l"), records(dbl.view(torch.int64), "d"), records(ns, "l")), (ints, dbl, ns)):
        for limit in LIMITS:
            for _ in range(CALLS):
                res, _, _ = dev.sort_rows(col, sel, limit=limit, capacity=N, d_order=d_order)
            assert res.code == 0 and res.n_written == (limit or N)
            want = torch.sort(values, stable=True)[1][:limit or N].to(torch.int32)
            assert torch.equal(d_order[:limit or N], want), name
        print(name, "ok", flush=True)
    torch.cuda.synchronize()
    dev.close()


def summarize(db_path, out_path):
    import sqlite3

    rows = list(sqlite3.connect(db_path).execute("select name, start, end from kernels order by start"))
    short = lambda n: re.sub(r"\(.*", "", n).split("::")[-1]
    calls, cur = [], None
    for name, start, end in rows:
        n = short(name)
        if n == "sr_keys":
            cur = collections.OrderedDict()
            calls.append(cur)
        if cur is not None and n[:3] in ("sr_", "sl_"):
            k = cur.setdefault(n, {"launches": 0, "us": 0.0})
            k["launches"] += 1
            k["us"] = round(k["us"] + (end - start) / 1e3, 1)
    assert len(calls) == len(COLUMNS) * len(LIMITS) * CALLS, len(calls)
    out = {"rows": N, "how": "rocprofv3 --kernel-trace --stats; the third of four calls"}
    for c, name in enumerate(COLUMNS):
        for j, limit in enumerate(LIMITS):
            kernels = calls[(c * len(LIMITS) + j) * CALLS + 2]
            out[f"{name}_limit_{limit}"] = {"sum_us": round(sum(k["us"] for k in kernels.values()), 1), "kernels": kernels}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    for key, v in out.items():
        if isinstance(v, dict):
            print(key, v["sum_us"], {k: (x["launches"], x["us"]) for k, x in v["kernels"].items()})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarize", metavar="DB", default=None)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "sort_rows", "sort_rows_kernel_trace.json"))
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize, a.json)
    else:
        workload()
