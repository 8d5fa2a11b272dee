#!/usr/bin/env python3
"""Rate of msj_sort_rows_device (row numbers by exact numeric order): the call alone, on records the earlier calls left on the
device, over a synthetic 1 GiB NDJSON window of lines
    {"ts":"2024-05-01T07:12:45.123Z","latency_ms":4217395,"score":517.204}
made on the device (the three values are scattered over the lines by multiplications modulo their ranges).  The columns are
    latency   /latency_ms, an int64 per line
    score     /score, a double per line
    ts        /ts cast to nanoseconds by msj_cast_strings_device: int64s above 2^53, whose keys have a low part
and the paths, per column: the full sort, limit 10 and limit 4 096 (the selection, chosen on the device), and each of the
three once more with the other path forced by msj_debug_set_sort_mode, the orders compared entry for entry.  Each is reported in
ms and rows per microsecond next to its yardsticks over the same N, measured in the same process: torch.sort(stable=True) on
an int64 tensor of the column (ascending; for /score the float64) plus the gather of the records by its indices that a caller
would need, against this call plus msj_take_rows_device; torch.topk for the limits (k smallest); the
msj_select_documents_device call that wrote the records; a device-to-device copy of the column's records.
The radix passes a column takes -- the key's digits that are not the same in every row, which is what sr_plan decides on the
device -- are counted over the same records by the host twin (tests/sort_rows_math_host.cpp: srm_passes).
Clocks are settled first (2 s of the same calls), then 20 calls, each timed by device events.  Prints and writes (--json,
default profiles/sort_rows/sort_rows_rate.json)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mojo_simdjson_amd import _lib  # noqa: E402
from mojo_simdjson_amd.device import Stage1Device  # noqa: E402
from mojo_simdjson_amd.document_stream import number_column  # noqa: E402
from cast_strings_rate import DAY_MS, put_digits  # noqa: E402
from validate_documents_rate import timed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = b'{"ts":"2024-05-01T00:00:00.000Z","latency_ms":1000000,"score":100.000}\n'
LIMITS = (0, 10, 4096)


def ndjson(total_bytes, dev):
    """The window, made on the device -> (d_buf, its bytes, its lines)"""
    width, lines = len(LINE), total_bytes // len(LINE)
    d = torch.frombuffer(bytearray(LINE), dtype=torch.uint8).to(dev.device).repeat(lines).view(lines, width)
    k = torch.arange(lines, dtype=torch.int64, device=dev.device)
    ms = (k * 7919) % DAY_MS
    at = LINE.index(b'"ts":"') + 6 + 11
    put_digits(d, at, ms // 3600000, 2)
    put_digits(d, at + 3, ms // 60000 % 60, 2)
    put_digits(d, at + 6, ms // 1000 % 60, 2)
    put_digits(d, at + 9, ms % 1000, 3)
    put_digits(d, LINE.index(b'"latency_ms":') + 13, 1000000 + (k * 104729) % 9000000, 7)
    score = (k * 15485863) % 900000
    at = LINE.index(b'"score":') + 8
    put_digits(d, at, 100 + score // 1000, 3)
    put_digits(d, at + 4, score % 1000, 3)
    return d.view(-1), width * lines, lines


def twin_passes():
    """srm_passes of the host twin, built into a temporary directory"""
    so = os.path.join(tempfile.mkdtemp(prefix="sort_rows_rate_"), "libsort_rows_math_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "sort_rows_math_host.cpp")])
    fn = ctypes.CDLL(so).srm_passes
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32], ctypes.c_uint32
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", nargs="*", default=["latency", "score", "ts"])
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "sort_rows", "sort_rows_rate.json"))
    a = ap.parse_args()
    dev = Stage1Device(0)
    dv = dev.device
    passes_of = twin_passes()
    out = {"library": _lib.load().msj_version().decode(), "line": LINE.decode(), "line_bytes": len(LINE)}
    d_buf, nbytes, lines = ndjson(a.mib << 20, dev)
    d_idx = torch.empty(nbytes // 2 + 1024, dtype=torch.int32, device=dv)
    cin, cout = dev.new_carry(), dev.new_carry()
    dev.shard(d_buf, nbytes, d_idx, cin, cout, is_final=False)
    carry = dev.fetch(cout)
    assert not carry.internal_error
    n = int(carry.count)
    d_type, d_depth, _, d_match, d_end, d_flags = dev.stage2_prep(d_buf, nbytes, d_idx, n, match=True)
    d_first, docs = dev.documents(d_buf, nbytes, d_idx, n, d_type, d_depth, is_final=True, d_carry=cout,
                                  d_doc_first=torch.empty(lines + 16, dtype=torch.int32, device=dv))
    assert docs.n_complete == docs.n_documents == lines, (docs.n_documents, docs.n_complete, lines)
    d_docs = torch.frombuffer(bytearray(bytes(docs)), dtype=torch.uint8).to(dv)
    d_numbers, d_num = dev.number_values(d_buf, nbytes, d_idx, n, d_flags, capacity=2 * lines + 16, sync=False)
    args = (d_buf, nbytes, d_idx, n, d_type, d_depth, d_match, d_end, d_flags)
    out.update({"bytes": nbytes, "tokens": n, "documents": lines})
    paths = dev.compile_paths(["/latency_ms", "/score", "/ts"])
    d_fields = torch.empty((3, lines, 2), dtype=torch.int64, device=dv)
    d_sel = torch.zeros(48, dtype=torch.uint8, device=dv)

    def select():
        dev.select_documents(paths, *args, d_first, d_docs, d_numbers=d_numbers, numbers_capacity=2 * lines + 16, d_numbers_result=d_num,
                             d_fields=d_fields, d_result=d_sel, sync=False)

    out["select_documents"] = timed(select, a.steps, a.settle)
    sel = _lib.MsjSelectDocumentsResult.from_buffer_copy(d_sel.cpu().numpy().tobytes())
    assert (sel.code, sel.n_documents, sel.n_found, sel.n_no_bits) == (0, lines, 3 * lines, 0), (sel.code, sel.n_found, sel.n_no_bits)
    _, d_ts, _ = dev.cast_strings(d_buf, nbytes, d_fields[2].contiguous(), d_sel, "timestamp", "ns", capacity=lines)
    columns = {"latency": (d_fields[0], torch.int64), "score": (d_fields[1], torch.float64), "ts": (d_ts, torch.int64)}
    d_copy = torch.empty((lines, 2), dtype=torch.int64, device=dv)
    out["copy_records"] = timed(lambda: d_copy.copy_(d_fields[0], non_blocking=True), a.steps, a.settle)
    d_res, d_osel, d_tres, d_tsel = (torch.zeros(48, dtype=torch.uint8, device=dv) for _ in range(4))
    d_taken = torch.empty((1, lines, 2), dtype=torch.int64, device=dv)
    for name in a.case:
        d_col, dtype = columns[name]
        d_col = d_col.contiguous()
        values, valid = number_column(d_col, dtype)
        assert bool(valid.all())
        host = d_col.cpu().numpy()
        r = {"rows": lines, "passes": int(passes_of(host.ctypes.data, lines, 0))}
        del host
        want = torch.sort(values, stable=True)[1].to(torch.int32)
        d_order = [torch.empty(lines, dtype=torch.int32, device=dv) for _ in range(2)]
        for limit in LIMITS:
            K = limit or lines

            def sort(which, take=False):
                dev.sort_rows(d_col, d_sel, limit=limit, capacity=lines, d_order=d_order[which], d_result=d_res, d_order_select=d_osel, sync=False)
                if take:
                    dev.take_rows(d_order[which], d_osel, d_col, d_sel, d_out=d_taken, out_capacity=K, d_result=d_tres, d_out_select=d_tsel, sync=False)

            c = {}
            dev.set_sort_mode(0)
            c.update(timed(lambda: sort(0), a.steps, a.settle))
            last = _lib.MsjSortRowsResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
            assert (last.code, last.n_rows, last.n_values, last.n_written) == (0, lines, lines, K), (last.code, last.n_rows, last.n_values, last.n_written)
            assert torch.equal(d_order[0][:K], want[:K]), "the order differs from torch.sort(stable=True)"
            c["with_take"] = timed(lambda: sort(0, True), a.steps, a.settle)
            assert torch.equal(d_taken[0, :K], d_col[want[:K].to(torch.int64)])
            other = 2 if limit == 0 else 1       # the path the device did not choose (without a limit there is one path only)
            if limit:
                dev.set_sort_mode(other)
                c["full_sort_forced"] = timed(lambda: sort(1), a.steps, a.settle)
                assert torch.equal(d_order[0][:K], d_order[1][:K]), "the two paths differ"
                dev.set_sort_mode(0)
            if limit == 0:
                def torch_sort(gather):
                    idx = torch.sort(values, stable=True)[1]
                    if gather:
                        torch.index_select(d_col, 0, idx)

                c["torch_sort"] = timed(lambda: torch_sort(False), a.steps, a.settle)
                c["torch_sort_gather"] = timed(lambda: torch_sort(True), a.steps, a.settle)
                c["ratio_to_torch_sort"] = c["median"] / c["torch_sort"]["median"]
                c["ratio_with_take_to_torch_sort_gather"] = c["with_take"]["median"] / c["torch_sort_gather"]["median"]
            else:
                c["torch_topk"] = timed(lambda: torch.topk(values, limit, largest=False, sorted=True), a.steps, a.settle)
                c["ratio_to_torch_topk"] = c["median"] / c["torch_topk"]["median"]
                c["ratio_to_full_sort_forced"] = c["median"] / c["full_sort_forced"]["median"]
            c.update({"rows_per_us": lines / c["median"] / 1e3, "ratio_to_copy": c["median"] / out["copy_records"]["median"],
                      "ratio_to_select": c["median"] / out["select_documents"]["median"]})
            r["full" if limit == 0 else f"limit_{limit}"] = c
            print(f"{name} limit {limit}: {lines} rows, {r['passes']} passes; sort {c['median']:.3f} ms (min {c['min']:.3f}, p95 {c['p95']:.3f}) = "
                  f"{c['rows_per_us']:.0f} rows/us; with take {c['with_take']['median']:.3f} ms; "
                  + (f"torch.sort {c['torch_sort']['median']:.3f} ms, with gather {c['torch_sort_gather']['median']:.3f} ms" if limit == 0 else
                     f"torch.topk {c['torch_topk']['median']:.3f} ms; the full sort forced {c['full_sort_forced']['median']:.3f} ms")
                  + f"; copy {out['copy_records']['median']:.3f} ms; select {out['select_documents']['median']:.3f} ms", flush=True)
        r["workspace_bytes"] = int(dev.lib.msj_sort_rows_workspace_bytes(lines))
        out[name] = r
        del d_order, want, values
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
