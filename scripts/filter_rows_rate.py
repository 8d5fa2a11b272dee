#!/usr/bin/env python3
"""Rate of msj_filter_rows_device and msj_take_rows_device (rows by predicate): the calls alone, on the records the select call
left on the device, over one synthetic 1 GiB NDJSON window of lines
    {"id":"0000001234","status":"s07","latency_ms":142}
made on the device (the id counts the lines, the status is one of 37 values in a scattered order, the latency 100 .. 199) --
    number   /latency_ms > 150.5            (an int64 record against a double: about half the rows)
    string   /status == "s07"               (one row in 37)
    both     the two together
each alone and followed by the take of the three columns.  Each is reported in ms, as a ratio of the
msj_select_documents_device call that wrote the records (that call is the yardstick, as in the other rate scripts) and as a
ratio of a device-to-device copy of the same records.  Beside them the same filter done with torch: a boolean mask, nonzero
and index_select over the three columns, the host wait for the count included (wall clock); the string predicate there
needs msj_string_column_device first and compares the fixed-width bytes.
Clocks are settled first (2 s of the same calls), then 20 calls, each timed by device events.  Prints and writes (--json,
default profiles/filter_rows/filter_rows_rate.json)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mojo_simdjson_amd import _lib  # noqa: E402
from mojo_simdjson_amd.device import Stage1Device  # noqa: E402
from mojo_simdjson_amd.document_stream import number_column  # noqa: E402
from validate_documents_rate import stats, timed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = b'{"id":"0000000000","status":"s00","latency_ms":100}\n'
STATUSES = 37
CASES = {"number": [(1, ">", 150.5)], "string": [(0, "==", "s07")], "both": [(0, "==", "s07"), (1, ">", 150.5)]}


def ndjson(total_bytes, dev):
    """The window, made on the device -> (d_buf, its bytes, its lines)"""
    width, lines = len(LINE), total_bytes // len(LINE)
    d = torch.frombuffer(bytearray(LINE), dtype=torch.uint8).to(dev.device).repeat(lines).view(lines, width)
    k = torch.arange(lines, dtype=torch.int64, device=dev.device)
    at = LINE.index(b"0000000000")
    for j in range(10):
        d[:, at + j] = ((k // 10 ** (9 - j)) % 10 + 48).to(torch.uint8)
    s = (k * 7919) % STATUSES
    at = LINE.index(b"s00") + 1
    d[:, at], d[:, at + 1] = (s // 10 + 48).to(torch.uint8), (s % 10 + 48).to(torch.uint8)
    lat = (k * 6151) % 100
    at = LINE.index(b":100") + 2
    d[:, at], d[:, at + 1] = (lat // 10 + 48).to(torch.uint8), (lat % 10 + 48).to(torch.uint8)
    return d.view(-1), width * lines, lines


def wall(fn, steps, settle):
    """fn with the host's wait in it, by the wall clock -> stats in ms"""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < settle:
        fn()
    ms = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", nargs="*", default=list(CASES))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "filter_rows", "filter_rows_rate.json"))
    a = ap.parse_args()
    dev = Stage1Device(0)
    dv = dev.device
    out = {"library": _lib.load().msj_version().decode()}
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
    d_numbers, d_num = dev.number_values(d_buf, nbytes, d_idx, n, d_flags, capacity=lines, sync=False)
    args = (d_buf, nbytes, d_idx, n, d_type, d_depth, d_match, d_end, d_flags)
    out.update({"bytes": nbytes, "tokens": n, "documents": lines})
    paths = dev.compile_paths(["/status", "/latency_ms", "/id"])
    d_fields = torch.empty((3, lines, 2), dtype=torch.int64, device=dv)
    d_sel = torch.zeros(48, dtype=torch.uint8, device=dv)

    def select():
        dev.select_documents(paths, *args, d_first, d_docs, d_numbers=d_numbers, numbers_capacity=lines, d_numbers_result=d_num,
                             d_fields=d_fields, d_result=d_sel, sync=False)

    sc = timed(select, a.steps, a.settle)
    sel = _lib.MsjSelectDocumentsResult.from_buffer_copy(d_sel.cpu().numpy().tobytes())
    assert (sel.code, sel.n_documents, sel.n_found, sel.n_no_bits) == (0, lines, 3 * lines, 0), (sel.code, sel.n_found, sel.n_no_bits)
    d_copy = torch.empty_like(d_fields)
    cp = timed(lambda: d_copy.copy_(d_fields, non_blocking=True), a.steps, a.settle)
    out.update({"select_documents": sc, "copy_of_the_records": cp, "record_bytes": int(d_fields.numel() * 8)})
    print(f"{lines} rows of 3 records: select_documents {sc['median']:.3f} ms, a device-to-device copy of the records {cp['median']:.3f} ms", flush=True)
    d_keep = torch.empty(lines, dtype=torch.uint8, device=dv)
    d_kept = torch.empty(lines, dtype=torch.int32, device=dv)
    d_res, d_ksel = torch.zeros(48, dtype=torch.uint8, device=dv), torch.zeros(48, dtype=torch.uint8, device=dv)
    d_tres, d_osel = torch.zeros(48, dtype=torch.uint8, device=dv), torch.zeros(48, dtype=torch.uint8, device=dv)
    d_out = d_copy  # (the copy's room serves the take)
    lat = (torch.arange(lines, dtype=torch.int64, device=dv) * 6151) % 100 + 100
    status = (torch.arange(lines, dtype=torch.int64, device=dv) * 7919) % STATUSES
    want = {"number": int((lat > 150).sum()), "string": int((status == 7).sum()), "both": int(((lat > 150) & (status == 7)).sum())}
    del lat, status
    for name in a.case:
        predicates = dev.compile_predicates(CASES[name])

        def filt():
            dev.filter_rows(predicates, d_buf, nbytes, d_fields, d_sel, d_keep=d_keep, d_kept=d_kept, d_result=d_res, d_kept_select=d_ksel, sync=False)

        def filt_take():
            filt()
            dev.take_rows(d_kept, d_ksel, d_fields, d_sel, d_out=d_out, d_result=d_tres, d_out_select=d_osel, sync=False)

        r, rt = timed(filt, a.steps, a.settle), timed(filt_take, a.steps, a.settle)
        res = _lib.MsjFilterRowsResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
        tres = _lib.MsjTakeRowsResult.from_buffer_copy(d_tres.cpu().numpy().tobytes())
        assert (res.code, res.n_rows, res.n_kept, res.n_no_bits, res.n_missing) == (0, lines, want[name], 0, 0), (res.code, res.n_kept, want[name])
        assert (tres.code, tres.n_rows, tres.n_found, tres.n_out_of_range) == (0, want[name], 3 * want[name], 0)

        def with_torch():
            keep = None
            if name in ("number", "both"):
                values, valid = number_column(d_fields[1])
                keep = valid & (values > 150.5)
            if name in ("string", "both"):
                _, _, d_valid, d_bytes = dev.string_column(d_buf, nbytes, d_fields, 0, d_sel, bytes_capacity=3 * lines, sync=False)
                same = (d_bytes[:3 * lines].view(lines, 3) == torch.tensor(list(b"s07"), dtype=torch.uint8, device=dv)).all(1) & d_valid.view(torch.bool)
                keep = same if keep is None else keep & same
            rows = keep.nonzero().view(-1)   # (the host waits here for the count)
            return rows, d_fields.index_select(1, rows)

        rows, _ = with_torch()
        assert rows.numel() == want[name] and bool((rows.to(torch.int32) == d_kept[:want[name]]).all())
        tt = wall(with_torch, a.steps, a.settle)
        r.update({"rows": lines, "n_kept": int(res.n_kept), "with_take": rt, "with_torch_wall": tt,
                  "ratio_to_select_documents": r["median"] / sc["median"], "ratio_to_copy": r["median"] / cp["median"],
                  "with_take_ratio_to_select_documents": rt["median"] / sc["median"], "with_take_ratio_to_copy": rt["median"] / cp["median"],
                  "rows_per_us": lines / r["median"] / 1e3, "workspace_bytes": int(dev.lib.msj_filter_rows_workspace_bytes(lines))})
        out[name] = r
        print(f"{name}: {res.n_kept} of {lines} rows kept; filter {r['median']:.3f} ms (min {r['min']:.3f}, p95 {r['p95']:.3f}) = "
              f"{r['rows_per_us']:.0f} rows/us, {r['ratio_to_select_documents']:.3f} of select_documents, {r['ratio_to_copy']:.2f} of the copy; "
              f"with the take of 3 columns {rt['median']:.3f} ms ({rt['median'] / sc['median']:.3f}, {rt['median'] / cp['median']:.2f}); "
              f"with torch {tt['median']:.3f} ms by the wall clock", flush=True)
        predicates.close()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
