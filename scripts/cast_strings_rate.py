#!/usr/bin/env python3
"""Rate of msj_cast_strings_device (timestamps and numbers written as strings): the call alone, on the records the select call
left on the device, over one synthetic 1 GiB NDJSON window of lines
    {"ts":"2024-05-01T00:00:00.000Z","tz":"2024-05-01T05:30:00.000+05:30","te":"\\u0032024-05-01T00:00:00.000Z","price":"100000.00"}
made on the device (the clock counts the lines in milliseconds, the price 100000.00 .. 999999.99 is scattered) --
    ts_ms / ts_ns   /ts, Z-terminated with milliseconds, to milliseconds and to nanoseconds
    tz_ms           /tz, the same instants written with a +05:30 offset
    price           /price as a number
    escaped_ms      /te: every value spelled with an escape, so every row goes through the list and the second kernel
each with both forms of the kernel's byte fetch (msj_debug_set_cast_fetch: "window" the aligned 16-byte words through LDS,
"bytes" byte loads).  Yardsticks in the same process, over the same rows: msj_string_column_device over /ts (it reads the same
bodies and writes them out), msj_filter_rows_device with one STR_PREFIX predicate on /ts (the same reads, a byte out), and a
device-to-device copy of the column's records.  Each cast is reported in ms and as a ratio of the three.
Clocks are settled first (2 s of the same calls), then 20 calls, each timed by device events.  Prints and writes (--json,
default profiles/cast_strings/cast_strings_rate.json)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mojo_simdjson_amd import _lib  # noqa: E402
from mojo_simdjson_amd.device import Stage1Device  # noqa: E402
from mojo_simdjson_amd.document_stream import number_column  # noqa: E402
from validate_documents_rate import stats, timed  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = (b'{"ts":"2024-05-01T00:00:00.000Z","tz":"2024-05-01T05:30:00.000+05:30","te":"\\u0032024-05-01T00:00:00.000Z",'
        b'"price":"100000.00"}\n')
T0_MS = 1714521600000   # 2024-05-01T00:00:00Z
DAY_MS = 86400000
CASES = {"ts_ms": (0, "timestamp", "ms"), "ts_ns": (0, "timestamp", "ns"), "tz_ms": (1, "timestamp", "ms"), "price": (3, "number", "ns"),
         "escaped_ms": (2, "timestamp", "ms")}
FETCH = {"window": _lib.CAST_FETCH_WINDOW, "bytes": _lib.CAST_FETCH_BYTES}


def put_digits(d, at, value, width):
    for j in range(width):
        d[:, at + j] = ((value // 10 ** (width - 1 - j)) % 10 + 48).to(torch.uint8)


def ndjson(total_bytes, dev):
    """The window, made on the device -> (d_buf, its bytes, its lines).  Line k's instant is T0_MS + k % DAY_MS milliseconds; /tz
    is the same instant on a clock 05:30 ahead (its hour wraps inside the day: the instant is then a day early, which the
    check below knows)"""
    width, lines = len(LINE), total_bytes // len(LINE)
    d = torch.frombuffer(bytearray(LINE), dtype=torch.uint8).to(dev.device).repeat(lines).view(lines, width)
    k = torch.arange(lines, dtype=torch.int64, device=dev.device)
    ms = k % DAY_MS
    for key, skip, shift in ((b'"ts":"', 11, 0), (b'"tz":"', 11, 19800000), (b'"te":"\\u0032', 10, 0)):
        at = LINE.index(key) + len(key) + skip
        local = (ms + shift) % DAY_MS
        put_digits(d, at, local // 3600000, 2)
        put_digits(d, at + 3, local // 60000 % 60, 2)
        put_digits(d, at + 6, local // 1000 % 60, 2)
        put_digits(d, at + 9, local % 1000, 3)
    price = (k * 7919) % 100000000
    at = LINE.index(b'"price":"') + 9
    put_digits(d, at, 100000 + price // 100 % 900000, 6)   # (no leading zero: a JSON number)
    put_digits(d, at + 7, price % 100, 2)
    return d.view(-1), width * lines, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", nargs="*", default=list(CASES))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "cast_strings", "cast_strings_rate.json"))
    a = ap.parse_args()
    dev = Stage1Device(0)
    dv = dev.device
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
    d_numbers, d_num = dev.number_values(d_buf, nbytes, d_idx, n, d_flags, capacity=16, sync=False)
    args = (d_buf, nbytes, d_idx, n, d_type, d_depth, d_match, d_end, d_flags)
    out.update({"bytes": nbytes, "tokens": n, "documents": lines})
    paths = dev.compile_paths(["/ts", "/tz", "/te", "/price"])
    d_fields = torch.empty((4, lines, 2), dtype=torch.int64, device=dv)
    d_sel = torch.zeros(48, dtype=torch.uint8, device=dv)
    dev.select_documents(paths, *args, d_first, d_docs, d_numbers=d_numbers, numbers_capacity=16, d_numbers_result=d_num, d_fields=d_fields,
                         d_result=d_sel, sync=False)
    sel = _lib.MsjSelectDocumentsResult.from_buffer_copy(d_sel.cpu().numpy().tobytes())
    assert (sel.code, sel.n_documents, sel.n_found) == (0, lines, 4 * lines), (sel.code, sel.n_found)
    del d_idx, d_type, d_depth, d_match, d_end, d_flags, d_first
    torch.cuda.empty_cache()

    # the yardsticks
    d_copy = torch.empty((lines, 2), dtype=torch.int64, device=dv)
    cp = timed(lambda: d_copy.copy_(d_fields[0], non_blocking=True), a.steps, a.settle)
    d_off, d_valid = torch.empty(lines + 1, dtype=torch.int64, device=dv), torch.empty(lines, dtype=torch.uint8, device=dv)
    d_bytes, d_scres = torch.empty(24 * lines, dtype=torch.uint8, device=dv), torch.zeros(48, dtype=torch.uint8, device=dv)

    def string_column():
        dev.string_column(d_buf, nbytes, d_fields, 0, d_sel, d_offsets=d_off, d_valid=d_valid, d_bytes=d_bytes, capacity=lines,
                          bytes_capacity=24 * lines, d_result=d_scres, sync=False)

    sc = timed(string_column, a.steps, a.settle)
    scres = _lib.MsjStringColumnResult.from_buffer_copy(d_scres.cpu().numpy().tobytes())
    assert (scres.code, scres.n_strings, scres.total_bytes) == (0, lines, 24 * lines), (scres.code, scres.n_strings, scres.total_bytes)
    del d_off, d_bytes
    predicates = dev.compile_predicates([(0, "prefix", "2024-05-01T01:0")])
    d_kept, d_fres, d_ksel = torch.empty(lines, dtype=torch.int32, device=dv), torch.zeros(48, dtype=torch.uint8, device=dv), torch.zeros(48, dtype=torch.uint8, device=dv)

    def prefix_filter():
        dev.filter_rows(predicates, d_buf, nbytes, d_fields[0], d_sel, d_keep=d_valid, d_kept=d_kept, d_result=d_fres, d_kept_select=d_ksel, sync=False)

    fp = timed(prefix_filter, a.steps, a.settle)
    fres = _lib.MsjFilterRowsResult.from_buffer_copy(d_fres.cpu().numpy().tobytes())
    assert fres.code == 0 and fres.n_rows == lines and 0 < fres.n_kept < lines
    predicates.close()
    del d_kept
    out.update({"copy_of_the_records": cp, "string_column": sc, "filter_rows_prefix": fp, "record_bytes": 16 * lines})
    print(f"{lines} rows of {len(LINE)} bytes: string_column over /ts {sc['median']:.3f} ms, filter_rows STR_PREFIX on /ts {fp['median']:.3f} ms, "
          f"a device-to-device copy of the records {cp['median']:.3f} ms", flush=True)

    d_out, d_res, d_osel = d_copy, torch.zeros(48, dtype=torch.uint8, device=dv), torch.zeros(48, dtype=torch.uint8, device=dv)
    k = torch.arange(lines, dtype=torch.int64, device=dv)
    for name in a.case:
        p, kind, unit = CASES[name]
        r = {}
        for form, fetch in FETCH.items():
            assert dev.lib.msj_debug_set_cast_fetch(dev.ctx, fetch) == 0

            def cast():
                dev.cast_strings(d_buf, nbytes, d_fields[p], d_sel, kind, unit, capacity=lines, d_out=d_out, d_result=d_res, d_out_select=d_osel,
                                 sync=False)

            t = timed(cast, a.steps, a.settle)
            res = _lib.MsjCastStringsResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
            assert (res.code, res.n_rows, res.n_cast, res.n_syntax, res.n_range, res.n_other) == (0, lines, lines, 0, 0, 0), (name, form, res.n_cast, res.n_syntax)
            if kind == "timestamp":
                per = _lib.CAST_UNIT_PER_SECOND[unit] // 1000
                ms = k % DAY_MS
                want = (T0_MS + ms - (DAY_MS if p == 1 else 0) * ((ms + 19800000) // DAY_MS)) * per
                values, valid = number_column(d_out, torch.int64)
                assert bool(valid.all()) and bool((values == want).all()), (name, form)
            else:   # a scattered sample against Python's float of the same text, on the host
                at = (torch.arange(4096, dtype=torch.int64, device=dv) * 2039) % lines
                price = ((at * 7919) % 100000000).cpu().tolist()
                want = [float("%d.%02d" % (100000 + x // 100 % 900000, x % 100)) for x in price]
                values, valid = number_column(d_out, torch.float64)
                assert bool(valid.all()) and values[at].cpu().tolist() == want, (name, form)
            del want, values, valid
            t.update({"ratio_to_string_column": t["median"] / sc["median"], "ratio_to_filter_rows_prefix": t["median"] / fp["median"],
                      "ratio_to_copy": t["median"] / cp["median"], "rows_per_us": lines / t["median"] / 1e3})
            r[form] = t
            print(f"{name} ({form}): {t['median']:.3f} ms (min {t['min']:.3f}, p95 {t['p95']:.3f}) = {t['rows_per_us']:.0f} rows/us, "
                  f"{t['ratio_to_string_column']:.3f} of string_column, {t['ratio_to_filter_rows_prefix']:.3f} of the prefix filter, "
                  f"{t['ratio_to_copy']:.2f} of the copy", flush=True)
        r["rows"] = lines
        out[name] = r
    dev.lib.msj_debug_set_cast_fetch(dev.ctx, _lib.CAST_FETCH_WINDOW)
    out["workspace_bytes"] = int(dev.lib.msj_cast_strings_workspace_bytes(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
