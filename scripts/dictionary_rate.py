#!/usr/bin/env python3
"""Rate of msj_dictionary_device (a byte column as codes plus distinct values): the call alone, on columns the string column
call left on the device, over one synthetic 1 GiB NDJSON window of lines
    {"id":"0000001234","status":"s07","n":4}
made on the device (the id counts the lines, the status is one of 37 values in a scattered order) --
    status  /status: 37 distinct values, the low-cardinality column
    id      /id: every row distinct
    keys    the keys of the root objects (Window.entries("").keys()): 3 names, three rows per line
Each is reported in ms, as a ratio of the msj_string_column_device call that produced its input over the same rows (that
call is the yardstick, as in the other rate scripts), and with the call's own max_probe.
Clocks are settled first (2 s of the same calls), then 20 calls, each timed by device events.  Prints and writes (--json,
default profiles/dictionary/dictionary_rate.json).  The per-kernel split comes from a run of its own:
    rocprofv3 --kernel-trace --stats -- python scripts/dictionary_rate.py --steps 3 --settle 0 --case id"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mojo_simdjson_amd import _lib  # noqa: E402
from mojo_simdjson_amd.device import Stage1Device  # noqa: E402
from validate_documents_rate import timed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = b'{"id":"0000000000","status":"s00","n":0}\n'
STATUSES = 37


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
    d[:, LINE.index(b'"n":') + 4] = (k % 10 + 48).to(torch.uint8)
    return d.view(-1), width * lines, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", nargs="*", default=["status", "id", "keys"])
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "dictionary", "dictionary_rate.json"))
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
    _, d_num = dev.number_values(d_buf, nbytes, d_idx, n, d_flags, capacity=0, sync=False)
    args = (d_buf, nbytes, d_idx, n, d_type, d_depth, d_match, d_end, d_flags)
    out.update({"bytes": nbytes, "tokens": n, "documents": lines})
    paths = dev.compile_paths(["/status", "/id", ""])
    d_fields = torch.empty((3, lines, 2), dtype=torch.int64, device=dv)
    d_sel = torch.zeros(48, dtype=torch.uint8, device=dv)
    dev.select_documents(paths, *args, d_first, d_docs, d_numbers_result=d_num, d_fields=d_fields, d_result=d_sel, sync=False)
    for name in a.case:
        if name == "keys":
            res, _, _, d_keys, _, d_rsel, _ = dev.object_entries(d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_fields[2], d_sel,
                                                                 d_numbers_result=d_num)
            assert (res.code, res.n_entries) == (0, 3 * lines), (res.code, res.n_entries)
            d_rows, p, rows = d_keys.unsqueeze(0), 0, 3 * lines
        else:
            d_rows, p, d_rsel, rows = d_fields, ("status", "id").index(name), d_sel, lines
        slay, d_off, d_valid, _ = dev.string_column(d_buf, nbytes, d_rows, p, d_rsel, strings=False)
        assert (slay.code, slay.n_rows, slay.n_strings) == (0, rows, rows), (slay.code, slay.n_rows, slay.n_strings)
        d_bytes = torch.empty(max(int(slay.total_bytes), 1), dtype=torch.uint8, device=dv)
        d_sres = torch.zeros(48, dtype=torch.uint8, device=dv)

        def strings():
            dev.string_column(d_buf, nbytes, d_rows, p, d_rsel, d_offsets=d_off, d_valid=d_valid, d_bytes=d_bytes, d_result=d_sres, sync=False)

        sc = timed(strings, a.steps, a.settle)
        first, d_codes, d_doff, d_dfirst, d_dbytes = dev.dictionary(d_off, d_bytes, d_valid, rows=rows, bytes_len=int(slay.total_bytes))
        want = {"status": STATUSES, "id": lines, "keys": 3}[name]
        assert (first.code, first.n_rows, first.n_values, first.n_distinct) == (0, rows, rows, want), (first.code, first.n_values, first.n_distinct)
        d_res = torch.zeros(48, dtype=torch.uint8, device=dv)
        d_n_rows = d_sres[8:16].view(torch.int64)  # the rows as the string column call left them on the device

        def dictionary():
            dev.dictionary(d_off, d_bytes, d_valid, rows=rows, d_n_rows=d_n_rows, bytes_len=int(slay.total_bytes), d_codes=d_codes,
                           d_dict_offsets=d_doff, d_dict_first=d_dfirst, d_dict_bytes=d_dbytes, d_result=d_res, sync=False)

        r = timed(dictionary, a.steps, a.settle)
        last = _lib.MsjDictionaryResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
        assert (last.code, last.n_distinct, last.dict_bytes) == (0, first.n_distinct, first.dict_bytes)
        r.update({"rows": rows, "column_bytes": int(slay.total_bytes), "n_distinct": int(last.n_distinct), "dict_bytes": int(last.dict_bytes),
                  "max_probe": int(last.max_probe), "string_column": sc, "ratio_to_string_column": r["median"] / sc["median"],
                  "rows_per_us": rows / r["median"] / 1e3, "workspace_bytes": int(dev.lib.msj_dictionary_workspace_bytes(rows))})
        out[name] = r
        print(f"{name}: {rows} rows, {int(slay.total_bytes)} B, {last.n_distinct} distinct; dictionary {r['median']:.3f} ms (min {r['min']:.3f}, p95 "
              f"{r['p95']:.3f}) = {r['rows_per_us']:.0f} rows/us, max_probe {last.max_probe}; string_column over the same rows "
              f"{sc['median']:.3f} ms, ratio {r['ratio_to_string_column']:.2f}", flush=True)
        del d_off, d_valid, d_bytes, d_codes, d_doff, d_dfirst, d_dbytes
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
