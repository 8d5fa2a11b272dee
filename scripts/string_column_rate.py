#!/usr/bin/env python3
"""Rate of msj_string_column_device (a selected path's strings as one column): the call alone, on the records the select
call left on the device, for two paths --
    short    /text on the 1 GiB NDJSON window of scripts/validate_documents_rate.py: plain strings of 0 .. 49 bytes
    escaped  /note on a window built the same way with one more key per line, a string of 11 .. 50 raw bytes that holds
             \\" \\n and a \\u escape (that window's lines have no escaped value of their own)
-- each beside msj_select_documents_device for that one path over the same arrays in the same process, and beside the
bytes the call must move: 16 B per record read, 9 B per row written (an offset and a validity byte), each body read once
and written once.
Clocks are settled first (2 s of the same calls), then 20 calls, each timed by device events.  Prints and writes (--json,
default profiles/string_column/string_column_rate.json).  The per-kernel split comes from a run of its own:
    rocprofv3 --kernel-trace --stats -- python scripts/string_column_rate.py --steps 3 --settle 0 --case short"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mojo_simdjson_amd import _lib  # noqa: E402
from mojo_simdjson_amd.device import Stage1Device  # noqa: E402
from validate_documents_rate import ndjson, timed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_BYTES_PER_S = 8e12
CASES = {"short": "/text", "escaped": "/note"}


def ndjson_with_notes(total_bytes, dev):
    """validate_documents_rate.ndjson with one more key per line: an escaped string"""
    block = b"".join(json.dumps({"id": i, "text": "t" * (i % 50), "note": 'q"' + "n" * (i % 40) + "\né",
                                 "tags": [i, i + 1], "user": {"name": "n", "ok": True}}, separators=(",", ":")).encode() + b"\n"
                     for i in range(12000))
    nrep = total_bytes // len(block)
    d_block = torch.frombuffer(bytearray(block), dtype=torch.uint8).to(dev.device)
    return d_block.repeat(nrep), len(block) * nrep, 12000 * nrep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", nargs="*", default=list(CASES))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "string_column", "string_column_rate.json"))
    a = ap.parse_args()
    dev = Stage1Device(0)
    dv = dev.device
    out = {"library": _lib.load().msj_version().decode()}
    for name in a.case:
        pointer = CASES[name]
        d_buf, nbytes, lines = (ndjson if name == "short" else ndjson_with_notes)(a.mib << 20, dev)
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
        d_verdicts = torch.empty((lines, 2), dtype=torch.int64, device=dv)
        _, vres = dev.validate_documents(*args, d_first, d_docs, d_numbers_result=d_num, d_verdicts=d_verdicts)
        assert (vres.code, vres.flags, vres.n_documents, vres.n_invalid) == (0, 0, lines, 0), (vres.code, vres.flags, vres.n_invalid)
        paths = dev.compile_paths([pointer])
        d_fields = torch.empty((1, lines, 2), dtype=torch.int64, device=dv)
        d_sel = torch.zeros(48, dtype=torch.uint8, device=dv)

        def select():
            dev.select_documents(paths, *args, d_first, d_docs, d_numbers_result=d_num, d_verdicts=d_verdicts, d_fields=d_fields, d_result=d_sel,
                                 sync=False)

        select()
        layout, d_off, d_valid, _ = dev.string_column(d_buf, nbytes, d_fields, 0, d_sel, strings=False)
        assert (layout.code, layout.n_rows, layout.n_strings) == (0, lines, lines), (layout.code, layout.n_rows, layout.n_strings)
        total = int(layout.total_bytes)
        d_bytes = torch.empty(max(total, 1), dtype=torch.uint8, device=dv)
        d_res = torch.zeros(48, dtype=torch.uint8, device=dv)
        res, _, _, _ = dev.string_column(d_buf, nbytes, d_fields, 0, d_sel, d_offsets=d_off, d_valid=d_valid, d_bytes=d_bytes, d_result=d_res)
        assert (res.code, res.total_bytes, res.n_escaped) == (0, total, lines if name == "escaped" else 0), (res.code, res.n_escaped)

        def column():
            dev.string_column(d_buf, nbytes, d_fields, 0, d_sel, d_offsets=d_off, d_valid=d_valid, d_bytes=d_bytes, d_result=d_res, sync=False)

        raw = int((d_fields[0, :, 0] >> 32).sum().item())   # the bodies as they stand in the window
        r = timed(column, a.steps, a.settle)
        sel = timed(select, a.steps, a.settle)
        parts = {"records": 16 * lines, "offsets_and_validity": 9 * lines, "bodies_read": raw, "bodies_written": total}
        alg = int(sum(parts.values()))
        r.update({"pointer": pointer, "bytes": nbytes, "tokens": n, "documents": lines, "total_bytes": total, "raw_body_bytes": raw,
                  "n_escaped": int(res.n_escaped), "must_move_bytes": alg, "must_move_parts": parts,
                  "must_move_gb_per_s": alg / r["median"] / 1e6, "share_of_8tb_per_s": alg / (r["median"] * 1e-3) / PEAK_BYTES_PER_S,
                  "rows_per_s": lines / (r["median"] * 1e-3), "select_documents": sel, "ratio_to_select_documents": r["median"] / sel["median"]})
        out[name] = r
        print(f"{name} {pointer}: {nbytes} B, {lines} rows, {total} B of strings ({res.n_escaped} escaped); string_column {r['median']:.3f} ms "
              f"(min {r['min']:.3f}, p95 {r['p95']:.3f}), must move {alg / 1e9:.3f} GB -> {r['must_move_gb_per_s']:.0f} GB/s = "
              f"{100 * r['share_of_8tb_per_s']:.1f} % of 8 TB/s; select_documents for the path {sel['median']:.3f} ms; ratio "
              f"{r['ratio_to_select_documents']:.2f}", flush=True)
        del d_buf, d_idx, d_type, d_depth, d_match, d_end, d_flags, d_first, d_verdicts, d_fields, d_off, d_valid, d_bytes, args
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
