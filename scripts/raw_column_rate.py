#!/usr/bin/env python3
"""Rate of msj_raw_column_device (a selected value's JSON text as a column): the call alone, verbatim and compact
(MSJ_RAW_COMPACT), on the records the select call left on the device, over three paths of the 1 GiB NDJSON window of
scripts/validate_documents_rate.py --
    short      /text: plain strings of 0 .. 49 bytes, beside msj_string_column_device over the same rows
    container  /user: an object of 23 bytes per line
    root       "": every line whole, beside a device-to-device copy of total_bytes
-- and beside the bytes the call must move: 16 B per record read, 9 B per row written (an offset and a validity byte), each
text read once and written once; the compact form also reads d_idx, d_end, d_flags and d_type of every token (10 B) and
writes and reads its 8-byte sum.
Clocks are settled first (2 s of the same calls), then 20 calls, each timed by device events.  Prints and writes (--json,
default profiles/raw_column/raw_column_rate.json).  The per-kernel split comes from a run of its own:
    rocprofv3 --kernel-trace --stats -- python scripts/raw_column_rate.py --steps 3 --settle 0 --case root"""
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
CASES = {"short": "/text", "container": "/user", "root": ""}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", nargs="*", default=list(CASES))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "raw_column", "raw_column_rate.json"))
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
    tokens = (d_buf, nbytes, d_idx, n, d_type, d_match, d_end, d_flags)
    out.update({"bytes": nbytes, "tokens": n, "documents": lines})
    for name in a.case:
        pointer = CASES[name]
        paths = dev.compile_paths([pointer])
        d_fields = torch.empty((1, lines, 2), dtype=torch.int64, device=dv)
        d_sel = torch.zeros(48, dtype=torch.uint8, device=dv)
        dev.select_documents(paths, *args, d_first, d_docs, d_numbers_result=d_num, d_fields=d_fields, d_result=d_sel, sync=False)
        d_off = torch.empty(lines + 1, dtype=torch.int64, device=dv)
        d_valid = torch.empty(lines, dtype=torch.uint8, device=dv)
        d_res = torch.zeros(48, dtype=torch.uint8, device=dv)
        case = {"pointer": pointer}
        for form, compact in (("verbatim", False), ("compact", True)):
            layout, _, _, _ = dev.raw_column(*tokens, d_fields[0], d_sel, d_offsets=d_off, d_valid=d_valid, compact=compact, text=False)
            assert (layout.code, layout.n_rows, layout.n_values) == (0, lines, lines), (layout.code, layout.n_rows, layout.n_values)
            total = int(layout.total_bytes)
            d_bytes = torch.empty(max(total, 1), dtype=torch.uint8, device=dv)
            res, _, _, _ = dev.raw_column(*tokens, d_fields[0], d_sel, d_offsets=d_off, d_valid=d_valid, d_bytes=d_bytes, compact=compact,
                                          d_result=d_res)
            assert (res.code, res.total_bytes) == (0, total), (res.code, res.total_bytes)

            def column():
                dev.raw_column(*tokens, d_fields[0], d_sel, d_offsets=d_off, d_valid=d_valid, d_bytes=d_bytes, compact=compact, d_result=d_res,
                               sync=False)

            r = timed(column, a.steps, a.settle)
            parts = {"records": 16 * lines, "offsets_and_validity": 9 * lines, "text_read": total, "text_written": total}
            if compact:
                parts["token_arrays_and_sums"] = (10 + 16) * n
            alg = int(sum(parts.values()))
            r.update({"total_bytes": total, "n_containers": int(res.n_containers), "must_move_bytes": alg, "must_move_parts": parts,
                      "must_move_gb_per_s": alg / r["median"] / 1e6, "share_of_8tb_per_s": alg / (r["median"] * 1e-3) / PEAK_BYTES_PER_S,
                      "text_gb_per_s": total / r["median"] / 1e6})
            if name == "root":
                d_copy = torch.empty_like(d_bytes)
                cp = timed(lambda: d_copy.copy_(d_bytes), a.steps, a.settle)
                r.update({"device_copy": cp, "ratio_to_device_copy": r["median"] / cp["median"]})
                del d_copy
            case[form] = r
            print(f"{name} {pointer!r} {form}: {lines} rows, {total} B of text; raw_column {r['median']:.3f} ms (min {r['min']:.3f}, p95 "
                  f"{r['p95']:.3f}), must move {alg / 1e9:.3f} GB -> {r['must_move_gb_per_s']:.0f} GB/s = {100 * r['share_of_8tb_per_s']:.1f} % of "
                  f"8 TB/s" + (f"; device copy of the text {r['device_copy']['median']:.3f} ms, ratio {r['ratio_to_device_copy']:.2f}"
                               if name == "root" else ""), flush=True)
            del d_bytes
        if name == "short":
            slay, s_off, s_valid, _ = dev.string_column(d_buf, nbytes, d_fields, 0, d_sel, strings=False)
            s_bytes = torch.empty(max(int(slay.total_bytes), 1), dtype=torch.uint8, device=dv)
            sc = timed(lambda: dev.string_column(d_buf, nbytes, d_fields, 0, d_sel, d_offsets=s_off, d_valid=s_valid, d_bytes=s_bytes,
                                                 d_result=d_res, sync=False), a.steps, a.settle)
            case["string_column"] = sc
            for form in ("verbatim", "compact"):
                case[form]["ratio_to_string_column"] = case[form]["median"] / sc["median"]
            print(f"short: string_column over the same rows {sc['median']:.3f} ms; ratios {case['verbatim']['ratio_to_string_column']:.2f} "
                  f"(verbatim) {case['compact']['ratio_to_string_column']:.2f} (compact)", flush=True)
            del s_bytes
        out[name] = case
        del d_fields, d_off, d_valid
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
