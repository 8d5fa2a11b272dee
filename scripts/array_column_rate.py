#!/usr/bin/env python3
"""Rate of msj_array_column_device (a selected path's arrays as a list column): the call alone, on the records the select
call left on the device, for three windows --
    tags     /tags on the 1 GiB NDJSON window of scripts/validate_documents_rate.py: two numbers per array
    wide     /v on a window whose lines are {"id":i,"v":[64 numbers]}
    strings  /s on a window whose lines carry an array of 0 .. 7 short strings, half of the lines with an escape; followed by
             msj_string_column_device over the element records with d_elements_select
-- each beside msj_select_documents_device for that one path over the same arrays in the same process, and beside the
bytes the call must move: per pass over the tokens (ac_count, ac_emit) a type byte and a depth word per token, 16 B per
record read and 16 B per descriptor written and read per row, 9 B per row written (an offset and a validity byte), 16 B per
element written; the gathers behind an element (d_idx / d_end / d_flags / d_match, the number record) are counted as 16 B.
Clocks are settled first (2 s of the same calls), then 20 calls, each timed by device events.  Prints and writes (--json,
default profiles/array_column/array_column_rate.json).  The per-kernel split comes from a run of its own:
    rocprofv3 --kernel-trace --stats -- python scripts/array_column_rate.py --steps 3 --settle 0 --case tags"""
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
CASES = {"tags": "/tags", "wide": "/v", "strings": "/s"}


def repeated(lines_of, total_bytes, dev, n=12000):
    block = b"".join(json.dumps(lines_of(i), separators=(",", ":")).encode() + b"\n" for i in range(n))
    nrep = total_bytes // len(block)
    d_block = torch.frombuffer(bytearray(block), dtype=torch.uint8).to(dev.device)
    return d_block.repeat(nrep), len(block) * nrep, n * nrep


def ndjson_wide(total_bytes, dev):
    return repeated(lambda i: {"id": i, "v": [i + j if j % 2 else (i + j) / 4 for j in range(64)]}, total_bytes, dev, 3000)


def ndjson_strings(total_bytes, dev):
    return repeated(lambda i: {"id": i, "s": [("e\n" if i % 2 else "p") + "t" * ((i + j) % 12) for j in range(i % 8)], "ok": True}, total_bytes, dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", nargs="*", default=list(CASES))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "array_column", "array_column_rate.json"))
    a = ap.parse_args()
    dev = Stage1Device(0)
    dv = dev.device
    out = {"library": _lib.load().msj_version().decode()}
    for name in a.case:
        pointer = CASES[name]
        d_buf, nbytes, lines = {"tags": ndjson, "wide": ndjson_wide, "strings": ndjson_strings}[name](a.mib << 20, dev)
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
        _, layout = dev.number_values(d_buf, nbytes, d_idx, n, d_flags, capacity=0)
        ncap = int(layout.n_numbers)
        d_numbers, d_num = dev.number_values(d_buf, nbytes, d_idx, n, d_flags, capacity=ncap, sync=False)
        args = (d_buf, nbytes, d_idx, n, d_type, d_depth, d_match, d_end, d_flags)
        tokens = args[2:]
        d_verdicts = torch.empty((lines, 2), dtype=torch.int64, device=dv)
        _, vres = dev.validate_documents(*args, d_first, d_docs, d_numbers_result=d_num, d_verdicts=d_verdicts)
        assert (vres.code, vres.flags, vres.n_documents, vres.n_invalid) == (0, 0, lines, 0), (vres.code, vres.flags, vres.n_invalid)
        paths = dev.compile_paths([pointer])
        d_fields = torch.empty((1, lines, 2), dtype=torch.int64, device=dv)
        d_sel = torch.zeros(48, dtype=torch.uint8, device=dv)

        def select():
            dev.select_documents(paths, *args, d_first, d_docs, d_numbers=d_numbers, numbers_capacity=ncap, d_numbers_result=d_num,
                                 d_verdicts=d_verdicts, d_fields=d_fields, d_result=d_sel, sync=False)

        select()
        kw = dict(d_numbers=d_numbers, numbers_capacity=ncap, d_numbers_result=d_num)
        first, d_off, d_valid, _, d_esel = dev.array_column(*tokens, d_first, d_docs, d_fields, 0, d_sel, elements=False, **kw)
        assert (first.code, first.n_rows, first.n_arrays) == (0, lines, lines), (first.code, first.n_rows, first.n_arrays)
        total = int(first.n_elements)
        d_elements = torch.empty((max(total, 1), 2), dtype=torch.int64, device=dv)
        d_res = torch.zeros(48, dtype=torch.uint8, device=dv)
        res, _, _, _, _ = dev.array_column(*tokens, d_first, d_docs, d_fields, 0, d_sel, d_offsets=d_off, d_valid=d_valid, d_elements=d_elements,
                                           d_result=d_res, d_elements_select=d_esel, **kw)
        assert (res.code, res.n_elements, res.n_no_bits) == (0, total, 0), (res.code, res.n_elements, res.n_no_bits)

        def column():
            dev.array_column(*tokens, d_first, d_docs, d_fields, 0, d_sel, d_offsets=d_off, d_valid=d_valid, d_elements=d_elements, d_result=d_res,
                             d_elements_select=d_esel, sync=False, **kw)

        r = timed(column, a.steps, a.settle)
        sel = timed(select, a.steps, a.settle)
        parts = {"token_passes": 2 * 5 * n, "records_and_descriptors": (16 + 16 + 16) * lines, "offsets_and_validity": 9 * lines,
                 "element_gathers": 16 * total, "elements_written": 16 * total}
        alg = int(sum(parts.values()))
        r.update({"pointer": pointer, "bytes": nbytes, "tokens": n, "documents": lines, "n_elements": total, "must_move_bytes": alg,
                  "must_move_parts": parts, "must_move_gb_per_s": alg / r["median"] / 1e6,
                  "share_of_8tb_per_s": alg / (r["median"] * 1e-3) / PEAK_BYTES_PER_S, "elements_per_s": total / (r["median"] * 1e-3),
                  "select_documents": sel, "ratio_to_select_documents": r["median"] / sel["median"]})
        print(f"{name} {pointer}: {nbytes} B, {n} tokens, {lines} rows, {total} elements; array_column {r['median']:.3f} ms "
              f"(min {r['min']:.3f}, p95 {r['p95']:.3f}), must move {alg / 1e9:.3f} GB -> {r['must_move_gb_per_s']:.0f} GB/s = "
              f"{100 * r['share_of_8tb_per_s']:.1f} % of 8 TB/s; select_documents for the path {sel['median']:.3f} ms; ratio "
              f"{r['ratio_to_select_documents']:.2f}", flush=True)
        if name == "strings":   # the list<string>: the string column over the element records
            lay, s_off, s_valid, _ = dev.string_column(d_buf, nbytes, d_elements.unsqueeze(0), 0, d_esel, capacity=total, strings=False)
            assert (lay.code, lay.n_rows, lay.n_strings) == (0, total, total), (lay.code, lay.n_rows, lay.n_strings)
            d_bytes = torch.empty(max(int(lay.total_bytes), 1), dtype=torch.uint8, device=dv)
            s_res = torch.zeros(48, dtype=torch.uint8, device=dv)

            def strings():
                dev.string_column(d_buf, nbytes, d_elements.unsqueeze(0), 0, d_esel, d_offsets=s_off, d_valid=s_valid, d_bytes=d_bytes,
                                  capacity=total, d_result=s_res, sync=False)

            s = timed(strings, a.steps, a.settle)
            s.update({"rows": total, "total_bytes": int(lay.total_bytes)})
            r["string_column_over_elements"] = s
            print(f"strings: string_column over the {total} elements, {int(lay.total_bytes)} B: {s['median']:.3f} ms", flush=True)
            del d_bytes, s_off, s_valid
        out[name] = r
        del d_buf, d_idx, d_type, d_depth, d_match, d_end, d_flags, d_first, d_verdicts, d_fields, d_off, d_valid, d_elements, d_numbers, args, tokens, kw
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
