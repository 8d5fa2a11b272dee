#!/usr/bin/env python3
"""Rate of msj_select_elements_device (fields by path inside the elements of a list column): the call alone, on the element
records the array-column call left on the device, over a 1 GiB NDJSON window whose lines hold a list of four small objects
    {"id":i,"meta":{"w":i,"h":1},"items":[{"sku":"s..","qty":..,"dims":{"w":..,"h":2},"a":1,"b":true,"c":null}, ...],"u":"x","v":2}
for 1, 4 and 16 one-segment paths and for one two-segment path (/dims/w) -- each beside msj_select_documents_device with the
same number of paths over the same arrays in the same process: both are one pass over the window per level, so the ratio of
the two shows what the missing depth filter and the search for a key's row cost.  Paths that name no key are part of the 16
on both sides (a list of small objects has no 16 keys).  Clocks are settled first (2 s of the same calls), then 20 calls,
each timed by device events.  Prints and writes (--json, default profiles/select_elements/select_elements_rate.json).  The
per-kernel split comes from a run of its own:
    rocprofv3 --kernel-trace --stats -- python scripts/select_elements_rate.py --steps 3 --settle 0"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mojo_simdjson_amd import _lib  # noqa: E402
from mojo_simdjson_amd.device import Stage1Device  # noqa: E402
from array_column_rate import repeated  # noqa: E402
from validate_documents_rate import timed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABSENT = ["/n%d" % k for k in range(11)]
ELEMENT_PATHS = {"1": ["/sku"], "4": ["/sku", "/qty", "/a", "/b"], "16": ["/sku", "/qty", "/dims", "/a", "/b", "/c"] + ABSENT[:10],
                 "two_segments": ["/dims/w"]}
DOCUMENT_PATHS = {"1": ["/id"], "4": ["/id", "/u", "/v", "/items"], "16": ["/id", "/u", "/v", "/items", "/meta"] + ABSENT,
                  "two_segments": ["/meta/w"]}


def line(i):
    items = [{"sku": "s%d" % (i + j), "qty": i + j, "dims": {"w": j + 0.5, "h": 2}, "a": 1, "b": True, "c": None} for j in range(4)]
    return {"id": i, "meta": {"w": i, "h": 1}, "items": items, "u": "x", "v": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "select_elements", "select_elements_rate.json"))
    a = ap.parse_args()
    dev = Stage1Device(0)
    dv = dev.device
    out = {"library": _lib.load().msj_version().decode()}
    d_buf, nbytes, lines = repeated(line, a.mib << 20, dev, 4000)
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
    kw = dict(d_numbers=d_numbers, numbers_capacity=ncap, d_numbers_result=d_num)
    # the list column of /items: the rows of every timed call
    d_sel, d_cols = dev.select_documents(dev.compile_paths(["/items"]), *args, d_first, d_docs, capacity=lines, sync=False, **kw)
    first, d_off, d_valid, _, d_esel = dev.array_column(*args[2:], d_first, d_docs, d_cols, 0, d_sel, elements=False, **kw)
    assert (first.code, first.n_rows, first.n_arrays) == (0, lines, lines), (first.code, first.n_rows, first.n_arrays)
    rows = int(first.n_elements)
    d_rows = torch.empty((rows, 2), dtype=torch.int64, device=dv)
    res, _, _, _, _ = dev.array_column(*args[2:], d_first, d_docs, d_cols, 0, d_sel, d_offsets=d_off, d_valid=d_valid, d_elements=d_rows,
                                       d_elements_select=d_esel, **kw)
    assert (res.code, res.n_elements) == (0, rows) and rows == 4 * lines, (res.code, res.n_elements, rows)
    out.update({"bytes": nbytes, "tokens": n, "documents": lines, "rows": rows})
    print(f"{nbytes} B, {n} tokens, {lines} documents, {rows} element rows", flush=True)
    for name in ELEMENT_PATHS:
        e_paths, d_paths = dev.compile_paths(ELEMENT_PATHS[name]), dev.compile_paths(DOCUMENT_PATHS[name])
        d_ef = torch.empty((e_paths.n_paths, rows, 2), dtype=torch.int64, device=dv)
        d_df = torch.empty((d_paths.n_paths, lines, 2), dtype=torch.int64, device=dv)
        d_eres, d_dres = torch.zeros(48, dtype=torch.uint8, device=dv), torch.zeros(48, dtype=torch.uint8, device=dv)

        def elements():
            dev.select_elements(e_paths, *args, d_rows, d_esel, d_fields=d_ef, d_result=d_eres, sync=False, **kw)

        def documents():
            dev.select_documents(d_paths, *args, d_first, d_docs, d_fields=d_df, d_result=d_dres, sync=False, **kw)

        elements(), documents()
        eres = _lib.MsjSelectDocumentsResult.from_buffer_copy(d_eres.cpu().numpy().tobytes())
        dres = _lib.MsjSelectDocumentsResult.from_buffer_copy(d_dres.cpu().numpy().tobytes())
        present = sum(p not in ABSENT for p in ELEMENT_PATHS[name])
        assert (eres.code, eres.n_documents, eres.n_found, eres.n_no_bits) == (0, rows, present * rows, 0), (eres.code, eres.n_found)
        assert (dres.code, dres.n_documents) == (0, lines), (dres.code, dres.n_documents)
        r, d = timed(elements, a.steps, a.settle), timed(documents, a.steps, a.settle)
        levels = 2 if name == "two_segments" else 1
        r.update({"paths": ELEMENT_PATHS[name], "levels": levels, "ms_per_level": r["median"] / levels, "select_documents": d,
                  "document_paths": DOCUMENT_PATHS[name], "ratio_to_select_documents": r["median"] / d["median"],
                  "fields_per_s": e_paths.n_paths * rows / (r["median"] * 1e-3)})
        print(f"{name}: select_elements {r['median']:.3f} ms (min {r['min']:.3f}, p95 {r['p95']:.3f}) for {e_paths.n_paths} path(s) x {rows} rows; "
              f"select_documents {d['median']:.3f} ms for {d_paths.n_paths} path(s) x {lines} documents; ratio "
              f"{r['ratio_to_select_documents']:.2f}", flush=True)
        out[name] = r
        del d_ef, d_df
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
