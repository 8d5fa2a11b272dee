#!/usr/bin/env python3
"""Rate of msj_array_elements_device (the arrays inside list rows as a list column): the call alone, on the rows the calls in
front of it left on the device, over one 1 GiB NDJSON window whose lines hold "coordinates" -- a list of four [x,y] pairs --
and "items" -- four small objects, each with a "tags" list of two strings.  Two runs:
    coordinates  the call over the elements of /coordinates (msj_array_column_device's d_elements): a list of lists
    tags         the call over the /tags column of /items (msj_select_elements_device's d_fields): a list inside a list of
                 structs
-- each beside msj_array_column_device over the same arrays in the same process (the path the rows came from), which is the
yardstick: both calls are two passes over the tokens, this one adds the row compaction and an LDS search per candidate.
Clocks are settled first (2 s of the same calls), then 20 calls, each timed by device events.  Prints and writes (--json,
default profiles/array_elements/array_elements_rate.json).  The per-kernel split comes from a run of its own:
    rocprofv3 --kernel-trace --stats -- python scripts/array_elements_rate.py --steps 3 --settle 0 --case coordinates"""
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


def line(i):
    return {"id": i, "coordinates": [[-122.4 + (i + j) % 97 / 100, 37.7 + (i * j) % 89 / 100] for j in range(4)],
            "items": [{"sku": "s%d" % ((i + j) % 1000), "tags": ["t%d" % (j % 7), "u" * (1 + (i + j) % 5)]} for j in range(4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", nargs="*", default=["coordinates", "tags"])
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "array_elements", "array_elements_rate.json"))
    a = ap.parse_args()
    dev = Stage1Device(0)
    dv = dev.device
    d_buf, nbytes, lines = repeated(line, a.mib << 20, dev, 6000)
    d_idx = torch.empty(nbytes + 1024, dtype=torch.int32, device=dv)   # (compact arrays of numbers: more than a token per two bytes)
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
    kw = dict(d_numbers=d_numbers, numbers_capacity=ncap, d_numbers_result=d_num)
    d_sel, d_fields = dev.select_documents(dev.compile_paths(["/coordinates", "/items"]), *args, d_first, d_docs, capacity=lines, sync=False, **kw)
    out = {"library": _lib.load().msj_version().decode(), "bytes": nbytes, "tokens": n, "documents": lines}
    for name, p in (("coordinates", 0), ("tags", 1)):
        if name not in a.case:
            continue
        # the parent list column, complete, and its own rate over these arrays: the yardstick
        first, d_off, d_valid, _, d_esel = dev.array_column(*tokens, d_first, d_docs, d_fields, p, d_sel, elements=False, **kw)
        assert (first.code, first.n_rows, first.n_arrays) == (0, lines, lines), (first.code, first.n_rows, first.n_arrays)
        parents = int(first.n_elements)
        d_parents = torch.empty((parents, 2), dtype=torch.int64, device=dv)
        d_res = torch.zeros(48, dtype=torch.uint8, device=dv)

        def column():
            dev.array_column(*tokens, d_first, d_docs, d_fields, p, d_sel, d_offsets=d_off, d_valid=d_valid, d_elements=d_parents, d_result=d_res,
                             d_elements_select=d_esel, sync=False, **kw)

        column()
        d_rows, d_rows_sel = d_parents, d_esel
        if name == "tags":
            d_rows_sel, d_tags = dev.select_elements(dev.compile_paths(["/tags"]), *args, d_parents, d_esel, capacity=parents, sync=False, **kw)
            d_rows = d_tags[0]
        lay, e_off, e_valid, _, e_sel = dev.array_elements(*tokens, d_rows, d_rows_sel, capacity=parents, elements=False, **kw)
        assert (lay.code, lay.n_rows, lay.n_arrays) == (0, parents, parents), (lay.code, lay.n_rows, lay.n_arrays)
        total = int(lay.n_elements)
        d_elements = torch.empty((total, 2), dtype=torch.int64, device=dv)
        e_res = torch.zeros(48, dtype=torch.uint8, device=dv)

        def elements():
            dev.array_elements(*tokens, d_rows, d_rows_sel, d_offsets=e_off, d_valid=e_valid, d_elements=d_elements, capacity=parents,
                               d_result=e_res, d_elements_select=e_sel, sync=False, **kw)

        elements()
        res = _lib.MsjArrayColumnResult.from_buffer_copy(e_res.cpu().numpy().tobytes())
        assert (res.code, res.n_elements, res.n_no_bits) == (0, total, 0) and total == 2 * parents, (res.code, res.n_elements, res.n_no_bits)
        r = timed(elements, a.steps, a.settle)
        col = timed(column, a.steps, a.settle)
        r.update({"rows": parents, "n_elements": total, "elements_per_s": total / (r["median"] * 1e-3), "array_column": col,
                  "array_column_elements": parents, "ratio_to_array_column": r["median"] / col["median"]})
        print(f"{name}: {nbytes} B, {n} tokens, {parents} rows, {total} elements; array_elements {r['median']:.3f} ms (min {r['min']:.3f}, p95 "
              f"{r['p95']:.3f}); array_column over the same arrays ({lines} rows, {parents} elements) {col['median']:.3f} ms; ratio "
              f"{r['ratio_to_array_column']:.2f}", flush=True)
        out[name] = r
        del d_parents, d_rows, d_elements, d_off, d_valid, e_off, e_valid
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
