#!/usr/bin/env python3
"""Rate of msj_object_entries_device (an object's members as a map column): the call alone, on the rows the calls in front of
it left on the device, over one 1 GiB NDJSON window whose lines hold "attrs" -- an object of four members -- and "tags" -- a
list of four elements of the same kinds --, and "items", two small objects with a "dims" object and a "tags" list of two
members each.  Two runs:
    attrs   the call over the /attrs column of the documents (msj_select_documents_device's d_fields): a map per document
    dims    the call over the /dims column of /items (msj_select_elements_device's d_fields): a map inside a list of structs
-- each beside msj_array_elements_device over the /tags column of the same rows in the same process, which is the yardstick:
the same row count, the same number of entries as elements, the same kernels over rows; this call looks one token behind
a candidate instead of in front of it, gathers the value's arrays at i + 2 and writes two records per entry.
Clocks are settled first (2 s of the same calls), then 20 calls, each timed by device events; the median counts.  Prints and
writes (--json, default profiles/object_entries/object_entries_rate.json).  The per-kernel split comes from a run of its own:
    rocprofv3 --kernel-trace --stats -- python scripts/object_entries_rate.py --steps 3 --settle 0 --case attrs"""
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
    kinds = lambda j: ["red%d" % (j % 7), "L" * (1 + (i + j) % 5), (i + j) % 1000, 0.5 + (i * j) % 89][j]
    return {"id": i, "attrs": {"color": kinds(0), "size": kinds(1), "qty": kinds(2), "weight": kinds(3)}, "tags": [kinds(j) for j in range(4)],
            "items": [{"sku": "s%d" % ((i + j) % 1000), "dims": {"w": (i + j) % 90, "h": "h%d" % (j % 7)}, "tags": [(i + j) % 90, "h%d" % (j % 7)]}
                      for j in range(2)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", nargs="*", default=["attrs", "dims"])
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "object_entries", "object_entries_rate.json"))
    a = ap.parse_args()
    dev = Stage1Device(0)
    dv = dev.device
    d_buf, nbytes, lines = repeated(line, a.mib << 20, dev, 6000)
    d_idx = torch.empty(nbytes + 1024, dtype=torch.int32, device=dv)
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
    d_sel, d_fields = dev.select_documents(dev.compile_paths(["/attrs", "/tags", "/items"]), *args, d_first, d_docs, capacity=lines, sync=False, **kw)
    out = {"library": _lib.load().msj_version().decode(), "bytes": nbytes, "tokens": n, "documents": lines}
    for name in ("attrs", "dims"):
        if name not in a.case:
            continue
        if name == "attrs":   # the rows are the documents: two columns of the select call
            rows, d_maps, d_lists, d_rows_sel = lines, d_fields[0], d_fields[1], d_sel
        else:                 # the rows are the elements of /items: two columns of a select-elements call over them
            first, _, _, _, d_esel = dev.array_column(*tokens, d_first, d_docs, d_fields, 2, d_sel, elements=False, **kw)
            rows = int(first.n_elements)
            _, _, _, d_parents, d_esel = dev.array_column(*tokens, d_first, d_docs, d_fields, 2, d_sel, elements_capacity=rows, **kw)
            d_rows_sel, d_cols = dev.select_elements(dev.compile_paths(["/dims", "/tags"]), *args, d_parents, d_esel, capacity=rows, sync=False, **kw)
            d_maps, d_lists = d_cols[0], d_cols[1]
        lay, m_off, m_valid, _, _, k_sel, v_sel = dev.object_entries(*tokens, d_maps, d_rows_sel, capacity=rows, entries=False, **kw)
        assert (lay.code, lay.n_rows, lay.n_objects) == (0, rows, rows), (lay.code, lay.n_rows, lay.n_objects)
        total = int(lay.n_entries)
        d_keys, d_values = (torch.empty((total, 2), dtype=torch.int64, device=dv) for _ in range(2))
        m_res = torch.zeros(48, dtype=torch.uint8, device=dv)

        def entries():
            dev.object_entries(*tokens, d_maps, d_rows_sel, d_offsets=m_off, d_valid=m_valid, d_keys=d_keys, d_values=d_values, capacity=rows,
                               d_result=m_res, d_keys_select=k_sel, d_values_select=v_sel, sync=False, **kw)

        entries()
        res = _lib.MsjObjectEntriesResult.from_buffer_copy(m_res.cpu().numpy().tobytes())
        assert (res.code, res.n_entries, res.n_no_bits) == (0, total, 0), (res.code, res.n_entries, res.n_no_bits)
        # the yardstick: msj_array_elements_device over the /tags column of the same rows
        lay, e_off, e_valid, _, e_sel = dev.array_elements(*tokens, d_lists, d_rows_sel, capacity=rows, elements=False, **kw)
        assert (lay.code, lay.n_rows, lay.n_arrays, lay.n_elements) == (0, rows, rows, total), (lay.code, lay.n_rows, lay.n_arrays, lay.n_elements)
        d_elements = torch.empty((total, 2), dtype=torch.int64, device=dv)
        e_res = torch.zeros(48, dtype=torch.uint8, device=dv)

        def elements():
            dev.array_elements(*tokens, d_lists, d_rows_sel, d_offsets=e_off, d_valid=e_valid, d_elements=d_elements, capacity=rows,
                               d_result=e_res, d_elements_select=e_sel, sync=False, **kw)

        elements()
        r = timed(entries, a.steps, a.settle)
        el = timed(elements, a.steps, a.settle)
        r.update({"rows": rows, "n_entries": total, "entries_per_s": total / (r["median"] * 1e-3), "array_elements": el,
                  "ratio_to_array_elements": r["median"] / el["median"]})
        print(f"{name}: {nbytes} B, {n} tokens, {rows} rows, {total} entries; object_entries {r['median']:.3f} ms (min {r['min']:.3f}, p95 "
              f"{r['p95']:.3f}); array_elements over /tags of the same rows ({total} elements) {el['median']:.3f} ms; ratio "
              f"{r['ratio_to_array_elements']:.2f}", flush=True)
        out[name] = r
        del d_keys, d_values, d_elements, m_off, m_valid, e_off, e_valid
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
