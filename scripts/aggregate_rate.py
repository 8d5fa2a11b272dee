#!/usr/bin/env python3
"""Rate of msj_aggregate_device (count, sum, min, max per group): the call alone, on records and codes the earlier calls left
on the device, over the synthetic 1 GiB NDJSON window of scripts/dictionary_rate.py, lines of
    {"id":"0000001234","status":"s07","n":4}
The aggregated column is /n (an int64 per line); the groups are
    status    /n by /status: 37 groups, the few-groups case the LDS path is for
    id        /n by /id: every row a group of its own, the global path
    ungrouped /n with no codes: one group, every wave of one group
Each is reported in ms and rows per microsecond, and against four yardsticks over the same rows: the msj_dictionary_device
call that made its codes (none for `ungrouped`); a device-to-device copy of the records (16 bytes per row: the least the call
has to read, twice); torch's bincount + index_add_ on float64 (count and sum alone, not exact, not reproducible); and the
same call with the LDS path switched off by msj_debug_set_aggregate_limits(0).  The records of the two paths are compared
byte for byte.
Clocks are settled first (2 s of the same calls), then 20 calls, each timed by device events.  Prints and writes (--json,
default profiles/aggregate/aggregate_rate.json)."""
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
from dictionary_rate import STATUSES, ndjson  # noqa: E402
from validate_documents_rate import timed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", nargs="*", default=["status", "id", "ungrouped"])
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "aggregate", "aggregate_rate.json"))
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
    paths = dev.compile_paths(["/status", "/id", "/n"])
    d_fields = torch.empty((3, lines, 2), dtype=torch.int64, device=dv)
    d_sel = torch.zeros(48, dtype=torch.uint8, device=dv)
    sel, _ = dev.select_documents(paths, *args, d_first, d_docs, d_numbers=d_numbers, numbers_capacity=lines, d_numbers_result=d_num,
                                  d_fields=d_fields, d_result=d_sel)
    assert (sel.code, sel.n_found, sel.n_no_bits) == (0, 3 * lines, 0), (sel.code, sel.n_found, sel.n_no_bits)
    d_n = d_fields[2]
    d_copy = torch.empty_like(d_n)
    copy = timed(lambda: d_copy.copy_(d_n), a.steps, a.settle)
    values, valid = number_column(d_n, torch.float64)
    assert bool(valid.all())
    want_sum = int(d_n[:, 0].sum().item())
    for name in a.case:
        r = {}
        if name == "ungrouped":
            d_codes, G = None, 1
        else:
            p = ("status", "id").index(name)
            slay, d_off, d_valid, _ = dev.string_column(d_buf, nbytes, d_fields, p, d_sel, strings=False)
            d_bytes = torch.empty(max(int(slay.total_bytes), 1), dtype=torch.uint8, device=dv)
            dev.string_column(d_buf, nbytes, d_fields, p, d_sel, d_offsets=d_off, d_valid=d_valid, d_bytes=d_bytes, sync=False)
            first, d_codes, d_doff, d_dfirst, d_dbytes = dev.dictionary(d_off, d_bytes, d_valid, rows=lines, bytes_len=int(slay.total_bytes))
            G = int(first.n_distinct)
            assert (first.code, G) == (0, {"status": STATUSES, "id": lines}[name])
            d_dres = torch.zeros(48, dtype=torch.uint8, device=dv)

            def dictionary():
                dev.dictionary(d_off, d_bytes, d_valid, rows=lines, bytes_len=int(slay.total_bytes), d_codes=d_codes, d_dict_offsets=d_doff,
                               d_dict_first=d_dfirst, d_dict_bytes=d_dbytes, d_result=d_dres, sync=False)

            r["dictionary"] = timed(dictionary, a.steps, a.settle)
        d_groups = [torch.zeros(G * 48, dtype=torch.uint8, device=dv) for _ in range(2)]
        d_res = torch.zeros(48, dtype=torch.uint8, device=dv)
        d_n_groups = None if d_codes is None else d_dres[24:32].view(torch.int64)   # n_distinct where the dictionary call left it

        def aggregate(which):
            dev.aggregate(d_n, d_sel, d_codes, n_groups=G, d_n_groups=d_n_groups, d_groups=d_groups[which], groups_capacity=G, d_result=d_res,
                          sync=False)

        dev.set_aggregate_limits()
        r.update(timed(lambda: aggregate(0), a.steps, a.settle))
        last = _lib.MsjAggregateResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
        assert (last.code, last.n_rows, last.n_groups, last.n_ungrouped, last.n_values) == (0, lines, G, 0, lines), (last.code, last.n_groups, last.n_values)
        dev.set_aggregate_limits(0)
        r["lds_off"] = timed(lambda: aggregate(1), a.steps, a.settle)
        dev.set_aggregate_limits()
        assert torch.equal(d_groups[0], d_groups[1]), "the two paths differ"
        words = d_groups[0].view(torch.int64).view(G, 6)
        assert int(words[:, 0].sum().item()) == lines and int(words[:, 2].sum().item()) == want_sum and bool((d_groups[0].view(G, 48)[:, 40] == ord("l")).all())
        codes64 = torch.zeros(lines, dtype=torch.int64, device=dv) if d_codes is None else d_codes.to(torch.int64)

        def with_torch():
            torch.bincount(codes64, minlength=G)
            torch.zeros(G, dtype=torch.float64, device=dv).index_add_(0, codes64, values)

        r["torch_bincount_index_add"] = timed(with_torch, a.steps, a.settle)
        r.update({"rows": lines, "groups": G, "copy_records": copy, "rows_per_us": lines / r["median"] / 1e3,
                  "ratio_to_copy": r["median"] / copy["median"], "ratio_to_torch": r["median"] / r["torch_bincount_index_add"]["median"],
                  "ratio_to_lds_off": r["median"] / r["lds_off"]["median"],
                  "workspace_bytes": int(dev.lib.msj_aggregate_workspace_bytes(lines, G, 1))})
        if "dictionary" in r:
            r["ratio_to_dictionary"] = r["median"] / r["dictionary"]["median"]
        out[name] = r
        print(f"{name}: {lines} rows, {G} groups; aggregate {r['median']:.3f} ms (min {r['min']:.3f}, p95 {r['p95']:.3f}) = {r['rows_per_us']:.0f} "
              f"rows/us; LDS off {r['lds_off']['median']:.3f} ms; copy of the records {copy['median']:.3f} ms; torch bincount + index_add_ "
              f"{r['torch_bincount_index_add']['median']:.3f} ms; dictionary {r.get('dictionary', {}).get('median', float('nan')):.3f} ms", flush=True)
        del d_groups, codes64
        if d_codes is not None:
            del d_off, d_valid, d_bytes, d_codes, d_doff, d_dfirst, d_dbytes
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
