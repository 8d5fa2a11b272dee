#!/usr/bin/env python3
"""Rate of msj_dictionary_extend_device (one dictionary across windows): the call alone, on the columns of
scripts/dictionary_rate.py's synthetic 1 GiB NDJSON window of lines
    {"id":"0000001234","status":"s07","n":4}
    status_all_prior   /status against the 37 values it has: every row matches a prior entry, nothing is appended
    id_none_prior      /id with P = 0: every row is a new value (the work of msj_dictionary_device)
    id_all_miss        /id against as many prior entries as rows, none of which any row has: every item is hashed and
                       inserted, the table is sized for twice the items, every row is appended
and the frozen form of each (MSJ_DICTIONARY_FROZEN: the rows look up only).  Each is reported in ms and as a ratio to
msj_dictionary_device over the same column in the same process -- that call is the yardstick.
Clocks are settled first (--settle seconds of the same calls), then --steps calls, each timed by device events.  Prints and
writes (--json, default profiles/dictionary_extend/dictionary_extend_rate.json).  The per-kernel split comes from a run of
its own:
    rocprofv3 --kernel-trace --stats -- python scripts/dictionary_extend_rate.py --steps 3 --settle 0 --case status"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mojo_simdjson_amd import _lib  # noqa: E402
from mojo_simdjson_amd.device import Stage1Device  # noqa: E402
from dictionary_rate import STATUSES, ndjson  # noqa: E402
from validate_documents_rate import timed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", nargs="*", default=["status", "id"])
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "dictionary_extend", "dictionary_extend_rate.json"))
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
    paths = dev.compile_paths(["/status", "/id"])
    d_fields = torch.empty((2, lines, 2), dtype=torch.int64, device=dv)
    d_sel = torch.zeros(48, dtype=torch.uint8, device=dv)
    dev.select_documents(paths, *args, d_first, d_docs, d_numbers_result=d_num, d_fields=d_fields, d_result=d_sel, sync=False)
    del d_type, d_depth, d_match, d_end, d_flags, d_first
    rows = lines
    for name in a.case:
        p = ("status", "id").index(name)
        slay, d_off, d_valid, d_bytes = dev.string_column(d_buf, nbytes, d_fields, p, d_sel)
        total = int(slay.total_bytes)
        assert (slay.code, slay.n_rows, slay.n_strings) == (0, rows, rows), (slay.code, slay.n_rows, slay.n_strings)
        first, d_codes, d_doff, d_dfirst, d_dbytes = dev.dictionary(d_off, d_bytes, d_valid, rows=rows, bytes_len=total)
        n_distinct, dict_bytes = int(first.n_distinct), int(first.dict_bytes)
        assert (first.code, first.n_values, n_distinct) == (0, rows, {"status": STATUSES, "id": lines}[name])
        d_res = torch.zeros(48, dtype=torch.uint8, device=dv)

        def dictionary():
            dev.dictionary(d_off, d_bytes, d_valid, rows=rows, bytes_len=total, d_codes=d_codes, d_dict_offsets=d_doff, d_dict_first=d_dfirst,
                           d_dict_bytes=d_dbytes, d_result=d_res, sync=False)

        yardstick = timed(dictionary, a.steps, a.settle)
        print(f"{name}: {rows} rows, {total} B, {n_distinct} distinct; msj_dictionary_device {yardstick['median']:.3f} ms", flush=True)
        out[name + "_dictionary"] = dict(yardstick, rows=rows, column_bytes=total, n_distinct=n_distinct)
        if name == "status":   # the dictionary the yardstick left is the prior one: every row matches
            cases = [("status_all_prior", n_distinct, d_doff, d_dfirst, d_dbytes, n_distinct, rows, n_distinct)]
        else:
            width = dict_bytes // n_distinct
            x_off = torch.zeros(2 * rows + 1, dtype=torch.int64, device=dv)
            x_first = torch.zeros(2 * rows, dtype=torch.int32, device=dv)
            x_bytes = torch.zeros(2 * dict_bytes, dtype=torch.uint8, device=dv)
            x_off[:rows + 1], x_bytes[:dict_bytes] = d_doff[:rows + 1], d_dbytes[:dict_bytes]
            x_bytes[:dict_bytes].view(rows, width)[:, 0] = ord("x")   # prior entries no row has
            cases = [("id_none_prior", 0, d_doff, d_dfirst, d_dbytes, rows, 0, 0),
                     ("id_all_miss", rows, x_off, x_first, x_bytes, 2 * rows, 0, rows)]
        d_xres = torch.zeros(64, dtype=torch.uint8, device=dv)
        for case, P, t_off, t_first, t_bytes, want_distinct, want_matched, frozen_distinct in cases:
            for frozen in (False, True):
                def extend():
                    dev.dictionary_extend(d_off, d_bytes, d_valid, t_off, t_first, t_bytes, n_prior=P, rows=rows, bytes_len=total, d_codes=d_codes,
                                          frozen=frozen, d_result=d_xres, sync=False)

                r = timed(extend, a.steps, a.settle)
                last = _lib.MsjDictionaryExtendResult.from_buffer_copy(d_xres.cpu().numpy().tobytes())
                assert (last.code, last.n_prior, last.n_values, last.n_matched) == (0, P, rows, want_matched), (last.code, last.n_matched)
                assert last.n_distinct == (frozen_distinct if frozen else want_distinct), last.n_distinct
                label = case + ("_frozen" if frozen else "")
                r.update({"rows": rows, "n_prior": P, "n_distinct": int(last.n_distinct), "n_matched": int(last.n_matched),
                          "max_probe": int(last.max_probe), "ratio_to_dictionary": r["median"] / yardstick["median"],
                          "workspace_bytes": int(dev.lib.msj_dictionary_extend_workspace_bytes(rows, t_first.numel()))})
                out[label] = r
                print(f"{label}: P {P}, {rows} rows; {r['median']:.3f} ms (min {r['min']:.3f}, p95 {r['p95']:.3f}), max_probe {last.max_probe}; "
                      f"ratio to msj_dictionary_device over the same column {r['ratio_to_dictionary']:.2f}", flush=True)
        del d_off, d_valid, d_bytes, d_codes, d_doff, d_dfirst, d_dbytes, cases
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
