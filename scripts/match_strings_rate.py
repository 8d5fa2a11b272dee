#!/usr/bin/env python3
"""Rate of msj_match_strings_device (substring patterns over a byte column): the call alone, on columns the string and raw
column calls left on the device, over one synthetic 1 GiB NDJSON window of lines
    {"id":"0000001234","status":"s07","message":"..."}
whose messages are 40 to 200 bytes of log-like text (a block of 12 000 lines, repeated) --
    rare      one single-piece pattern that 1 line in 1 000 holds, over /message
    short     the same pattern over /status (three bytes a row)
    common    the one-byte piece "e": a hit at about every tenth byte, the atomic-heavy case
    like      a three-piece AT_END pattern (GET %/img/%.png) over /message
    sixteen   16 single-piece patterns in one call over /message
    grep      one pattern over raw(""): the lines themselves
Each is reported in ms and as a ratio of three yardsticks measured in the same process: the msj_string_column_device /
msj_raw_column_device call that wrote its input, a device-to-device copy of the column's bytes, and MSJ_PRED_STR_PREFIX
through msj_filter_rows_device on the same rows.
Clocks are settled first (1 s of the same calls), then 20 calls, each timed by device events.  Prints and writes (--json,
default profiles/match_strings/match_strings_rate.json).  The per-kernel split comes from a run of its own:
    rocprofv3 --kernel-trace --stats -- python scripts/match_strings_rate.py --steps 3 --settle 0 --case rare sixteen"""
import argparse
import json
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mojo_simdjson_amd import _lib  # noqa: E402
from mojo_simdjson_amd.device import Stage1Device  # noqa: E402
from validate_documents_rate import timed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = ("request", "served", "from", "cache", "upstream", "replied", "in", "ms", "user", "session", "renewed", "GET /img/logo.png",
         "POST /api/v1/orders", "connection", "closed", "by", "peer", "retry", "scheduled", "disk", "usage", "at", "percent", "ok")
RARE = ("timeout", "deadlock", "segfault", "overflow", "corrupt", "evicted", "throttled", "panic", "unreachable", "expired", "refused",
        "rollback", "checksum", "quorum", "stalled", "poisoned")
BLOCK_LINES = 12000


def ndjson(total_bytes, dev):
    """The window: a block of 12 000 lines made on the host, repeated on the device -> (d_buf, its bytes, its lines)"""
    rng = random.Random(1)
    lines = []
    for k in range(BLOCK_LINES):
        words = []
        while sum(len(w) + 1 for w in words) < rng.randrange(40, 200):
            words.append(rng.choice(WORDS))
        if k % 1000 == 7:
            words.insert(rng.randrange(len(words)), RARE[(k // 1000) % len(RARE)])
        lines.append(json.dumps({"id": "%010d" % k, "status": "s%02d" % (k * 7919 % 37), "message": " ".join(words)}, separators=(",", ":")).encode())
    block = b"\n".join(lines) + b"\n"
    nrep = total_bytes // len(block)
    d_block = torch.frombuffer(bytearray(block), dtype=torch.uint8).to(dev.device)
    return d_block.repeat(nrep), len(block) * nrep, BLOCK_LINES * nrep


CASES = {"rare": ("/message", [b"timeout"]), "short": ("/status", [b"timeout"]), "common": ("/message", [b"e"]),
         "like": ("/message", [([b"GET ", b"/img/", b".png"], {"at_end"})]), "sixteen": ("/message", [w.encode() for w in RARE]),
         "grep": ("", [b"timeout"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", nargs="*", default=list(CASES))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "match_strings", "match_strings_rate.json"))
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
    pointers = ["/message", "/status", ""]
    paths = dev.compile_paths(pointers)
    d_fields = torch.empty((3, lines, 2), dtype=torch.int64, device=dv)
    d_sel = torch.zeros(48, dtype=torch.uint8, device=dv)
    dev.select_documents(paths, *args, d_first, d_docs, d_numbers_result=d_num, d_fields=d_fields, d_result=d_sel, sync=False)
    columns = {}
    for name in a.case:
        pointer, specs = CASES[name]
        p = pointers.index(pointer)
        if pointer not in columns:  # the column and its yardsticks, once
            d_cres = torch.zeros(48, dtype=torch.uint8, device=dv)
            if pointer == "":
                lay, d_off, d_valid, _ = dev.raw_column(d_buf, nbytes, d_idx, n, d_type, d_match, d_end, d_flags, d_fields[p], d_sel, text=False)
                total = int(lay.total_bytes)
                d_bytes = torch.empty(max(total, 1), dtype=torch.uint8, device=dv)

                def column():
                    dev.raw_column(d_buf, nbytes, d_idx, n, d_type, d_match, d_end, d_flags, d_fields[p], d_sel, d_offsets=d_off, d_valid=d_valid,
                                   d_bytes=d_bytes, d_result=d_cres, sync=False)
            else:
                lay, d_off, d_valid, _ = dev.string_column(d_buf, nbytes, d_fields, p, d_sel, strings=False)
                total = int(lay.total_bytes)
                d_bytes = torch.empty(max(total, 1), dtype=torch.uint8, device=dv)

                def column(p=p, d_off=d_off, d_valid=d_valid, d_bytes=d_bytes, d_cres=d_cres):
                    dev.string_column(d_buf, nbytes, d_fields, p, d_sel, d_offsets=d_off, d_valid=d_valid, d_bytes=d_bytes, d_result=d_cres, sync=False)
            col = timed(column, a.steps, a.settle)
            d_copy = torch.empty_like(d_bytes)
            copy = timed(lambda: d_copy.copy_(d_bytes), a.steps, a.settle)
            del d_copy
            predicates = dev.compile_predicates([(0, "prefix", "timeout")])
            d_keep, d_kept = torch.empty(lines, dtype=torch.uint8, device=dv), torch.empty(lines, dtype=torch.int32, device=dv)
            d_fres, d_ksel = torch.zeros(48, dtype=torch.uint8, device=dv), torch.zeros(48, dtype=torch.uint8, device=dv)
            prefix = timed(lambda: dev.filter_rows(predicates, d_buf, nbytes, d_fields[p:p + 1], d_sel, capacity=lines, d_keep=d_keep, d_kept=d_kept,
                                                   d_result=d_fres, d_kept_select=d_ksel, sync=False), a.steps, a.settle)
            columns[pointer] = (d_off, d_valid, d_bytes, total, col, copy, prefix, d_cres)
        d_off, d_valid, d_bytes, total, col, copy, prefix, d_cres = columns[pointer]
        patterns = dev.compile_patterns(specs)
        d_out = torch.empty((len(specs), lines, 2), dtype=torch.int64, device=dv)
        d_res, d_msel = torch.zeros(48, dtype=torch.uint8, device=dv), torch.zeros(48, dtype=torch.uint8, device=dv)
        d_n_rows = d_cres[8:16].view(torch.int64)  # the rows as the column call left them on the device

        def match():
            dev.match_strings(patterns, d_off, d_valid, d_bytes, rows=lines, d_n_rows=d_n_rows, bytes_len=total, d_fields=d_out, d_result=d_res,
                              d_select=d_msel, sync=False)

        r = timed(match, a.steps, a.settle)
        last = _lib.MsjMatchStringsResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
        assert (last.code, last.n_rows) == (0, lines), (last.code, last.n_rows)
        r.update({"rows": lines, "column_bytes": total, "patterns": len(specs), "max_pieces": int(last.max_pieces), "n_matched": int(last.n_matched),
                  "column_call": col, "copy": copy, "prefix_filter": prefix, "ratio_to_column_call": r["median"] / col["median"],
                  "ratio_to_copy": r["median"] / copy["median"], "ratio_to_prefix_filter": r["median"] / prefix["median"],
                  "gb_per_s": total / r["median"] / 1e6, "workspace_bytes": int(dev.lib.msj_match_strings_workspace_bytes(lines, len(specs)))})
        out[name] = r
        print(f"{name}: {lines} rows, {total} B, {len(specs)} patterns, {last.n_matched} matched; match {r['median']:.3f} ms (min {r['min']:.3f}, p95 "
              f"{r['p95']:.3f}) = {r['gb_per_s']:.0f} GB/s; column call {col['median']:.3f} ms (ratio {r['ratio_to_column_call']:.2f}), copy "
              f"{copy['median']:.3f} ms ({r['ratio_to_copy']:.2f}), prefix filter {prefix['median']:.3f} ms ({r['ratio_to_prefix_filter']:.2f})", flush=True)
        del d_out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
