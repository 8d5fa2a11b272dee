#!/usr/bin/env python3
"""Rate of msj_select_documents_device (fields by path for every document of a window): the call alone on the 1 GiB NDJSON
window of scripts/validate_documents_rate.py with 1 path of depth 1, 8 paths of depth 1 (four of them absent) and 4 paths of
depth 3 (the lines nest two deep: their third level has no key, so its pass ends at the candidate test) -- each beside
msj_validate_documents_device over the same arrays in the same process, and beside the bytes the call must move: 5 B per
token per level (type and depth), 9 B plus the key's bytes per candidate (a string at the level's depth with ':' behind it:
d_idx, d_end, d_flags), 16 B per record.
Clocks are settled first (2 s of the same calls), then 20 calls, each timed by device events.  Prints and writes (--json,
default profiles/r11/select_documents_rate_r11.json).  The per-kernel split comes from a run of its own:
    rocprofv3 --kernel-trace --stats -- python scripts/select_documents_rate.py --steps 3 --settle 0 --case paths_8_depth_1"""
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
CASES = {"paths_1_depth_1": ["/id"],
         "paths_8_depth_1": ["/id", "/text", "/tags", "/user", "/lang", "/ts", "/geo", "/i"],
         "paths_4_depth_3": ["/user/name/first", "/user/ok/x", "/user/none/x", "/tags/0/1"]}


def candidates(d_type, d_depth, d_idx, d_end, n, level):
    """Strings at depth level + 1 with ':' behind them, and the bytes of their bodies"""
    t = d_type[:n]
    is_key = (t[:-1] == ord('"')) & (t[1:] == ord(":")) & (d_depth[:n - 1] == level + 1)
    count = int(is_key.sum().item())
    body = (d_end[:n - 1].long() - d_idx[:n - 1].long() - 1)[is_key]
    return count, int(body.sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", nargs="*", default=list(CASES))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "r11", "select_documents_rate_r11.json"))
    a = ap.parse_args()
    dev = Stage1Device(0)
    dv = dev.device
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
    _, num = dev.number_values(d_buf, nbytes, d_idx, n, d_flags, capacity=0)
    cap = int(num.n_numbers)
    d_numbers, d_num = dev.number_values(d_buf, nbytes, d_idx, n, d_flags, capacity=cap, sync=False)
    args = (d_buf, nbytes, d_idx, n, d_type, d_depth, d_match, d_end, d_flags)
    d_verdicts = torch.empty((lines, 2), dtype=torch.int64, device=dv)
    d_vres = torch.zeros(48, dtype=torch.uint8, device=dv)
    _, vres = dev.validate_documents(*args, d_first, d_docs, d_numbers_result=d_num, d_verdicts=d_verdicts)
    assert (vres.code, vres.flags, vres.n_documents, vres.n_invalid) == (0, 0, lines, 0), (vres.code, vres.flags, vres.n_invalid)

    def verdicts():
        dev.validate_documents(*args, d_first, d_docs, d_numbers_result=d_num, d_verdicts=d_verdicts, d_result=d_vres, sync=False)

    out = {"library": _lib.load().msj_version().decode(), "bytes": nbytes, "tokens": n, "documents": lines, "numbers": cap}
    out["validate_documents"] = timed(verdicts, a.steps, a.settle)
    per_level = [candidates(d_type, d_depth, d_idx, d_end, n, level) for level in range(3)]
    out["candidates_per_level"] = [{"keys": c, "key_bytes": b} for c, b in per_level]
    for name in a.case:
        pointers = CASES[name]
        paths = dev.compile_paths(pointers)
        levels = max(p.count("/") for p in pointers)
        d_fields = torch.empty((len(pointers), lines, 2), dtype=torch.int64, device=dv)
        d_res = torch.zeros(48, dtype=torch.uint8, device=dv)
        res, _ = dev.select_documents(paths, *args, d_first, d_docs, d_numbers=d_numbers, numbers_capacity=cap, d_numbers_result=d_num,
                                      d_verdicts=d_verdicts, d_fields=d_fields)
        assert (res.code, res.n_documents, res.n_paths, res.n_no_bits) == (0, lines, len(pointers), 0), (res.code, res.n_documents, res.n_no_bits)

        def select():
            dev.select_documents(paths, *args, d_first, d_docs, d_numbers=d_numbers, numbers_capacity=cap, d_numbers_result=d_num,
                                 d_verdicts=d_verdicts, d_fields=d_fields, d_result=d_res, sync=False)

        r = timed(select, a.steps, a.settle)
        parts = {"token_arrays": 5 * n * levels, "candidates": sum(9 * c + b for c, b in per_level[:levels]),
                 "records": 16 * lines * len(pointers)}
        alg = int(sum(parts.values()))
        r.update({"pointers": pointers, "levels": levels, "n_found": int(res.n_found), "must_move_bytes": alg, "must_move_parts": parts,
                  "must_move_gb_per_s": alg / r["median"] / 1e6, "share_of_8tb_per_s": alg / (r["median"] * 1e-3) / PEAK_BYTES_PER_S,
                  "ratio_to_validate_documents": r["median"] / out["validate_documents"]["median"]})
        out[name] = r
        print(f"{name}: {nbytes} B, {n} tokens, {lines} documents, {res.n_found} found; select_documents {r['median']:.3f} ms (min "
              f"{r['min']:.3f}, p95 {r['p95']:.3f}), must move {alg / 1e9:.3f} GB -> {r['must_move_gb_per_s']:.0f} GB/s = "
              f"{100 * r['share_of_8tb_per_s']:.1f} % of 8 TB/s; validate_documents over the same arrays "
              f"{out['validate_documents']['median']:.3f} ms; ratio {r['ratio_to_validate_documents']:.2f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
