#!/usr/bin/env python3
"""Rate of msj_tape_documents_device (a tape for every document of a window): the call alone on 1 GiB of NDJSON -- the lines
of scripts/validate_documents_rate.py, and the same lines with escapes in their text, one window each -- and, in the same
process, msj_tape_device over the same token arrays taken as ONE document: that call makes the same passes over the window and
moves nearly the same bytes (no document look-up, no records, 2 root words instead of 2 per document), so the ratio is what
the documents cost.
Clocks are settled first (2 s of the same calls), then 20 calls, each timed by device events.  Prints and writes (--json,
default profiles/r10/tape_documents_rate_r10.json) per workload: ms per call of both, the ratio, the bytes each must move
(itemised) and that over the time as a share of 8 TB/s.  The per-kernel split comes from a run of its own:
    rocprofv3 --kernel-trace --stats -- python scripts/tape_documents_rate.py --steps 3 --settle 0 --case ndjson"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mojo_simdjson_amd import _lib  # noqa: E402
from mojo_simdjson_amd.device import Stage1Device  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_BYTES_PER_S = 8e12


def stats(ms):
    ms = sorted(ms)
    return {"median": ms[len(ms) // 2], "min": ms[0], "p95": ms[min(len(ms) - 1, int(round(0.95 * (len(ms) - 1))))]}


def timed(fn, steps, settle):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    while time.perf_counter() - t0 < settle:  # settle the clocks
        fn()
        torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return stats(ms)


def ndjson(total_bytes, dev, escaped):
    text = (lambda i: "t\né\"" * (i % 13)) if escaped else (lambda i: "t" * (i % 50))
    block = b"".join(json.dumps({"id": i, "text": text(i), "tags": [i, i + 1], "user": {"name": "n", "ok": True}},
                                separators=(",", ":")).encode() + b"\n" for i in range(12000))
    nrep = max(total_bytes // len(block), 1)
    d_block = torch.frombuffer(bytearray(block), dtype=torch.uint8).to(dev.device)
    return d_block.repeat(nrep), len(block) * nrep, 12000 * nrep


def must_move(n, n_strings, n_numbers, tape_words, string_bytes, documents):
    """Bytes a tape call has to move at the least, once each: type, flags, depth and match per token (10 n); idx and end at
    the strings (8 each); the number records (16 each); 8 bytes per word out; string_bytes in (the bodies; the prefixes are
    not read) and string_bytes out; per document (the window call only) its start (4), its verdict (16) and its record (32)."""
    parts = {"token_arrays": 10 * n, "string_idx_end": 8 * n_strings, "number_records": 16 * n_numbers, "tape_out": 8 * tape_words,
             "string_in_out": 2 * string_bytes - 4 * n_strings, "documents": 52 * documents}
    return int(sum(parts.values())), parts


def run_case(dev, name, mib, steps, settle):
    dv = dev.device
    d_buf, nbytes, lines = ndjson(mib << 20, dev, name == "ndjson_escaped")
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
    d_verdicts, vres = dev.validate_documents(*args, d_first, d_docs, d_numbers=d_numbers, numbers_capacity=cap, d_numbers_result=d_num,
                                              capacity=lines)
    assert (vres.code, vres.flags, vres.n_invalid) == (0, 0, 0), (vres.code, vres.flags, vres.n_invalid)
    # sizes from a layout-only call, then the arrays both calls write into
    lay, _, _, d_recs = dev.tape_documents(*args, d_first, d_docs, d_numbers, cap, d_verdicts=d_verdicts, tape_capacity=2, strings=False,
                                           capacity=lines)
    assert lay.code == 1, lay.code  # MSJ_CAPACITY: the true sizes
    d_tape = torch.empty(int(lay.tape_words), dtype=torch.int64, device=dv)
    d_sbuf = torch.empty(int(lay.string_bytes), dtype=torch.uint8, device=dv)
    d_res = torch.zeros(64, dtype=torch.uint8, device=dv)
    d_res1 = torch.zeros(32, dtype=torch.uint8, device=dv)
    full, _, _, _ = dev.tape_documents(*args, d_first, d_docs, d_numbers, cap, d_verdicts=d_verdicts, d_tape=d_tape, d_string_buf=d_sbuf,
                                       d_doc_tapes=d_recs)
    assert (full.code, full.n_documents, full.n_built) == (0, lines, lines), (full.code, full.n_documents, full.n_built)
    one, _, _ = dev.tape(*args, d_numbers, cap, d_tape=d_tape, d_string_buf=d_sbuf)
    assert one.code == 0 and one.string_bytes == full.string_bytes and one.tape_words == full.tape_words - 2 * lines + 2

    def per_document():
        dev.tape_documents(*args, d_first, d_docs, d_numbers, cap, d_verdicts=d_verdicts, d_tape=d_tape, d_string_buf=d_sbuf,
                           d_doc_tapes=d_recs, d_result=d_res, sync=False)

    def one_document():
        dev.tape(*args, d_numbers, cap, d_tape=d_tape, d_string_buf=d_sbuf, d_result=d_res1, sync=False)

    n_strings = int(full.n_strings)
    out = {"bytes": nbytes, "tokens": n, "documents": lines, "numbers": cap, "tape_words": int(full.tape_words),
           "string_bytes": int(full.string_bytes), "n_strings": n_strings,
           "escaped_strings": int(torch.count_nonzero(d_flags[:n] & 2).item())}
    out["tape_documents"] = timed(per_document, steps, settle)
    out["tape_one_document"] = timed(one_document, steps, settle)
    for key, words, documents in (("tape_documents", int(full.tape_words), lines), ("tape_one_document", int(one.tape_words), 0)):
        alg, items = must_move(n, n_strings, cap, words, int(full.string_bytes), documents)
        m = out[key]["median"]
        out[key].update({"must_move_bytes": alg, "must_move_parts": items, "must_move_gb_per_s": alg / m / 1e6,
                         "share_of_8tb_per_s": alg / (m * 1e-3) / PEAK_BYTES_PER_S})
    m, s = out["tape_documents"], out["tape_one_document"]
    out["ratio_to_one_document"] = m["median"] / s["median"]
    print(f"{name}: {nbytes} B, {n} tokens, {lines} documents, {out['tape_words']} words, {out['string_bytes']} string bytes; "
          f"tape_documents {m['median']:.3f} ms (min {m['min']:.3f}, p95 {m['p95']:.3f}), must move {m['must_move_bytes'] / 1e9:.3f} GB -> "
          f"{m['must_move_gb_per_s']:.0f} GB/s = {100 * m['share_of_8tb_per_s']:.1f} % of 8 TB/s; tape over the same arrays as one document "
          f"{s['median']:.3f} ms, must move {s['must_move_bytes'] / 1e9:.3f} GB -> {s['must_move_gb_per_s']:.0f} GB/s; ratio "
          f"{out['ratio_to_one_document']:.2f}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", nargs="*", default=["ndjson", "ndjson_escaped"])
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "r10", "tape_documents_rate_r10.json"))
    a = ap.parse_args()
    dev = Stage1Device(0)
    results = {"library": _lib.load().msj_version().decode()}
    for name in a.case:
        results[name + "_1gib" if a.mib == 1024 else f"{name}_{a.mib}mib"] = run_case(dev, name, a.mib, a.steps, a.settle)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(results, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
