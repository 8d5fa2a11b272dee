#!/usr/bin/env python3
"""Rate of msj_validate_documents_device (a verdict for every document of a window): the call alone on 1 GiB of NDJSON --
the lines of tests/test_documents.py::test_document_stream_one_gib, one window -- and, in the same process, msj_validate_device
over the same token arrays: that call does the same pass over the window taken as ONE document and moves the same bytes (it
stops caring at the second line, which changes nothing about what it reads), so the ratio is what the documents cost.
Clocks are settled first (2 s of the same calls), then 20 calls, each timed by device events.  Prints and writes (--json,
default profiles/r09/validate_documents_rate_r09.json): ms per call of both, the ratio, documents and tokens."""
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


def stats(ms):
    ms = sorted(ms)
    return {"median": ms[len(ms) // 2], "min": ms[0], "p95": ms[min(len(ms) - 1, int(round(0.95 * (len(ms) - 1))))]}


def timed(fn, steps, settle):
    t0 = time.perf_counter()
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


def ndjson(total_bytes, dev):
    block = b"".join(json.dumps({"id": i, "text": "t" * (i % 50), "tags": [i, i + 1], "user": {"name": "n", "ok": True}},
                                separators=(",", ":")).encode() + b"\n" for i in range(12000))
    nrep = total_bytes // len(block)
    d_block = torch.frombuffer(bytearray(block), dtype=torch.uint8).to(dev.device)
    return d_block.repeat(nrep), len(block) * nrep, 12000 * nrep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "r09", "validate_documents_rate_r09.json"))
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
    _, d_num = dev.number_values(d_buf, nbytes, d_idx, n, d_flags, capacity=0, sync=False)
    d_verdicts = torch.empty((lines, 2), dtype=torch.int64, device=dv)
    d_vres = torch.zeros(48, dtype=torch.uint8, device=dv)
    d_res = torch.zeros(32, dtype=torch.uint8, device=dv)
    args = (d_buf, nbytes, d_idx, n, d_type, d_depth, d_match, d_end, d_flags)
    _, res = dev.validate_documents(*args, d_first, d_docs, d_numbers_result=d_num, d_verdicts=d_verdicts)
    assert (res.code, res.flags, res.n_documents, res.n_invalid) == (0, 0, lines, 0), (res.code, res.flags, res.n_documents, res.n_invalid)

    def per_document():
        dev.validate_documents(*args, d_first, d_docs, d_numbers_result=d_num, d_verdicts=d_verdicts, d_result=d_vres, sync=False)

    def one_document():
        dev.validate(*args, d_num, d_result=d_res, sync=False)

    out = {"library": _lib.load().msj_version().decode(), "bytes": nbytes, "tokens": n, "documents": lines,
           "n_escaped": int(res.n_escaped)}
    out["validate_documents"] = timed(per_document, a.steps, a.settle)
    out["validate_one_document"] = timed(one_document, a.steps, a.settle)
    m, s = out["validate_documents"]["median"], out["validate_one_document"]["median"]
    out["ratio_to_one_document"] = m / s
    print(f"ndjson: {nbytes} B, {n} tokens, {lines} documents; validate_documents {m:.3f} ms (min {out['validate_documents']['min']:.3f}, "
          f"p95 {out['validate_documents']['p95']:.3f}); validate over the same arrays as one document {s:.3f} ms; ratio {m / s:.2f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
