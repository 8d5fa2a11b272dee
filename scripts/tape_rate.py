#!/usr/bin/env python3
"""Rate of msj_tape_device (the document's tape and string buffer): the call alone on 1 GiB of the minified, utf8 and
pretty4 workloads -- ONE document each, "[unit,unit,...]" of a 64 MiB unit -- in its layout-only form (d_string_buf NULL)
and with the string buffer, and, in the same process, the prep call it consumes (msj_stage2_prep_device with d_match) on
the same input.
Clocks are settled first (2 s of the same calls), then 20 calls, each timed by device events.  Prints and, with --json,
writes per workload: ms per call for the three, the bytes the tape call must move (itemised below), that over the time as a
share of 8 TB/s, and the ratio to the prep call.  The per-kernel split comes from a run of its own:
    rocprofv3 --kernel-trace --stats -- python scripts/tape_rate.py --steps 3 --settle 0 --case minified"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mojo_simdjson_amd import _lib, synth  # noqa: E402
from mojo_simdjson_amd.device import Stage1Device  # noqa: E402

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


def must_move(n, typ, flags, n_numbers, tape_words, string_bytes, strings):
    """Bytes msj_tape_device has to move at the least, once each: type, flags, depth and match per token (10 n); idx and end
    at the strings (8 each); the number records (16 each); 8 bytes per word out; with the string buffer, string_bytes in
    (the bodies; the prefixes are not read) and string_bytes out."""
    n_strings = int(np.count_nonzero(typ == ord('"')))
    parts = {"token_arrays": 10 * n, "string_idx_end": 8 * n_strings, "number_records": 16 * n_numbers, "tape_out": 8 * tape_words,
             "string_in_out": (2 * string_bytes - 4 * n_strings) if strings else 0}
    return int(sum(parts.values())), parts


def run_case(dev, name, unit, reps, steps, settle):
    dv = dev.device
    d_unit = torch.from_numpy(unit).to(dv)
    one = lambda c: torch.tensor([ord(c)], dtype=torch.uint8, device=dv)
    parts = [one("[")]
    for r in range(reps):
        parts += [d_unit] if r + 1 == reps else [d_unit, one(",")]
    d_buf = torch.cat(parts + [one("]")])
    del parts
    nbytes = d_buf.numel()
    d_idx = torch.empty(nbytes // 2 + 8, dtype=torch.int32, device=dv)
    d_carry = dev.new_carry()
    dev.index(d_buf, d_idx, d_carry)
    carry = dev.fetch(d_carry)
    assert carry.code == 0
    n = int(carry.count)
    d_type, d_depth, _, d_match, d_end, d_flags = dev.stage2_prep(d_buf, nbytes, d_idx, n, match=True)
    _, num = dev.number_values(d_buf, nbytes, d_idx, n, d_flags, capacity=0)
    cap = int(num.n_numbers)
    d_numbers, d_num = dev.number_values(d_buf, nbytes, d_idx, n, d_flags, capacity=cap, sync=False)
    d_verdict = dev.validate(d_buf, nbytes, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_num, sync=False)
    args = (d_buf, nbytes, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_numbers, cap)
    layout, d_tape, _ = dev.tape(*args, d_verdict=d_verdict, strings=False)
    assert layout.code == 0, layout.code
    d_sbuf = torch.empty(int(layout.string_bytes), dtype=torch.uint8, device=dv)
    d_res = torch.zeros(32, dtype=torch.uint8, device=dv)
    d_tok = torch.zeros(24, dtype=torch.uint8, device=dv)
    full, _, _ = dev.tape(*args, d_verdict=d_verdict, d_tape=d_tape, d_string_buf=d_sbuf)
    assert full.code == 0 and (full.tape_words, full.string_bytes) == (layout.tape_words, layout.string_bytes)

    def tape_layout():
        dev.tape(*args, d_verdict=d_verdict, d_tape=d_tape, strings=False, d_result=d_res, sync=False)

    def tape_full():
        dev.tape(*args, d_verdict=d_verdict, d_tape=d_tape, d_string_buf=d_sbuf, d_result=d_res, sync=False)

    def prep():
        rc = dev.lib.msj_stage2_prep_device(dev.ctx, d_buf.data_ptr(), nbytes, d_idx.data_ptr(), n, d_type.data_ptr(), d_depth.data_ptr(),
                                            d_match.data_ptr(), d_end.data_ptr(), d_flags.data_ptr(), d_tok.data_ptr(), dev._stream())
        assert rc == 0

    typ, flags = d_type.cpu().numpy(), d_flags.cpu().numpy()
    out = {"bytes": nbytes, "tokens": n, "numbers": cap, "tape_words": int(full.tape_words), "string_bytes": int(full.string_bytes),
           "n_strings": int(full.n_strings), "escaped_strings": int(np.count_nonzero(flags & 2))}
    for key, fn, strings in (("tape_layout", tape_layout, False), ("tape_full", tape_full, True)):
        out[key] = timed(fn, steps, settle)
        alg, items = must_move(n, typ, flags, cap, int(full.tape_words), int(full.string_bytes), strings)
        m = out[key]["median"]
        out[key].update({"must_move_bytes": alg, "must_move_parts": items, "must_move_gb_per_s": alg / m / 1e6,
                         "share_of_8tb_per_s": alg / (m * 1e-3) / PEAK_BYTES_PER_S})
    out["prep_match"] = timed(prep, steps, settle)
    for key in ("tape_layout", "tape_full"):
        out[key]["ratio_to_prep"] = out[key]["median"] / out["prep_match"]["median"]
        o = out[key]
        print(f"{name} {key}: {nbytes} B, {n} tokens, {out['tape_words']} words, {out['string_bytes']} string bytes; {o['median']:.3f} ms "
              f"(min {o['min']:.3f}, p95 {o['p95']:.3f}); prep with partners {out['prep_match']['median']:.3f} ms, ratio "
              f"{o['ratio_to_prep']:.2f}; must move {o['must_move_bytes'] / 1e9:.3f} GB -> {o['must_move_gb_per_s']:.0f} GB/s = "
              f"{100 * o['share_of_8tb_per_s']:.1f} % of 8 TB/s", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--unit-mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", nargs="*", default=["minified", "utf8", "pretty4"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = Stage1Device(0)
    results = {"library": _lib.load().msj_version().decode()}
    for name in a.case:
        results[name + "_1gib"] = run_case(dev, name, synth.workload(name, a.unit_mib << 20), a.reps, a.steps, a.settle)
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
