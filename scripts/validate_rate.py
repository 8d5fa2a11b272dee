#!/usr/bin/env python3
"""Rate of msj_validate_device (stage 2's verdict for a document): the call alone on 1 GiB of the minified, utf8 and
pretty4 workloads -- ONE document each, "[unit,unit,...]" of a 64 MiB unit -- and, in the same process, the prep call it
consumes (msj_stage2_prep_device with d_match) on the same input.
Clocks are settled first (2 s of the same calls), then 20 calls, each timed by device events.  Prints and, with --json,
writes per workload: ms per call, the bytes the call must move (computed below from n, the atoms and the escaped bytes),
that over the time as a share of 8 TB/s, and the ratio to the prep call."""
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


def must_move(n, typ, flags, idx, end, big_tokens):
    """Bytes msj_validate_device has to read: type + partner of every token (5 n); depth of the opening brackets, index
    of the atoms, index + end + flags of the strings, counted in the 64-byte lines they sit in; the 64-byte lines of the
    buffer that hold an atom or an escaped body; type + depth again for the containers whose commas are counted."""
    def lines(tokens, width):
        return int(np.unique(tokens * width // 64).size) * 64

    opens = np.nonzero((typ == ord("{")) | (typ == ord("[")))[0]
    atoms = np.nonzero((typ == ord("t")) | (typ == ord("f")) | (typ == ord("n")))[0]
    strings = np.nonzero(typ == ord('"'))[0]
    escaped = np.nonzero((flags & 2) != 0)[0]
    total = 5 * n + lines(opens, 4) + lines(atoms, 4) + lines(strings, 1) + 2 * lines(escaped, 4)
    buf_lines = np.unique(idx[atoms] // 64).size
    esc_bytes = int((end[escaped].astype(np.int64) - idx[escaped].astype(np.int64)).sum())
    total += 64 * int(buf_lines) + esc_bytes + 32 * int(escaped.size)  # (half a line of slack at each end of a body)
    total += 5 * big_tokens
    return int(total), {"atoms": int(atoms.size), "escaped_strings": int(escaped.size), "escaped_bytes": esc_bytes,
                        "opening_brackets": int(opens.size)}


def run_case(dev, name, unit, reps, steps, settle):
    dv = dev.device
    d_unit = torch.from_numpy(unit).to(dv)
    one = lambda c: torch.tensor([ord(c)], dtype=torch.uint8, device=dv)
    parts = [one("[")]
    for r in range(reps):
        parts += [d_unit] if r + 1 == reps else [d_unit, one(",")]
    d_buf = torch.cat(parts + [one("]")])
    nbytes = d_buf.numel()
    d_idx = torch.empty(nbytes // 2 + 8, dtype=torch.int32, device=dv)
    d_carry = dev.new_carry()
    dev.index(d_buf, d_idx, d_carry)
    carry = dev.fetch(d_carry)
    assert carry.code == 0
    n = int(carry.count)
    d_type, d_depth, _, d_match, d_end, d_flags = dev.stage2_prep(d_buf, nbytes, d_idx, n, match=True)
    _, d_num = dev.number_values(d_buf, nbytes, d_idx, n, d_flags, capacity=0, sync=False)
    d_res = torch.zeros(32, dtype=torch.uint8, device=dv)
    d_tok = torch.zeros(24, dtype=torch.uint8, device=dv)
    res = dev.validate(d_buf, nbytes, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_num)
    assert res.code == 0 and res.flags == 0, (res.code, res.flags, res.error_token)

    def validate():
        dev.validate(d_buf, nbytes, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_num, d_result=d_res, sync=False)

    def prep():
        rc = dev.lib.msj_stage2_prep_device(dev.ctx, d_buf.data_ptr(), nbytes, d_idx.data_ptr(), n, d_type.data_ptr(), d_depth.data_ptr(),
                                            d_match.data_ptr(), d_end.data_ptr(), d_flags.data_ptr(), d_tok.data_ptr(), dev._stream())
        assert rc == 0

    typ = d_type.cpu().numpy()
    match = d_match.cpu().numpy().view(np.uint32)
    closers = np.nonzero(((typ == ord("}")) | (typ == ord("]"))) & (match != 0xFFFFFFFF))[0]
    span = closers.astype(np.int64) - match[closers].astype(np.int64) - 1
    big_tokens = int(span[span >= 2 * 0xFFFFFF + 1].sum())
    alg, parts_ = must_move(n, typ, d_flags.cpu().numpy(), d_idx[:n].cpu().numpy().view(np.uint32),
                            d_end.cpu().numpy().view(np.uint32), big_tokens)
    out = {"bytes": nbytes, "tokens": n, "n_escaped": int(res.n_escaped), "must_move_bytes": alg, "counted_tokens": big_tokens, **parts_}
    out["validate"] = timed(validate, steps, settle)
    out["prep_match"] = timed(prep, steps, settle)
    m = out["validate"]["median"]
    out["must_move_gb_per_s"] = alg / m / 1e6
    out["share_of_8tb_per_s"] = alg / (m * 1e-3) / PEAK_BYTES_PER_S
    out["ratio_to_prep"] = m / out["prep_match"]["median"]
    print(f"{name}: {nbytes} B, {n} tokens; validate {m:.3f} ms (min {out['validate']['min']:.3f}, p95 {out['validate']['p95']:.3f}); "
          f"prep with partners {out['prep_match']['median']:.3f} ms; ratio {out['ratio_to_prep']:.2f}; must move {alg / 1e9:.3f} GB -> "
          f"{out['must_move_gb_per_s']:.0f} GB/s = {100 * out['share_of_8tb_per_s']:.1f} % of 8 TB/s")
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
