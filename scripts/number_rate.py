#!/usr/bin/env python3
"""Rate of msj_number_values_device (number values for stage 2): the call alone, and the span call + the number call, on
  - the 1 GiB minified workload (a 64 MiB unit replicated),
  - a 1 GiB number-dense workload: a JSON array of repr() of random doubles, a 64 MiB unit replicated.
Clocks are settled first (2 s of the same calls), then 20 steps, each timed by device events; prints ms per call,
numbers per second, a median / min / p95 line per case, and the byte count the call needs (flags, index lines, the
lines that hold numbers, the records) against the time.  --json PATH also writes the results."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mojo_simdjson_amd import synth  # noqa: E402
from mojo_simdjson_amd.device import Stage1Device  # noqa: E402


def number_dense(target, seed=1):
    rng = np.random.default_rng(seed)
    out, size = [], 1
    while size < target:
        raw = rng.integers(0, 0x7FF0000000000000, 100_000, dtype=np.uint64) | (rng.integers(0, 2, 100_000, dtype=np.uint64) << np.uint64(63))
        part = ",".join(repr(v) for v in raw.view(np.float64).tolist()).encode()
        out.append(part)
        size += len(part) + 1
    body = b",".join(out)[: target - 2]
    body = body[: body.rfind(b",")]
    return np.frombuffer(b"[" + body + b"]", dtype=np.uint8).copy()


def stats(ms):
    ms = sorted(ms)
    return {"median": ms[len(ms) // 2], "min": ms[0], "p95": ms[min(len(ms) - 1, int(round(0.95 * (len(ms) - 1))))]}


def run_case(dev, name, unit, reps, steps, settle):
    d_buf = torch.from_numpy(unit).to(dev.device).repeat(reps)
    nbytes = d_buf.numel()
    d_idx = torch.empty(nbytes // 2, dtype=torch.int32, device=dev.device)
    d_res = dev.new_carry()
    dev.index(d_buf, d_idx, d_res)
    n = int(dev.fetch(d_res).count)
    d_end, d_flags = dev.token_spans(d_buf, nbytes, d_idx, n)
    d_numbers, res = dev.number_values(d_buf, nbytes, d_idx, n, d_flags)
    d_nres = torch.zeros(32, dtype=torch.uint8, device=dev.device)

    def numbers_only():
        dev.number_values(d_buf, nbytes, d_idx, n, d_flags, d_result=d_nres, sync=False)

    def spans_and_numbers():
        dev.lib.msj_token_spans_device(dev.ctx, d_buf.data_ptr(), nbytes, d_idx.data_ptr(), n, d_end.data_ptr(), d_flags.data_ptr(),
                                       dev._stream())
        dev.number_values(d_buf, nbytes, d_idx, n, d_flags, d_result=d_nres, sync=False)

    out = {"bytes": nbytes, "tokens": n, "numbers": res.n_numbers, "errors": res.n_errors, "slow": res.n_slow}
    # what the call has to move: flags, the index lines, the 64-byte lines holding numbers, the 16-byte records
    idx_h = d_idx[:n].cpu().numpy().view(np.uint32)
    fl = d_flags[:n].cpu().numpy()
    num_tok = np.nonzero(fl & 4)[0]
    idx_lines = np.unique(num_tok // 16).size * 64
    buf_lines = np.unique(idx_h[num_tok] // 64).size * 64
    out["alg_bytes"] = int(n + idx_lines + buf_lines + 16 * num_tok.size)
    for label, fn in (("numbers", numbers_only), ("spans+numbers", spans_and_numbers)):
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
        st = stats(ms)
        out[label] = st
        print(f"{name} {label}: {st['median']:.3f} ms per call ({res.n_numbers / st['median'] / 1e6:.2f} G numbers/s); "
              f"median {st['median']:.3f} min {st['min']:.3f} p95 {st['p95']:.3f} ms")
    m = out["numbers"]["median"]
    print(f"{name}: {nbytes} B, {n} tokens, {res.n_numbers} numbers, {res.n_slow} exact-path, {res.n_errors} errors; "
          f"{out['alg_bytes'] / 1e9:.3f} GB needed -> {out['alg_bytes'] / m / 1e6:.0f} GB/s at {m:.3f} ms")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--unit-mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", choices=["both", "minified", "dense"], default="both")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = Stage1Device(0)
    results = {}
    if a.case in ("both", "minified"):
        results["minified_1gib"] = run_case(dev, "minified", synth.workload("minified", a.unit_mib << 20), a.reps, a.steps, a.settle)
        torch.cuda.empty_cache()
    if a.case in ("both", "dense"):
        results["number_dense_1gib"] = run_case(dev, "number-dense", number_dense(a.unit_mib << 20), a.reps, a.steps, a.settle)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
