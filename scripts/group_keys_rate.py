#!/usr/bin/env python3
"""Rate of msj_bucket_rows_device and msj_group_keys_device (rows grouped by numbers, time buckets and several keys at once):
the calls alone, on records and codes that lie on the device, over one synthetic 1 GiB NDJSON window of lines
    {"ts":"2024-05-01T00:00:00.000Z","status":"s00","code":200,"latency_ms":100000}
made on the device (the clock counts the lines in milliseconds, so a minute is 60 000 lines; 23 statuses, 4 codes) --
    bucket          /ts cast to milliseconds, floored to the minute
    keys_b          the key of (bucket): W = 11
    keys_sb         (status code, bucket): W = 16
    keys_nsb        (/code as a number, status code, bucket): W = 27
next to each a device-to-device copy that moves as many bytes as the call reads plus writes (a copy of n bytes reads n and
writes n, so it copies half that sum), which is the yardstick: both kernels only move bytes.  Then msj_dictionary_device over
each key column, and, through the record views, the whole ``stats(["/latency_ms"], by=["/status", ("/ts", "bucket", 60000)],
cast={"/ts": ("timestamp", "ms")})`` beside today's ``stats(["/latency_ms"], by="/status")`` (host clock: they wait for their
small results).  Clocks are settled first (2 s of the same calls), then 20 calls, each timed by device events.  Prints and
writes (--json, default profiles/group_keys/group_keys_rate.json)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mojo_simdjson_amd import _lib  # noqa: E402
from mojo_simdjson_amd.device import Stage1Device  # noqa: E402
from mojo_simdjson_amd.document_stream import DocumentStream, number_column  # noqa: E402
from cast_strings_rate import put_digits  # noqa: E402
from validate_documents_rate import stats, timed  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = b'{"ts":"2024-05-01T00:00:00.000Z","status":"s00","code":200,"latency_ms":100000}\n'
T0_MS = 1714521600000   # 2024-05-01T00:00:00Z
DAY_MS = 86400000
STATUSES, CODES = 23, (200, 404, 500, 503)
POINTERS = ["/ts", "/status", "/code", "/latency_ms"]


def ndjson(total_bytes, dev):
    """The window, made on the device -> (d_buf, its bytes, its lines).  Line k's instant is T0_MS + k % DAY_MS milliseconds"""
    width, lines = len(LINE), total_bytes // len(LINE)
    d = torch.frombuffer(bytearray(LINE), dtype=torch.uint8).to(dev.device).repeat(lines).view(lines, width)
    k = torch.arange(lines, dtype=torch.int64, device=dev.device)
    ms = k % DAY_MS
    at = LINE.index(b'"ts":"') + 6 + 11
    put_digits(d, at, ms // 3600000, 2)
    put_digits(d, at + 3, ms // 60000 % 60, 2)
    put_digits(d, at + 6, ms // 1000 % 60, 2)
    put_digits(d, at + 9, ms % 1000, 3)
    put_digits(d, LINE.index(b'"status":"s') + 11, (k * 7) % STATUSES, 2)
    put_digits(d, LINE.index(b'"code":') + 7, torch.tensor(CODES, dtype=torch.int64, device=dev.device)[(k * 5) % len(CODES)], 3)
    put_digits(d, LINE.index(b'"latency_ms":') + 13, 100000 + (k * 7919) % 900000, 6)
    return d.view(-1), width * lines, lines


def wall(fn, steps):
    """fn, which waits for its own results, by the host clock -> ms"""
    fn()
    ms = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "group_keys", "group_keys_rate.json"))
    a = ap.parse_args()
    dev = Stage1Device(0)
    dv = dev.device
    out = {"library": _lib.load().msj_version().decode(), "line": LINE.decode(), "line_bytes": len(LINE)}
    d_buf, nbytes, lines = ndjson(a.mib << 20, dev)
    (win,) = list(DocumentStream(dev, d_buf, nbytes, window=(nbytes + 4096) // 16 * 16, select=POINTERS))
    R = win.n_documents
    assert R == lines
    out.update({"bytes": nbytes, "documents": R})
    d_sel = win.d_select
    d_ts, d_ts_sel = win.cast("/ts", "timestamp", "ms")
    d_ts = d_ts.contiguous()
    d_status = win.categories("/status").codes.contiguous()
    d_code = win.d_fields[2].contiguous()
    res48 = lambda: torch.zeros(48, dtype=torch.uint8, device=dv)

    def copy_of(n_bytes):
        """A device-to-device copy that moves n_bytes in all: half of them read and written"""
        src = torch.empty(n_bytes // 2, dtype=torch.uint8, device=dv)
        dst = torch.empty_like(src)
        t = timed(lambda: dst.copy_(src, non_blocking=True), a.steps, a.settle)
        del src, dst
        return t

    def report(name, t, moved, cp):
        t.update({"bytes_moved": moved, "copy": cp, "ratio_to_copy": t["median"] / cp["median"], "rows_per_us": R / t["median"] / 1e3,
                  "gb_per_s": moved / t["median"] / 1e6})
        out[name] = t
        print(f"{name}: {t['median']:.3f} ms (min {t['min']:.3f}, p95 {t['p95']:.3f}) = {t['rows_per_us']:.0f} rows/us, {t['gb_per_s']:.0f} GB/s; "
              f"the copy of the same bytes {cp['median']:.3f} ms: {t['ratio_to_copy']:.2f} of it", flush=True)

    # the bucket
    d_minute, d_bres, d_bsel = torch.empty((R, 2), dtype=torch.int64, device=dv), res48(), res48()

    def bucket():
        dev.bucket_rows(d_ts, d_ts_sel, 60000, 0, capacity=R, d_out=d_minute, d_result=d_bres, d_out_select=d_bsel, sync=False)

    t = timed(bucket, a.steps, a.settle)
    bres = _lib.MsjBucketRowsResult.from_buffer_copy(d_bres.cpu().numpy().tobytes())
    assert (bres.code, bres.n_rows, bres.n_bucketed) == (0, R, R), (bres.code, bres.n_bucketed)
    k = torch.arange(R, dtype=torch.int64, device=dv)
    values, valid = number_column(d_minute, torch.int64)
    assert bool(valid.all()) and bool((values == (T0_MS + k % DAY_MS) // 60000 * 60000).all())
    del values, valid, k
    report("bucket", t, 32 * R, copy_of(32 * R))

    # the keys, and the dictionary call that follows each
    cases = {"keys_b": [d_minute], "keys_sb": [d_status, d_minute], "keys_nsb": [d_code, d_status, d_minute]}
    for name, parts in cases.items():
        W = sum(11 if p.dtype == torch.int64 else 5 for p in parts)
        read = sum(16 if p.dtype == torch.int64 else 4 for p in parts)
        d_off, d_valid = torch.empty(R + 1, dtype=torch.int64, device=dv), torch.empty(R, dtype=torch.uint8, device=dv)
        d_bytes, d_kres = torch.empty(R * W, dtype=torch.uint8, device=dv), res48()

        def keys():
            dev.group_keys(parts, d_sel, capacity=R, d_offsets=d_off, d_valid=d_valid, d_bytes=d_bytes, d_result=d_kres, sync=False)

        t = timed(keys, a.steps, a.settle)
        kres = _lib.MsjGroupKeysResult.from_buffer_copy(d_kres.cpu().numpy().tobytes())
        assert (kres.code, kres.n_rows, kres.n_keys, kres.key_width, kres.bytes_len) == (0, R, R, W, R * W), (kres.code, kres.n_keys)
        moved = (read + W + 9) * R
        t["key_width"] = W
        report(name, t, moved, copy_of(moved))
        d_codes, d_dres = torch.empty(R, dtype=torch.int32, device=dv), res48()
        cap = 1 << 16
        d_doff, d_dfirst = torch.empty(cap + 1, dtype=torch.int64, device=dv), torch.empty(cap, dtype=torch.int32, device=dv)
        d_dbytes = torch.empty(cap * W, dtype=torch.uint8, device=dv)

        def dictionary():
            dev.dictionary(d_off, d_bytes, d_valid, rows=R, bytes_len=R * W, d_codes=d_codes, d_dict_offsets=d_doff, d_dict_first=d_dfirst,
                           d_dict_bytes=d_dbytes, d_result=d_dres, sync=False)

        t = timed(dictionary, a.steps, a.settle)
        dres = _lib.MsjDictionaryResult.from_buffer_copy(d_dres.cpu().numpy().tobytes())
        assert dres.code == 0 and 0 < dres.n_distinct <= cap, (dres.code, dres.n_distinct)
        t.update({"n_distinct": int(dres.n_distinct), "rows_per_us": R / t["median"] / 1e3})
        out["dictionary_after_" + name] = t
        print(f"msj_dictionary_device over {name}: {t['median']:.3f} ms, {dres.n_distinct} distinct keys", flush=True)
        del d_off, d_valid, d_bytes, d_codes, d_doff, d_dfirst, d_dbytes

    # the whole query through the record views, beside today's
    by_list = wall(lambda: win.stats(["/latency_ms"], by=["/status", ("/ts", "bucket", 60000)], cast={"/ts": ("timestamp", "ms")}), 5)
    by_path = wall(lambda: win.stats(["/latency_ms"], by="/status"), 5)
    got = win.stats(["/latency_ms"], by=["/status", ("/ts", "bucket", 60000)], cast={"/ts": ("timestamp", "ms")})
    assert got.n_groups == min(STATUSES * ((R + 59999) // 60000), R) and int(got.n_rows.sum()) == R, got.n_groups
    out.update({"stats_by_status_and_minute": dict(by_list, n_groups=got.n_groups), "stats_by_status": by_path})
    print(f"stats by [status, minute]: {by_list['median']:.1f} ms for {got.n_groups} groups; stats by status: {by_path['median']:.1f} ms", flush=True)
    out["workspace_bytes"] = int(dev.lib.msj_group_keys_workspace_bytes(R))
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
