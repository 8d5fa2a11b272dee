#!/usr/bin/env python3
"""Rate of msj_join_rows_device (the equi-join of two code columns): the call alone, on the columns of
scripts/dictionary_rate.py's synthetic 1 GiB NDJSON window of lines
    {"id":"0000001234","status":"s07","n":4}
    dimension   the window's /id column (every row another value) against a right side of unique keys -- every second id,
                shuffled --, INNER and LEFT: half the left rows find their one partner
    status      the /status column of 37 values against a 37-row right side: every left row finds one partner
    skewed      a many-to-many join over made-up codes: 2^20 keys, one of them held by sqrt(L) rows of each side, the other
                left rows with a key finding 16 partners each, M held near 2 L
Each is reported in ms next to three yardsticks in the same process:
    dictionary_pair   the two msj_dictionary_extend_device calls that made the codes (right side appended to a fresh
                      dictionary, left side looked up frozen); not there for the made-up codes
    sort_rows         msj_sort_rows_device over the R right codes as int64 records
    torch             the same join written with torch: stable sort of the right codes, bincount, cumsum,
                      repeat_interleave, gathers (it has to bring M to the host to size its output; that wait is in its time)
and the pairs are compared with the torch formulation's, entry by entry.  Clocks are settled first (--settle seconds of
the same calls), then --steps calls, each timed by device events.  Prints and writes (--json, default
profiles/join_rows/join_rows_rate.json).  The per-kernel split comes from a run of its own:
    rocprofv3 --kernel-trace --stats -- python scripts/join_rows_rate.py --steps 3 --settle 0 --case dimension"""
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


def torch_join(lk, rk, G, left_outer):
    """The yardstick -> (left rows int64[M], right rows int64[M], -1 where there is none)"""
    rows = torch.nonzero((rk >= 0) & (rk < G)).view(-1)
    keys = rk[rows].to(torch.int64)
    _, order = torch.sort(keys, stable=True)
    order = rows[order]
    counts = torch.bincount(keys, minlength=G)
    start = torch.cumsum(counts, 0) - counts
    has_key = (lk >= 0) & (lk < G)
    key = lk.to(torch.int64).clamp(0, G - 1)
    c = torch.where(has_key, counts[key], torch.zeros_like(key))
    n = c.clamp(min=1) if left_outer else c
    off = torch.cumsum(n, 0) - n
    M = int(n.sum())
    left = torch.repeat_interleave(torch.arange(lk.numel(), device=lk.device), n, output_size=M)
    within = torch.arange(M, device=lk.device) - off[left]
    found = c[left] > 0
    place = torch.where(found, start[key[left]] + within, torch.zeros_like(within))
    right = torch.where(found, order[place], torch.full_like(place, -1))
    return left, right


def records_of(codes):
    """int32 codes as msj_field records of type 'l' (int64[rows, 2]): what msj_sort_rows_device orders"""
    rec = torch.zeros((codes.numel(), 2), dtype=torch.int64, device=codes.device)
    rec[:, 0] = codes.to(torch.int64)
    rec[:, 1] = ord("l") << 32
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", nargs="*", default=["dimension", "status", "skewed"])
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "join_rows", "join_rows_rate.json"))
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
    L = lines
    gen = torch.Generator(device=dv)
    gen.manual_seed(11)

    def measure(label, lk, rk, G, hows, dictionary_pair):
        R = rk.numel()
        d_res = torch.zeros(64, dtype=torch.uint8, device=dv)
        d_sort = torch.zeros(48, dtype=torch.uint8, device=dv)
        rec, d_rsel = records_of(rk), torch.tensor(list(bytes(_lib.MsjSelectDocumentsResult(0, 0, R, 1, R, 0, 0))), dtype=torch.uint8, device=dv)
        d_order = torch.empty(max(R, 1), dtype=torch.int32, device=dv)
        sort = timed(lambda: dev.sort_rows(rec, d_rsel, d_order=d_order, d_result=d_sort, sync=False), a.steps, a.settle)
        del rec, d_order
        for how in hows:
            first, *_ = dev.join_rows(lk, rk, n_keys=G, how=how, pairs_capacity=0)
            M = int(first.n_pairs)
            d_l, d_r = torch.empty(max(M, 1), dtype=torch.int32, device=dv), torch.empty(max(M, 1), dtype=torch.int32, device=dv)
            d_off = torch.empty(L + 1, dtype=torch.int64, device=dv)

            def join():
                dev.join_rows(lk, rk, n_keys=G, how=how, pairs_capacity=M, d_left_rows=d_l, d_right_rows=d_r, d_offsets=d_off, d_result=d_res, sync=False)

            r = timed(join, a.steps, a.settle)
            last = _lib.MsjJoinRowsResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
            assert (last.code, last.n_pairs, last.n_left, last.n_right, last.n_keys) == (0, M, lk.numel(), R, G), (last.code, last.n_pairs)
            t_left, t_right = torch_join(lk, rk, G, how == "left")
            assert torch.equal(t_left.to(torch.int32), d_l[:M]) and torch.equal(t_right.to(torch.int32), d_r[:M]), f"{label} {how}: the pairs differ"
            assert int(d_off[-1]) == M
            del t_left, t_right
            th = timed(lambda: torch_join(lk, rk, G, how == "left"), max(a.steps // 2, 2), min(a.settle, 1.0))
            r.update({"left_rows": lk.numel(), "right_rows": R, "n_keys": G, "n_pairs": M, "n_left_matched": int(last.n_left_matched),
                      "pairs_per_us": M / r["median"] / 1e3, "left_rows_per_us": lk.numel() / r["median"] / 1e3,
                      "workspace_bytes": dev.join_rows_workspace_bytes(lk.numel(), R, G),
                      "yardsticks": {"dictionary_pair": dictionary_pair, "sort_rows": sort, "torch": th},
                      "ratio_to_torch": r["median"] / th["median"], "ratio_to_sort_rows": r["median"] / sort["median"],
                      "ratio_to_dictionary_pair": r["median"] / dictionary_pair["median"] if dictionary_pair else None})
            out[f"{label}_{how}"] = r
            pair = f"{dictionary_pair['median']:.3f}" if dictionary_pair else "-"
            print(f"{label} {how}: L {lk.numel()}, R {R}, G {G}, M {M}; join {r['median']:.3f} ms (min {r['min']:.3f}, p95 {r['p95']:.3f}); the two "
                  f"dictionary calls {pair} ms, sort_rows over R {sort['median']:.3f} ms, torch {th['median']:.3f} ms", flush=True)
            del d_l, d_r, d_off
            torch.cuda.empty_cache()

    def coded(name, pick):
        """The codes of a column of the window through the two dictionary calls: the right side is the rows `pick` names, appended
        to a fresh dictionary; the left side, every row, looked up frozen -> (left codes, right codes, G, the pair's time)"""
        p = ("status", "id").index(name)
        slay, d_off, d_valid, d_bytes = dev.string_column(d_buf, nbytes, d_fields, p, d_sel)
        total = int(slay.total_bytes)
        assert (slay.code, slay.n_rows, slay.n_strings) == (0, L, L) and total % L == 0
        width, R = total // L, pick.numel()
        r_bytes = d_bytes[:total].view(L, width)[pick].contiguous().view(-1)
        r_off = torch.arange(R + 1, dtype=torch.int64, device=dv) * width
        r_valid = torch.ones(R, dtype=torch.uint8, device=dv)
        t_off, t_first = torch.zeros(R + 1, dtype=torch.int64, device=dv), torch.zeros(R, dtype=torch.int32, device=dv)
        t_bytes = torch.zeros(R * width, dtype=torch.uint8, device=dv)
        r_codes, l_codes = torch.empty(R, dtype=torch.int32, device=dv), torch.empty(L, dtype=torch.int32, device=dv)
        r_res, l_res = torch.zeros(64, dtype=torch.uint8, device=dv), torch.zeros(64, dtype=torch.uint8, device=dv)

        def pair():
            dev.dictionary_extend(r_off, r_bytes, r_valid, t_off, t_first, t_bytes, rows=R, bytes_len=R * width, d_codes=r_codes, d_result=r_res, sync=False)
            dev.dictionary_extend(d_off, d_bytes, d_valid, t_off, t_first, t_bytes, d_n_prior=r_res[24:32].view(torch.int64), rows=L, bytes_len=total,
                                  d_codes=l_codes, frozen=True, d_result=l_res, sync=False)

        t = timed(pair, a.steps, a.settle)
        G = int(_lib.MsjDictionaryExtendResult.from_buffer_copy(r_res.cpu().numpy().tobytes()).n_distinct)
        return l_codes, r_codes, G, t

    if "dimension" in a.case:
        pick = (torch.randperm(L // 2, device=dv, generator=gen) * 2).to(torch.int64)
        lk, rk, G, t = coded("id", pick)
        assert G == L // 2
        measure("dimension", lk, rk, G, ("inner", "left"), t)
        del lk, rk, pick
    if "status" in a.case:
        pick = torch.arange(STATUSES, dtype=torch.int64, device=dv)   # (k * 7919) % 37 over 37 consecutive rows: every status once
        lk, rk, G, t = coded("status", pick)
        assert G == STATUSES
        measure("status", lk, rk, G, ("inner",), t)
        del lk, rk, pick
    if "skewed" in a.case:
        G, R, hot = 1 << 20, L // 8, int(L ** 0.5)
        per_key = 16
        rk = torch.randint(1, R // per_key, (R,), device=dv, generator=gen, dtype=torch.int32)
        lk = torch.where(torch.rand(L, device=dv, generator=gen) < 1.0 / per_key, torch.randint(1, R // per_key, (L,), device=dv, generator=gen, dtype=torch.int32),
                         torch.full((L,), -1, dtype=torch.int32, device=dv))
        rk[torch.randperm(R, device=dv, generator=gen)[:hot]] = 0
        lk[torch.randperm(L, device=dv, generator=gen)[:hot]] = 0
        measure("skewed", lk, rk, G, ("inner",), None)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
