#!/usr/bin/env python3
"""Rate of msj_dictionary_order_device and msj_rank_rows_device: the calls alone, on the columns of
scripts/dictionary_rate.py's synthetic 1 GiB NDJSON window of lines
    {"id":"0000001234","status":"s07","n":4}
    status   the /status dictionary: 37 values, the one-workgroup path
    id       the /id dictionary: every row another value of ten digits, the grid path, two rounds
    url      a made-up dictionary of 2^20 URL-like values that share their first 40 bytes (five rounds with every entry
             tied, a sixth that tells them apart)
Each order is reported in ms next to three yardsticks in the same process:
    dictionary   the msj_dictionary_device call that made the dictionary (not there for the made-up one)
    sort_rows    msj_sort_rows_device over as many int64 records: what V keys cost there
    torch        torch.sort of the values' first eight bytes as int64 (it does not finish the order)
and is compared with the order of the values on the host (status) or with torch's sort of the digits as numbers (id, url).
    idle_round   what a round that finds nothing tied costs on the grid path: capacity 2^20, values that differ inside their
                 first word, max_rounds 1 against 33 -- the number behind kDefaultRoundsGrid (dictionary_order_math.h)
    rank_rows    msj_rank_rows_device over the window's /id codes next to a device-to-device copy of as many records
    order_by_id  the chain ``order_by("/id", cast={"/id": "string"})`` runs: string column, dictionary, order, rank records,
                 sort, with nothing waited for in between
Clocks are settled first (--settle seconds of the same calls), then --steps calls, each timed by device events.  Prints and
writes (--json, default profiles/dictionary_order/dictionary_order_rate.json).  The per-kernel split comes from a run of its
own:
    rocprofv3 --kernel-trace --stats -- python scripts/dictionary_order_rate.py --steps 3 --settle 0 --case id"""
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
from join_rows_rate import records_of  # noqa: E402
from validate_documents_rate import timed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
URL_PREFIX = b"https://cdn.example.org/assets/v2/image/"
assert len(URL_PREFIX) == 40


def first_words(d_offsets, d_bytes, V):
    """The first eight bytes of every value as a big-endian int64 (zero-padded; values here have at least eight)"""
    at = d_offsets[:V].view(-1, 1) + torch.arange(8, device=d_bytes.device).view(1, -1)
    b = d_bytes[at].to(torch.int64)
    w = torch.zeros(V, dtype=torch.int64, device=d_bytes.device)
    for k in range(8):
        w |= b[:, k] << (8 * (7 - k))
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of the same calls before the timed steps")
    ap.add_argument("--case", nargs="*", default=["status", "id", "url", "idle_round", "rank_rows", "order_by_id"])
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "dictionary_order", "dictionary_order_rate.json"))
    a = ap.parse_args()
    dev = Stage1Device(0)
    dv = dev.device
    lib = _lib.load()
    out = {"library": lib.msj_version().decode()}
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

    def yardsticks(V, words):
        rec = records_of(torch.arange(V, dtype=torch.int32, device=dv).flip(0))
        d_rsel = torch.tensor(list(bytes(_lib.MsjSelectDocumentsResult(0, 0, V, 1, V, 0, 0))), dtype=torch.uint8, device=dv)
        d_order, d_sort = torch.empty(max(V, 1), dtype=torch.int32, device=dv), torch.zeros(48, dtype=torch.uint8, device=dv)
        sort = timed(lambda: dev.sort_rows(rec, d_rsel, d_order=d_order, d_result=d_sort, sync=False), a.steps, a.settle)
        del rec, d_order
        th = timed(lambda: torch.sort(words, stable=True), max(a.steps // 2, 2), min(a.settle, 1.0))
        return sort, th

    def order_case(label, d_off, d_bytes, V, capacity, max_rounds, made_by, check):
        d_sorted, d_rank = torch.empty(max(capacity, 1), dtype=torch.int32, device=dv), torch.empty(max(capacity, 1), dtype=torch.int32, device=dv)
        d_res = torch.zeros(48, dtype=torch.uint8, device=dv)

        def order():
            dev.dictionary_order(d_off, d_bytes, n_entries=V, capacity=capacity, max_rounds=max_rounds, d_sorted=d_sorted, d_rank=d_rank, d_result=d_res,
                                 sync=False)

        r = timed(order, a.steps, a.settle)
        last = _lib.MsjDictionaryOrderResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
        assert (last.code, last.n_entries, last.n_values, last.n_tied, last.n_equal) == (0, V, V, 0, 0), (last.code, last.n_tied, last.n_equal)
        check(d_sorted[:V], d_rank[:V])
        sort, th = yardsticks(V, first_words(d_off, d_bytes, V))
        group = capacity <= _lib.ORDER_GROUP_ENTRIES
        r.update({"entries": V, "capacity": capacity, "path": "one workgroup" if group else "grid", "rounds_run": int(last.depth) // 8,
                  "rounds_enqueued": max_rounds or (_lib.ORDER_DEFAULT_ROUNDS_GROUP if group else _lib.ORDER_DEFAULT_ROUNDS_GRID),
                  "entries_per_us": V / r["median"] / 1e3, "workspace_bytes": dev.dictionary_order_workspace_bytes(capacity),
                  "yardsticks": {"dictionary": made_by, "sort_rows": sort, "torch_sort_first_word": th},
                  "ratio_to_dictionary": r["median"] / made_by["median"] if made_by else None, "ratio_to_sort_rows": r["median"] / sort["median"],
                  "ratio_to_torch_sort_first_word": r["median"] / th["median"]})
        out[label] = r
        made = f"{made_by['median']:.3f}" if made_by else "-"
        print(f"{label}: V {V}, {r['path']}, {r['rounds_run']} rounds of {r['rounds_enqueued']}; order {r['median']:.3f} ms (min {r['min']:.3f}, p95 "
              f"{r['p95']:.3f}); the dictionary call {made} ms, sort_rows over V {sort['median']:.3f} ms, torch.sort of the first words "
              f"{th['median']:.3f} ms", flush=True)
        return d_sorted, d_rank, d_res

    def column_dictionary(name, capacity):
        """The column's strings and its dictionary -> (the string column, the dictionary's tensors, V, the dictionary call's time)"""
        p = ("status", "id").index(name)
        slay, d_off, d_valid, d_bytes = dev.string_column(d_buf, nbytes, d_fields, p, d_sel)
        total = int(slay.total_bytes)
        first, d_codes, d_doff, d_dfirst, d_dbytes = dev.dictionary(d_off, d_bytes, d_valid, rows=L, bytes_len=total, dict_capacity=capacity,
                                                                    dict_bytes_capacity=total if name == "id" else 4096)
        assert first.code == 0, first.code
        d_res = torch.zeros(48, dtype=torch.uint8, device=dv)
        t = timed(lambda: dev.dictionary(d_off, d_bytes, d_valid, rows=L, bytes_len=total, d_codes=d_codes, d_dict_offsets=d_doff, d_dict_first=d_dfirst,
                                         d_dict_bytes=d_dbytes, d_result=d_res, sync=False), a.steps, a.settle)
        return (d_off, d_bytes, d_valid, total), (d_codes, d_doff, d_dbytes), int(first.n_distinct), t

    def digits_check(d_off, d_bytes, V, at, width):
        """The values' decimal digits at [at, at + width) as numbers, sorted by torch: the expected order (all distinct)"""
        idx = d_off[:V].view(-1, 1) + torch.arange(at, at + width, device=dv).view(1, -1)
        num = ((d_bytes[idx].to(torch.int64) - 48) * (10 ** torch.arange(width - 1, -1, -1, device=dv, dtype=torch.int64)).view(1, -1)).sum(1)
        want = torch.argsort(num, stable=True).to(torch.int32)

        def check(srt, rnk):
            assert torch.equal(srt, want), "the order differs from the order of the numbers"
            assert torch.equal(srt[rnk.long()], torch.arange(V, dtype=torch.int32, device=dv))
        return check

    if "status" in a.case:
        _, (d_codes, d_doff, d_dbytes), V, t = column_dictionary("status", 64)
        assert V == STATUSES
        host = d_dbytes.cpu().numpy().tobytes()
        off = d_doff.cpu().tolist()
        want = sorted(range(V), key=lambda c: host[off[c]:off[c + 1]])

        def check(srt, rnk):
            assert srt.cpu().tolist() == want
        order_case("status", d_doff, d_dbytes, V, 64, 0, t, check)
    id_state = None
    if "id" in a.case or "rank_rows" in a.case:
        column, (d_codes, d_doff, d_dbytes), V, t = column_dictionary("id", L)
        assert V == L
        d_sorted, d_rank, d_ores = order_case("id", d_doff, d_dbytes, V, L, 0, t, digits_check(d_doff, d_dbytes, V, 0, 10))
        id_state = (d_codes, d_rank, d_ores)
    if "rank_rows" in a.case and id_state:
        d_codes, d_rank, d_ores = id_state
        d_rec, d_rres, d_rsel = torch.empty((L, 2), dtype=torch.int64, device=dv), torch.zeros(48, dtype=torch.uint8, device=dv), torch.zeros(48, dtype=torch.uint8, device=dv)
        r = timed(lambda: dev.rank_rows(d_codes, d_rank, d_ores, rows=L, rank_capacity=L, d_fields=d_rec, capacity=L, d_result=d_rres, d_select=d_rsel,
                                        sync=False), a.steps, a.settle)
        last = _lib.MsjRankRowsResult.from_buffer_copy(d_rres.cpu().numpy().tobytes())
        assert (last.code, last.n_rows, last.n_ranked) == (0, L, L) and torch.equal(d_rec[:, 0], d_rank[d_codes.long()].to(torch.int64))
        d_copy = torch.empty_like(d_rec)
        cp = timed(lambda: d_copy.copy_(d_rec), a.steps, min(a.settle, 1.0))
        r.update({"rows": L, "rows_per_us": L / r["median"] / 1e3, "yardsticks": {"copy_of_the_records": cp}, "ratio_to_copy": r["median"] / cp["median"]})
        out["rank_rows"] = r
        print(f"rank_rows: {L} rows {r['median']:.3f} ms (min {r['min']:.3f}); a copy of its records {cp['median']:.3f} ms", flush=True)
        del d_rec, d_copy
    id_state = None
    torch.cuda.empty_cache()
    if "url" in a.case:
        V = 1 << 20
        k = torch.randperm(V, device=dv, generator=torch.Generator(device=dv).manual_seed(5))
        width = len(URL_PREFIX) + 8
        d_ubytes = torch.frombuffer(bytearray(URL_PREFIX + b"00000000"), dtype=torch.uint8).to(dv).repeat(V).view(V, width)
        for j in range(8):
            d_ubytes[:, len(URL_PREFIX) + j] = ((k // 10 ** (7 - j)) % 10 + 48).to(torch.uint8)
        d_ubytes = d_ubytes.view(-1)
        d_uoff = torch.arange(V + 1, dtype=torch.int64, device=dv) * width
        order_case("url", d_uoff, d_ubytes, V, V, 8, None, digits_check(d_uoff, d_ubytes, V, len(URL_PREFIX), 8))
    if "idle_round" in a.case:
        V = 1 << 20
        k = torch.randperm(V, device=dv, generator=torch.Generator(device=dv).manual_seed(6))
        d_ibytes = torch.zeros((V, 8), dtype=torch.uint8, device=dv)
        for j in range(8):
            d_ibytes[:, j] = ((k // 10 ** (7 - j)) % 10 + 48).to(torch.uint8)
        d_ibytes, d_ioff = d_ibytes.view(-1), torch.arange(V + 1, dtype=torch.int64, device=dv) * 8
        d_s, d_r, d_res = torch.empty(V, dtype=torch.int32, device=dv), torch.empty(V, dtype=torch.int32, device=dv), torch.zeros(48, dtype=torch.uint8, device=dv)
        t = {}
        for rounds in (1, 33):
            t[rounds] = timed(lambda: dev.dictionary_order(d_ioff, d_ibytes, n_entries=V, capacity=V, max_rounds=rounds, d_sorted=d_s, d_rank=d_r,
                                                           d_result=d_res, sync=False), a.steps, a.settle)
            last = _lib.MsjDictionaryOrderResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
            assert (last.code, last.depth, last.n_tied) == (0, 8, 0)
        idle = (t[33]["median"] - t[1]["median"]) / 32
        launches = 7 + 3 * 12   # a round's launches at capacity 2^20: twelve digits
        out["idle_round"] = {"capacity": V, "one_round": t[1], "thirty_three_rounds": t[33], "idle_round_ms": idle, "launches_per_round": launches,
                             "idle_launch_us": idle / launches * 1e3}
        print(f"idle_round: capacity {V}: 1 round {t[1]['median']:.3f} ms, 33 rounds {t[33]['median']:.3f} ms: an idle round {idle * 1e3:.1f} us, "
              f"{idle / launches * 1e3:.2f} us per launch of {launches}", flush=True)
    if "order_by_id" in a.case:
        (d_off, d_bytes, d_valid, total), (d_codes, d_doff, d_dbytes), V, _ = column_dictionary("id", L)
        d_dfirst = torch.empty(L, dtype=torch.int32, device=dv)
        d_s, d_r = torch.empty(L, dtype=torch.int32, device=dv), torch.empty(L, dtype=torch.int32, device=dv)
        d_rec, d_order = torch.empty((L, 2), dtype=torch.int64, device=dv), torch.empty(L, dtype=torch.int32, device=dv)
        res = [torch.zeros(48, dtype=torch.uint8, device=dv) for _ in range(7)]

        def chain():
            dev.string_column(d_buf, nbytes, d_fields, 1, d_sel, d_offsets=d_off, d_valid=d_valid, d_bytes=d_bytes, d_result=res[0], sync=False)
            dev.dictionary(d_off, d_bytes, d_valid, rows=L, bytes_len=total, d_codes=d_codes, d_dict_offsets=d_doff, d_dict_first=d_dfirst,
                           d_dict_bytes=d_dbytes, d_result=res[1], sync=False)
            dev.dictionary_order(d_doff, d_dbytes, d_n_entries=res[1][24:32].view(torch.int64), capacity=L, d_sorted=d_s, d_rank=d_r, d_result=res[2],
                                 sync=False)
            dev.rank_rows(d_codes, d_r, res[2], rows=L, rank_capacity=L, d_fields=d_rec, capacity=L, d_result=res[3], d_select=res[4], sync=False)
            dev.sort_rows(d_rec, res[4], d_order=d_order, d_result=res[5], d_order_select=res[6], sync=False)

        r = timed(chain, max(a.steps // 2, 2), a.settle)
        last = _lib.MsjSortRowsResult.from_buffer_copy(res[5].cpu().numpy().tobytes())
        assert (last.code, last.n_rows, last.n_values, last.n_written) == (0, L, L, L)
        assert torch.equal(d_order, torch.arange(L, dtype=torch.int32, device=dv)), "the window's ids ascend: the order is the rows"
        r.update({"rows": L, "rows_per_us": L / r["median"] / 1e3})
        out["order_by_id"] = r
        print(f"order_by_id: string column, dictionary, order, rank records and sort of {L} rows {r['median']:.3f} ms (min {r['min']:.3f})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
