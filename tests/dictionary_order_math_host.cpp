// Test-only harness: compiles mojo_simdjson_amd/csrc/dictionary_order_math.h for the host (g++), so that the arithmetic of
// msj_dictionary_order_device and msj_rank_rows_device -- the same entry test, word fetch, key, digits, tied test and row
// record the kernels run (csrc/dictionary_order_kernel.hip) -- is checked on a CPU-only box against the definition written
// in Python (tests/test_dictionary_order_math.py), and so that the GPU tests have an expected value.  The whole call
// serially, in the kernels' steps: the order by depth 0, then per round the tied entries in position order, their keys, a
// stable order of them -- the grid path's digit passes with the constant digits skipped, or the one-workgroup path's count
// of the keys in front --, the write-back, the heads and the running maximum of their places; the counters from the two
// arrays alone.  NOT part of the product.
#include <string.h>

#include <vector>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/dictionary_order_math.h"

using namespace msj::dord;

namespace {
bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
}  // namespace

extern "C" {

// the pieces on their own
void dom_fetch_word(const uint8_t *bytes, uint64_t bytes_capacity, uint64_t begin, uint64_t len, uint64_t depth, uint64_t *word, uint32_t *nvalid) {
    const Word w = fetch_word(MemoryBytes{bytes}, bytes_capacity, begin, len, depth);
    *word = w.word, *nvalid = w.nvalid;
}
uint32_t dom_key_digits(uint64_t capacity) { return key_digits(capacity); }
uint32_t dom_digit(uint64_t word, uint32_t rank, uint32_t nvalid, uint32_t d) {
    Word w;
    w.word = word, w.nvalid = nvalid;
    return digit_of(key_of(rank, w), d);
}
int32_t dom_use_group_path(uint64_t capacity, uint32_t mode) { return use_group_path(capacity, mode); }
uint32_t dom_rounds_of(uint32_t max_rounds, int32_t group) { return rounds_of(max_rounds, group != 0); }

// The whole call, serially; ctx_ok: whether the context is given; mode: msj_debug_set_order_mode's.  passes_run, if given,
// receives the digit passes the grid path ran.  -> 0, or what the entry point refuses on the host, in the header's order,
// with nothing written
int32_t dom_dictionary_order(int32_t ctx_ok, const uint64_t *offsets, const uint8_t *bytes, uint64_t bytes_capacity, uint64_t n_entries,
                             const uint64_t *d_n_entries, uint64_t capacity, uint64_t depth, uint32_t max_rounds, uint32_t flags, uint32_t mode,
                             uint32_t *sorted, uint32_t *rank, msj_dictionary_order_result *res, uint64_t *passes_run) {
    if (!ctx_ok || !res) return MSJ_ERR_BAD_ARGUMENT;
    if ((capacity > 0 && (!offsets || !sorted || !rank)) || (bytes_capacity > 0 && !bytes)) return MSJ_ERR_BAD_ARGUMENT;
    if (bad_numbers(depth, max_rounds, flags)) return MSJ_ERR_BAD_ARGUMENT;
    if (capacity >= (1ull << 40)) return MSJ_CAPACITY;
    if (!aligned_to(offsets, 8) || !aligned_to(d_n_entries, 8) || !aligned_to(res, 8) || !aligned_to(sorted, 4) || !aligned_to(rank, 4))
        return MSJ_ERR_BAD_ARGUMENT;

    const uint64_t V = d_n_entries ? *d_n_entries : n_entries;
    memset(res, 0, sizeof *res);
    res->flags = flags, res->n_entries = V;
    if (passes_run) *passes_run = 0;
    if (entries_over(V, capacity)) {
        res->code = MSJ_CAPACITY;
        return 0;
    }
    if (V == 0) return 0;
    const bool group = use_group_path(capacity, mode);
    const uint32_t rounds = rounds_of(max_rounds, group), digits = key_digits(capacity);
    const MemoryBytes src{bytes};
    if (!(flags & kContinue)) {
        uint64_t n_values = 0, at = 0;
        for (uint64_t c = 0; c < V; c++) n_values += value_of(offsets, bytes_capacity, c).has;
        for (uint64_t c = 0, others = n_values; c < V; c++) {
            const bool has = value_of(offsets, bytes_capacity, c).has;
            sorted[has ? at++ : others++] = (uint32_t)c;
            rank[c] = has ? 0u : kNoRank;
        }
    }
    uint64_t rounds_run = 0;
    for (uint32_t t = 0; t < rounds; t++) {
        const uint64_t B = depth + (uint64_t)kWordBytes * t;
        std::vector<Key> key;
        std::vector<uint32_t> ent, pos;
        for (uint64_t p = 0; p < V; p++) {
            Entry x;
            if (!tied_at(sorted, rank, offsets, bytes_capacity, V, p, B, x)) continue;
            key.push_back(key_of(rank[x.e], fetch_word(src, bytes_capacity, x.v.begin, x.v.len, B)));
            ent.push_back(x.e), pos.push_back((uint32_t)p);
        }
        const uint64_t n = key.size();
        if (n == 0) break;
        rounds_run = t + 1;
        std::vector<Key> key2(n);
        std::vector<uint32_t> ent2(n);
        if (group) {
            for (uint64_t i = 0; i < n; i++) {
                uint64_t to = 0;
                for (uint64_t j = 0; j < n; j++) to += key_less(key[j], key[i]) || (j < i && key_equal(key[j], key[i]));
                key2[to] = key[i], ent2[to] = ent[i];
            }
            key.swap(key2), ent.swap(ent2);
        } else {
            Key any = {0, 0}, all = {~0ull, ~0ull};
            for (const Key &k : key) any.word |= k.word, any.rn |= k.rn, all.word &= k.word, all.rn &= k.rn;
            const uint32_t mask = varying_digits(any, all, digits);
            for (uint32_t d = 0; d < digits; d++) {
                if (!((mask >> d) & 1u)) continue;
                if (passes_run) ++*passes_run;
                uint64_t to[kBuckets + 1] = {};
                for (uint64_t i = 0; i < n; i++) to[digit_of(key[i], d) + 1]++;
                for (uint32_t b = 0; b < kBuckets; b++) to[b + 1] += to[b];
                for (uint64_t i = 0; i < n; i++) {
                    const uint64_t at = to[digit_of(key[i], d)]++;
                    key2[at] = key[i], ent2[at] = ent[i];
                }
                key.swap(key2), ent.swap(ent2);
            }
        }
        uint32_t most = 0;
        for (uint64_t i = 0; i < n; i++) {
            sorted[pos[i]] = ent[i];
            if (i == 0 || !key_equal(key[i - 1], key[i])) most = pos[i] + 1 > most ? pos[i] + 1 : most;
            rank[ent[i]] = most ? most - 1 : 0u;
        }
    }
    const uint64_t B = depth + kWordBytes * rounds_run;
    for (uint64_t p = 0; p < V; p++) {
        Entry x;
        const bool tied = tied_at(sorted, rank, offsets, bytes_capacity, V, p, B, x);
        res->n_values += x.v.has, res->n_tied += tied;
        res->n_equal += is_repeat(x.v.has, tied, x.v.has ? rank[x.e] : 0u, p);
    }
    res->depth = B;
    res->code = order_code(res->n_tied);
    return 0;
}

int32_t dom_rank_rows(int32_t ctx_ok, const int32_t *codes, uint64_t rows, const uint64_t *d_n_rows, const uint32_t *rank, uint64_t rank_capacity,
                      const msj_dictionary_order_result *order, msj_field *fields, uint64_t capacity, msj_rank_rows_result *res,
                      msj_select_documents_result *sel) {
    if (!ctx_ok || !res || !sel || !order) return MSJ_ERR_BAD_ARGUMENT;
    if ((rows > 0 && !codes) || (capacity > 0 && !fields) || (rank_capacity > 0 && !rank)) return MSJ_ERR_BAD_ARGUMENT;
    if (rows >= (1ull << 40) || capacity >= (1ull << 40)) return MSJ_CAPACITY;
    if ((const void *)res == (const void *)sel) return MSJ_ERR_BAD_ARGUMENT;
    if (!aligned_to(fields, 16) || !aligned_to(codes, 4) || !aligned_to(rank, 4) || !aligned_to(d_n_rows, 8) || !aligned_to(order, 8) ||
        !aligned_to(res, 8) || !aligned_to(sel, 8))
        return MSJ_ERR_BAD_ARGUMENT;
    const uint64_t R = d_n_rows ? *d_n_rows : rows, V = order->n_entries;
    memset(res, 0, sizeof *res);
    memset(sel, 0, sizeof *sel);
    if (order->code != 0) {
        res->code = sel->code = order->code;
        return 0;
    }
    res->n_rows = R;
    if (rank_rows_over(R, rows, capacity, V, rank_capacity)) {
        res->code = sel->code = MSJ_CAPACITY;
        return 0;
    }
    sel->n_documents = R, sel->n_paths = 1;
    for (uint64_t k = 0; k < R; k++) {
        RowRecord r;
        const uint32_t kind = row_record(codes[k], V, rank, r);
        res->n_ranked += kind == kRanked, res->n_null += kind == kNull, res->n_unknown += kind == kUnknown;
        msj_field f;
        memset(&f, 0, sizeof f);
        f.bits = r.bits, f.token = r.token, f.type = r.type, f.flags = r.flags, f.code = r.code;
        fields[k] = f;
    }
    sel->n_found = res->n_ranked;
    return 0;
}

}  // extern "C"
