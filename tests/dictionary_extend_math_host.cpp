// Test-only harness: compiles mojo_simdjson_amd/csrc/dictionary_extend_math.h (over dictionary_math.h) for the host (g++), so
// that the arithmetic of msj_dictionary_extend_device -- the same entry test, row test, hash, byte compare and table walk the
// kernels run (csrc/dictionary_extend_kernel.hip) -- is checked on a CPU-only box against a yardstick written in Python
// (tests/test_dictionary_extend_math.py), and so that the GPU tests have an expected value.  NOT part of the product.
#include <string.h>

#include <vector>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/dictionary_extend_math.h"

using namespace msj::dictx;

namespace {
struct HostItemTable {
    std::vector<uint32_t> &t;
    uint32_t load(uint64_t i) const { return t[i]; }
    uint32_t claim(uint64_t i, uint32_t k) const {
        const uint32_t seen = t[i];
        if (seen == kEmpty) t[i] = k;
        return seen;
    }
    void lower(uint64_t i, uint32_t k) const {
        if (k < t[i]) t[i] = k;
    }
};
}  // namespace

extern "C" {

// The whole call, serially: the counts first (nothing is read of an array before they pass), the entry or row test and the
// hash per item, the walk through the table item by item, then the rows in order with every store checked against its
// capacity -- or, frozen, the rows' lookups.  n_rows / n_prior_word: host copies of the device words, or null.  order: 0
// the items ascending, 1 descending -- the outputs may not depend on it (the device inserts in any order)
void dxm_dictionary_extend(const uint64_t *offsets, const uint8_t *valid, uint64_t rows, const uint64_t *n_rows, const uint8_t *bytes,
                           uint64_t bytes_len, uint64_t n_prior, const uint64_t *n_prior_word, int32_t *codes, uint64_t *dict_offsets,
                           uint32_t *dict_first, uint64_t dict_capacity, uint8_t *dict_bytes, uint64_t dict_bytes_capacity, uint32_t flags,
                           int order, msj_dictionary_extend_result *out) {
    memset(out, 0, sizeof *out);
    out->flags = flags;
    const uint64_t R = n_rows ? *n_rows : rows, P = n_prior_word ? *n_prior_word : n_prior;
    out->n_rows = R, out->n_prior = P;
    const Counts cn = counts_of(R, rows, P, dict_offsets, dict_capacity, dict_bytes_capacity);
    if (cn.over) {
        out->code = MSJ_CAPACITY;
        return;
    }
    const bool frozen = (flags & kFrozen) != 0;
    const uint64_t N = P + R, S = extend_slots(P, R, flags), base = cn.base;
    const Source src{offsets, valid, bytes, bytes_len, dict_offsets, dict_bytes, dict_bytes_capacity};
    std::vector<uint32_t> table(S, kEmpty), slot(N, 0);
    std::vector<uint64_t> hash(N, 0);
    std::vector<Item> item(N);
    for (uint64_t i = 0; i < N; i++) {
        item[i] = item_of(src, P, i);
        hash[i] = hash_finish(hash_piece(item[i].p, item[i].len, 0, 1), item[i].len, flags);
    }
    HostItemTable t{table};
    const auto same_as = [&](uint64_t i) {
        return [&hash, &item, i](uint32_t r) {
            return hash[r] == hash[i] && item[r].len == item[i].len && equal_piece(item[i].p, item[r].p, item[i].len, 0, 1);
        };
    };
    const uint64_t inserted = frozen ? P : N;
    for (uint64_t j = 0; j < inserted; j++) {
        const uint64_t i = order ? inserted - 1 - j : j;
        if (!item[i].has) continue;
        const Walk wk = insert_row(t, S, hash[i], (uint32_t)i, same_as(i));
        slot[i] = (uint32_t)wk.slot;
        if (wk.probes > out->max_probe) out->max_probe = wk.probes;
        if (!wk.found) out->code = kExhausted;
    }
    if (frozen) {
        for (uint64_t k = 0; k < R; k++) {
            const uint64_t i = P + k;
            if (!item[i].has) {
                codes[k] = -1;
                continue;
            }
            out->n_values++;
            const Walk wk = lookup_item(t, S, hash[i], same_as(i));
            if (wk.probes > out->max_probe) out->max_probe = wk.probes;
            codes[k] = wk.found ? (int32_t)table[wk.slot] : kNoEntry;
            if (wk.found) out->n_matched++;
        }
        out->n_distinct = P, out->dict_bytes = base;
        return;
    }
    if (P == 0 && dict_offsets) dict_offsets[0] = 0;
    uint64_t n = P, total = base;
    for (uint64_t k = 0; k < R; k++) {
        const uint64_t i = P + k;
        if (!item[i].has) {
            codes[k] = -1;
            continue;
        }
        out->n_values++;
        const uint32_t r = table[slot[i]];
        if (r < P) {
            codes[k] = (int32_t)r, out->n_matched++;
            continue;
        }
        if (r != i) {
            codes[k] = codes[r - P];  // (r < i: the slot holds the smallest item of the value)
            continue;
        }
        codes[k] = (int32_t)n;
        if (n < dict_capacity) dict_first[n] = (uint32_t)k, dict_offsets[n + 1] = total + item[i].len;
        if (dict_bytes && n < dict_capacity)
            for (uint64_t b = 0; b < item[i].len && total + b < dict_bytes_capacity; b++) dict_bytes[total + b] = item[i].p[b];
        n++, total += item[i].len;
    }
    out->n_distinct = n, out->dict_bytes = total;
    const bool layout_only = !dict_offsets && !dict_first && !dict_bytes;
    if (out->code == 0) out->code = extend_code(n, total, layout_only, dict_capacity, dict_bytes_capacity, flags);
}

uint64_t dxm_extend_slots(uint64_t P, uint64_t R, uint32_t flags) { return extend_slots(P, R, flags); }

}  // extern "C"
