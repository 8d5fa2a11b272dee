// Test-only harness: compiles mojo_simdjson_amd/csrc/dictionary_math.h for the host (g++), so that the arithmetic of
// msj_dictionary_device -- the same row test, hash, byte compare and table walk the kernels run
// (csrc/dictionary_kernel.hip) -- is checked on a CPU-only box against a yardstick written in Python
// (tests/test_dictionary_math.py), and so that the GPU tests have an expected value.  NOT part of the product.
#include <string.h>

#include <vector>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/dictionary_math.h"

using namespace msj::dict;

namespace {
struct HostTable {
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

// The whole call, serially: the row test and the hash per row, the walk through the table row by row, the first rows in
// order, then the dictionary with every store checked against its capacity.  n_rows: a host copy of the device word, or
// null.  order: 0 the rows ascending, 1 descending -- the codes may not depend on it (the device inserts in any order)
void dcm_dictionary(const uint64_t *offsets, const uint8_t *valid, uint64_t rows, const uint64_t *n_rows, const uint8_t *bytes,
                    uint64_t bytes_len, int32_t *codes, uint64_t *dict_offsets, uint32_t *dict_first, uint64_t dict_capacity,
                    uint8_t *dict_bytes, uint64_t dict_bytes_capacity, uint32_t flags, int order, msj_dictionary_result *out) {
    memset(out, 0, sizeof *out);
    out->flags = flags;
    const uint64_t R = n_rows ? *n_rows : rows;
    out->n_rows = R;
    if (rows_over(R, rows)) {
        out->code = MSJ_CAPACITY;
        return;
    }
    const uint64_t S = table_slots(R);
    std::vector<uint32_t> table(S, kEmpty), slot(R, 0);
    std::vector<uint64_t> hash(R, 0);
    std::vector<Row> row(R);
    for (uint64_t k = 0; k < R; k++) {
        row[k] = row_of(offsets, valid, k, bytes_len);
        hash[k] = hash_finish(hash_piece(bytes + row[k].at, row[k].len, 0, 1), row[k].len, flags);
    }
    HostTable t{table};
    for (uint64_t j = 0; j < R; j++) {
        const uint64_t k = order ? R - 1 - j : j;
        if (!row[k].has) continue;
        const Row y = row[k];
        const uint64_t hy = hash[k];
        const Walk wk = insert_row(t, S, hy, (uint32_t)k, [&](uint32_t r) {
            return hash[r] == hy && row[r].len == y.len && equal_piece(bytes + y.at, bytes + row[r].at, y.len, 0, 1);
        });
        slot[k] = (uint32_t)wk.slot;
        if (wk.probes > out->max_probe) out->max_probe = wk.probes;
        if (!wk.found) out->code = kExhausted;
    }
    if (dict_offsets) dict_offsets[0] = 0;
    uint64_t n = 0, total = 0;
    for (uint64_t k = 0; k < R; k++) {
        if (!row[k].has) {
            codes[k] = -1;
            continue;
        }
        out->n_values++;
        const uint32_t r = table[slot[k]];
        if (r != k) {
            codes[k] = codes[r];  // (r < k: the slot holds the smallest row of the value)
            continue;
        }
        codes[k] = (int32_t)n;
        if (n < dict_capacity) dict_first[n] = (uint32_t)k, dict_offsets[n + 1] = total + row[k].len;
        if (dict_bytes && n < dict_capacity)
            for (uint64_t b = 0; b < row[k].len && total + b < dict_bytes_capacity; b++) dict_bytes[total + b] = bytes[row[k].at + b];
        n++, total += row[k].len;
    }
    out->n_distinct = n, out->dict_bytes = total;
    const bool layout_only = !dict_offsets && !dict_first && !dict_bytes;
    if (out->code == 0) out->code = dict_code(n, total, layout_only, dict_capacity, dict_bytes_capacity);
}

// the hash of one value, its sum taken in `pieces` strided pieces, the last piece first
uint64_t dcm_hash(const uint8_t *p, uint64_t len, uint32_t flags, uint64_t pieces) {
    uint64_t sum = 0;
    for (uint64_t j = pieces; j-- > 0;) sum += hash_piece(p, len, j, pieces);
    return hash_finish(sum, len, flags);
}
uint64_t dcm_table_slots(uint64_t R) { return table_slots(R); }
int dcm_equal(const uint8_t *a, const uint8_t *b, uint64_t len, uint64_t pieces) {
    int eq = 1;
    for (uint64_t j = 0; j < pieces; j++) eq &= equal_piece(a, b, len, j, pieces) ? 1 : 0;
    return eq;
}

}  // extern "C"
