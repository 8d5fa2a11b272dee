// Test-only harness: compiles mojo_simdjson_amd/csrc/object_entries_math.h for the host (g++), so that the arithmetic of
// msj_object_entries_device -- the same verdict on the rows, live rows, order test, row test, candidate test, entry test, code
// rule and records the kernels compute (csrc/object_entries_kernel.hip) -- is checked on a CPU-only box against the definition
// written in Python (tests/test_object_entries_math.py), and so that the GPU tests have an expected value.  NOT part of the
// product.
#include <string.h>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/object_entries_math.h"

namespace oem {

using namespace msj::oent;

// MSJ_TWIN_NO_DEPTH_CLAUSE / MSJ_TWIN_NO_COLON_CLAUSE: the mutations tests/test_object_entries_math.py names -- the entry test
// without its depth clause, the candidate test without its ':' clause
static bool entry_of(uint64_t i, int32_t depth_i, const Desc &d) {
#ifdef MSJ_TWIN_NO_DEPTH_CLAUSE
    return i > (uint64_t)d.v && i + 2 < (uint64_t)d.m;
#else
    return is_entry_of(i, depth_i, d);
#endif
}
static bool key_candidate(uint32_t t, uint32_t t_next) {
#ifdef MSJ_TWIN_NO_COLON_CLAUSE
    return t == '"';
#else
    return is_key_candidate(t, t_next);
#endif
}

}  // namespace oem

extern "C" {

// The whole call, the definition's way: row by row; a live row's tokens are those behind its own token up to and including
// the next live row's.  rows_select / nr: host copies of the device structs; numbers, nr, keys + values, the two select
// results may be NULL as in the call.
void oem_object_entries(const uint32_t *idx, uint64_t n, const uint8_t *typ, const int32_t *dep, const uint32_t *mat, const uint32_t *end,
                        const uint8_t *flags, const msj_number *numbers, uint64_t numbers_capacity, const msj_numbers_result *nr,
                        const msj_field *rows, const msj_select_documents_result *rows_select, uint64_t *offsets, uint8_t *valid,
                        uint64_t capacity, msj_field *keys, msj_field *values, uint64_t entries_capacity, msj_object_entries_result *out,
                        msj_select_documents_result *keys_select, msj_select_documents_result *values_select) {
    using namespace oem;
    memset(out, 0, sizeof *out);
    const uint64_t R = rows_select->n_documents;
    uint64_t n_rows;
    out->code = head_code(rows_select->code, R, capacity, n_rows);
    out->n_rows = n_rows;
    if (out->code == 0) {
        bool have = false;
        uint32_t prev = 0;
        for (uint64_t r = 0; r < R && out->code == 0; r++) {
            if (!is_live(rows[r].code)) continue;
            if (have && !in_order(prev, rows[r].token)) out->code = msj::oent::kBadArgument;
            have = true, prev = rows[r].token;
        }
    }
    if (out->code == 0) {
        uint64_t n_records = 0;
        if (numbers && nr) n_records = nr->n_numbers < numbers_capacity ? nr->n_numbers : numbers_capacity;
        const msj_number *records = n_records ? numbers : nullptr;
        uint64_t total = 0;
        for (uint64_t r = 0; r < R; r++) {
            offsets[r] = total;
            valid[r] = 0;
            if (!is_live(rows[r].code)) continue;
            bool other;
            const Desc d = msj::oent::row_of(rows[r], n, typ, dep, mat, other);
            valid[r] = (uint8_t)d.valid;
            out->n_objects += d.valid, out->n_other += other;
            if (!d.valid) continue;
            uint64_t last = 0xFFFFFFFFull;  // the last token that is this row's: the next live row's own
            for (uint64_t q = r + 1; q < R; q++)
                if (is_live(rows[q].code)) {
                    last = rows[q].token;
                    break;
                }
            for (uint64_t i = (uint64_t)d.v + 1; i + 2 < d.m && i <= last; i++) {  // (m < n: i + 1 indexes the arrays)
                if (!key_candidate(typ[i], typ[i + 1]) || !entry_of(i, dep[i], d)) continue;
                if (keys && total < entries_capacity) {
                    keys[total] = value_field<msj_field, msj_number>(i, idx, typ, mat, end, flags, records, n_records);
                    const msj_field rec = value_field<msj_field, msj_number>(i + 2, idx, typ, mat, end, flags, records, n_records);
                    values[total] = rec;
                    out->n_no_bits += (rec.flags & kFieldNoBits) != 0;
                }
                total++;
            }
        }
        if (offsets) offsets[R] = total;  // (NULL only with capacity 0: R is 0 then)
        out->n_entries = total;
        out->code = entries_code(total, keys != nullptr, entries_capacity);
    }
    msj_select_documents_result *both[2] = {keys_select, values_select};
    for (int k = 0; k < 2; k++) {
        if (!both[k]) continue;
        memset(both[k], 0, sizeof *both[k]);
        both[k]->code = out->code;
        both[k]->n_documents = both[k]->n_found = out->n_entries;
        both[k]->n_paths = 1;
        both[k]->n_no_bits = k ? out->n_no_bits : 0;
    }
}

// the pieces on their own
int oem_is_key_candidate(uint32_t t, uint32_t t_next) { return msj::oent::is_key_candidate(t, t_next); }
int oem_is_entry_of(uint64_t i, int32_t depth_i, uint32_t v, uint32_t m, int32_t child_depth) {
    return msj::oent::is_entry_of(i, depth_i, msj::oent::Desc{v, m, child_depth, 1u});
}

}  // extern "C"
