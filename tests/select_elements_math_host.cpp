// Test-only harness: compiles mojo_simdjson_amd/csrc/select_elements_math.h for the host (g++), so that the lookup of
// msj_select_elements_device -- the same verdict on the rows, order test, row states, member test, key compare and records the
// kernels compute (csrc/select_elements_kernel.hip) -- is checked on a CPU-only box against the definition written in Python
// (tests/test_select_elements_math.py), and so that the GPU tests have an expected value.  NOT part of the product.
#include <string.h>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/select_elements_math.h"

using namespace msj::selem;

extern "C" {

// The whole call, the definition's way: per (path, row) one serial lookup, level by level, over the members of the object
// reached -- the keys that belong to this row, i.e. those at or in front of the next row's token.  rows_select / nr: host
// copies of the device structs; numbers, nr may be NULL as in the call.
void sem_select_elements(const void *blob, const uint8_t *buf, uint64_t len, const uint32_t *idx, uint64_t n, const uint8_t *typ,
                         const int32_t *dep, const uint32_t *mat, const uint32_t *end, const uint8_t *flags, const msj_number *numbers,
                         uint64_t numbers_capacity, const msj_numbers_result *nr, const msj_field *rows,
                         const msj_select_documents_result *rows_select, msj_field *fields, uint64_t capacity,
                         msj_select_documents_result *out) {
    const Paths &paths = *static_cast<const Paths *>(blob);
    const msj::val::ByteReader r{buf, len};
    memset(out, 0, sizeof *out);
    const uint64_t R = rows_select->n_documents;
    out->code = head_code(rows_select->code, R, capacity, paths.n_paths, out->n_documents, out->n_paths);
    if (out->code != 0) return;
    for (uint64_t k = 1; k < R; k++)
        if (!in_order(rows[k - 1].token, rows[k].token)) {
            out->code = msj::selem::kBadArgument;
            return;
        }
    uint64_t n_records = 0;
    if (numbers && nr) n_records = nr->n_numbers < numbers_capacity ? nr->n_numbers : numbers_capacity;
    const msj_number *records = n_records ? numbers : nullptr;
    for (uint32_t p = 0; p < paths.n_paths; p++) {
        const uint32_t levels = paths.levels[p];
        for (uint64_t k = 0; k < R; k++) {
            // key i is this row's iff this is the last row whose token lies below i: token_k < i <= token_(k + 1)
            const uint64_t last_key = k + 1 < R ? rows[k + 1].token : 0xFFFFFFFFull;
            uint32_t s = row_state(rows[k].code, rows[k].type, rows[k].token, levels, n, typ, mat);
            for (uint32_t l = 0; l < levels && state_is_token(s); l++) {
                const uint32_t lo = s, m = mat[lo];  // (container_state: m in (lo, n))
                uint32_t found = kNotFound;
                for (uint64_t i = (uint64_t)lo + 1; i < m && i <= last_key && found == kNotFound; i++) {
                    if (!is_key(typ[i], typ[i + 1]) || !is_direct_member(i, dep[i], lo, dep[lo], m)) continue;  // (i + 1 <= m)
                    if (key_equals(r, (uint64_t)idx[i] + 1, end[i], (flags[i] & kSpanEscaped) != 0, paths.bytes[l][p], paths.len[l][p]))
                        found = (uint32_t)i;
                }
                s = next_state(s, found, l + 1 == levels, n, typ, mat);
            }
            const msj_field rec = field_of_state<msj_field, msj_number>(s, idx, typ, mat, end, flags, records, n_records);
            fields[p * capacity + k] = rec;
            out->n_found += rec.code == 0;
            out->n_no_bits += (rec.flags & kFieldNoBits) != 0;
        }
    }
}

// the pieces on their own
uint32_t sem_rows_below(const uint32_t *start, uint32_t count, uint32_t x) { return rows_below(start, count, x); }
uint64_t sem_state_rows(uint64_t n, uint64_t capacity) { return state_rows(n, capacity); }
uint32_t sem_row_state(uint32_t rec_code, uint32_t rec_type, uint32_t v, uint32_t levels, uint64_t n, const uint8_t *typ, const uint32_t *mat) {
    return row_state(rec_code, rec_type, v, levels, n, typ, mat);
}

}  // extern "C"
