// Test-only harness: compiles mojo_simdjson_amd/csrc/array_elements_math.h for the host (g++), so that the arithmetic of
// msj_array_elements_device -- the same verdict on the rows, live rows, order test, row test, element test, code rule and
// records the kernels compute (csrc/array_elements_kernel.hip) -- is checked on a CPU-only box against the definition written
// in Python (tests/test_array_elements_math.py), and so that the GPU tests have an expected value.  NOT part of the product.
#include <string.h>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/array_elements_math.h"

using namespace msj::aelem;

// MSJ_TWIN_NO_DEPTH_CLAUSE: the mutation tests/test_array_elements_math.py names -- the element test without its depth clause
static bool element_of(uint64_t i, int32_t depth_i, const Desc &d) {
#ifdef MSJ_TWIN_NO_DEPTH_CLAUSE
    return i > (uint64_t)d.v && i < (uint64_t)d.m;
#else
    return is_element_of(i, depth_i, d);
#endif
}

extern "C" {

// The whole call, the definition's way: row by row; a live row's tokens are those behind its own token up to and including
// the next live row's.  rows_select / nr: host copies of the device structs; numbers, nr, elements, elements_select may be
// NULL as in the call.
void aem_array_elements(const uint32_t *idx, uint64_t n, const uint8_t *typ, const int32_t *dep, const uint32_t *mat, const uint32_t *end,
                        const uint8_t *flags, const msj_number *numbers, uint64_t numbers_capacity, const msj_numbers_result *nr,
                        const msj_field *rows, const msj_select_documents_result *rows_select, uint64_t *offsets, uint8_t *valid,
                        uint64_t capacity, msj_field *elements, uint64_t elements_capacity, msj_array_column_result *out,
                        msj_select_documents_result *elements_select) {
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
            if (have && !in_order(prev, rows[r].token)) out->code = msj::aelem::kBadArgument;  // (qualified: tests/cpp/array_elements_sanitize.cpp includes the sibling twins beside this one)
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
            const Desc d = row_of(rows[r], n, typ, dep, mat, other);
            valid[r] = (uint8_t)d.valid;
            out->n_arrays += d.valid, out->n_other += other;
            if (!d.valid) continue;
            uint64_t last = 0xFFFFFFFFull;  // the last token that is this row's: the next live row's own
            for (uint64_t q = r + 1; q < R; q++)
                if (is_live(rows[q].code)) {
                    last = rows[q].token;
                    break;
                }
            for (uint64_t i = (uint64_t)d.v + 1; i < d.m && i <= last; i++) {
                if (!is_candidate(typ[i - 1], typ[i]) || !element_of(i, dep[i], d)) continue;
                if (elements && total < elements_capacity) {
                    const msj_field rec = value_field<msj_field, msj_number>(i, idx, typ, mat, end, flags, records, n_records);
                    elements[total] = rec;
                    out->n_no_bits += (rec.flags & kFieldNoBits) != 0;
                }
                total++;
            }
        }
        if (offsets) offsets[R] = total;  // (NULL only with capacity 0: R is 0 then)
        out->n_elements = total;
        out->code = elements_code(total, elements != nullptr, elements_capacity);
    }
    if (elements_select) {
        memset(elements_select, 0, sizeof *elements_select);
        elements_select->code = out->code;
        elements_select->n_documents = elements_select->n_found = out->n_elements;
        elements_select->n_paths = 1;
        elements_select->n_no_bits = out->n_no_bits;
    }
}

// the pieces on their own
uint64_t aem_dense_rows(uint64_t n, uint64_t capacity) { return dense_rows(n, capacity); }
uint32_t aem_rank_word(uint64_t live_in_front, int live) { return rank_word(live_in_front, live != 0); }
uint64_t aem_offset_of_row(uint32_t word, uint64_t dense, const uint32_t *start, const uint64_t *dense_offset, uint64_t n, uint64_t n_elements) {
    return offset_of_row(word, dense, start, dense_offset, n, n_elements);
}

}  // extern "C"
