// Test-only harness: compiles mojo_simdjson_amd/csrc/array_column_math.h for the host (g++), so that the arithmetic of
// msj_array_column_device -- the same row test, element test, code rule and records the kernels compute
// (csrc/array_column_kernel.hip) -- is checked on a CPU-only box against the definition written in Python
// (tests/test_array_column_math.py), and so that the GPU tests have an expected value.  NOT part of the product.
#include <string.h>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/array_column_math.h"

using namespace msj::acol;

extern "C" {

// The whole call, the definition's way: row by row, the tokens between an array and its partner in token order.  docs, nr,
// sel: host copies of the device structs; numbers, nr, elements, elements_select may be NULL as in the call.
void acm_array_column(const uint32_t *idx, uint64_t n, const uint8_t *typ, const int32_t *dep, const uint32_t *mat, const uint32_t *end,
                      const uint8_t *flags, const uint32_t *first, const msj_documents_result *docs, const msj_number *numbers,
                      uint64_t numbers_capacity, const msj_numbers_result *nr, const msj_field *column,
                      const msj_select_documents_result *sel, uint64_t *offsets, uint8_t *valid, uint64_t capacity, msj_field *elements,
                      uint64_t elements_capacity, msj_array_column_result *out, msj_select_documents_result *elements_select) {
    const Window win = window_of(docs->n_complete, docs->tokens_complete, n, capacity, (docs->n_complete > 0 && n > 0) ? first[0] : 0);
    memset(out, 0, sizeof *out);
    if (elements_select) memset(elements_select, 0, sizeof *elements_select);
    uint64_t n_rows;
    out->code = head_code(sel->code, sel->n_documents, win, n_rows);
    out->n_rows = n_rows;
    if (out->code == 0) {
        uint64_t n_records = 0;
        if (numbers && nr) n_records = nr->n_numbers < numbers_capacity ? nr->n_numbers : numbers_capacity;
        const msj_number *records = n_records ? numbers : nullptr;
        uint64_t total = 0;
        for (uint64_t k = 0; k < win.D; k++) {
            uint64_t f, e;
            const bool ok = document_bounds(first, win, k, f, e);
            bool other;
            const Desc d = row_of(column[k], ok, f, e, typ, dep, mat, other);
            valid[k] = (uint8_t)d.valid;
            out->n_arrays += d.valid, out->n_other += other;
            offsets[k] = total;
            if (!d.valid) continue;
            for (uint64_t i = (uint64_t)d.v + 1; i < d.m; i++) {
                if (!is_candidate(typ[i - 1], typ[i]) || !is_element_of(i, dep[i], d)) continue;
                if (elements && total < elements_capacity) {
                    const msj_field rec = value_field<msj_field, msj_number>(i, idx, typ, mat, end, flags, records, n_records);
                    elements[total] = rec;
                    out->n_no_bits += (rec.flags & kFieldNoBits) != 0;
                }
                total++;
            }
        }
        if (offsets) offsets[win.D] = total;  // (NULL only with capacity 0: D is 0 then)
        out->n_elements = total;
        out->code = elements_code(total, elements != nullptr, elements_capacity);
    }
    if (elements_select) {
        elements_select->code = out->code;
        elements_select->n_documents = elements_select->n_found = out->n_elements;
        elements_select->n_paths = 1;
        elements_select->n_no_bits = out->n_no_bits;
    }
}

// the pieces on their own
int acm_is_candidate(uint32_t t_prev, uint32_t t) { return is_candidate(t_prev, t); }
// -> valid | other << 1; v, m, child_depth: the descriptor
int acm_row(const msj_field *r, int bounds_ok, uint64_t f, uint64_t e, const uint8_t *typ, const int32_t *dep, const uint32_t *mat, uint32_t *v,
            uint32_t *m, int32_t *child_depth) {
    bool other;
    const Desc d = row_of(*r, bounds_ok != 0, f, e, typ, dep, mat, other);
    *v = d.v, *m = d.m, *child_depth = d.child_depth;
    return (int)d.valid | ((int)other << 1);
}

}  // extern "C"
