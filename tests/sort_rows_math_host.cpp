// Test-only harness: compiles mojo_simdjson_amd/csrc/sort_rows_math.h for the host (g++), so that the arithmetic of
// msj_sort_rows_device -- the same value test, key and verdicts the kernels run (csrc/sort_rows_kernel.hip) -- is checked on a
// CPU-only box against the definition written in Python with Fraction (tests/test_sort_rows_math.py), and so that the GPU
// tests have an expected value.  The order itself is a serial stable sort of the keys.  NOT part of the product.
#include <string.h>

#include <algorithm>
#include <vector>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/sort_rows_math.h"

using namespace msj::srows;

namespace {
bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
}  // namespace

extern "C" {

// the pieces on their own: out = {hi, lo, null}
uint32_t srm_value_kind(const msj_field *f) { return value_kind(*f); }
void srm_key(const msj_field *f, uint32_t flags, uint64_t *out) {
    const Key k = make_key(value_kind(*f) == kValue, f->type, f->bits, flags);
    out[0] = k.hi, out[1] = k.lo, out[2] = k.null;
}
uint32_t srm_digit(uint64_t hi, uint64_t aux, uint32_t d) { return digit_of(hi, aux, d); }
uint64_t srm_aux(uint64_t lo, uint64_t null, uint64_t position) { return aux_word(Key{0, (uint32_t)lo, (uint32_t)null}, position); }
int32_t srm_takes_selection(uint32_t mode, uint64_t limit, uint64_t N) { return takes_selection(mode, limit, N); }
// the radix passes a column of n records takes: the key's digits that are not the same in every row
uint32_t srm_passes(const msj_field *fields, uint64_t n, uint32_t flags) {
    uint32_t first[kDigits] = {}, differs = 0;
    for (uint64_t k = 0; k < n; k++) {
        const Key key = make_key(value_kind(fields[k]) == kValue, fields[k].type, fields[k].bits, flags);
        const uint64_t aux = aux_word(key, 0);
        for (uint32_t d = 0; d < kDigits; d++) {
            const uint32_t x = digit_of(key.hi, aux, d);
            if (k == 0) first[d] = x;
            else if (x != first[d]) differs |= 1u << d;
        }
    }
    return (uint32_t)__builtin_popcount(differs);
}

// The whole call, serially.  The select results: host copies of the device words.  -> 0, or what the entry point refuses on
// the host: MSJ_ERR_BAD_ARGUMENT / MSJ_CAPACITY, in the header's order, with nothing written
int32_t srm_sort_rows(const msj_field *fields, uint64_t stride, const msj_select_documents_result *sel, const uint32_t *rows_in,
                      const msj_select_documents_result *in_sel, uint32_t flags, uint64_t limit, uint32_t *order, uint64_t capacity,
                      msj_sort_rows_result *res, msj_select_documents_result *order_sel) {
    if (!res || !sel) return MSJ_ERR_BAD_ARGUMENT;
    if ((rows_in == nullptr) != (in_sel == nullptr)) return MSJ_ERR_BAD_ARGUMENT;
    if ((stride > 0 && !fields) || (capacity > 0 && !order)) return MSJ_ERR_BAD_ARGUMENT;
    if (flags & ~kKnownFlags) return MSJ_ERR_BAD_ARGUMENT;
    if (stride >= (1ull << 40) || capacity >= (1ull << 40)) return MSJ_CAPACITY;
    if ((const void *)res == (const void *)sel || (const void *)res == (const void *)in_sel || (const void *)res == (const void *)order_sel)
        return MSJ_ERR_BAD_ARGUMENT;
    if (order_sel && (order_sel == sel || order_sel == in_sel)) return MSJ_ERR_BAD_ARGUMENT;
    if (order && rows_in) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(rows_in), b = reinterpret_cast<uintptr_t>(order);
        const uint64_t b_rows = limit > 0 && limit < capacity ? limit : capacity;
        if (a < b + 4 * b_rows && b < a + 4 * capacity) return MSJ_ERR_BAD_ARGUMENT;
    }
    if (!aligned_to(fields, 16) || !aligned_to(order, 4) || !aligned_to(rows_in, 4) || !aligned_to(sel, 8) || !aligned_to(in_sel, 8) ||
        !aligned_to(res, 8) || !aligned_to(order_sel, 8))
        return MSJ_ERR_BAD_ARGUMENT;

    const int32_t in_code = in_sel ? in_sel->code : 0;
    const uint64_t R = sel->n_documents, N = rows_in ? in_sel->n_documents : R;
    memset(res, 0, sizeof *res);
    res->code = head_code(in_code, sel->code, R, stride, N, capacity, MSJ_CAPACITY);
    const bool skip = in_code != 0 || sel->code != 0;
    if (!skip) res->flags = flags, res->n_rows = N;
    std::vector<uint32_t> sorted;
    if (res->code == 0) {
        std::vector<Key> keys(N);
        for (uint64_t j = 0; j < N; j++) {
            const uint64_t row = rows_in ? rows_in[j] : j;
            keys[j] = Key{0, 0, 1};
            if (row >= R) {
                res->n_out_of_range++;
                continue;
            }
            const uint32_t kind = value_kind(fields[row]);
            res->n_values += kind == kValue, res->n_skipped += kind == kSkipped;
            keys[j] = make_key(kind == kValue, fields[row].type, fields[row].bits, flags);
        }
        sorted.resize(N);
        for (uint64_t j = 0; j < N; j++) sorted[j] = (uint32_t)j;
        std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return key_less(keys[a], keys[b]); });
        res->n_written = rows_written(flags, limit, N, res->n_values);
        for (uint64_t i = 0; i < res->n_written; i++) order[i] = rows_in ? rows_in[sorted[i]] : sorted[i];
    }
    if (order_sel) {
        memset(order_sel, 0, sizeof *order_sel);
        order_sel->code = res->code, order_sel->n_documents = order_sel->n_found = res->n_written, order_sel->n_paths = 1;
    }
    return 0;
}

}  // extern "C"
