// Test-only harness: compiles mojo_simdjson_amd/csrc/filter_rows_math.h for the host (g++), so that the arithmetic of
// msj_predicates_create, msj_filter_rows_device and msj_take_rows_device -- the same compile step, exact number compare,
// string compares, row verdict and offset gather the kernels run (csrc/filter_rows_kernel.hip) -- is checked on a CPU-only
// box against a yardstick written in Python (tests/test_filter_rows_math.py), and so that the GPU tests have an expected
// value.  NOT part of the product.
#include <string.h>

#include <vector>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/filter_rows_math.h"

using namespace msj::frows;
using msj::val::ByteReader;

extern "C" {

uint64_t frm_predicates_bytes(void) { return sizeof(Predicates); }
// msj_predicates_create's host part into `out` (frm_predicates_bytes bytes) -> 0 or -1
int frm_compile(const msj_predicate *specs, uint32_t n, uint32_t flags, void *out) {
    return compile_predicates(specs, n, flags, *static_cast<Predicates *>(out));
}

// the pieces on their own
int frm_cmp_int_double(int64_t i, double d) { return cmp_int_double(i, d); }
int frm_starts_with(const uint8_t *buf, uint64_t len, uint64_t b, uint64_t q, int escaped, const uint8_t *seg, uint32_t n) {
    return starts_with(ByteReader{buf, len}, b, q, escaped != 0, seg, n);
}
// predicate i on one record -> kHolds | kMetCode | kMetNoBits
uint32_t frm_eval(const void *preds, uint32_t i, const msj_field *f, const uint8_t *buf, uint64_t len) {
    const Predicates &P = *static_cast<const Predicates *>(preds);
    return eval_pred(P.p[i], P.bytes[i], *f, ByteReader{buf, len});
}

// The whole filter call, serially.  sel, list_n_rows: host copies of the device words.  -> 0, or -1 for what the entry point
// refuses on the host (a predicate's column at or past n_columns)
int frm_filter_rows(const void *preds, const uint8_t *buf, uint64_t len, const msj_field *fields, uint64_t stride, uint32_t n_columns,
                    const msj_select_documents_result *sel, uint8_t *keep, uint32_t *kept, uint64_t capacity, const uint64_t *list_offsets,
                    uint64_t list_rows, const uint64_t *list_n_rows, uint64_t *list_out, msj_filter_rows_result *out,
                    msj_select_documents_result *kept_select) {
    const Predicates &P = *static_cast<const Predicates *>(preds);
    if (n_columns == 0 || n_columns > kMaxColumns || P.max_column >= n_columns) return -1;
    const ByteReader r{buf, len};
    memset(out, 0, sizeof *out);
    if (kept_select) memset(kept_select, 0, sizeof *kept_select), kept_select->n_paths = 1;
    if (sel->code != 0) {
        out->code = sel->code;
        if (kept_select) kept_select->code = sel->code;
        return 0;
    }
    const uint64_t R = sel->n_documents;
    out->n_rows = R, out->flags = P.flags;
    if (rows_over(R, capacity)) {
        out->code = MSJ_CAPACITY;
        if (kept_select) kept_select->code = MSJ_CAPACITY;
        return 0;
    }
    std::vector<uint32_t> rank(R);
    uint64_t n_kept = 0;
    for (uint64_t k = 0; k < R; k++) {
        RowVerdict v = verdict_begin();
        for (uint32_t i = 0; i < P.n; i++) verdict_add(v, eval_pred(P.p[i], P.bytes[i], fields[(uint64_t)P.p[i].column * stride + k], r));
        const bool kp = row_kept(v, P.flags);
        keep[k] = kp;
        rank[k] = (uint32_t)n_kept;
        if (kp && kept) kept[n_kept] = (uint32_t)k;
        n_kept += kp;
        out->n_missing += (v.met & kMetCode) != 0, out->n_no_bits += (v.met & kMetNoBits) != 0;
    }
    out->n_kept = n_kept;
    if (list_offsets) {
        const uint64_t Pn = list_n_rows ? *list_n_rows : list_rows;
        if (rows_over(Pn, list_rows)) out->code = MSJ_CAPACITY;
        else
            for (uint64_t q = 0; q <= Pn; q++) list_out[q] = rebased_offset(list_offsets[q], R, rank.data(), n_kept);
    }
    if (kept_select) kept_select->code = out->code, kept_select->n_documents = kept_select->n_found = n_kept;
    return 0;
}

// The whole take call, serially
void frm_take_rows(const uint32_t *take, const msj_select_documents_result *take_sel, const msj_field *fields, uint64_t stride,
                   uint32_t n_columns, const msj_select_documents_result *rows_sel, msj_field *outf, uint64_t out_stride, uint64_t out_capacity,
                   msj_take_rows_result *out, msj_select_documents_result *out_select) {
    memset(out, 0, sizeof *out);
    if (out_select) memset(out_select, 0, sizeof *out_select), out_select->n_paths = n_columns;
    const int32_t code = take_sel->code != 0 ? take_sel->code : rows_sel->code;
    const uint64_t K = take_sel->n_documents, R = rows_sel->n_documents;
    if (code == 0) out->n_rows = K;
    out->code = code != 0 ? code : take_over(K, out_capacity, R, stride) ? MSJ_CAPACITY : 0;
    if (out_select) out_select->code = out->code;
    if (out->code != 0) return;
    for (uint64_t j = 0; j < K; j++) {
        const uint64_t src = take[j];
        out->n_out_of_range += src >= R;
        for (uint32_t c = 0; c < n_columns; c++) {
            const msj_field f = src < R ? fields[(uint64_t)c * stride + src] : missing_field<msj_field>();
            out->n_found += f.code == 0, out->n_no_bits += (f.flags & kFieldNoBits) != 0;
            outf[(uint64_t)c * out_stride + j] = f;
        }
    }
    if (out_select) out_select->n_documents = K, out_select->n_found = out->n_found, out_select->n_no_bits = out->n_no_bits;
}

}  // extern "C"
