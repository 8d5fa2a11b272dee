// Test-only harness: compiles mojo_simdjson_amd/csrc/cast_strings_math.h for the host (g++), so that the arithmetic of
// msj_cast_strings_device -- the same timestamp grammar, calendar, number wrapper and record-in / record-out the kernels run
// (csrc/cast_strings_kernel.hip) -- is checked on a CPU-only box against a yardstick written in Python
// (tests/test_cast_strings_math.py), and so that the GPU tests have an expected value.  NOT part of the product.
#include <string.h>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/cast_strings_math.h"

using namespace msj::cast;
using msj::val::ByteReader;

extern "C" {

// the pieces on their own: a value's bytes [0, n) -> the outcome (kCast 1, kSyntax 2, kRange 3)
int64_t csm_days_from_civil(uint32_t y, uint32_t m, uint32_t d) { return days_from_civil(y, m, d); }
uint32_t csm_parse_timestamp(const uint8_t *value, uint64_t n, uint32_t unit, uint64_t *bits) {
    return parse_timestamp(ByteReader{value, n}, 0, n, unit, *bits);
}
uint32_t csm_parse_number(const uint8_t *value, uint64_t n, uint64_t *bits, uint32_t *type) {
    return parse_number<true>(ByteReader{value, n}, 0, n, *bits, *type);
}
// one record -> the outcome (kPassed 0 .. kOther 4)
uint32_t csm_cast_record(const msj_field *f, const uint8_t *buf, uint64_t len, uint32_t kind, uint32_t unit, uint32_t flags, msj_field *out) {
    return cast_record(*f, ByteReader{buf, len}, kind, unit, flags, *out);
}

// The whole call, serially.  sel: a host copy of the device words; out may be rows (in place).  -> 0, or -1 for what the
// entry point refuses on the host (an unknown kind, unit or flag)
int csm_cast_strings(const uint8_t *buf, uint64_t len, const msj_field *rows, const msj_select_documents_result *sel, uint32_t kind,
                     uint32_t unit, uint32_t flags, msj_field *out, uint64_t capacity, msj_cast_strings_result *res,
                     msj_select_documents_result *out_select) {
    if (check_kind(kind, unit, flags) != 0) return -1;
    const ByteReader r{buf, len};
    memset(res, 0, sizeof *res);
    res->flags = result_flags(kind, unit, flags);
    if (out_select) memset(out_select, 0, sizeof *out_select), out_select->n_paths = 1;
    const uint64_t R = sel->n_documents;
    if (sel->code != 0) {
        res->code = sel->code;
    } else {
        res->n_rows = R;
        if (rows_over(R, capacity)) res->code = MSJ_CAPACITY;
    }
    if (out_select) out_select->code = res->code;
    if (res->code != 0) return 0;
    uint64_t n_no_bits = 0;
    for (uint64_t k = 0; k < R; k++) {
        const msj_field f = rows[k];
        msj_field o;
        const uint32_t outcome = cast_record(f, r, kind, unit, flags, o);
        out[k] = o;
        res->n_cast += outcome == kCast, res->n_syntax += outcome == kSyntax, res->n_range += outcome == kRange, res->n_other += outcome == kOther;
        n_no_bits += (o.flags & kFieldNoBits) != 0;
    }
    if (out_select) out_select->n_documents = R, out_select->n_found = res->n_cast, out_select->n_no_bits = n_no_bits;
    return 0;
}

}  // extern "C"
