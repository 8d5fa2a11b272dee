// Test-only harness: compiles mojo_simdjson_amd/csrc/string_column_math.h for the host (g++), so that the arithmetic of
// msj_string_column_device -- the same row test, lengths, code rule and byte -> row mapping the kernels compute
// (csrc/string_column_kernel.hip) -- is checked on a CPU-only box against the definition written in Python
// (tests/test_string_column_math.py), and so that the GPU tests have an expected value.  NOT part of the product.
#include <string.h>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/string_column_math.h"

using namespace msj::scol;
using msj::val::ByteReader;

namespace {
struct HostWriter {  // byte o of a row's body: checked against the capacity, like the kernels' writer
    uint8_t *out;
    uint64_t base, cap;
    void put(uint64_t o, uint32_t byte) const {
        const uint64_t a = base + o;
        if (out && a < cap) out[a] = (uint8_t)byte;
    }
};
}  // namespace

extern "C" {

// The whole call, serially: the lengths, the offsets, then the bytes the way the copy kernel goes -- every output byte of a
// plain row through row_of_byte over the offsets, every escaped row through tape_math.h's unescape into the checked
// writer.  sel: a host copy of the device struct
void scm_string_column(const uint8_t *buf, uint64_t len, const msj_field *column, const msj_select_documents_result *sel,
                       uint64_t *offsets, uint8_t *valid, uint64_t capacity, uint8_t *bytes, uint64_t bytes_capacity,
                       msj_string_column_result *out) {
    const ByteReader r{buf, len};
    memset(out, 0, sizeof *out);
    if (sel->code != 0) {
        out->code = sel->code;
        return;
    }
    const uint64_t D = sel->n_documents;
    out->n_rows = D;
    if (rows_over(D, capacity)) {
        out->code = MSJ_CAPACITY;
        return;
    }
    if (offsets) offsets[0] = 0;
    uint64_t total = 0;
    for (uint64_t k = 0; k < D; k++) {
        const Row y = row_of(column[k], len);
        valid[k] = y.valid;
        out->n_strings += y.valid, out->n_escaped += y.escaped, out->n_other += y.other;
        total += ulen(r, y);
        offsets[k + 1] = total;
    }
    out->total_bytes = total;
    out->code = bytes_code(total, bytes != nullptr, bytes_capacity);
    if (!bytes) return;
    const uint64_t end = total < bytes_capacity ? total : bytes_capacity;
    for (uint64_t pos = 0; pos < end; pos++) {
        const uint32_t k = row_of_byte(offsets, (uint32_t)D, pos);
        const Row y = row_of(column[k], len);
        if (!y.escaped) bytes[pos] = (uint8_t)r.at(y.b + (pos - offsets[k]));
    }
    for (uint64_t k = 0; k < D; k++) {
        const Row y = row_of(column[k], len);
        if (y.escaped) (void)unescape_serial(r, HostWriter{bytes, offsets[k], bytes_capacity}, y.b, y.b + y.r);
    }
}

// the pieces on their own
uint32_t scm_row_of_byte(const uint64_t *off, uint32_t n, uint64_t pos) { return row_of_byte(off, n, pos); }
// -> valid | escaped << 1 | other << 2; b / r: the span (0, 0 when not valid)
int scm_row(const msj_field *f, uint64_t len, uint64_t *b, uint64_t *r) {
    const Row y = row_of(*f, len);
    *b = y.b, *r = y.r;
    return (int)y.valid | ((int)y.escaped << 1) | ((int)y.other << 2);
}
uint64_t scm_ulen(const uint8_t *buf, uint64_t len, const msj_field *f) { return ulen(ByteReader{buf, len}, row_of(*f, len)); }
int scm_is_long(const msj_field *f, uint64_t len, uint32_t lane_body) { return is_long(row_of(*f, len), lane_body); }

}  // extern "C"
