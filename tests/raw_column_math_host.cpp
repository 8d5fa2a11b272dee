// Test-only harness: compiles mojo_simdjson_amd/csrc/raw_column_math.h for the host (g++), so that the arithmetic of
// msj_raw_column_device -- the same token texts, row test, lengths and searches the kernels compute
// (csrc/raw_column_kernel.hip) -- is checked on a CPU-only box against a yardstick written in Python
// (tests/test_raw_column_math.py), and so that the GPU tests have an expected value.  NOT part of the product.
#include <string.h>

#include <vector>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/raw_column_math.h"

using namespace msj::rcol;

namespace {
struct HostP {  // P of the header: n + 1 sums
    const uint64_t *p;
    uint64_t operator()(uint64_t i) const { return p[i]; }
};
std::vector<uint64_t> prefix(const Tokens &t) {
    std::vector<uint64_t> p(t.n + 1, 0);
    for (uint64_t i = 0; i < t.n; i++) p[i + 1] = p[i] + text_len(t, i);
    return p;
}
}  // namespace

extern "C" {

// The whole call, serially: the lengths, the offsets, then every output byte the way the copy kernels find it -- its row
// through row_of_byte over the offsets, its source through verbatim_source or, in the compact form, through the search in
// P.  sel: a host copy of the device struct
void rcm_raw_column(const uint8_t *buf, uint64_t len, const uint32_t *idx, uint64_t n, const uint8_t *type, const uint32_t *end,
                    const uint8_t *tflags, const msj_field *rows, const msj_select_documents_result *sel, uint64_t *offsets, uint8_t *valid,
                    uint64_t capacity, uint8_t *bytes, uint64_t bytes_capacity, uint32_t flags, msj_raw_column_result *out) {
    const Tokens t{buf, len, idx, n, type, end, tflags};
    const bool compact = (flags & kCompact) != 0;
    memset(out, 0, sizeof *out);
    out->flags = flags;
    if (sel->code != 0) {
        out->code = sel->code;
        return;
    }
    const uint64_t R = sel->n_documents;
    out->n_rows = R;
    if (rows_over(R, capacity)) {
        out->code = MSJ_CAPACITY;
        return;
    }
    std::vector<uint64_t> sums;
    if (compact) sums = prefix(t);
    const HostP P{sums.data()};
    if (offsets) offsets[0] = 0;
    uint64_t total = 0;
    for (uint64_t k = 0; k < R; k++) {
        const Row y = row_of(rows[k], n);
        valid[k] = y.valid;
        out->n_values += y.valid, out->n_containers += y.container, out->n_other += y.other;
        total += compact ? compact_len(P, y) : verbatim_len(t, y);
        offsets[k + 1] = total;
    }
    out->total_bytes = total;
    out->code = bytes_code(total, bytes != nullptr, bytes_capacity);
    if (!bytes) return;
    const uint64_t stop = total < bytes_capacity ? total : bytes_capacity;
    for (uint64_t pos = 0; pos < stop; pos++) {
        const uint32_t k = row_of_byte(offsets, (uint32_t)R, pos);
        const Row y = row_of(rows[k], n);
        const uint64_t o = pos - offsets[k];
        const uint64_t at = compact ? compact_source(t, P, y, P(y.token), o) : verbatim_source(idx[y.token], o);
        bytes[pos] = at < len ? buf[at] : 0xEE;  // (never: the header keeps every source inside the window)
        if (at >= len) out->code = -99;
    }
}

// the pieces on their own
uint64_t rcm_text_len(const uint8_t *buf, uint64_t len, const uint32_t *idx, uint64_t n, const uint8_t *type, const uint32_t *end,
                      const uint8_t *tflags, uint64_t i) {
    return text_len(Tokens{buf, len, idx, n, type, end, tflags}, i);
}
// -> valid | container << 1 | other << 2; token / last (0, 0 when not valid)
int rcm_row(const msj_field *f, uint64_t n, uint32_t *token, uint32_t *last) {
    const Row y = row_of(*f, n);
    *token = y.token, *last = y.last;
    return (int)y.valid | ((int)y.container << 1) | ((int)y.other << 2);
}
uint64_t rcm_token_of_byte(const uint64_t *p, uint64_t token, uint64_t last, uint64_t q) { return token_of_byte(HostP{p}, token, last, q); }

}  // extern "C"
