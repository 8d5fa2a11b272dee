// Test-only harness: compiles mojo_simdjson_amd/csrc/select_math.h for the host (g++), so that the lookup of
// msj_select_documents_device -- the same pointer parser, member test, key compare, state words and records the kernels
// compute (csrc/select_kernel.hip) -- is checked on a CPU-only box against the definition written in Python
// (tests/select_reference.py), and so that the GPU tests have an expected value.  NOT part of the product.
#include <string.h>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/select_math.h"

using namespace msj::sel;
using msj::val::ByteReader;

extern "C" {

uint64_t sm_paths_bytes(void) { return sizeof(Paths); }

// msj_paths_create without the device: 0, 22, or -1 (what the entry point answers with MSJ_ERR_BAD_ARGUMENT).  levels_out:
// kMaxPaths entries
int sm_compile_paths(const char *const *pointers, uint32_t n_paths, void *blob, uint32_t *levels_out) {
    Paths *p = static_cast<Paths *>(blob);
    const int rc = compile_paths(pointers, n_paths, *p);
    if (rc == 0 && levels_out) memcpy(levels_out, p->levels, sizeof p->levels);
    return rc;
}
// segment l of path p of a compiled blob: its length (or -1: the path has no such segment), its bytes into out (256)
int sm_segment(const void *blob, uint32_t p, uint32_t l, uint8_t *out) {
    const Paths *b = static_cast<const Paths *>(blob);
    if (b->len[l][p] == kNoLevel) return -1;
    memcpy(out, b->bytes[l][p], b->len[l][p]);
    return b->len[l][p];
}

// The whole call, the definition's way: per (path, document) one serial lookup, level by level, over the members of the
// object reached -- with the state words, the compare and the record of select_math.h.  docs / nr: host copies of the
// device structs; verdicts, numbers, nr may be NULL as in the call.
void sm_select_documents(const void *blob, const uint8_t *buf, uint64_t len, const uint32_t *idx, uint64_t n, const uint8_t *typ,
                         const int32_t *dep, const uint32_t *mat, const uint32_t *end, const uint8_t *flags, const uint32_t *first,
                         const msj_documents_result *docs, const msj_number *numbers, uint64_t numbers_capacity,
                         const msj_numbers_result *nr, const msj_document_verdict *verdicts, msj_field *fields, uint64_t capacity,
                         msj_select_documents_result *out) {
    const Paths &paths = *static_cast<const Paths *>(blob);
    const ByteReader r{buf, len};
    const Window win = window_of(docs->n_complete, docs->tokens_complete, n, capacity, (docs->n_complete > 0 && n > 0) ? first[0] : 0);
    memset(out, 0, sizeof *out);
    out->code = win.over ? MSJ_CAPACITY : 0;
    out->n_documents = win.D;
    out->n_paths = paths.n_paths;
    if (win.over || win.D == 0) return;
    uint64_t n_records = 0;
    if (numbers && nr) n_records = nr->n_numbers < numbers_capacity ? nr->n_numbers : numbers_capacity;
    const msj_number *records = n_records ? numbers : nullptr;
    for (uint32_t p = 0; p < paths.n_paths; p++) {
        const uint32_t levels = paths.levels[p];
        for (uint64_t k = 0; k < win.D; k++) {
            uint64_t f, e;
            const bool ok = document_bounds(first, win, k, f, e);
            const int32_t code = verdicts ? verdicts[k].code : 0;
            uint32_t s = first_state(code, ok, levels, ok ? typ[f] : 0u, ok ? mat[f] : kNoPartner, f, e);
            for (uint32_t l = 0; l < levels && state_is_token(s); l++) {
                const uint32_t lo = s, m = mat[lo];  // (container_state: m in (lo, e))
                uint32_t found = kNotFound;
                for (uint64_t i = (uint64_t)lo + 1; i < m && found == kNotFound; i++) {
                    if (typ[i] != '"' || dep[i] != dep[lo] + 1 || typ[i + 1] != ':') continue;  // (i + 1 <= m)
                    if (key_equals(r, (uint64_t)idx[i] + 1, end[i], (flags[i] & kSpanEscaped) != 0, paths.bytes[l][p], paths.len[l][p]))
                        found = (uint32_t)i;
                }
                s = next_state(s, found, l + 1 == levels, e, typ, mat);
            }
            const msj_field rec = field_of_state<msj_field, msj_number>(s, idx, typ, mat, end, flags, records, n_records);
            fields[p * capacity + k] = rec;
            out->n_found += rec.code == 0;
            out->n_no_bits += (rec.flags & kFieldNoBits) != 0;
        }
    }
}

// the pieces on their own
uint32_t sm_state_code(uint32_t code) { return state_code(code); }
uint32_t sm_state_to_code(uint32_t s) { return state_to_code(s); }
int sm_length_may_match(uint64_t raw, int escaped, uint32_t n) { return length_may_match(raw, escaped != 0, n); }
int sm_key_equals(const uint8_t *buf, uint64_t len, uint64_t b, uint64_t q, int escaped, const uint8_t *seg, uint32_t n) {
    return key_equals(ByteReader{buf, len}, b, q, escaped != 0, seg, n);
}
int64_t sm_find_number(const msj_number *records, uint64_t n_records, uint32_t token) { return find_number(records, n_records, token); }

}  // extern "C"
