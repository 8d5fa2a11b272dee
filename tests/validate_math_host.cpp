// Test-only harness: compiles mojo_simdjson_amd/csrc/validate_math.h for the host (g++), so that the per-token rule of
// msj_validate_device (csrc/validate_kernel.hip) -- the same code the kernels run -- is checked against a serial walker
// on a CPU-only box, and so that the GPU tests have an expected value at any size.  NOT part of the product.
#include <string.h>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/validate_math.h"

using namespace msj::val;

namespace {
struct Arrays {
    const uint8_t *typ;
    const int32_t *dep;
    const uint32_t *mat;
    int64_t n;
    uint32_t type(int64_t j) const { return j >= 0 && j < n ? typ[j] : 0u; }
    uint32_t match(int64_t j) const { return j >= 0 && j < n ? mat[j] : kNoPartner; }
    int32_t depth(int64_t j) const { return dep[j]; }
};
}  // namespace

extern "C" {

// the whole call: numbers_first_error = msj_numbers_result.first_error, has_numbers = 0 for d_numbers == NULL
void vm_validate(const uint8_t *buf, uint64_t len, const uint32_t *idx, uint64_t n, const uint8_t *typ, const int32_t *dep,
                 const uint32_t *mat, const uint32_t *end, const uint8_t *flags, int32_t has_numbers, uint64_t numbers_first_error,
                 uint32_t max_depth, msj_validate_result *out) {
    const Arrays a{typ, dep, mat, (int64_t)n};
    const ByteReader r{buf, len};
    uint64_t best = kNoError, n_escaped = 0, n_big = 0;
    uint64_t big_open[MSJ_VALIDATE_BIG_CONTAINERS], big_close[MSJ_VALIDATE_BIG_CONTAINERS];
    for (int64_t i = 0; i <= (int64_t)n; i++) {
        uint32_t role;
        uint64_t e = kNoError;
        const uint32_t code = token_rule(a, i, (int64_t)n, max_depth, role);
        if (code) {
            e = pack_error((uint64_t)i, 0, code);
        } else if (role == kRoleScalar) {
            const uint32_t t = typ[i];
            if (t == '"') {
                if (flags[i] & MSJ_SPAN_ESCAPED) {
                    n_escaped++;
                    if (string_bad_serial(r, (uint64_t)idx[i] + 1, end[i])) e = pack_error((uint64_t)i, 1, kString);
                }
            } else if (t == 't' || t == 'f' || t == 'n') {
                const uint32_t c = atom_code(r, idx[i], t);
                if (c) e = pack_error((uint64_t)i, 1, c);
            }
        }
        if (e < best) best = e;
        if (i < (int64_t)n && is_close(typ[i]) && mat[i] != kNoPartner && mat[i] < (uint64_t)i && (uint64_t)i - mat[i] - 1 >= kBigSpan) {
            if (n_big < MSJ_VALIDATE_BIG_CONTAINERS) big_open[n_big] = mat[i], big_close[n_big] = (uint64_t)i;
            n_big++;
        }
    }
    uint32_t fl = has_numbers ? 0u : MSJ_VALIDATE_NUMBERS_UNCHECKED;
    if (has_numbers && numbers_first_error < n) {
        const uint64_t e = pack_error(numbers_first_error, 1, kNumber);
        if (e < best) best = e;
    }
    if (n_big > MSJ_VALIDATE_BIG_CONTAINERS) {
        fl |= MSJ_VALIDATE_COUNTS_CLIPPED;
    } else {
        for (uint64_t c = 0; c < n_big; c++) {
            uint64_t commas = 0;
            const int32_t d = dep[big_open[c]] + 1;
            for (uint64_t j = big_open[c] + 1; j < big_close[c]; j++) commas += (typ[j] == ',' && dep[j] == d);
            if (1 + commas > kMaxElements) {
                const uint64_t e = pack_error(big_close[c], 1, kCapacity);
                if (e < best) best = e;
            }
        }
    }
    out->flags = fl;
    out->n_escaped = n_escaped;
    if (best == kNoError) {
        out->code = 0;
        out->error_token = out->error_offset = ~0ull;
    } else {
        out->code = (int32_t)packed_code(best);
        out->error_token = packed_token(best);
        out->error_offset = out->error_token == n ? len : idx[out->error_token];
    }
}

// one string body [b, e): 1 if an escape is in error.  which = 0: the serial walk; 1: 64 bytes per step, every byte on
// its own (the way a wave takes a long body); 2: the same for each piece of `step` bytes on its own (the way the waves of
// the grid share a huge body)
int32_t vm_string_bad(const uint8_t *buf, uint64_t len, uint64_t b, uint64_t e, int32_t which, uint64_t step) {
    const ByteReader r{buf, len};
    if (which == 0) return string_bad_serial(r, b, e);
    if (which == 1) return string_bad_steps(r, b, e, b, e);
    bool bad = false;
    for (uint64_t lo = b; lo < e; lo += step) bad |= string_bad_steps(r, b, e, lo, lo + step < e ? lo + step : e);
    return bad;
}

}  // extern "C"
