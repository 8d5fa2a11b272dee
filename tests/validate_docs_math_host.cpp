// Test-only harness: compiles mojo_simdjson_amd/csrc/validate_docs_math.h for the host (g++), so that the per-document form
// of the rule -- the same accessor and document look-up the kernels of msj_validate_documents_device run
// (csrc/validate_docs_kernel.hip) -- is checked on a CPU-only box against the one-document twin on every document's
// sub-arrays (tests/validate_math_host.cpp), and so that the GPU tests have an expected value.  NOT part of the product.
#include <string.h>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/validate_docs_math.h"

using namespace msj::val;

namespace {
// the window's arrays: nothing at or past T
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

// The whole call, the kernels' way: one loop over the window's tokens, every token with its document's [f, e), a minimum per
// document.  docs / numbers_result: host copies of the device structs (numbers_result NULL as in the call).  words: D
// uint64 of scratch.
void vdm_validate_documents(const uint8_t *buf, uint64_t len, const uint32_t *idx, uint64_t n, const uint8_t *typ, const int32_t *dep,
                            const uint32_t *mat, const uint32_t *end, const uint8_t *flags, const uint32_t *first,
                            const msj_documents_result *docs, const msj_number *numbers, uint64_t numbers_capacity,
                            const msj_numbers_result *nr, uint32_t max_depth, msj_document_verdict *verdicts, uint64_t capacity,
                            msj_validate_documents_result *out) {
    const uint64_t T = docs->tokens_complete < n ? docs->tokens_complete : n;
    uint64_t D = docs->n_complete < T ? docs->n_complete : T;
    memset(out, 0, sizeof *out);
    out->first_invalid = ~0ull;
    out->n_documents = D;
    if (D > capacity) {
        out->code = MSJ_CAPACITY;
        out->n_documents = docs->n_complete;
        return;
    }
    if (D == 0) return;
    const bool usable = nr && nr->n_errors > 0 && numbers && nr->n_numbers <= numbers_capacity;
    if (!nr || (nr->n_errors > 0 && !usable)) out->flags |= MSJ_VALIDATE_NUMBERS_UNCHECKED;
    uint64_t *word = reinterpret_cast<uint64_t *>(verdicts);  // two per document; the error word is the second
    for (uint64_t k = 0; k < D; k++) word[2 * k] = 0, word[2 * k + 1] = kNoError;
    auto report = [&](uint64_t tok, uint64_t e) {
        const uint64_t k = docs_starting_up_to(first, D, tok);
        if (k && e < word[2 * k - 1]) word[2 * k - 1] = e;
    };
    const Arrays a{typ, dep, mat, (int64_t)T};
    const ByteReader r{buf, len};
    uint64_t n_big = 0, big_open[MSJ_VALIDATE_BIG_CONTAINERS], big_close[MSJ_VALIDATE_BIG_CONTAINERS];
    uint64_t k_next = 0;   // documents that start at or in front of the token at hand
    int64_t f = -1;        // the start of the document that holds it
    for (int64_t i = 0; i <= (int64_t)T; i++) {
        const bool starts = k_next < D && first[k_next] == (uint64_t)i;
        uint32_t role;
        if ((starts || i == (int64_t)T) && f >= 0) {  // the end of the stream of the document in front
            const uint32_t code = doc_token_rule(a, f, i, i, max_depth, role);
            if (code) report((uint64_t)f, pack_error((uint64_t)i, 0, code));
        }
        if (starts) f = i, k_next++;
        if (i == (int64_t)T || f < 0) continue;
        const int64_t e = k_next < D ? (int64_t)first[k_next] : (int64_t)T;
        uint64_t err = kNoError;
        const uint32_t code = doc_token_rule(a, f, e, i, max_depth, role);
        if (code) {
            err = pack_error((uint64_t)i, 0, code);
        } else if (role == kRoleScalar) {
            const uint32_t t = typ[i];
            if (t == '"') {
                if (flags[i] & MSJ_SPAN_ESCAPED) {
                    out->n_escaped++;
                    if (string_bad_serial(r, (uint64_t)idx[i] + 1, end[i])) err = pack_error((uint64_t)i, 1, kString);
                }
            } else if (t == 't' || t == 'f' || t == 'n') {
                const uint32_t c = atom_code(r, idx[i], t);
                if (c) err = pack_error((uint64_t)i, 1, c);
            }
        }
        if (err != kNoError) report((uint64_t)f, err);
        if (is_close(typ[i]) && mat[i] != kNoPartner && (int64_t)mat[i] >= f && (int64_t)mat[i] < i &&
            (uint64_t)(i - (int64_t)mat[i] - 1) >= kBigSpan) {
            if (n_big < MSJ_VALIDATE_BIG_CONTAINERS) big_open[n_big] = mat[i], big_close[n_big] = (uint64_t)i;
            n_big++;
        }
    }
    if (usable)
        for (uint64_t j = 0; j < nr->n_numbers; j++)
            if (numbers[j].kind >= MSJ_NUMBER_ERR_SYNTAX && numbers[j].token < T) report(numbers[j].token, pack_error(numbers[j].token, 1, kNumber));
    if (n_big > MSJ_VALIDATE_BIG_CONTAINERS) {
        out->flags |= MSJ_VALIDATE_COUNTS_CLIPPED;
    } else {
        for (uint64_t c = 0; c < n_big; c++) {
            uint64_t commas = 0;
            const int32_t d = dep[big_open[c]] + 1;
            for (uint64_t j = big_open[c] + 1; j < big_close[c]; j++) commas += (typ[j] == ',' && dep[j] == d);
            if (1 + commas > kMaxElements) report(big_close[c], pack_error(big_close[c], 1, kCapacity));
        }
    }
    for (uint64_t k = 0; k < D; k++) {
        const uint64_t e = word[2 * k + 1];
        if (e == kNoError) continue;
        verdicts[k].code = (int32_t)packed_code(e);
        verdicts[k].reserved = 0;
        verdicts[k].error_token = packed_token(e);
        out->n_invalid++;
        if (k < out->first_invalid) out->first_invalid = k;
    }
}

// the document look-up on its own
uint64_t vdm_docs_starting_up_to(const uint32_t *first, uint64_t n_docs, uint64_t token) { return docs_starting_up_to(first, n_docs, token); }

}  // extern "C"
