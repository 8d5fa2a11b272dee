// Test-only harness: compiles mojo_simdjson_amd/csrc/join_rows_math.h for the host (g++), so that the arithmetic of
// msj_join_rows_device -- the same key test, digits, pairs per row, pair-to-row search and pair the kernels run
// (csrc/join_rows_kernel.hip) -- is checked on a CPU-only box against the definition written in Python
// (tests/test_join_rows_math.py), and so that the GPU tests have an expected value.  The whole call serially, in the
// kernels' steps: count[key], a stable order of the right rows by the key's digits, the runs, n(l) and the offsets, then
// every pair BY ITS POSITION through row_of_pair.  NOT part of the product.
#include <string.h>

#include <vector>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/join_rows_math.h"

using namespace msj::jrows;

namespace {
bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
bool overlaps(const void *p, unsigned __int128 p_bytes, const void *q, unsigned __int128 q_bytes) {
    const unsigned __int128 a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return p && q && a < b + q_bytes && b < a + p_bytes;
}
}  // namespace

extern "C" {

// the pieces on their own
int32_t jrm_is_key(int32_t key, uint64_t G) { return is_key(key, G); }
uint32_t jrm_key_digits(uint64_t G) { return key_digits(G); }
uint32_t jrm_key_passes(uint64_t G) { return key_passes(G); }
uint32_t jrm_digit(uint32_t key, uint32_t pass) { return digit_of(key, pass); }
uint64_t jrm_pairs_of_row(uint32_t kind, uint64_t c) { return pairs_of_row(kind, c); }
uint64_t jrm_row_of_pair(const uint64_t *offsets, uint64_t lo, uint64_t hi, uint64_t j) { return row_of_pair(offsets, lo, hi, j); }

// The whole call, serially; ctx_ok: whether the context is given.  -> 0, or what the entry point refuses on the host:
// MSJ_ERR_BAD_ARGUMENT / MSJ_CAPACITY, in the header's order, with nothing written
int32_t jrm_join_rows(int32_t ctx_ok, const int32_t *left_keys, uint64_t left_rows, const uint64_t *n_left, const int32_t *right_keys,
                      uint64_t right_rows, const uint64_t *n_right, uint64_t n_keys, const uint64_t *d_n_keys, uint64_t keys_capacity,
                      uint32_t flags, uint32_t *out_left, uint32_t *out_right, uint64_t pairs_capacity, uint64_t *offsets,
                      msj_join_rows_result *res, msj_select_documents_result *left_sel, msj_select_documents_result *right_sel) {
    if (!ctx_ok || !res) return MSJ_ERR_BAD_ARGUMENT;
    if ((left_rows > 0 && !left_keys) || (right_rows > 0 && !right_keys)) return MSJ_ERR_BAD_ARGUMENT;
    if (pairs_capacity > 0 && !out_left) return MSJ_ERR_BAD_ARGUMENT;
    if (flags & ~kKnownFlags) return MSJ_ERR_BAD_ARGUMENT;
    if (offsets) {
        const unsigned __int128 bytes = ((unsigned __int128)left_rows + 1) * 8;
        if (overlaps(left_keys, (unsigned __int128)left_rows * 4, offsets, bytes) || overlaps(right_keys, (unsigned __int128)right_rows * 4, offsets, bytes) ||
            overlaps(n_left, 8, offsets, bytes) || overlaps(n_right, 8, offsets, bytes) || overlaps(d_n_keys, 8, offsets, bytes))
            return MSJ_ERR_BAD_ARGUMENT;
    }
    if (left_rows >= (1ull << 40) || right_rows >= (1ull << 40) || keys_capacity >= (1ull << 40) || pairs_capacity >= (1ull << 40)) return MSJ_CAPACITY;
    if (!aligned_to(left_keys, 4) || !aligned_to(right_keys, 4) || !aligned_to(out_left, 4) || !aligned_to(out_right, 4) || !aligned_to(offsets, 8) ||
        !aligned_to(n_left, 8) || !aligned_to(n_right, 8) || !aligned_to(d_n_keys, 8) || !aligned_to(res, 8) || !aligned_to(left_sel, 8) ||
        !aligned_to(right_sel, 8))
        return MSJ_ERR_BAD_ARGUMENT;
    if ((const void *)res == (const void *)left_sel || (const void *)res == (const void *)right_sel) return MSJ_ERR_BAD_ARGUMENT;

    const uint64_t L = n_left ? *n_left : left_rows, R = n_right ? *n_right : right_rows, G = d_n_keys ? *d_n_keys : n_keys;
    const uint32_t kind = flags & 3u;
    memset(res, 0, sizeof *res);
    res->flags = flags, res->n_left = L, res->n_right = R, res->n_keys = G;
    const bool stop = counts_over(L, left_rows, R, right_rows, G, keys_capacity);
    uint64_t M = 0;
    if (!stop) {
        const uint64_t keys = most_keys(G);
        // count[key], then the right rows with a key in the stable order of the key's digits, the least significant first
        std::vector<uint32_t> start(keys + 1, 0), key_a, row_a, key_b, row_b;
        for (uint64_t r = 0; r < R; r++) {
            if (!is_key(right_keys[r], keys)) {
                res->n_right_null++;
                continue;
            }
            start[right_keys[r]]++;
            key_a.push_back((uint32_t)right_keys[r]), row_a.push_back((uint32_t)r);
        }
        const uint64_t valid = key_a.size();
        key_b.resize(valid), row_b.resize(valid);
        for (uint32_t p = 0; p < key_passes(G); p++) {
            uint64_t at[kBuckets + 1] = {};
            for (uint64_t i = 0; i < valid; i++) at[digit_of(key_a[i], p) + 1]++;
            for (uint32_t b = 0; b < kBuckets; b++) at[b + 1] += at[b];
            for (uint64_t i = 0; i < valid; i++) {
                const uint64_t to = at[digit_of(key_a[i], p)]++;
                key_b[to] = key_a[i], row_b[to] = row_a[i];
            }
            key_a.swap(key_b), row_a.swap(row_b);
        }
        uint32_t run = 0;
        for (uint64_t k = 0; k <= keys; k++) {
            const uint32_t c = start[k];
            start[k] = run, run += c;
        }
        // the left rows
        std::vector<uint64_t> own(L + 1);
        std::vector<uint32_t> runs(L);
        for (uint64_t l = 0; l < L; l++) {
            uint32_t c = 0, first = 0;
            if (is_key(left_keys[l], keys)) first = start[left_keys[l]], c = start[(uint64_t)left_keys[l] + 1] - first;
            else res->n_left_null++;
            res->n_left_matched += c != 0;
            own[l] = M, M += pairs_of_row(kind, c);
            runs[l] = run_of_row(kind, c, first);
        }
        own[L] = M;
        if (offsets) memcpy(offsets, own.data(), 8 * (L + 1));
        // the pairs, by position
        if (!pairs_over(M, pairs_capacity)) {
            for (uint64_t j = 0; j < M; j++) {
                const uint64_t l = row_of_pair(own.data(), 0, L, j);
                out_left[j] = (uint32_t)l;
                if (!out_right) continue;
                const uint32_t place = right_place(kind, runs[l], j - own[l]);
                out_right[j] = place == kNoRow ? kNoRow : row_a[place];
            }
        }
    }
    res->n_pairs = M;
    res->code = stop || pairs_over(M, pairs_capacity) ? MSJ_CAPACITY : 0;
    msj_select_documents_result s;
    memset(&s, 0, sizeof s);
    s.code = res->code, s.n_documents = s.n_found = M, s.n_paths = 1;
    if (left_sel) *left_sel = s;
    if (right_sel) *right_sel = s;
    return 0;
}

}  // extern "C"
