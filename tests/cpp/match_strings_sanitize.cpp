// Stand-alone program (its own main; built by tests/test_match_strings_sanitizers.py with -fsanitize=address,undefined): the
// host form of the arithmetic of msj_patterns_create and msj_match_strings_device (tests/match_strings_math_host.cpp over
// csrc/match_strings_math.h) on arrays from anywhere.  The masked 16-byte word -- the one reader of a column's bytes, shared
// with the kernels -- at every residue of the base and every end, the bytes ending exactly where their allocation ends and
// the bytes in front of them poisoned by granule and filled; and then, round after round, hostile arrays: offsets from
// anywhere, valid bytes from anywhere, R below, at and above the room, patterns of every shape, few blocks and short stages.  Every array is an
// allocation of exactly its size, so a read or a write outside is the sanitizer's to report.  Asserted here, by a matcher
// that shares nothing with the header (memcmp over every position sequence): the records of every call whose offsets pass;
// that nothing at or past R is written.  NOT part of the product.
#include <sanitizer/asan_interface.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../match_strings_math_host.cpp"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

int failures = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) printf("FAILED %s (line %d)\n", #x, __LINE__), failures++; \
    } while (0)

const uint8_t kAlphabet[7] = {0x00, 'a', 'A', 'b', 0x7f, 0x80, 0xff};

// `len` bytes at an address that is `residue` mod 16 and that end where their allocation ends, so a read behind them is the
// sanitizer's to report.  In front of them the allocation goes on for `residue` bytes: they are poisoned as far as the
// sanitizer can (whole 8-byte granules: all of them for residue 0 and 8, the granule that bytes[0] shares never), filled with
// 0xEE, and a word that took one of them in differs from the expected value, which has 0 there
struct Placed {
    uint8_t *base, *bytes;
    uint64_t residue;
    Placed(uint64_t residue_, uint64_t len) : residue(residue_) {
        base = static_cast<uint8_t *>(malloc(residue + len + (residue + len == 0)));  // (malloc's blocks are 16-byte aligned)
        if ((reinterpret_cast<uintptr_t>(base) & 15) != 0) abort();
        bytes = base + residue;
        for (uint64_t i = 0; i < residue; i++) base[i] = 0xEE;
        ASAN_POISON_MEMORY_REGION(base, residue);
    }
    ~Placed() {
        ASAN_UNPOISON_MEMORY_REGION(base, residue);
        free(base);
    }
};

void words_everywhere() {
    for (uint64_t residue = 0; residue < 16; residue++)
        for (uint64_t len = 0; len < 70; len++) {
            Placed room(residue, len);
            for (uint64_t i = 0; i < len; i++) room.bytes[i] = (uint8_t)(1 + (rnd() % 255));
            CHECK(len == 0 || phase_of(room.bytes) == residue);
            const uint32_t phase = phase_of(room.bytes);
            for (uint64_t a = 0; a < 128; a += 16) {
                const Word16 w = load_word16(room.bytes, phase, len, a);
                for (uint32_t k = 0; k < 16; k++) {
                    const uint64_t c = a + k;
                    const uint8_t want = c >= phase && c - phase < len ? room.bytes[c - phase] : 0;
                    CHECK((uint8_t)(w.w[k >> 2] >> (8 * (k & 3))) == want);
                }
            }
        }
}

uint8_t lower(uint8_t c) { return c >= 'A' && c <= 'Z' ? c + 32 : c; }
bool same(const uint8_t *v, const uint8_t *s, uint32_t n, bool nocase) {
    for (uint32_t i = 0; i < n; i++)
        if ((nocase ? lower(v[i]) : v[i]) != (nocase ? lower(s[i]) : s[i])) return false;
    return true;
}
// the definition: can pieces j .. be placed at or behind `at` in v[0, n)
bool chain(const uint8_t *v, uint64_t n, const msj_pattern &p, const uint8_t *const *piece, uint32_t j, uint64_t at) {
    const uint32_t len = p.piece_len[j];
    for (uint64_t q = at; q + len <= n; q++) {
        if (!same(v + q, piece[j], len, p.flags & MSJ_MATCH_NOCASE_ASCII)) continue;
        if (j + 1 == p.n_pieces) {
            if (!(p.flags & MSJ_MATCH_AT_END) || q + len == n) return true;
        } else if (chain(v, n, p, piece, j + 1, q + len)) {
            return true;
        }
    }
    return false;
}
// -> the smallest p_0, or -1
int64_t first_match(const uint8_t *v, uint64_t n, const msj_pattern &p) {
    const uint8_t *piece[4];
    uint64_t at = 0;
    for (uint32_t j = 0; j < p.n_pieces; j++) piece[j] = p.bytes + at, at += p.piece_len[j];
    const uint32_t len = p.piece_len[0];
    for (uint64_t q = 0; q + len <= n; q++) {
        if ((p.flags & MSJ_MATCH_AT_START) && q != 0) break;
        if (!same(v + q, piece[0], len, p.flags & MSJ_MATCH_NOCASE_ASCII)) continue;
        if (p.n_pieces == 1 ? (!(p.flags & MSJ_MATCH_AT_END) || q + len == n) : chain(v, n, p, piece, 1, q + len)) return (int64_t)q;
    }
    return -1;
}

void hostile_round(uint32_t round) {
    const uint64_t rows = rnd() % 40, bytes_len = rnd() % 3 ? rnd() % 300 : 8100 + rnd() % 400;
    const uint64_t capacity = rows + rnd() % 3;
    // offsets: mostly ascending inside bytes_len, sometimes from anywhere
    const bool wild = rnd() % 4 == 0;
    std::vector<uint64_t> offsets(rows + 1);
    uint64_t at = rnd() % 3;
    for (uint64_t k = 0; k <= rows; k++) {
        offsets[k] = at < bytes_len ? at : bytes_len;
        at += rnd() % 3 ? rnd() % 12 : rnd() % 3 ? 0 : rnd() % 200;
        if (wild && rnd() % 16 == 0) offsets[k] = rnd() % 5 ? rnd() % (bytes_len + 40) : rnd();
    }
    std::vector<uint8_t> valid(rows);
    for (auto &b : valid) b = rnd() % 5 ? (uint8_t)(1 + rnd() % 255) : 0;
    Placed room(rnd() % 16, bytes_len);
    for (uint64_t i = 0; i < bytes_len; i++) room.bytes[i] = kAlphabet[rnd() % (round % 2 ? 4 : 7)];
    // patterns: pieces cut from the bytes, or from the alphabet
    const uint32_t n_patterns = 1 + rnd() % 16;
    std::vector<uint32_t> desc(6 * n_patterns);
    std::vector<uint8_t> pbytes;
    for (uint32_t i = 0; i < n_patterns; i++) {
        const uint32_t n = 1 + rnd() % 4;
        desc[6 * i] = n, desc[6 * i + 1] = rnd() % 8;
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t len = rnd() % 8 ? 1 + rnd() % 6 : 1 + rnd() % 255;
            desc[6 * i + 2 + j] = len;
            const uint64_t from = bytes_len > len && rnd() % 4 ? rnd() % (bytes_len - len) : bytes_len;
            for (uint32_t x = 0; x < len; x++) pbytes.push_back(from < bytes_len ? room.bytes[from + x] : kAlphabet[rnd() % 7]);
        }
    }
    uint64_t n_rows = rnd() % 4 ? rows : rnd() % (rows + 3);
    std::vector<uint64_t> n_rows_word(1, n_rows);
    std::vector<msj_field> fields(n_patterns * capacity);
    if (!fields.empty()) memset(fields.data(), 0xA5, fields.size() * sizeof(msj_field));
    std::vector<msj_match_strings_result> res(1);
    std::vector<msj_select_documents_result> sel(1);
    const uint32_t blocks = rnd() % 3 ? 0 : 1 + rnd() % 3, stage = rnd() % 3 ? 0 : 256;
    const int32_t rc = msm_match_strings(1, desc.data(), pbytes.data(), n_patterns, rows ? offsets.data() : nullptr, rows ? valid.data() : nullptr, rows,
                                         n_rows_word.data(), bytes_len ? room.bytes : nullptr, bytes_len, capacity ? fields.data() : nullptr, capacity,
                                         res.data(), sel.data(), blocks, stage);
    CHECK(rc == 0);
    if (rc != 0) return;
    const uint64_t R = n_rows;
    bool ascending = true;
    for (uint64_t k = 0; k < R && k < rows; k++) ascending &= offsets[k] <= offsets[k + 1] && offsets[k + 1] <= bytes_len;
    const bool over = R > rows || R > capacity;
    CHECK(res[0].code == (over ? MSJ_CAPACITY : ascending ? 0 : MSJ_ERR_BAD_ARGUMENT) && sel[0].code == res[0].code);
    const uint64_t written = res[0].code == 0 ? R : 0;
    const std::vector<msj_pattern> specs = specs_of(desc.data(), pbytes.data(), n_patterns);
    uint64_t n_matched = 0;
    for (uint32_t p = 0; p < n_patterns; p++)
        for (uint64_t k = 0; k < capacity; k++) {
            const msj_field &f = fields[p * capacity + k];
            if (k >= written) {
                const uint8_t *raw = reinterpret_cast<const uint8_t *>(&f);
                bool untouched = true;
                for (uint32_t x = 0; x < sizeof f; x++) untouched &= raw[x] == 0xA5;
                CHECK(untouched);
                continue;
            }
            const int64_t want = valid[k] ? first_match(room.bytes + offsets[k], offsets[k + 1] - offsets[k], specs[p]) : -1;
            if (want < 0) {
                CHECK(f.code == 20 && f.bits == 0 && f.type == 0 && f.token == 0xFFFFFFFFu && f.flags == 0);
            } else {
                CHECK(f.code == 0 && f.bits == (uint64_t)want && f.type == 'l' && f.token == 0xFFFFFFFFu && f.flags == 0);
                n_matched++;
            }
        }
    if (res[0].code == 0) CHECK(res[0].n_matched == n_matched && sel[0].n_found == n_matched && res[0].n_rows == R && sel[0].n_paths == n_patterns);
}

}  // namespace

int main() {
    words_everywhere();
    for (uint32_t round = 0; round < 3000; round++) hostile_round(round);
    if (failures) {
        printf("match_strings_sanitize: %d failures\n", failures);
        return 1;
    }
    printf("match_strings_sanitize ok\n");
    return 0;
}
