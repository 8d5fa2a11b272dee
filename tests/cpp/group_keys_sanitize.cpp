// Stand-alone program (its own main; built by tests/test_group_keys_sanitizers.py with -fsanitize=address,undefined): the host
// form of the arithmetic of msj_bucket_rows_device and msj_group_keys_device (tests/group_keys_math_host.cpp over
// csrc/group_keys_math.h) on records and codes from anywhere.  Every array is an allocation of exactly its size -- the records
// R * 16 bytes, the codes R * 4, the offsets (R + 1) * 8, the valid bytes R, the key bytes R * W -- so a read or a write outside
// is the sanitizer's to report, and every shift, negation and subtraction of the floor runs under UBSan on the extremes.  R in
// {0, 1, 255, 256, 257}, every n_parts from 1 to 8, the flags on and off.  Asserted here, by arithmetic that shares nothing
// with the header (__int128): every bucket; that memcmp of two keys is the order of their parts.  NOT part of the product.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../group_keys_math_host.cpp"

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

const uint64_t kEdgeBits[] = {0, 1, ~0ull, 1ull << 63, (1ull << 63) - 1, (1ull << 63) + 1, 0x43E0000000000000ull /* 2^63 */, 0xC3E0000000000000ull,
                              0xC3E0000000000001ull, 0x43DFFFFFFFFFFFFFull, 0x4340000000000000ull /* 2^53 */, 0xC340000000000001ull, 0x3FE0000000000000ull,
                              0xBFE0000000000000ull, 0x8000000000000000ull, 0x7FF0000000000000ull, 0xFFF0000000000000ull, 0x7FF8000000000001ull,
                              0x0000000000000001ull, 0x8000000000000001ull, 0x7FEFFFFFFFFFFFFFull, 0xFFEFFFFFFFFFFFFFull};
const uint8_t kTypes[] = {'l', 'd', 'l', 'd', '"', 't', '{', 0, 0xFF};
const int64_t kEdgeInts[] = {INT64_MIN, INT64_MIN + 1, -60001, -1, 0, 1, 60000, INT64_MAX - 1, INT64_MAX};

msj_field hostile_field() {
    msj_field f;
    f.bits = rnd() % 3 ? kEdgeBits[rnd() % (sizeof kEdgeBits / sizeof *kEdgeBits)] + (rnd() % 3 ? 0 : rnd() % 5 - 2) : rnd();
    f.token = (uint32_t)rnd();
    f.type = kTypes[rnd() % sizeof kTypes];
    f.flags = rnd() % 4 ? 0 : (uint8_t)rnd();
    f.code = rnd() % 5 ? 0 : (uint16_t)(rnd() % 3 ? 20 : rnd());
    return f;
}
int32_t hostile_code() { return rnd() % 3 ? (int32_t)(rnd() % 5) - 1 : (int32_t)rnd(); }

// the value of a number-value record as value = num / 2^shift (shift >= 0) or num * 2^-shift: only the floor is needed here
bool is_value(const msj_field &f) {
    if (f.code != 0 || (f.type != 'l' && f.type != 'd') || (f.flags & 64)) return false;
    return f.type == 'l' || ((f.bits >> 52) & 0x7FF) != 0x7FF;
}
// floor of a finite double as __int128 when |value| < 2^100, else saturated
__int128 wide_floor(uint64_t bits) {
    const bool neg = bits >> 63;
    const int biased = (int)((bits >> 52) & 0x7FF);
    const uint64_t m = (bits & ((1ull << 52) - 1)) | (biased ? 1ull << 52 : 0);
    const int q = (biased ? biased : 1) - 1075;
    __int128 mag;
    bool rest = false;
    if (q >= 0) mag = q > 60 ? ((__int128)1 << 120) : (__int128)m << q;
    else if (-q >= 64) mag = 0, rest = m != 0;
    else mag = m >> -q, rest = (m & ((1ull << -q) - 1)) != 0;
    if (m == 0) return 0;
    return neg ? -mag - (rest ? 1 : 0) : mag;
}

void bucket_round(uint64_t R) {
    std::vector<msj_field> rows(R), out(R);
    for (auto &f : rows) f = hostile_field();
    const int64_t width = rnd() % 3 ? 1 + (int64_t)(rnd() % 100000) : rnd() % 2 ? INT64_MAX - (int64_t)(rnd() % 3) : 1 + (int64_t)(rnd() >> 1);
    const int64_t origin = rnd() % 2 ? kEdgeInts[rnd() % 9] : (int64_t)rnd();
    std::vector<msj_select_documents_result> sel(2);
    std::vector<msj_bucket_rows_result> res(1);
    memset(sel.data(), 0, 2 * sizeof sel[0]);
    sel[0].n_documents = R;
    const bool in_place = rnd() % 2;
    if (in_place) out = rows;
    const int32_t rc = gkm_bucket_rows(R ? (in_place ? out.data() : rows.data()) : nullptr, &sel[0], width, origin, 0, R ? out.data() : nullptr, R,
                                       res.data(), &sel[1]);
    CHECK(rc == 0 && res[0].code == 0 && res[0].n_rows == R);
    uint64_t n_bucketed = 0;
    for (uint64_t k = 0; k < R; k++) {
        const msj_field &f = rows[k], &o = out[k];
        if (f.code != 0) {
            CHECK(memcmp(&f, &o, sizeof f) == 0);
        } else if (!is_value(f)) {
            CHECK(o.code == ((f.type == 'l' || f.type == 'd') ? 9 : 17) && o.bits == 0 && o.token == 0xFFFFFFFFu && o.type == 0 && o.flags == 0);
        } else {
            const __int128 v = f.type == 'l' ? (__int128)(int64_t)f.bits : wide_floor(f.bits);
            __int128 r = (v - origin) % width;
            if (r < 0) r += width;
            const __int128 s = v - r;
            const bool fits = v >= INT64_MIN && v <= INT64_MAX && s >= INT64_MIN;
            if (fits) {
                CHECK(o.code == 0 && o.type == 'l' && (int64_t)o.bits == (int64_t)s && o.token == f.token && o.flags == 0);
                n_bucketed++;
            } else {
                CHECK(o.code == 9 && o.bits == 0 && o.token == 0xFFFFFFFFu);
            }
        }
    }
    CHECK(res[0].n_bucketed == n_bucketed && sel[1].n_found == n_bucketed && sel[1].n_documents == R);
}

void keys_round(uint64_t R, uint32_t n_parts) {
    std::vector<std::vector<msj_field>> records(n_parts);
    std::vector<std::vector<int32_t>> codes(n_parts);
    std::vector<msj_key_part> parts(n_parts);
    uint32_t W = 0;
    for (uint32_t j = 0; j < n_parts; j++) {
        parts[j].kind = rnd() % 2 ? MSJ_KEY_NUMBER : MSJ_KEY_CODE, parts[j].flags = rnd() % 2 ? MSJ_KEY_NULL_IS_GROUP : 0;
        if (parts[j].kind == MSJ_KEY_NUMBER) {
            records[j].resize(R);
            for (auto &f : records[j]) f = hostile_field();
            parts[j].d_column = R ? records[j].data() : nullptr, W += 11;
        } else {
            codes[j].resize(R);
            for (auto &c : codes[j]) c = hostile_code();
            parts[j].d_column = R ? codes[j].data() : nullptr, W += 5;
        }
    }
    std::vector<uint64_t> offsets(R + 1, ~0ull);
    std::vector<uint8_t> valid(R, 0xA5);
    uint8_t *bytes = R ? static_cast<uint8_t *>(malloc(R * W)) : nullptr;  // (malloc's blocks are 16-byte aligned)
    if ((reinterpret_cast<uintptr_t>(bytes) & 15) != 0) abort();
    std::vector<msj_select_documents_result> sel(1);
    std::vector<msj_group_keys_result> res(1);
    memset(sel.data(), 0, sizeof sel[0]);
    sel[0].n_documents = R;
    const int32_t rc = gkm_group_keys(parts.data(), n_parts, R, &sel[0], offsets.data(), R ? valid.data() : nullptr, bytes, R, R * W, res.data());
    CHECK(rc == 0 && res[0].code == 0 && res[0].n_rows == R && res[0].key_width == W && res[0].bytes_len == R * W);
    uint64_t n_keys = 0;
    for (uint64_t k = 0; k <= R; k++) CHECK(offsets[k] == k * W);
    for (uint64_t k = 0; k < R; k++) {
        bool ok = true;
        uint32_t at = 0;
        for (uint32_t j = 0; j < n_parts; j++) {
            const bool null = parts[j].kind == MSJ_KEY_NUMBER ? !is_value(records[j][k]) : codes[j][k] < 0;
            CHECK(bytes[k * W + at] == (null ? 1 : 0));
            ok &= !null || parts[j].flags;
            at += parts[j].kind == MSJ_KEY_NUMBER ? 11 : 5;
        }
        CHECK(valid[k] == (ok ? 1 : 0));
        n_keys += ok;
    }
    CHECK(res[0].n_keys == n_keys);
    // memcmp against the parts, pair by pair over a sample: a CODE part by its integers, a NUMBER part's tie by its decode
    for (uint32_t t = 0; t < 200 && R > 1; t++) {
        const uint64_t a = rnd() % R, b = rnd() % R;
        int want = 0;
        for (uint32_t j = 0; j < n_parts && want == 0; j++) {
            if (parts[j].kind == MSJ_KEY_CODE) {
                const int64_t x = codes[j][a] < 0 ? (1ll << 40) : codes[j][a], y = codes[j][b] < 0 ? (1ll << 40) : codes[j][b];
                want = x < y ? -1 : x > y;
            } else {
                const bool nx = !is_value(records[j][a]), ny = !is_value(records[j][b]);
                if (nx || ny) {
                    want = nx == ny ? 0 : nx ? 1 : -1;
                } else {
                    const msj::srows::Key x = msj::srows::make_key(true, records[j][a].type, records[j][a].bits, 0);
                    const msj::srows::Key y = msj::srows::make_key(true, records[j][b].type, records[j][b].bits, 0);
                    want = msj::srows::key_less(x, y) ? -1 : msj::srows::key_less(y, x) ? 1 : 0;
                }
            }
        }
        const int got = memcmp(bytes + a * W, bytes + b * W, W);
        CHECK((got < 0 ? -1 : got > 0) == want);
    }
    free(bytes);
}

}  // namespace

int main() {
    const uint64_t sizes[] = {0, 1, 255, 256, 257};
    for (uint32_t round = 0; round < 40; round++)
        for (uint64_t R : sizes) bucket_round(R);
    for (uint32_t round = 0; round < 6; round++)
        for (uint64_t R : sizes)
            for (uint32_t n_parts = 1; n_parts <= 8; n_parts++) keys_round(R, n_parts);
    if (failures) {
        printf("group_keys_sanitize: %d failures\n", failures);
        return 1;
    }
    printf("group_keys_sanitize ok\n");
    return 0;
}
