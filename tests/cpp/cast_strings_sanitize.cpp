// Stand-alone program (its own main; built by tests/test_cast_strings_sanitizers.py with -fsanitize=address,undefined): the
// host form of the arithmetic of msj_cast_strings_device (tests/cast_strings_math_host.cpp over csrc/cast_strings_math.h) on
// arrays from anywhere.  A pinned corpus -- the fixed points of the timestamp grammar, the int64 edges in nanoseconds, numbers
// of 128 and 129 bytes, a number that takes the exact path, escapes on the first and the last byte, a damaged escape at the
// window's end -- and then, round after round, hostile records: spans at len - 1, len, len + 1 and 2^32 - 1, wild tags, flags
// and codes, a row count below and above the capacity, in place and out of place, both kinds, every unit.  Every array is a
// std::vector of exactly its size, so a read or a write outside is the sanitizer's to report.  Asserted here: the pinned
// values, that the counts add up, that nothing past R is written, that in place equals out of place, that a record with a
// code passes unchanged.  NOT part of the product.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../cast_strings_math_host.cpp"

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

msj_field field(uint64_t bits, uint8_t type, uint8_t flags = 0, uint16_t code = 0, uint32_t token = 0) {
    msj_field f;
    f.bits = bits, f.token = token, f.type = type, f.flags = flags, f.code = code;
    return f;
}
bool same(const msj_field &a, const msj_field &b) {
    return a.bits == b.bits && a.token == b.token && a.type == b.type && a.flags == b.flags && a.code == b.code;
}

struct Window {
    std::vector<uint8_t> data;
    std::vector<msj_field> rows;  // a record per body
};
Window window_of(const std::vector<std::string> &bodies) {
    Window w;
    uint32_t token = 1;
    for (const std::string &b : bodies) {
        w.data.push_back('"');
        const bool escaped = b.find('\\') != std::string::npos;
        w.rows.push_back(field(w.data.size() | ((uint64_t)b.size() << 32), '"', escaped ? 2 : 0, 0, token++));
        w.data.insert(w.data.end(), b.begin(), b.end());
    }
    return w;  // (the last body ends at the window's end)
}

struct Pin {
    const char *body;
    uint32_t kind, unit, outcome;
    int64_t value;
    uint8_t type;
};

void pinned() {
    const std::string n128(128, '1'), n129(129, '1');
    const Pin pins[] = {
        {"0000-01-01T00:00:00Z", kTimestamp, kUnitS, kCast, -62167219200ll, 'l'},
        {"9999-12-31T23:59:59Z", kTimestamp, kUnitS, kCast, 253402300799ll, 'l'},
        {"2262-04-11T23:47:16.854775807Z", kTimestamp, kUnitNs, kCast, INT64_MAX, 'l'},
        {"1677-09-21T00:12:43.145224192Z", kTimestamp, kUnitNs, kCast, INT64_MIN, 'l'},
        {"2262-04-11T23:47:16.854775808Z", kTimestamp, kUnitNs, kRange, 0, 0},
        {"1677-09-21T00:12:43.145224191Z", kTimestamp, kUnitNs, kRange, 0, 0},
        {"0000-01-01T00:00:00+23:59", kTimestamp, kUnitNs, kRange, 0, 0},
        {"9999-12-31T23:59:59-23:59", kTimestamp, kUnitUs, kCast, (253402300799ll + 86340) * 1000000, 'l'},
        {"\\u0032024-05-01", kTimestamp, kUnitS, kCast, 1714521600ll, 'l'},
        {"2024-05-01T12:34:56.789\\u005a", kTimestamp, kUnitMs, kCast, 1714566896789ll, 'l'},
        {"2024-05-01T12:34:56.123456789+05:30", kTimestamp, kUnitNs, kCast, 1714547096123456789ll, 'l'},
        {"2024-05-01T12:34:56.123456789+05:300", kTimestamp, kUnitNs, kSyntax, 0, 0},
        {"2024-02-30", kTimestamp, kUnitS, kSyntax, 0, 0},
        {"2016-12-31T23:59:60Z", kTimestamp, kUnitS, kSyntax, 0, 0},
        {"", kTimestamp, kUnitS, kSyntax, 0, 0},
        {"9007199254740993", kNumber, 0, kCast, 9007199254740993ll, 'l'},
        {"-0", kNumber, 0, kCast, 0, 'l'},
        {"12.50", kNumber, 0, kCast, 0x4029000000000000ll, 'd'},
        {"1e400", kNumber, 0, kRange, 0, 0},
        {"1 ", kNumber, 0, kSyntax, 0, 0},
        {"+1", kNumber, 0, kSyntax, 0, 0},
        {"", kNumber, 0, kSyntax, 0, 0},
        {"\\u0031e-3", kNumber, 0, kCast, 0x3F50624DD2F1A9FCll, 'd'},
        {"9007199254740993.00000000000000000000000000001e0", kNumber, 0, kCast, 0x4340000000000001ll, 'd'},  // (the exact path)
        {n128.c_str(), kNumber, 0, kRange, 0, 0},
        {n129.c_str(), kNumber, 0, kSyntax, 0, 0},
        {"12\\", kNumber, 0, kCast, 12, 'l'},  // (a damaged escape at the window's end gives no byte)
    };
    for (const Pin &p : pins) {
        const Window w = window_of({p.body});
        msj_field out;
        const uint32_t o = csm_cast_record(&w.rows[0], w.data.data(), w.data.size(), p.kind, p.unit, 0, &out);
        CHECK(o == p.outcome);
        if (o != p.outcome) printf("  %s: outcome %u\n", p.body, o);
        if (p.outcome == kCast) CHECK(out.code == 0 && out.type == p.type && (int64_t)out.bits == p.value && out.token == 1 && out.flags == 0);
        else CHECK(out.code == kNumberError && out.token == 0xFFFFFFFFu && out.bits == 0 && out.type == 0 && out.flags == 0);
    }
}

msj_field hostile_record(uint64_t len) {
    static const uint8_t tags[] = {'"', '"', '"', '"', 'l', 'd', '{', '[', 't', 'f', 'n', 0, 'x', 0xFF};
    static const uint16_t codes[] = {0, 0, 0, 0, 0, 0, 9, 17, 20, 3, 0xFFFF};
    const uint64_t starts[] = {len - 1, len, len + 1, 0xFFFFFFFFull, 0, rnd() % (len + 2), rnd() % (len + 2), rnd() % (len + 2)};
    const uint64_t sizes[] = {0, 1, 2, 10, 35, 36, 128, 129, 0xFFFFFFFFull, rnd() % 40, rnd() % 40, rnd() % 300, 6 * 35, 6 * 35 + 1, 6 * 128 + 1};
    const uint64_t b = starts[rnd() % 8] & 0xFFFFFFFFull, r = sizes[rnd() % 15];
    const uint64_t bits = rnd() % 4 ? b | (r << 32) : rnd();
    return field(bits, tags[rnd() % sizeof tags], (uint8_t)(rnd() % 4 ? (rnd() & 2) : rnd()), codes[rnd() % 11], (uint32_t)rnd());
}

void hostile_round(uint32_t round) {
    // a window of bytes a cast may meet, escapes and digits among them
    static const char alphabet[] = "0123456789-:.TZ+ \\u00eE\"";
    const uint64_t len = 1 + rnd() % 300;
    std::vector<uint8_t> data(len);
    for (uint8_t &c : data) c = rnd() % 8 ? alphabet[rnd() % (sizeof alphabet - 1)] : (uint8_t)rnd();
    if (round % 3 == 0 && len >= 24) memcpy(data.data() + len - 24, "2024-05-01T12:34:56.789Z", 24);
    const uint64_t rows = rnd() % 70, capacity = rows ? rows - (rnd() % 8 == 0) : 0, R = rnd() % 8 == 0 ? rows + 1 : rnd() % (rows + 1);
    std::vector<msj_field> in(rows);
    for (msj_field &f : in) f = hostile_record(len);
    const uint32_t kind = round & 1 ? kTimestamp : kNumber, unit = kind == kTimestamp ? (round >> 1) % 4 : 0, flags = (round >> 3) & 1;
    msj_select_documents_result sel = {};
    sel.n_documents = R, sel.n_paths = 1, sel.code = rnd() % 16 == 0 ? 7 : 0;
    const msj_field fill = field(0x7777777777777777ull, 0x77, 0x77, 0x7777, 0x77777777u);
    std::vector<msj_field> out(capacity, fill), place(in.begin(), in.begin() + capacity);
    msj_cast_strings_result res, res2;
    msj_select_documents_result osel, osel2;
    CHECK(csm_cast_strings(data.data(), len, in.data(), &sel, kind, unit, flags, out.data(), capacity, &res, &osel) == 0);
    CHECK(csm_cast_strings(data.data(), len, place.data(), &sel, kind, unit, flags, place.data(), capacity, &res2, &osel2) == 0);
    CHECK(memcmp(&res, &res2, sizeof res) == 0 && memcmp(&osel, &osel2, sizeof osel) == 0);
    CHECK(res.flags == (kind | unit << 8 | flags << 16) && osel.code == res.code && osel.n_paths == 1);
    if (sel.code != 0 || R > capacity) {
        CHECK(res.code == (sel.code != 0 ? sel.code : MSJ_CAPACITY) && res.n_rows == (sel.code != 0 ? 0 : R));
        CHECK(res.n_cast + res.n_syntax + res.n_range + res.n_other == 0 && osel.n_documents == 0);
        for (uint64_t k = 0; k < capacity; k++) CHECK(same(out[k], fill) && same(place[k], in[k]));
        return;
    }
    uint64_t passed = 0;
    for (uint64_t k = 0; k < R; k++) {
        CHECK(same(out[k], place[k]));
        if (in[k].code != 0) {
            CHECK(same(out[k], in[k]));
            passed++;
            continue;
        }
        CHECK(out[k].code == 0 ? (out[k].type == 'l' || out[k].type == 'd') : (out[k].code == kNumberError || out[k].code == kIncorrectType));
    }
    for (uint64_t k = R; k < capacity; k++) CHECK(same(out[k], fill) && same(place[k], in[k]));
    CHECK(res.code == 0 && res.n_rows == R && res.n_cast + res.n_syntax + res.n_range + res.n_other + passed == R);
    CHECK(osel.n_documents == R && osel.n_found == res.n_cast);
}

}  // namespace

int main() {
    pinned();
    for (uint32_t round = 0; round < 3000; round++) hostile_round(round);
    if (failures) return printf("%d checks failed\n", failures), 1;
    printf("cast_strings_sanitize ok\n");
    return 0;
}
