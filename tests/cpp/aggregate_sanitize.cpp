// Stand-alone program (its own main; built by tests/test_aggregate_sanitizers.py with -fsanitize=address,undefined): the host
// form of the arithmetic of msj_aggregate_device (tests/aggregate_math_host.cpp over csrc/aggregate_math.h) on arrays from
// anywhere.  A pinned corpus -- the int64 edges through the int path and out of it, sums that cancel, subnormals, a sum
// beyond DBL_MAX, the zeros' tie rules, an int beside the double next to it -- and then, round after round, hostile
// records: wild tags, flags and codes, NaN and infinity patterns, every exponent from the smallest subnormal to the largest
// double in one group, codes of -1, G, INT32_MIN and INT32_MAX, a row count below and above the stride, a group count below
// and above the capacity.  Every array is a std::vector of exactly its size, so a read or a write outside is the
// sanitizer's to report, and every shift and signed operation of the header is the undefined-behaviour sanitizer's.
// Asserted here: the pinned values, that the counts add up, that nothing at or past G is written, that a permutation of the
// rows changes no byte, that the minimum and maximum found apart and merged equal those found row after row.  NOT part of
// the product.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../aggregate_math_host.cpp"

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

msj_field field(uint64_t bits, uint8_t type, uint8_t flags = 0, uint16_t code = 0) {
    msj_field f;
    f.bits = bits, f.token = 0, f.type = type, f.flags = flags, f.code = code;
    return f;
}
msj_field of_int(int64_t v) { return field((uint64_t)v, 'l'); }
msj_field of_double(double d) {
    uint64_t bits;
    memcpy(&bits, &d, 8);
    return field(bits, 'd');
}
uint64_t bits_of(double d) { return of_double(d).bits; }

msj_aggregate one_group(const std::vector<msj_field> &rows, int split = 0) {
    msj_select_documents_result sel = {};
    sel.n_documents = rows.size(), sel.n_paths = 1;
    msj_aggregate out;
    msj_aggregate_result res;
    CHECK(agm_aggregate(rows.data(), rows.size(), 1, &sel, nullptr, 1, &out, 1, &res, split) == 0 && res.code == 0);
    return out;
}

void pinned() {
    msj_aggregate r = one_group({of_int(INT64_MAX), of_int(1), of_int(-1)});
    CHECK(r.sum_type == 'l' && (int64_t)r.sum_bits == INT64_MAX && r.flags == 0 && (int64_t)r.min_bits == -1 && (int64_t)r.max_bits == INT64_MAX);
    r = one_group({of_int(INT64_MAX), of_int(1)});
    CHECK(r.sum_type == 'd' && r.sum_bits == bits_of(9223372036854775808.0) && r.flags == MSJ_AGG_INT_OVERFLOW);
    r = one_group({of_int(INT64_MIN), of_int(INT64_MIN)});
    CHECK(r.sum_type == 'd' && r.sum_bits == bits_of(-18446744073709551616.0) && r.flags == MSJ_AGG_INT_OVERFLOW && (int64_t)r.min_bits == INT64_MIN);
    r = one_group({of_double(1e308), of_double(-1e308), of_double(1.0)});
    CHECK(r.sum_type == 'd' && r.sum_bits == 0 && r.n_values == 3);   // (1.0 lies more than 95 places below 1e308)
    r = one_group(std::vector<msj_field>(10, of_double(0.1)));
    CHECK(r.sum_bits == bits_of(1.0));
    r = one_group({of_double(9007199254740992.0), of_double(1.0), of_double(1.0)});
    CHECK(r.sum_bits == bits_of(9007199254740994.0));
    r = one_group({of_double(5e-324), of_double(5e-324), of_double(5e-324), of_double(-5e-324)});
    CHECK(r.sum_bits == 2 && r.min_bits == bits_of(-5e-324) && r.max_bits == 1);
    r = one_group({of_double(1.7e308), of_double(1.7e308)});
    CHECK(r.sum_bits == bits_of(INFINITY) && r.flags == MSJ_AGG_INFINITE);
    r = one_group({of_double(-0.0), of_int(0), of_double(0.0)});
    CHECK(r.sum_type == 'd' && r.sum_bits == 0 && r.min_type == 'l' && r.max_type == 'l' && r.min_bits == 0 && r.max_bits == 0);
    r = one_group({of_double(0.0), of_double(-0.0)});
    CHECK(r.min_type == 'd' && r.min_bits == bits_of(-0.0) && r.max_type == 'd' && r.max_bits == 0);
    r = one_group({of_int(9007199254740993ll), of_double(9007199254740992.0)});
    CHECK(r.min_type == 'd' && r.min_bits == bits_of(9007199254740992.0) && r.max_type == 'l' && r.max_bits == 9007199254740993ull);
    r = one_group({field(1, 'l', MSJ_FIELD_NO_BITS), field(bits_of(INFINITY), 'd'), field(3, 'l', 0, 20), field(3, '"')});
    CHECK(r.n_rows == 4 && r.n_values == 0 && r.sum_type == 0 && r.sum_bits == 0 && r.flags == 0);
    bool inf;
    CHECK(round_scaled(S128{(1ull << 53) + 1, 0}, 0, &inf) == bits_of(9007199254740992.0) && !inf);
    CHECK(round_scaled(S128{(1ull << 53) + 3, 0}, 0, &inf) == bits_of(9007199254740996.0) && !inf);
    CHECK(round_scaled(S128{1, 0}, -1075, &inf) == 0 && round_scaled(S128{3, 0}, -1075, &inf) == 2 && round_scaled(S128{0, INT64_MIN >> 1}, 928, &inf) == bits_of(-INFINITY) && inf);
}

msj_field hostile_record(int centre) {
    static const uint8_t tags[] = {'l', 'l', 'l', 'd', 'd', 'd', 'd', '"', '{', '[', 't', 'f', 'n', 0, 'x', 0xFF};
    static const uint16_t codes[] = {0, 0, 0, 0, 0, 0, 0, 0, 9, 17, 20, 0xFFFF};
    const uint8_t type = tags[rnd() % sizeof tags];
    uint64_t bits = rnd();
    switch (rnd() % 8) {
        case 0: bits = rnd() % 3 ? 0 : 1ull << 63; break;                                        // the zeros
        case 1: bits = (rnd() & ((1ull << 52) - 1)) | (rnd() << 63); break;                      // subnormals
        case 2: bits = (rnd() & ~(0x7FFull << 52)) | (0x7FFull << 52); break;                    // NaN, infinity
        case 3: bits = rnd() % 2 ? (uint64_t)INT64_MAX - rnd() % 3 : (uint64_t)INT64_MIN + rnd() % 3; break;
        case 4: bits = (uint64_t)((int64_t)rnd() >> (rnd() % 64)); break;                          // ints of every size
        case 5: case 6: bits = (rnd() & ~(0x7FFull << 52)) | ((uint64_t)std::min(2046, std::max(0, centre + (int)(rnd() % 64) - 60)) << 52); break;
        default: break;
    }
    return field(bits, type, (uint8_t)(rnd() % 4 ? 0 : rnd() % 2 ? MSJ_FIELD_NO_BITS : rnd()), codes[rnd() % 12]);
}

void hostile_round(uint32_t round) {
    const uint64_t stride = rnd() % 200, n_columns = 1 + rnd() % 3;
    const uint64_t R = rnd() % 8 == 0 ? stride + 1 : rnd() % (stride + 1);
    const uint64_t G = rnd() % 40, capacity = rnd() % 8 == 0 && G ? G - 1 : G + rnd() % 3;
    const bool with_codes = round % 4 != 0;
    std::vector<msj_field> in(n_columns * stride);
    const int centre = (int)(rnd() % 2047);
    for (msj_field &f : in) f = hostile_record(centre);
    std::vector<int32_t> codes(with_codes ? stride : 0);
    for (int32_t &c : codes) c = rnd() % 8 ? (int32_t)(rnd() % (G + 1)) : rnd() % 4 == 0 ? INT32_MIN : rnd() % 3 == 0 ? INT32_MAX : rnd() % 2 ? -1 : (int32_t)G;
    msj_select_documents_result sel = {};
    sel.n_documents = R, sel.n_paths = 1, sel.code = rnd() % 16 == 0 ? 7 : 0;
    msj_aggregate fill;
    memset(&fill, 0xA5, sizeof fill);
    std::vector<msj_aggregate> out(n_columns * capacity, fill), split(out), again(out);
    msj_aggregate_result res, res2, res3;
    const int32_t *pc = with_codes ? codes.data() : nullptr;
    CHECK(agm_aggregate(in.data(), stride, (uint32_t)n_columns, &sel, pc, G, out.data(), capacity, &res, 0) == 0);
    CHECK(agm_aggregate(in.data(), stride, (uint32_t)n_columns, &sel, pc, G, split.data(), capacity, &res2, 1) == 0);
    CHECK(memcmp(&res, &res2, sizeof res) == 0 && (out.empty() || memcmp(out.data(), split.data(), out.size() * sizeof fill) == 0));
    if (sel.code != 0 || R > stride || G > capacity) {
        CHECK(res.code == (sel.code != 0 ? sel.code : MSJ_CAPACITY) && res.n_values + res.n_skipped + res.n_ungrouped == 0);
        for (const msj_aggregate &a : out) CHECK(memcmp(&a, &fill, sizeof fill) == 0);
        return;
    }
    // the rows (of every column, and the codes) in another order: the same bytes
    std::vector<uint64_t> perm(R);
    for (uint64_t k = 0; k < R; k++) perm[k] = k;
    for (uint64_t k = R; k > 1; k--) std::swap(perm[k - 1], perm[rnd() % k]);
    std::vector<msj_field> shuffled(in);
    std::vector<int32_t> shuffled_codes(codes);
    for (uint64_t k = 0; k < R; k++) {
        for (uint64_t c = 0; c < n_columns; c++) shuffled[c * stride + k] = in[c * stride + perm[k]];
        if (with_codes) shuffled_codes[k] = codes[perm[k]];
    }
    CHECK(agm_aggregate(shuffled.data(), stride, (uint32_t)n_columns, &sel, with_codes ? shuffled_codes.data() : nullptr, G, again.data(), capacity, &res3, 1) == 0);
    CHECK(memcmp(&res, &res3, sizeof res) == 0 && (out.empty() || memcmp(out.data(), again.data(), out.size() * sizeof fill) == 0));
    uint64_t grouped = 0, values = 0;
    for (uint64_t c = 0; c < n_columns; c++) {
        for (uint64_t g = 0; g < capacity; g++) {
            const msj_aggregate &a = out[c * capacity + g];
            if (g >= G) {
                CHECK(memcmp(&a, &fill, sizeof fill) == 0);
                continue;
            }
            CHECK(a.n_values <= a.n_rows && a.reserved == 0 && (a.n_values != 0) == (a.sum_type != 0));
            CHECK(a.n_values == 0 ? (a.min_type | a.max_type | a.flags) == 0 && (a.sum_bits | a.min_bits | a.max_bits) == 0
                                  : (a.min_type == 'l' || a.min_type == 'd') && (a.max_type == 'l' || a.max_type == 'd'));
            if (a.n_values) CHECK(cmp_values(a.min_type, a.min_bits, a.max_type, a.max_bits) <= 0);
            if (c == 0) grouped += a.n_rows;
            values += a.n_values;
        }
    }
    CHECK(res.code == 0 && res.n_rows == R && res.n_groups == G && grouped + res.n_ungrouped == R && values == res.n_values);
}

}  // namespace

int main() {
    pinned();
    for (uint32_t round = 0; round < 3000; round++) hostile_round(round);
    if (failures) return printf("%d checks failed\n", failures), 1;
    printf("aggregate_sanitize ok\n");
    return 0;
}
