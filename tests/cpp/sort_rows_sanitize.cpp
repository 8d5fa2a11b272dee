// Stand-alone program (its own main; built by tests/test_sort_rows_sanitizers.py with -fsanitize=address,undefined): the host
// form of the arithmetic of msj_sort_rows_device (tests/sort_rows_math_host.cpp over csrc/sort_rows_math.h) on arrays from
// anywhere.  A pinned corpus -- the zeros, an int beside the doubles next to it, the int64 edges against +-2^63, subnormals,
// rows without a value in both directions -- and then, round after round, hostile records and row lists: wild tags, flags
// and codes, NaN and infinity patterns, ints of every size and doubles next to them, row numbers at and past R, repeats, a
// row count below and above the stride, a list longer than the capacity, limits around K.  Every array is a std::vector of
// exactly its size, so a read or a write outside is the sanitizer's to report, and every shift and signed operation of the
// header is the undefined-behaviour sanitizer's.  Asserted here: the pinned orders; that the counts add up; that
// neighbouring entries of the order are in order by the exact compare of aggregate_math.h (cmp_values, which shares no code
// with the key), equal values by position; that nothing at or past K is written; that the key's digits put the key
// together again.  NOT part of the product.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../sort_rows_math_host.cpp"

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

constexpr uint32_t kFill = 0xA5A5A5A5u;

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

std::vector<uint32_t> order_of(const std::vector<msj_field> &rows, uint32_t flags = 0, uint64_t limit = 0) {
    msj_select_documents_result sel = {};
    sel.n_documents = rows.size(), sel.n_paths = 1;
    const uint64_t room = limit && limit < rows.size() ? limit : rows.size();
    std::vector<uint32_t> out(room, kFill);
    msj_sort_rows_result res;
    CHECK(srm_sort_rows(rows.data(), rows.size(), &sel, nullptr, nullptr, flags, limit, out.data(), rows.size(), &res, nullptr) == 0 && res.code == 0);
    out.resize(res.n_written);
    return out;
}

void pinned() {
    using V = std::vector<uint32_t>;
    // equal reals keep their order, whatever their type; the rows without a value last, in theirs
    const std::vector<msj_field> zeros = {of_double(0.0), field(1, 'l', MSJ_FIELD_NO_BITS), of_int(0), of_double(-0.0), field(0, 'n'), of_double(-5e-324), of_double(5e-324)};
    CHECK(order_of(zeros) == (V{5, 0, 2, 3, 6, 1, 4}));
    CHECK(order_of(zeros, MSJ_SORT_DESCENDING) == (V{6, 0, 2, 3, 5, 1, 4}));
    CHECK(order_of(zeros, MSJ_SORT_VALUES_ONLY | MSJ_SORT_DESCENDING, 4) == (V{6, 0, 2, 3}));
    CHECK(order_of(zeros, MSJ_SORT_VALUES_ONLY, 9) == (V{5, 0, 2, 3, 6}));
    const std::vector<msj_field> beside = {of_double(9007199254740994.0), of_int(9007199254740993ll), of_double(9007199254740992.0), of_int(9007199254740992ll), of_int(3), of_double(3.0)};
    CHECK(order_of(beside) == (V{4, 5, 2, 3, 1, 0}));
    const std::vector<msj_field> edges = {of_double(9223372036854775808.0), of_int(INT64_MAX), of_int(INT64_MIN), of_double(-9223372036854775808.0), of_int(INT64_MIN + 1),
                                          of_double(9223372036854774784.0), of_double(-9223372036854777856.0), of_double(INFINITY), of_double(-1.7976931348623157e308)};
    CHECK(order_of(edges) == (V{8, 6, 2, 3, 4, 5, 1, 0, 7}));
    // the key's parts: an int's floor among the doubles and what it lies above it, towards minus infinity on both sides
    Key k = int_key((1ll << 62) + 1023);
    CHECK(k.lo == 1023 && k.hi == int_key(1ll << 62).hi && int_key(1ll << 62).lo == 0);
    k = int_key(-(1ll << 62) - 1);
    CHECK(k.lo == 1023 && k.hi == double_key(of_double(-4611686018427388928.0).bits).hi);
    CHECK(int_key(INT64_MIN).lo == 0 && int_key(INT64_MIN).hi == double_key(of_double(-9223372036854775808.0).bits).hi);
    CHECK(int_key(INT64_MAX).lo == 1023 && int_key(-9007199254740993ll).lo == 1 && int_key(9007199254740993ll).lo == 1 && int_key(9007199254740992ll).lo == 0);
    for (int64_t v : {0ll, 1ll, -1ll, 3ll, -77ll, (1ll << 53) - 1, -(1ll << 53), 1ll << 53}) CHECK(int_key(v).lo == 0 && int_key(v).hi == double_key(of_double((double)v).bits).hi);
}

msj_field hostile_record() {
    static const uint8_t tags[] = {'l', 'l', 'l', 'l', 'd', 'd', 'd', 'd', '"', '{', '[', 't', 'n', 0, 'x', 0xFF};
    static const uint16_t codes[] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 9, 20, 0xFFFF};
    const uint8_t type = tags[rnd() % sizeof tags];
    uint64_t bits = rnd();
    switch (rnd() % 8) {
        case 0: bits = rnd() % 3 ? 0 : 1ull << 63; break;                                        // the zeros
        case 1: bits = (rnd() & ((1ull << 52) - 1)) | (rnd() << 63); break;                      // subnormals
        case 2: bits = (rnd() & ~(0x7FFull << 52)) | (0x7FFull << 52); break;                    // NaN, infinity
        case 3: bits = rnd() % 2 ? (uint64_t)INT64_MAX - rnd() % 3 : (uint64_t)INT64_MIN + rnd() % 3; break;
        case 4: bits = (uint64_t)((int64_t)rnd() >> (rnd() % 64)); break;                          // ints of every size
        case 5: {                                                                                // an int above 2^53 and the doubles around it, as either
            const int64_t v = (int64_t)((1ull << (53 + rnd() % 10)) + rnd() % 5000) * (rnd() % 2 ? 1 : -1);
            return rnd() % 2 ? of_int(v + (int64_t)(rnd() % 3) - 1) : of_double((double)v);
        }
        case 6: bits = rnd() % 16; break;                                                        // many equal values
        default: break;
    }
    return field(bits, type, (uint8_t)(rnd() % 5 ? 0 : rnd() % 2 ? MSJ_FIELD_NO_BITS : rnd()), codes[rnd() % 12]);
}

void hostile_round() {
    const uint64_t stride = rnd() % 200;
    const uint64_t R = rnd() % 8 == 0 ? stride + 1 : rnd() % (stride + 1);
    const bool listed = rnd() % 2;
    const uint64_t capacity = listed ? 1 + rnd() % 300 : stride;  // (a list without room is no list: its pointer would be NULL)
    const uint64_t N = !listed ? R : rnd() % 8 == 0 ? capacity + 1 + rnd() % 3 : rnd() % (capacity + 1);
    const uint32_t flags = (uint32_t)(rnd() % 4);
    const uint64_t limit = rnd() % 3 == 0 ? 0 : 1 + rnd() % (N + 3);
    std::vector<msj_field> in(stride);
    for (msj_field &f : in) f = hostile_record();
    std::vector<uint32_t> rows_in(listed ? capacity : 0);
    for (uint32_t &r : rows_in) r = rnd() % 10 == 0 ? (uint32_t)rnd() : rnd() % 10 == 1 ? (uint32_t)R : (uint32_t)(rnd() % (R + 2));
    msj_select_documents_result sel = {}, in_sel = {}, out_sel;
    sel.n_documents = R, sel.n_paths = 1, sel.code = rnd() % 16 == 0 ? 7 : 0;
    in_sel.n_documents = N, in_sel.n_paths = 1, in_sel.code = rnd() % 16 == 0 ? 9 : 0;
    std::vector<uint32_t> out(limit && limit < capacity ? limit : capacity, kFill);
    msj_sort_rows_result res;
    CHECK(srm_sort_rows(in.data(), stride, &sel, listed ? rows_in.data() : nullptr, listed ? &in_sel : nullptr, flags, limit, out.data(), capacity, &res, &out_sel) == 0);
    CHECK(out_sel.code == res.code && out_sel.n_documents == res.n_written && out_sel.n_found == res.n_written && out_sel.n_paths == 1);
    const int32_t code = listed && in_sel.code ? in_sel.code : sel.code;
    if (code != 0 || R > stride || N > capacity) {
        CHECK(res.code == (code ? code : MSJ_CAPACITY) && res.n_values + res.n_skipped + res.n_written + res.n_out_of_range == 0);
        CHECK(res.n_rows == (code ? 0 : N));
        for (uint32_t x : out) CHECK(x == kFill);
        return;
    }
    const uint64_t M = (flags & MSJ_SORT_VALUES_ONLY) ? res.n_values : N;
    CHECK(res.code == 0 && res.flags == flags && res.n_rows == N && res.n_values <= N && res.n_written == (limit && limit < M ? limit : M));
    for (uint64_t i = res.n_written; i < out.size(); i++) CHECK(out[i] == kFill);
    // neighbours in order, by a compare that shares nothing with the key; every written row is one of the input
    auto is_value = [&](uint32_t row) { return row < R && value_kind(in[row]) == kValue; };
    uint64_t values = 0;
    for (uint64_t i = 0; i < res.n_written; i++) {
        const uint32_t row = out[i];
        CHECK(listed ? std::find(rows_in.begin(), rows_in.begin() + N, row) != rows_in.begin() + N : row < R);
        values += is_value(row);
        if (i == 0) continue;
        const uint32_t prev = out[i - 1];
        if (!is_value(prev)) CHECK(!is_value(row));
        if (!listed && is_value(prev) == is_value(row) && !is_value(row)) CHECK(prev < row);  // (input order among the rows without a value)
        if (is_value(prev) && is_value(row)) {
            const int c = msj::agg::cmp_values(in[prev].type, in[prev].bits, in[row].type, in[row].bits);
            CHECK((flags & MSJ_SORT_DESCENDING) ? c >= 0 : c <= 0);
            if (c == 0 && !listed) CHECK(prev < row);  // stable
        }
    }
    CHECK(values == (res.n_written < res.n_values ? res.n_written : res.n_values));
    // the digits of every key
    for (uint64_t k = 0; k < R && k < stride; k++) {
        const Key key = make_key(value_kind(in[k]) == kValue, in[k].type, in[k].bits, flags);
        const uint64_t aux = aux_word(key, k);
        uint64_t hi = 0, lo = 0;
        for (uint32_t d = 2; d < 10; d++) hi |= (uint64_t)digit_of(key.hi, aux, d) << (8 * (d - 2));
        lo = digit_of(key.hi, aux, 0) | digit_of(key.hi, aux, 1) << 8;
        CHECK(hi == key.hi && lo == key.lo && key.lo < 1024 && digit_of(key.hi, aux, 10) == key.null && position_of(aux) == k);
    }
}

}  // namespace

int main() {
    pinned();
    for (uint32_t round = 0; round < 4000; round++) hostile_round();
    if (failures) return printf("%d checks failed\n", failures), 1;
    printf("sort_rows_sanitize ok\n");
    return 0;
}
