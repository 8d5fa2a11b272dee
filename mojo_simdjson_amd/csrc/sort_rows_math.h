// sort_rows_math.h -- the arithmetic of msj_sort_rows_device (sort_rows_kernel.hip): which record is a number value
// (aggregate_math.h's rule), the order-preserving key of a value, the key's digits as the radix passes see them, what the call
// says of itself (the code, the rows it writes, which of its two paths it takes).  Host + device like its siblings, so that
// tests/test_sort_rows_math.py runs the same code on the CPU (g++, tests/sort_rows_math_host.cpp).
//
// The key (include/msj_stage1.h).  Let d be the value rounded toward minus infinity to a binary64: a
// double is itself with -0.0 made +0.0, an int64 is its floor among the doubles.  hi is d's pattern made unsigned-ordered
// (the whole pattern complemented when the sign is set, else bit 63 set); lo = value - d, 0 for a double and an integer in
// [0, 1024) for an int64 (a last place of an int64's floor is at most 2^10).  (hi, lo) compared lexicographically is the
// order of the reals, and equal reals have equal keys.  Descending complements (hi, lo).  A row without a value has the
// null bit, which lies above everything in both directions, and hi = lo = 0.  All of it is integer arithmetic.
#pragma once
#include <stdint.h>

#include "aggregate_math.h"

namespace msj {
namespace srows {

using msj::agg::floor_log2;
using msj::agg::kNoNumber;
using msj::agg::kSkipped;
using msj::agg::kValue;
using msj::agg::magnitude;
using msj::agg::value_kind;
using msj::scol::kMaxRows;

constexpr uint32_t kDescending = 1u, kValuesOnly = 2u;  // MSJ_SORT_DESCENDING, MSJ_SORT_VALUES_ONLY
constexpr uint32_t kKnownFlags = kDescending | kValuesOnly;
constexpr uint32_t kModeAuto = 0, kModeFull = 1, kModeSelect = 2;  // msj_debug_set_sort_mode
constexpr uint64_t kSign = 1ull << 63;

struct Key {
    uint64_t hi;
    uint32_t lo;    // 10 bits
    uint32_t null;  // 1: a row without a value
};

// the pattern of the double whose value is +-m, m != 0 with at most 53 significant bits (m <= 2^63)
MSJ_HD uint64_t double_bits_of(bool neg, uint64_t m) {
    const uint32_t e = floor_log2(m);
    const uint64_t frac = e >= 52 ? m >> (e - 52) : m << (52 - e);
    return (neg ? kSign : 0) | ((uint64_t)(e + 1023) << 52) | (frac & ((1ull << 52) - 1));
}
MSJ_HD uint64_t ordered(uint64_t bits) { return (bits >> 63) ? ~bits : bits | kSign; }

// the ascending key of an int64: its floor among the doubles and what it lies above that
MSJ_HD Key int_key(int64_t v) {
    Key k{0, 0, 0};
    if (v == 0) {
        k.hi = ordered(0);
        return k;
    }
    const uint64_t m = magnitude(v);
    uint64_t dm = m;
    if (m >= (1ull << 53)) {
        const uint64_t mask = (1ull << (floor_log2(m) - 52)) - 1;  // (at most 11 bits; m + mask <= 2^63 + 2^11)
        if (v > 0) dm = m & ~mask, k.lo = (uint32_t)(m & mask);
        else dm = (m + mask) & ~mask, k.lo = (uint32_t)(dm - m);    // (towards minus infinity: the magnitude grows)
    }
    k.hi = ordered(double_bits_of(v < 0, dm));
    return k;
}
// ... of a finite double
MSJ_HD Key double_key(uint64_t bits) {
    if ((bits << 1) == 0) bits = 0;  // -0.0 is +0.0
    return Key{ordered(bits), 0, 0};
}
// the key of a record's (type, bits) when it is a value (value_kind == kValue), else the null key
MSJ_HD Key make_key(bool value, uint32_t type, uint64_t bits, uint32_t flags) {
    if (!value) return Key{0, 0, 1};
    Key k = type == 'l' ? int_key((int64_t)bits) : double_key(bits);
    if (flags & kDescending) k.hi = ~k.hi, k.lo = ~k.lo & 0x3FFu;
    return k;
}
MSJ_HD bool key_less(const Key &a, const Key &b) {
    if (a.null != b.null) return a.null < b.null;
    if (a.hi != b.hi) return a.hi < b.hi;
    return a.lo < b.lo;
}

// ---- the key as the kernels keep it: two words per row, and its eleven digits, the least significant first --------------------
// aux = position in the input sequence (31 bits) | lo << 32 | null << 42.  Digits 0, 1: lo (8 + 2 bits); 2 .. 9: hi, a byte
// each; 10: the null bit
constexpr uint32_t kDigits = 11, kBuckets = 256;
MSJ_HD uint64_t aux_word(const Key &k, uint64_t position) { return position | (uint64_t)k.lo << 32 | (uint64_t)k.null << 42; }
MSJ_HD uint32_t position_of(uint64_t aux) { return (uint32_t)(aux & 0x7FFFFFFFu); }
MSJ_HD bool digit_in_hi(uint32_t d) { return d >= 2 && d <= 9; }
MSJ_HD uint32_t digit_of_word(uint64_t word, uint32_t d) {  // word: hi for digit_in_hi(d), else aux
    if (d == 0) return (uint32_t)(word >> 32) & 0xFFu;
    if (d == 1) return (uint32_t)(word >> 40) & 0x3u;
    if (d == 10) return (uint32_t)(word >> 42) & 0x1u;
    return (uint32_t)(word >> (8 * (d - 2))) & 0xFFu;
}
MSJ_HD uint32_t digit_of(uint64_t hi, uint64_t aux, uint32_t d) { return digit_of_word(digit_in_hi(d) ? hi : aux, d); }
// the key's digits from 10 down to `low` against pd[]: -1 below, 0 the same, 1 above
MSJ_HD int cmp_digits(uint64_t hi, uint64_t aux, const uint32_t *pd, uint32_t low) {
    for (uint32_t d = kDigits; d-- > low;) {
        const uint32_t x = digit_of(hi, aux, d);
        if (x != pd[d]) return x < pd[d] ? -1 : 1;
    }
    return 0;
}

// ---- what the call says of itself -------------------------------------------------------------------------------------------
// the code: a code of d_rows_in_select wins over one of d_rows_select; then the sizes
MSJ_HD int32_t head_code(int32_t in_code, int32_t rows_code, uint64_t R, uint64_t stride, uint64_t N, uint64_t capacity, int32_t capacity_code) {
    if (in_code != 0) return in_code;
    if (rows_code != 0) return rows_code;
    return R > stride || N > capacity || N >= kMaxRows ? capacity_code : 0;
}
// K, the entries of d_order
MSJ_HD uint64_t rows_written(uint32_t flags, uint64_t limit, uint64_t N, uint64_t n_values) {
    const uint64_t M = (flags & kValuesOnly) ? n_values : N;
    return limit == 0 || limit > M ? M : limit;
}
// The cut-over between the two paths: the selection where a limit asks for at most an eighth of at least 16 384 rows --
// below that the full sort's passes cost less than the selection's histograms and its compaction
constexpr uint64_t kSelectMinRows = 16384, kSelectRatio = 8;
MSJ_HD bool takes_selection(uint32_t mode, uint64_t limit, uint64_t N) {
    if (limit == 0 || N == 0 || mode == kModeFull) return false;
    if (mode == kModeSelect) return true;
    return N >= kSelectMinRows && limit <= N / kSelectRatio;
}
// the selection ends early when the rows at or below the prefix it has fixed are this few: they are all kept and sorted.
// Forced (kModeSelect) it never ends early, so that small inputs reach the last digit and the ties at the cut
MSJ_HD uint64_t select_enough(uint32_t mode, uint64_t k) { return mode == kModeSelect ? 0 : 2 * k + 4096; }

}  // namespace srows
}  // namespace msj
