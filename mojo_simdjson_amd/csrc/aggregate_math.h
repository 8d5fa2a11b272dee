// aggregate_math.h -- the arithmetic of msj_aggregate_device (aggregate_kernel.hip): which record is a number value, the
// exponent of an int64 and of a double, a value as three signed 32-bit limbs of its fixed-point form for a group's
// exponent, the limb sums put together as one signed 128-bit integer, that integer rounded ONCE to a binary64, the min / max
// merge rule, and the 48-byte record made from a group's accumulators.  Host + device like its siblings, so that
// tests/test_aggregate_math.py runs the same code on the CPU (g++, tests/aggregate_math_host.cpp).
//
// Definition (include/msj_stage1.h).  A group's sum is an exact int64 while every value is an 'l' and
// the integer sum fits.  Otherwise, with E the largest floor(log2|v|) over the group's non-zero values, every value becomes
// the integer t = trunc(v * 2^(95 - E)), |t| < 2^96; S = sum of t is exact (fewer than 2^31 rows: |S| < 2^127); the result
// is S * 2^(E - 95) rounded once to the nearest binary64, ties to even.  Everything up to the rounding is integer addition,
// so no order of the rows and no schedule of the lanes can change a bit of it.
#pragma once
#include <stdint.h>

#include "filter_rows_math.h"

namespace msj {
namespace agg {

using msj::frows::cmp_int_double;
using msj::frows::double_of;
using msj::frows::is_finite_bits;
using msj::frows::kMaxColumns;
using msj::frows::rows_over;
using msj::sel::kFieldNoBits;

constexpr uint32_t kIntOverflow = 1u, kInfinite = 2u;  // msj_aggregate.flags: MSJ_AGG_INT_OVERFLOW, MSJ_AGG_INFINITE
constexpr int kTop = 95;                               // the largest value's leading bit in its fixed-point form
constexpr uint32_t kExpBias = 1075;                    // an exponent is kept as E + 1075 >= 1; 0: no non-zero value
constexpr uint64_t kSign = 1ull << 63;

// ---- which record is a number value ------------------------------------------------------------------------------------------
constexpr uint32_t kNoNumber = 0, kValue = 1, kSkipped = 2;
// kValue: code 0, type 'l' or 'd', bits present, a 'd' finite.  kSkipped: code 0 and type 'l' / 'd', but no usable bits
template <class Field>
MSJ_HD uint32_t value_kind(const Field &f) {
    if (f.code != 0 || (f.type != 'l' && f.type != 'd')) return kNoNumber;
    if (f.flags & kFieldNoBits) return kSkipped;
    return f.type == 'd' && !is_finite_bits(f.bits) ? kSkipped : kValue;
}
// row k's group: d_codes[k] when that lies in [0, G), codes == NULL: 0; -1: the row is in no group
MSJ_HD int64_t group_of(const int32_t *codes, uint64_t k, uint64_t G) {
    const int64_t g = codes ? (int64_t)codes[k] : 0;
    return g >= 0 && (uint64_t)g < G ? g : -1;
}

// ---- exponents (as E + kExpBias; 0 for the value 0) --------------------------------------------------------------------------
MSJ_HD uint64_t magnitude(int64_t v) { return v < 0 ? 0ull - (uint64_t)v : (uint64_t)v; }  // (INT64_MIN: 2^63)
MSJ_HD uint32_t floor_log2(uint64_t m) { return 63u - (uint32_t)__builtin_clzll(m); }      // m != 0
MSJ_HD uint32_t exp_key_int(int64_t v) { return v == 0 ? 0 : floor_log2(magnitude(v)) + kExpBias; }
// a finite double is m * 2^q: m the 53-bit significand as an integer, q = max(biased, 1) - 1075
MSJ_HD uint64_t significand(uint64_t bits) {
    const uint64_t frac = bits & ((1ull << 52) - 1);
    return ((bits >> 52) & 0x7FFu) ? frac | (1ull << 52) : frac;
}
MSJ_HD int quantum(uint64_t bits) {
    const int biased = (int)((bits >> 52) & 0x7FFu);
    return (biased ? biased : 1) - 1075;
}
MSJ_HD uint32_t exp_key_double(uint64_t bits) {
    const uint64_t m = significand(bits);
    return m == 0 ? 0 : (uint32_t)((int)floor_log2(m) + quantum(bits) + (int)kExpBias);
}
MSJ_HD uint32_t exp_key(uint32_t type, uint64_t bits) { return type == 'l' ? exp_key_int((int64_t)bits) : exp_key_double(bits); }

// ---- a value as limbs --------------------------------------------------------------------------------------------------------
// the int path: v = l[1] * 2^32 + l[0], l[0] in [0, 2^32), l[1] in [-2^31, 2^31)
MSJ_HD void int_limbs(int64_t v, int64_t l[2]) { l[0] = (int64_t)((uint64_t)v & 0xFFFFFFFFull), l[1] = v >> 32; }
// the double path: t = trunc(v * 2^(95 - E)) = sign * (l[2] * 2^64 + l[1] * 2^32 + l[0]), each |l[i]| < 2^32 with the
// value's sign.  ekey: the group's E + kExpBias, at least the value's own (a smaller one drops the bits above 2^96: nothing
// is read or written by it).  The magnitude m * 2^q is shifted by s = q + 95 - E: to the left at most 95 places, to the
// right any number -- the bits below 2^(E - 95) are cut, towards zero
MSJ_HD void value_limbs(uint32_t type, uint64_t bits, uint32_t ekey, int64_t l[3]) {
    l[0] = l[1] = l[2] = 0;
    const bool neg = type == 'l' ? (int64_t)bits < 0 : (bits >> 63) != 0;
    const uint64_t m = type == 'l' ? magnitude((int64_t)bits) : significand(bits);
    const int s = (type == 'l' ? 0 : quantum(bits)) + kTop - ((int)ekey - (int)kExpBias);
    if (m == 0 || ekey == 0 || s <= -64) return;
    uint64_t p[3];
    int w = 0;
    if (s < 0) {
        p[0] = (m >> -s) & 0xFFFFFFFFull, p[1] = (m >> -s) >> 32, p[2] = 0;
    } else {
        const int b = s & 31;
        const uint64_t lo = m << b, hi = b ? m >> (64 - b) : 0;
        p[0] = lo & 0xFFFFFFFFull, p[1] = lo >> 32, p[2] = hi;
        w = s >> 5;
    }
    for (int i = 0; i + w < 3; i++) l[i + w] = neg ? -(int64_t)p[i] : (int64_t)p[i];
}

// ---- the limb sums as one signed 128-bit integer -----------------------------------------------------------------------------
struct S128 {
    uint64_t lo;
    int64_t hi;
};
// a0 + a1 * 2^32 + a2 * 2^64 (two's complement; with fewer than 2^31 rows every |a| < 2^63 and the sum needs no 129th bit)
MSJ_HD S128 recombine(int64_t a0, int64_t a1, int64_t a2) {
    uint64_t lo = (uint64_t)a0, hi = a0 < 0 ? ~0ull : 0ull;
    const uint64_t lo1 = (uint64_t)a1 << 32;
    lo += lo1;
    hi += (uint64_t)(a1 >> 32) + (lo < lo1 ? 1u : 0u) + (uint64_t)a2;
    return S128{lo, (int64_t)hi};
}
MSJ_HD bool fits_int64(const S128 &s) { return s.hi == ((int64_t)s.lo < 0 ? -1 : 0); }

// s * 2^scale rounded once to the nearest binary64, ties to even, subnormals included -> the pattern.  Beyond DBL_MAX:
// +-infinity and *infinite set.  s == 0: +0.0
MSJ_HD uint64_t round_scaled(const S128 &s, int scale, bool *infinite) {
    *infinite = false;
    const bool neg = s.hi < 0;
    uint64_t lo = s.lo, hi = (uint64_t)s.hi;
    if (neg) lo = 0ull - lo, hi = ~hi + (lo == 0 ? 1u : 0u);
    if ((lo | hi) == 0) return 0;
    const uint64_t sign = neg ? kSign : 0;
    const int p = hi ? 64 + (int)floor_log2(hi) : (int)floor_log2(lo);  // the leading bit of |s|
    const int e = p + scale;                                            // ... of the real number
    const int lsb = e - 52 > -1074 ? e - 52 : -1074;                    // the result's last place
    const int cut = lsb - scale;                                        // ... as a bit of |s|: what lies below is rounded away
    uint64_t mant;
    if (cut <= 0) {
        mant = lo << -cut;  // (p - cut <= 52: |s| has at most 53 bits here, all in lo)
    } else if (cut > 128) {
        return sign;        // (|s| < 2^128 <= half a last place)
    } else {
        // |s| = mant * 2^cut + rest; half = 2^(cut - 1)
        uint64_t rest_lo, rest_hi, half_lo, half_hi;
        if (cut >= 128) mant = 0, rest_lo = lo, rest_hi = hi;
        else if (cut >= 64) mant = cut == 64 ? hi : hi >> (cut - 64), rest_lo = lo, rest_hi = cut == 64 ? 0 : hi & ((1ull << (cut - 64)) - 1);
        else mant = (lo >> cut) | (hi << (64 - cut)), rest_lo = lo & ((1ull << cut) - 1), rest_hi = 0;  // (1 <= cut; p - cut <= 52: the bits of hi the shift drops are 0)
        if (cut - 1 >= 64) half_lo = 0, half_hi = 1ull << (cut - 1 - 64);
        else half_lo = 1ull << (cut - 1), half_hi = 0;
        const bool above = rest_hi > half_hi || (rest_hi == half_hi && rest_lo > half_lo);
        const bool tie = rest_hi == half_hi && rest_lo == half_lo;
        if (above || (tie && (mant & 1))) mant++;
    }
    // mant has its leading bit at 2^52 (a normal), below it (a subnormal: lsb == -1074), or after a carry at 2^53: one sum
    // serves all three
    const uint64_t mag = ((uint64_t)(lsb + 1074) << 52) + mant;
    if (mag >= 0x7FF0000000000000ull) {
        *infinite = true;
        return sign | 0x7FF0000000000000ull;
    }
    return sign | mag;
}

// ---- min / max ---------------------------------------------------------------------------------------------------------------
// order-preserving keys: a < b as numbers iff key(a) < key(b) as uint64; among doubles -0.0 lies below +0.0
MSJ_HD uint64_t int_key(int64_t v) { return (uint64_t)v ^ kSign; }
MSJ_HD int64_t int_of_key(uint64_t k) { return (int64_t)(k ^ kSign); }
MSJ_HD uint64_t double_key(uint64_t bits) { return (bits >> 63) ? ~bits : bits | kSign; }
MSJ_HD uint64_t double_of_key(uint64_t k) { return (k >> 63) ? k & ~kSign : ~k; }
// a value (type, bits) against another as real numbers, int64 against double exactly: -1, 0, 1.  Both finite
MSJ_HD int cmp_values(uint32_t ta, uint64_t a, uint32_t tb, uint64_t b) {
    if (ta == 'l' && tb == 'l') return (int64_t)a < (int64_t)b ? -1 : (int64_t)a > (int64_t)b ? 1 : 0;
    if (ta == 'l') return cmp_int_double((int64_t)a, double_of(b));
    if (tb == 'l') return -cmp_int_double((int64_t)b, double_of(a));
    const double x = double_of(a), y = double_of(b);
    return x < y ? -1 : x > y ? 1 : 0;
}
// the merge rule: does the candidate replace what is held?  want = -1 for a minimum, 1 for a maximum.  Between equal reals
// the 'l' wins, whichever way round; between two equal doubles the key decides (-0.0 below +0.0)
MSJ_HD bool replaces(int want, uint32_t t_new, uint64_t b_new, uint32_t t_old, uint64_t b_old) {
    const int c = cmp_values(t_new, b_new, t_old, b_old);
    if (c != 0) return c == want;
    if (t_new != t_old) return t_new == 'l';
    if (t_new == 'l') return false;
    return want < 0 ? double_key(b_new) < double_key(b_old) : double_key(b_new) > double_key(b_old);
}

// ---- a group's accumulators --------------------------------------------------------------------------------------------------
// All zero before the first row; every member grows by an integer add or an integer max alone, so any order of the rows and
// any split of them over lanes ends in the same words.  The minima are kept as the maximum of the inverted key
struct Acc {
    uint64_t n_rows, n_values, n_double;
    uint64_t ekey;              // the largest exp_key
    uint64_t int_min_inv, int_max, dbl_min_inv, dbl_max;  // keys; read only where n_values - n_double / n_double say there is one
    int64_t a[3];               // the limb sums: int_limbs while n_double == 0, else value_limbs
    uint64_t reserved;
};
static_assert(sizeof(Acc) == 96, "layout");

// pass 1 of one value
MSJ_HD void acc_note(Acc &x, uint32_t type, uint64_t bits) {
    x.n_values++;
    const uint64_t e = exp_key(type, bits);
    if (e > x.ekey) x.ekey = e;
    if (type == 'l') {
        const uint64_t k = int_key((int64_t)bits);
        if (~k > x.int_min_inv) x.int_min_inv = ~k;
        if (k > x.int_max) x.int_max = k;
    } else {
        const uint64_t k = double_key(bits);
        x.n_double++;
        if (~k > x.dbl_min_inv) x.dbl_min_inv = ~k;
        if (k > x.dbl_max) x.dbl_max = k;
    }
}
// pass 2 of one value: its limbs for what pass 1 found
MSJ_HD void pass2_limbs(uint64_t n_double, uint64_t ekey, uint32_t type, uint64_t bits, int64_t l[3]) {
    if (n_double == 0) int_limbs((int64_t)bits, l), l[2] = 0;
    else value_limbs(type, bits, (uint32_t)ekey, l);
}

// the 48-byte record of a group.  Record: msj_aggregate
template <class Record>
MSJ_HD Record finish_group(const Acc &x) {
    Record r;
    r.n_rows = x.n_rows, r.n_values = x.n_values;
    r.sum_bits = r.min_bits = r.max_bits = 0;
    r.sum_type = r.min_type = r.max_type = r.flags = 0;
    r.reserved = 0;
    if (x.n_values == 0) return r;
    const S128 s = recombine(x.a[0], x.a[1], x.a[2]);
    if (x.n_double == 0 && fits_int64(s)) {
        r.sum_type = 'l', r.sum_bits = s.lo;
    } else {
        // (all 'l' and too large: the int limbs are S with E - 95 = 0, every t exact)
        bool infinite;
        r.sum_type = 'd';
        r.sum_bits = round_scaled(s, x.n_double == 0 ? 0 : (int)x.ekey - (int)kExpBias - kTop, &infinite);
        if (x.n_double == 0) r.flags |= kIntOverflow;
        if (infinite) r.flags |= kInfinite;
    }
    const bool ints = x.n_values > x.n_double, doubles = x.n_double != 0;
    const uint64_t imin = (uint64_t)int_of_key(~x.int_min_inv), imax = (uint64_t)int_of_key(x.int_max);
    const uint64_t dmin = double_of_key(~x.dbl_min_inv), dmax = double_of_key(x.dbl_max);
    if (ints && !(doubles && replaces(-1, 'd', dmin, 'l', imin))) r.min_type = 'l', r.min_bits = imin;
    else r.min_type = 'd', r.min_bits = dmin;
    if (ints && !(doubles && replaces(1, 'd', dmax, 'l', imax))) r.max_type = 'l', r.max_bits = imax;
    else r.max_type = 'd', r.max_bits = dmax;
    return r;
}

// ---- the call's verdict on itself --------------------------------------------------------------------------------------------
MSJ_HD bool groups_over(uint64_t G, uint64_t groups_capacity) { return G > groups_capacity; }

}  // namespace agg
}  // namespace msj
