// number_math.h -- per-number arithmetic of msj_number_values_device (numbers_kernel.hip): the text of one JSON number
// to an exact int64 or the nearest binary64.  Host + device like token_math.h, so that tests/test_number_math.py runs the
// same code on the CPU (g++, tests/number_math_host.cpp).  No fast-math flag may reach this file: the fast path relies
// on IEEE-correct FP64 multiply and divide.
//
// Definition (include/msj_stage1.h): RFC 8259 plus the value Python's json gives.
//   text      -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)? starting at the token, followed by a structural byte, a
//             blank, or the end of the buffer (bytes at or past len read as blanks); anything else: ERR_SYNTAX
//   integer   no fraction, no exponent: the exact int64; outside [-2^63, 2^63 - 1]: ERR_RANGE; -0 is 0
//   float     the binary64 nearest to the exact decimal value, ties to even, sign kept on underflow; a value whose
//             correct rounding is +-infinity: ERR_RANGE
//
// Three paths (Clinger 1990; Lemire, "Number parsing at a gigabyte per second", 2021):
//   fast      w <= 2^53, no digit dropped, |q| <= 22: one FP64 multiply or divide, exact by IEEE rounding
//   lemire    w * T(q) as a 192-bit product with T(q) the 128-bit significand of 5^q (pow5_table.h).  |T(q) - 5^q 2^s| < 1,
//             so the exact product lies within 2^64 of the computed one; the result is accepted only if no rounding
//             boundary lies inside that interval (no slack where T(q) is exact, q in [0, 55]: ties decide there).  With
//             digits dropped it is run on w and w + 1 and accepted only if both agree.
//   exact     the rest: the first kExactDigits significant digits as a big integer (plus a sticky bit for the digits
//             after them) against the halfway point between the two candidate doubles, by big integers.  A halfway
//             point of binary64 has at most 768 significant digits, so kExactDigits = 800 decides at any length.
#pragma once
#include <stdint.h>

#include "pow5_table.h"

#if !defined(MSJ_HD)
#if defined(__HIPCC__)
#define MSJ_HD __host__ __device__ __forceinline__
#else
#define MSJ_HD static inline
#endif
#endif
// member functions (MSJ_HD is `static` on the host)
#if defined(__HIPCC__)
#define MSJ_HM __host__ __device__ __forceinline__
#else
#define MSJ_HM inline
#endif

namespace msj {
namespace num {

constexpr uint32_t kInt64 = 1, kDouble = 2, kErrSyntax = 3, kErrRange = 4;  // MSJ_NUMBER_*
constexpr uint32_t kPending = 0;                                              // not decided by the fast paths
constexpr int kExactDigits = 800;
constexpr int64_t kExpCap = 1000000000000000ll;  // explicit exponents saturate here (a 10^15 exponent decides alone)

MSJ_HD bool is_digit(uint32_t c) { return c - '0' < 10u; }
MSJ_HD bool ends_number(uint32_t c) {  // structural or blank
    return c == ',' || c == ':' || c == '[' || c == ']' || c == '{' || c == '}' || c == ' ' || c == '\t' || c == '\n' ||
           c == '\r';
}

// 64 x 64 -> 128
MSJ_HD uint64_t mul_lo_hi(uint64_t a, uint64_t b, uint64_t &hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    hi = __umul64hi(a, b);
    return a * b;
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    hi = (uint64_t)(p >> 64);
    return (uint64_t)p;
#endif
}
MSJ_HD int clz64(uint64_t x) {  // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

// Where the runs of digits of one number lie.  The scanner asks three questions about runs of bytes; the lane and the
// host answer them one byte at a time (SerialRuns), the wave path of numbers longer than 1024 characters 64 bytes at a
// time (numbers_kernel.hip).  Every answer is exact, so both give the same Shape.
struct SerialRuns {
    const uint8_t *buf;
    uint64_t len;
    MSJ_HM uint32_t at(uint64_t p) const { return p < len ? buf[p] : 0x20u; }
    MSJ_HM uint64_t run_end(uint64_t p) const {  // first position >= p that is not a digit
        while (is_digit(at(p))) p++;
        return p;
    }
    MSJ_HM uint64_t first_nonzero(uint64_t b, uint64_t e) const {  // first position in [b, e) whose digit is not '0', else e
        while (b < e && buf[b] == '0') b++;
        return b;
    }
    MSJ_HM bool any_nonzero(uint64_t b, uint64_t e) const { return first_nonzero(b, e) < e; }
};

struct Shape {
    uint32_t syntax_ok, neg, is_int;
    uint64_t int_b, int_e;    // integer digits
    uint64_t frac_b, frac_e;  // fraction digits (empty: no fraction)
    int64_t exp10;            // explicit exponent, saturated at +-kExpCap
    uint64_t sig;             // position of the first significant (non-zero) digit; int_e == frac_e == sig: value 0
};

template <class R>
MSJ_HD Shape scan_shape(const R &r, uint64_t start) {
    Shape s = {};
    uint64_t p = start;
    s.neg = r.at(p) == '-';
    p += s.neg;
    s.int_b = p;
    const uint32_t c0 = r.at(p);
    if (c0 == '0') {
        p++;
    } else if (is_digit(c0)) {
        p = r.run_end(p + 1);
    } else {
        return s;  // syntax_ok = 0
    }
    s.int_e = p;
    s.frac_b = s.frac_e = p;
    bool is_int = true;
    if (r.at(p) == '.') {
        s.frac_b = p + 1;
        s.frac_e = r.run_end(p + 1);
        if (s.frac_e == s.frac_b) return s;
        p = s.frac_e;
        is_int = false;
    }
    const uint32_t e = r.at(p);
    if (e == 'e' || e == 'E') {
        p++;
        const uint32_t sg = r.at(p);
        const bool eneg = sg == '-';
        p += (sg == '-' || sg == '+');
        const uint64_t eb = p, ee = r.run_end(p);
        if (ee == eb) return s;
        const uint64_t ez = r.first_nonzero(eb, ee);
        int64_t v = 0;
        if (ee - ez > 15) {
            v = kExpCap;
        } else {
            for (uint64_t k = ez; k < ee; k++) v = v * 10 + (r.at(k) - '0');
            v = v > kExpCap ? kExpCap : v;
        }
        s.exp10 = eneg ? -v : v;
        p = ee;
        is_int = false;
    }
    if (!ends_number(r.at(p))) return s;
    s.syntax_ok = 1;
    s.is_int = is_int;
    s.sig = r.first_nonzero(s.int_b, s.int_e);
    if (s.sig == s.int_e) {
        s.sig = r.first_nonzero(s.frac_b, s.frac_e);
        if (s.sig == s.frac_e) s.int_e = s.frac_e = s.sig;  // all zeros
    }
    return s;
}

// The significant digits as a sequence: [sig, int_e) then [frac_b, frac_e), or [sig, frac_e) when sig is a fraction digit.
struct Digits {
    uint64_t a_b, a_e, b_b, b_e;
    MSJ_HM uint64_t count() const { return (a_e - a_b) + (b_e - b_b); }
    MSJ_HM uint64_t pos(uint64_t k) const { return k < a_e - a_b ? a_b + k : b_b + (k - (a_e - a_b)); }
};
MSJ_HD Digits digits_of(const Shape &s) {
    Digits d;
    if (s.sig < s.int_e) {
        d.a_b = s.sig, d.a_e = s.int_e, d.b_b = s.frac_b, d.b_e = s.frac_e;
    } else {
        d.a_b = d.a_e = s.sig, d.b_b = s.sig, d.b_e = s.frac_e;
    }
    return d;
}
// value = digits * 10^(exp10 - fraction digits): the exponent of the last significant digit
MSJ_HD int64_t exp_of_last(const Shape &s) { return s.exp10 - (int64_t)(s.frac_e - s.frac_b); }

// digits [k, count) hold a non-zero one
template <class R>
MSJ_HD bool tail_nonzero(const R &r, const Digits &d, uint64_t k) {
    const uint64_t na = d.a_e - d.a_b;
    if (k < na) return r.any_nonzero(d.a_b + k, d.a_e) || r.any_nonzero(d.b_b, d.b_e);
    return r.any_nonzero(d.b_b + (k - na), d.b_e);
}

// What the exact path needs beyond the Shape: whether any significant digit after the first kExactDigits is non-zero
// (the wave path computes it in parallel and hands it over; the lane path reads it at its 1024 characters at most).
struct Scan {
    Shape s;
    uint64_t w;        // first <= 19 significant digits
    int64_t q;         // value ~ w * 10^q (exact unless dropped)
    uint32_t dropped;  // a non-zero digit after the 19th significant one
    uint32_t sticky;   // a non-zero digit after the kExactDigits-th
};

template <class R>
MSJ_HD Scan scan_number(const R &r, uint64_t start) {
    Scan sc = {};
    sc.s = scan_shape(r, start);
    if (!sc.s.syntax_ok) return sc;
    const Digits d = digits_of(sc.s);
    const uint64_t n = d.count();
    const uint64_t k = n < 19 ? n : 19;
    uint64_t w = 0;
    for (uint64_t i = 0; i < k; i++) w = w * 10 + (r.at(d.pos(i)) - '0');
    sc.w = w;
    sc.q = exp_of_last(sc.s) + (int64_t)(n - k);
    if (n > 19) sc.dropped = tail_nonzero(r, d, 19);
    if (n > (uint64_t)kExactDigits) sc.sticky = sc.dropped && tail_nonzero(r, d, kExactDigits);
    return sc;
}

// --- integers --------------------------------------------------------------------------------------------------------
template <class R>
MSJ_HD uint32_t to_int64(const R &r, const Scan &sc, uint64_t &bits) {
    bits = 0;
    const uint64_t nd = sc.s.int_e - sc.s.sig;  // "0" and "-0": sig == int_e
    if (nd > 19) return kErrRange;
    const uint64_t lim = sc.s.neg ? (1ull << 63) : (1ull << 63) - 1;
    if (sc.w > lim) return kErrRange;
    bits = sc.s.neg ? (uint64_t)0 - sc.w : sc.w;
    return kInt64;
}

// --- Clinger ---------------------------------------------------------------------------------------------------------
MSJ_HD double pow10_exact(int k) {  // 10^k, k in [0, 22]: exact in binary64
    double p = 1.0;
    for (int i = 0; i < k; i++) p *= 10.0;
    return p;
}
MSJ_HD uint64_t dbits(double d) {
    union {
        double d;
        uint64_t u;
    } x;
    x.d = d;
    return x.u;
}

// --- Eisel-Lemire with an interval test ------------------------------------------------------------------------------
MSJ_HD int floor_log2_pow5(int q) { return (152170 * q) >> 16; }  // q in [-342, 308]; checked exhaustively by the CPU test

struct Approx {
    uint64_t m0;   // candidate significand (truncated), the double's value ~ m0 * 2^e2
    int e2;        // exponent of its unit: -1074 for subnormals
    uint32_t ok;   // rounding decided
    uint64_t bits; // when ok: the binary64 bits without the sign (>= 0x7FF0... : overflow)
};

// w != 0, q in [kPow5Min, kPow5Max]
MSJ_HD Approx lemire(uint64_t w, int q) {
    Approx a = {};
    const int lz = clz64(w);
    w <<= lz;
    const uint64_t th = kPow5[q - kPow5Min][0], tl = kPow5[q - kPow5Min][1];
    // P = w * (th:tl) = p2:p1:p0
    uint64_t h1, h0;
    const uint64_t p0 = mul_lo_hi(w, tl, h0);
    uint64_t p1 = mul_lo_hi(w, th, h1);
    p1 += h0;
    uint64_t p2 = h1 + (p1 < h0);
    const int t = 190 + (int)(p2 >> 63);                 // top bit of P
    const int E = q + floor_log2_pow5(q) - 127 - lz;     // value ~ P * 2^E
    int e2 = t + E - 52;
    if (e2 < -1074) e2 = -1074;
    const int sh = e2 - E;  // bits of P below the unit
    a.e2 = e2;
    const bool exact = q >= 0 && q <= 55;
    if (sh >= 192) {
        // below a quarter of the smallest subnormal even with the error: zero; else undecided (P < 2^192 <= unit)
        a.m0 = 0;
        a.ok = sh >= 194;
        a.bits = 0;
        return a;
    }
    // m0 = P >> sh, r = P mod 2^sh = r2:r1:r0.  sh >= 138 (normals: t - 52; subnormals more), so m0 comes from p2 alone
    const uint64_t m0 = p2 >> (sh - 128), r2 = p2 & ((1ull << (sh - 128)) - 1), r1 = p1, r0 = p0;
    a.m0 = m0;
    // half = 2^(sh-1) = H * 2^64, H = 2^(sh-129) < 2^64; R = r2:r1 is r in units of 2^64 (r0 matters for exact ties only)
    const uint64_t H = 1ull << (sh - 129);
    bool up;
    if (exact) {
        // r vs half exactly; tie -> even
        const bool gt = r2 > H || (r2 == H && (r1 > 0 || r0 > 0));
        const bool eq = r2 == H && r1 == 0 && r0 == 0;
        up = gt || (eq && (m0 & 1));
    } else {
        // the exact product X lies in (P - 2^64, P + 2^64): decided iff that interval stays on one side of the halfway
        // point.  With r = R * 2^64 + r0, r0 < 2^64: below iff R + 2 <= H, above iff R >= H + 1.  (Leaving the bucket
        // [m0, m0 + 1) across its lower or upper edge rounds to the same double as P does: the edge is a representable value.)
        const uint64_t lo2 = r1 + 2, hi2 = r2 + (lo2 < r1);
        const bool below = hi2 < H || (hi2 == H && lo2 == 0);
        const bool above = r2 > H || (r2 == H && r1 >= 1);
        if (!(below || above)) return a;  // ok = 0
        up = above;
    }
    const uint64_t m = m0 + (up ? 1u : 0u);
    a.ok = 1;
    a.bits = ((uint64_t)(e2 + 1074) << 52) + m;  // m in [2^52, 2^53]: carries into the exponent; subnormal: e2 + 1074 = 0
    return a;
}

// --- the exact path: big integers of kWords 64-bit words ---------------------------------------------------------------
// Sizes: digits < 10^800 < 2^2658; the halfway point's 5^c has c <= 800 + 343 + 19; each side of the comparison stays
// below 2^2700.  kWords = 46 holds 2944 bits.
constexpr int kWords = 46;
struct Big {
    uint64_t w[kWords];
    int n;  // words in use
};
MSJ_HD void big_set(Big &b, uint64_t v) {
    b.n = v ? 1 : 0;
    b.w[0] = v;
}
MSJ_HD void big_muladd(Big &b, uint64_t m, uint64_t add) {
    uint64_t carry = add;
    for (int i = 0; i < b.n; i++) {
        uint64_t hi;
        const uint64_t lo = mul_lo_hi(b.w[i], m, hi);
        const uint64_t s = lo + carry;
        carry = hi + (s < lo);
        b.w[i] = s;
    }
    if (carry && b.n < kWords) b.w[b.n++] = carry;
}
MSJ_HD void big_mulpow5(Big &b, int64_t c) {
    const uint64_t p27 = 7450580596923828125ull;  // 5^27
    while (c >= 27) {
        big_muladd(b, p27, 0);
        c -= 27;
    }
    uint64_t p = 1;
    while (c-- > 0) p *= 5;
    if (p != 1) big_muladd(b, p, 0);
}
MSJ_HD void big_shl(Big &b, int64_t s) {
    if (b.n == 0 || s <= 0) return;
    const int ws = (int)(s >> 6), bs = (int)(s & 63);
    int n = b.n + ws + 1;
    if (n > kWords) n = kWords;
    for (int i = n - 1; i >= 0; i--) {
        const int j = i - ws;
        uint64_t v = 0;
        if (j >= 0 && j < b.n) v = b.w[j] << bs;
        if (bs && j - 1 >= 0 && j - 1 < b.n) v |= b.w[j - 1] >> (64 - bs);
        b.w[i] = v;
    }
    b.n = n;
    while (b.n > 0 && b.w[b.n - 1] == 0) b.n--;
}
MSJ_HD int big_cmp(const Big &a, const Big &b) {
    if (a.n != b.n) return a.n < b.n ? -1 : 1;
    for (int i = a.n - 1; i >= 0; i--)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
    return 0;
}

// D (the decimal) against h = (2 m0 + 1) * 2^(e2 - 1); -> the result's bits without sign
template <class R>
MSJ_HD uint64_t exact_round(const R &r, const Scan &sc, uint64_t m0, int e2) {
    const Digits d = digits_of(sc.s);
    const uint64_t n = d.count();
    const uint64_t k = n < (uint64_t)kExactDigits ? n : (uint64_t)kExactDigits;
    Big lhs, rhs;
    big_set(lhs, 0);
    uint64_t i = 0;
    while (i < k) {
        uint64_t chunk = 0, mul = 1;
        for (int j = 0; j < 19 && i < k; j++, i++) {
            chunk = chunk * 10 + (r.at(d.pos(i)) - '0');
            mul *= 10;
        }
        if (lhs.n == 0) {
            big_set(lhs, chunk);
        } else {
            big_muladd(lhs, mul, chunk);
        }
    }
    const int64_t qd = exp_of_last(sc.s) + (int64_t)(n - k);  // D_t = lhs * 10^qd
    big_set(rhs, 2 * m0 + 1);
    // lhs * 5^qd * 2^qd  vs  rhs * 2^(e2 - 1)
    if (qd >= 0) {
        big_mulpow5(lhs, qd);
    } else {
        big_mulpow5(rhs, -qd);
    }
    const int64_t d2 = qd - (int64_t)(e2 - 1);
    if (d2 >= 0) {
        big_shl(lhs, d2);
    } else {
        big_shl(rhs, -d2);
    }
    int c = big_cmp(lhs, rhs);
    if (c == 0 && sc.sticky) c = 1;
    const bool up = c > 0 || (c == 0 && (m0 & 1));
    const uint64_t m = m0 + (up ? 1u : 0u);
    return ((uint64_t)(e2 + 1074) << 52) + m;
}

constexpr uint64_t kInf = 0x7FF0000000000000ull;

struct Result {
    uint64_t bits;
    uint32_t kind;  // kPending: needs the exact path
    uint32_t path;  // 0 fast (and every non-float), 1 lemire, 2 exact
    // carried to the exact path
    uint64_t m0;
    int e2;
};

MSJ_HD Result finish_double(uint64_t mag, uint32_t neg, uint32_t path) {
    Result res = {};
    res.path = path;
    if (mag >= kInf) {
        res.kind = kErrRange;
        return res;
    }
    res.kind = kDouble;
    res.bits = mag | ((uint64_t)neg << 63);
    return res;
}

// Everything but the exact path.  kind = kPending: call exact_round with m0 / e2.
template <class R>
MSJ_HD Result convert_fast(const R &r, const Scan &sc) {
    Result res = {};
    if (!sc.s.syntax_ok) {
        res.kind = kErrSyntax;
        return res;
    }
    if (sc.s.is_int) {
        res.kind = to_int64(r, sc, res.bits);
        return res;
    }
    const uint32_t neg = sc.s.neg;
    if (sc.w == 0) return finish_double(0, neg, 0);
    if (!sc.dropped && sc.w <= (1ull << 53) && sc.q >= -22 && sc.q <= 22) {
        double v = (double)sc.w;
        v = sc.q < 0 ? v / pow10_exact((int)-sc.q) : v * pow10_exact((int)sc.q);
        return finish_double(dbits(v), neg, 0);
    }
    if (sc.q < kPow5Min) return finish_double(0, neg, 0);  // below 10^-323: zero; above 10^308: infinity
    if (sc.q > kPow5Max) return finish_double(kInf, neg, 0);
    const Approx a = lemire(sc.w, (int)sc.q);
    res.m0 = a.m0;
    res.e2 = a.e2;
    if (a.ok) {
        if (!sc.dropped) return finish_double(a.bits, neg, 1);
        // the decimal lies in [w, w + 1) * 10^q: both ends must round alike
        uint64_t w1 = sc.w + 1;
        int q1 = (int)sc.q;
        if (w1 == 10000000000000000000ull) {  // 19 nines + 1
            w1 = 1000000000000000000ull;
            q1++;
        }
        if (q1 <= kPow5Max) {
            const Approx b = lemire(w1, q1);
            if (b.ok && b.bits == a.bits) return finish_double(a.bits, neg, 1);
        }
    }
    res.kind = kPending;
    res.path = 2;
    return res;
}

template <class R>
MSJ_HD Result convert_exact(const R &r, const Scan &sc, const Result &fast) {
    return finish_double(exact_round(r, sc, fast.m0, fast.e2), sc.s.neg, 2);
}

template <class R>
MSJ_HD Result convert(const R &r, uint64_t start) {
    const Scan sc = scan_number(r, start);
    const Result f = convert_fast(r, sc);
    return f.kind == kPending ? convert_exact(r, sc, f) : f;
}

}  // namespace num
}  // namespace msj
