// validate_math.h -- the per-token rule of msj_validate_device (validate_kernel.hip): stage 2's verdict for one document
// without the walk.  Host + device like number_math.h, so that tests/test_validate_math.py runs the same code on the CPU
// (g++, tests/validate_math_host.cpp).
//
// Definition (include/msj_stage1.h): the code and the token at which the reference's walk_document
// (generic/stage2/json_iterator.mojo:40-254) with TapeBuilder's visitors would stop.  The walker's state in front of token
// i follows from the tokens i-1 .. i-3 and one hop through the bracket partners, as long as no earlier token is in error;
// the walker returns the code of the FIRST token in error.  So every token is judged on its own (token_rule) and the
// verdict is the minimum over the tokens that report something.
//
//   in front of i                      i must be
//   nothing (i == 0)                   a value; a root bracket also needs the matching last token
//   {                                  } or a key string
//   [                                  ] or a value
//   :                                  a value
//   ,                                  in_object(i-2): a key string; else a value
//   a string that is a key             :
//   any other scalar, } or ]           root: i == n; in_object(i-1): , or }; else , or ]
//   anything else                      (an earlier token is in error: nothing)
//
// vstart(j) = j for a scalar, the partner for a closing bracket; in_object(j) = type[vstart(j) - 1] == ':', "root" when
// vstart(j) == 0, "unknown" (nothing is reported) when there is no usable partner.  Inside an object every value is
// preceded by ':', inside an array by '[' or ',': that is the whole reason one hop is enough.
#pragma once
#include <stdint.h>

#if !defined(MSJ_HD)
#if defined(__HIPCC__)
#define MSJ_HD __host__ __device__ __forceinline__
#else
#define MSJ_HD static inline
#endif
#endif
// member functions (MSJ_HD is `static` on the host)
#if !defined(MSJ_HM)
#if defined(__HIPCC__)
#define MSJ_HM __host__ __device__ __forceinline__
#else
#define MSJ_HM inline
#endif
#endif

namespace msj {
namespace val {

// reference codes (errors.py, dom_parser_implementation.hpp)
constexpr uint32_t kCapacity = 1, kTape = 3, kDepth = 4, kString = 5, kTAtom = 6, kFAtom = 7, kNAtom = 8, kNumber = 9;
constexpr uint32_t kMaxElements = 0xFFFFFFu;                    // tape_builder.mojo:257-264
constexpr uint64_t kBigSpan = 2ull * kMaxElements + 1ull;       // tokens between the brackets from which the count can overflow
constexpr uint32_t kNoPartner = 0xFFFFFFFFu;
constexpr uint32_t kSpanEscaped = 2u;                           // MSJ_SPAN_ESCAPED

// what token_rule leaves to the content check
constexpr uint32_t kRoleNone = 0, kRoleScalar = 1;

// One code per token, first token wins; at a token a structure / depth error (rank 0) comes before a content error
// (rank 1).  The minimum of these words over the tokens is the verdict.
constexpr uint64_t kNoError = ~0ull;
MSJ_HD uint64_t pack_error(uint64_t token, uint32_t rank, uint32_t code) { return (token << 8) | ((uint64_t)rank << 4) | code; }
MSJ_HD uint64_t packed_token(uint64_t e) { return e >> 8; }
MSJ_HD uint32_t packed_code(uint64_t e) { return (uint32_t)(e & 15u); }

MSJ_HD bool is_open(uint32_t t) { return t == '{' || t == '['; }
MSJ_HD bool is_close(uint32_t t) { return t == '}' || t == ']'; }
MSJ_HD bool is_scalar(uint32_t t) {  // first byte of a value that is not a container (visit_primitive :309-329)
    return t == '"' || t == '-' || t - '0' < 10u || t == 't' || t == 'f' || t == 'n';
}
MSJ_HD bool ends_atom(uint32_t c) {  // structural or blank
    return c == ',' || c == ':' || c == '[' || c == ']' || c == '{' || c == '}' || c == ' ' || c == '\t' || c == '\n' ||
           c == '\r';
}

// in_object: 0 = array, 1 = object, 2 = root, 3 = unknown.  A: type(j) (0 outside [0, n)), match(j), for int64 j.
constexpr uint32_t kInArray = 0, kInObject = 1, kInRoot = 2, kInUnknown = 3;
template <class A>
MSJ_HD uint32_t in_object(const A &a, int64_t j) {
    if (j < 0) return kInUnknown;
    int64_t s = j;
    if (is_close(a.type(j))) {
        const uint32_t m = a.match(j);
        if (m == kNoPartner || (int64_t)m >= j) return kInUnknown;  // no index from d_match is used unchecked
        s = (int64_t)m;
    }
    if (s == 0) return kInRoot;
    return a.type(s - 1) == ':' ? kInObject : kInArray;
}

// token i expected to be a value: the structure / depth code, or 0 with `role` = what is left to check
template <class A>
MSJ_HD uint32_t value_rule(const A &a, int64_t i, uint32_t t, uint32_t max_depth, uint32_t &role) {
    if (is_open(t)) {
        if (a.type(i + 1) == t + 2u) return 0;  // '{' + 2 = '}', '[' + 2 = ']': empty containers never count
        const int64_t d = (int64_t)a.depth(i) + 1;
        if (t == '{' ? d > (int64_t)max_depth : d >= (int64_t)max_depth) return kDepth;  // :87 and :176, as written
        return 0;
    }
    if (is_scalar(t)) {
        role = kRoleScalar;
        return 0;
    }
    return kTape;
}
MSJ_HD uint32_t key_rule(uint32_t t, uint32_t &role) {
    if (t != '"') return kTape;
    role = kRoleScalar;
    return 0;
}

// The local rule: the structure / depth code of token i in [0, n] (token n is the end of the stream), 0 = none.
template <class A>
MSJ_HD uint32_t token_rule(const A &a, int64_t i, int64_t n, uint32_t max_depth, uint32_t &role) {
    role = kRoleNone;
    const uint32_t t = a.type(i);
    if (i == 0) {
        if (is_open(t) && a.type(n - 1) != t + 2u) return kTape;  // :54-59
        return value_rule(a, i, t, max_depth, role);
    }
    const uint32_t p = a.type(i - 1);
    if (p == '{') return t == '}' ? 0 : key_rule(t, role);
    if (p == '[') return t == ']' ? 0 : value_rule(a, i, t, max_depth, role);
    if (p == ':') return value_rule(a, i, t, max_depth, role);
    if (p == ',') {
        const uint32_t k = in_object(a, i - 2);
        if (k == kInUnknown || k == kInRoot) return 0;  // an earlier token is in error
        return k == kInObject ? key_rule(t, role) : value_rule(a, i, t, max_depth, role);
    }
    if (is_scalar(p) || is_close(p)) {
        if (p == '"') {
            const uint32_t q = a.type(i - 2);
            if (q == '{' || (q == ',' && in_object(a, i - 3) == kInObject)) return t == ':' ? 0 : kTape;  // a key
        }
        const uint32_t k = in_object(a, i - 1);
        if (k == kInUnknown) return 0;
        if (k == kInRoot) return i == n ? 0 : kTape;  // :248-253
        if (t == ',') return 0;
        return t == (k == kInObject ? (uint32_t)'}' : (uint32_t)']') ? 0 : kTape;
    }
    return 0;  // p is no token the walker can stand behind: token i - 1 is in error
}

// ---- content -------------------------------------------------------------------------------------------------------
// R: at(p) = the byte at offset p (bytes at or past len read as blanks)

// t / f / n: the atom's code, 0 if it spells true / false / null and ends there (atom_parsing.mojo:34-80)
template <class R>
MSJ_HD uint32_t atom_code(const R &r, uint64_t p, uint32_t t) {
    if (t == 't') return (r.at(p + 1) == 'r' && r.at(p + 2) == 'u' && r.at(p + 3) == 'e' && ends_atom(r.at(p + 4))) ? 0 : kTAtom;
    if (t == 'f')
        return (r.at(p + 1) == 'a' && r.at(p + 2) == 'l' && r.at(p + 3) == 's' && r.at(p + 4) == 'e' && ends_atom(r.at(p + 5))) ? 0 : kFAtom;
    return (r.at(p + 1) == 'u' && r.at(p + 2) == 'l' && r.at(p + 3) == 'l' && ends_atom(r.at(p + 4))) ? 0 : kNAtom;
}

MSJ_HD uint32_t hex_digit(uint32_t c) {  // 0..15, or 0x10000
    if (c - '0' < 10u) return c - '0';
    c |= 0x20u;
    if (c - 'a' < 6u) return c - 'a' + 10u;
    return 0x10000u;
}
// the four hex digits at p: the code unit, or >= 0x10000 if one of them is no hex digit
template <class R>
MSJ_HD uint32_t hex4(const R &r, uint64_t p) {
    return (hex_digit(r.at(p)) << 12) | (hex_digit(r.at(p + 1)) << 8) | (hex_digit(r.at(p + 2)) << 4) | hex_digit(r.at(p + 3));
}

// Which backslashes start an escape?  Those with an even number of backslashes directly in front: every escape other than
// "\\" continues with a byte that is no backslash, so the walker's position inside a run of backslashes is the parity
// alone.  For 64 bytes at once, without a walk: `bs` has a bit per backslash, `carry` says that the first byte is
// escaped (an odd run ended right in front of the step) and receives the same for the next step.  The subtraction lets
// every run of backslashes flip the alternating bits from its first escape on (the odd / even trick of simdjson's
// escape scanner).
MSJ_HD uint64_t escape_start_mask(uint64_t bs, uint64_t &carry) {
    const uint64_t kOdd = 0xAAAAAAAAAAAAAAAAull;
    const uint64_t potential = bs & ~carry;
    const uint64_t starts = ((((potential << 1) | kOdd) - potential) ^ kOdd) & bs;
    carry = starts >> 63;
    return starts;
}

// Parity of the run of backslashes that ends directly in front of s (body starts at b): the carry a scan that starts at s
// begins with.  Serial; the kernels have a wave-wide form of their own.
template <class R>
MSJ_HD uint64_t run_parity_before(const R &r, uint64_t b, uint64_t s) {
    uint64_t q = s;
    while (q > b && r.at(q - 1) == '\\') q--;
    return (s - q) & 1u;
}

// The escape that starts at the backslash at p, body [b, e): true if it is in error (string_parsing.mojo:267-327).
// kLocal = false: the walker's view, it never stands on the second half of a pair, so a low surrogate is an error.
// kLocal = true: the view of a lane that looks at p alone: a low surrogate is fine when the escape 6 bytes in front is a
// high surrogate's (which then checked the pair itself); `start6` says whether the byte 6 in front starts an escape.
// The escape length (2, 6 or 12) goes to `adv`.
template <bool kLocal, class R>
MSJ_HD bool escape_bad(const R &r, uint64_t b, uint64_t e, uint64_t p, bool start6, uint32_t &adv) {
    adv = 2;
    if (p + 1 >= e) return true;
    const uint32_t c = r.at(p + 1);
    if (c == '"' || c == '\\' || c == '/' || c == 'b' || c == 'f' || c == 'n' || c == 'r' || c == 't') return false;
    if (c != 'u' || p + 6 > e) return true;
    const uint32_t cp = hex4(r, p + 2);
    if (cp > 0xFFFFu) return true;
    adv = 6;
    if (cp - 0xD800u < 0x400u) {  // high: the low half must follow at once
        if (p + 12 > e || r.at(p + 6) != '\\' || r.at(p + 7) != 'u') return true;
        if (hex4(r, p + 8) - 0xDC00u >= 0x400u) return true;
        adv = 12;
        return false;
    }
    if (cp - 0xDC00u < 0x400u) {  // low on its own
        if (!kLocal) return true;
        if (p < b + 6 || !start6 || r.at(p - 5) != 'u') return true;
        return hex4(r, p - 4) - 0xD800u >= 0x400u;
    }
    return false;
}

// the walk over one body, serially: true if an escape is in error
template <class R>
MSJ_HD bool string_bad_serial(const R &r, uint64_t b, uint64_t e) {
    uint64_t p = b;
    while (p < e) {
        if (r.at(p) != '\\') {
            p++;
            continue;
        }
        uint32_t adv;
        if (escape_bad<false>(r, b, e, p, false, adv)) return true;
        p += adv;
    }
    return false;
}

// The same verdict 64 bytes per step, every byte on its own -- what a wave does for a long body and, for the bytes
// [lo, hi) of a huge one, each wave of the grid.  The scan starts one step in front of lo (the escape starts of that step
// are what a low surrogate in the first 6 bytes looks back to) with the parity of the run in front of it; nothing
// before lo is reported.  Linear in hi - lo at any content.
struct ScanState {
    uint64_t carry, prev_starts;
};
MSJ_HD uint64_t scan_begin(uint64_t b, uint64_t lo) { return lo >= b + 64 ? lo - 64 : b; }
// lane `l` of the step at p0, after the wave agreed on `starts` (escape_start_mask of the step's backslashes)
template <class R>
MSJ_HD bool step_lane_bad(const R &r, uint64_t b, uint64_t e, uint64_t lo, uint64_t p0, uint32_t l, uint64_t starts, uint64_t prev_starts) {
    const uint64_t p = p0 + l;
    if (!((starts >> l) & 1u) || p < lo) return false;
    const bool start6 = l >= 6 ? (starts >> (l - 6)) & 1u : (prev_starts >> (58 + l)) & 1u;
    uint32_t adv;
    return escape_bad<true>(r, b, e, p, start6, adv);
}
// the host's form of the whole scan (the twin of validate_kernel.hip: wave_body)
template <class R>
MSJ_HD bool string_bad_steps(const R &r, uint64_t b, uint64_t e, uint64_t lo, uint64_t hi) {
    const uint64_t s = scan_begin(b, lo);
    ScanState st{run_parity_before(r, b, s), 0};
    for (uint64_t p0 = s; p0 < hi; p0 += 64) {
        uint64_t bs = 0;
        for (uint32_t l = 0; l < 64; l++) bs |= (uint64_t)(p0 + l < hi && r.at(p0 + l) == '\\') << l;
        const uint64_t starts = escape_start_mask(bs, st.carry);
        for (uint32_t l = 0; l < 64; l++)
            if (step_lane_bad(r, b, e, lo, p0, l, starts, st.prev_starts)) return true;
        st.prev_starts = starts;
    }
    return false;
}

struct ByteReader {
    const uint8_t *buf;
    uint64_t len;
    MSJ_HM uint32_t at(uint64_t p) const { return p < len ? buf[p] : 0x20u; }
};

}  // namespace val
}  // namespace msj
