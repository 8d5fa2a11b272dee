// group_keys_math.h -- the arithmetic of msj_bucket_rows_device and msj_group_keys_device (group_keys_kernel.hip): a number
// floored to a multiple of a width, one record in and one record out; a key part's bytes -- a NUMBER from sort_rows_math.h's
// ascending key, a CODE big-endian -- and the NUMBER part decoded back to its canonical value; the key's width and what the
// two calls say of themselves.  Host + device like its siblings, so that tests/test_group_keys_math.py runs the same code
// on the CPU (g++, tests/group_keys_math_host.cpp).
//
// The bucket (include/msj_stage1.h).  f is the value of an 'l' and floor(value) of a 'd'; the result
// is s = origin + floor((f - origin) / width) * width = f - r with r = (f - origin) mod width in [0, width).  f - origin
// has 65 bits, so it is taken as an unsigned 64-bit difference in two cases: f >= origin, where r is the difference's
// remainder, and f < origin, where r is width minus the remainder of origin - f (0 when that is 0).  No 128-bit word and no
// multiply; s <= f, so only s < INT64_MIN leaves int64.
#pragma once
#include <stdint.h>

#include "sort_rows_math.h"

namespace msj {
namespace gkeys {

using msj::agg::floor_log2;
using msj::agg::kNoNumber;
using msj::agg::kSkipped;
using msj::agg::kValue;
using msj::agg::quantum;
using msj::agg::significand;
using msj::agg::value_kind;
using msj::scol::kMaxRows;
using msj::sel::kFieldNoBits;
using msj::sel::kIncorrectType;

constexpr uint32_t kNumber = 1, kCode = 2;  // msj_key_part.kind: MSJ_KEY_NUMBER, MSJ_KEY_CODE
constexpr uint32_t kNullIsGroup = 1;        // msj_key_part.flags: MSJ_KEY_NULL_IS_GROUP
constexpr uint32_t kMaxParts = 8, kNumberBytes = 11, kCodeBytes = 5, kMaxWidth = kMaxParts * kNumberBytes;
constexpr uint32_t kNumberError = 9;  // the reference's errors.mojo: NUMBER_ERROR (msj_cast_strings_device's code)
constexpr uint64_t kSign = 1ull << 63;

// ---- the bucket ---------------------------------------------------------------------------------------------------------------
// floor of a finite double as an int64 -> false: it lies outside int64.  *whole: the double is an integer
MSJ_HD bool floor_of_double(uint64_t bits, int64_t *f, bool *whole) {
    const bool neg = (bits >> 63) != 0;
    const uint64_t m = significand(bits);
    const int q = quantum(bits);  // the value is +-m * 2^q, m < 2^53
    *whole = true, *f = 0;
    if (m == 0) return true;
    if (q >= 0) {
        const uint32_t e = floor_log2(m) + (uint32_t)q;  // the leading bit of the magnitude
        if (e > 63) return false;
        const uint64_t mag = m << q;
        if (e == 63 && !(neg && mag == kSign)) return false;  // (only -2^63 itself)
        *f = (int64_t)(neg ? 0ull - mag : mag);
        return true;
    }
    const uint64_t t = -q >= 64 ? 0 : m >> -q;                       // (t < 2^53)
    const bool rest = -q >= 64 ? true : (m & ((1ull << -q) - 1)) != 0;
    *whole = !rest;
    *f = neg ? -(int64_t)(t + (rest ? 1u : 0u)) : (int64_t)t;
    return true;
}
// r = (f - origin) mod width in [0, width); width >= 1
MSJ_HD uint64_t bucket_remainder(int64_t f, uint64_t width, int64_t origin) {
    if (f >= origin) return ((uint64_t)f - (uint64_t)origin) % width;
    const uint64_t m = ((uint64_t)origin - (uint64_t)f) % width;
    return m ? width - m : 0;
}
// s = f - r -> false: s < INT64_MIN
MSJ_HD bool bucket_floor(int64_t f, uint64_t width, int64_t origin, int64_t *s) {
    const uint64_t r = bucket_remainder(f, width, origin);
    if (r > ((uint64_t)f ^ kSign)) return false;  // (f - INT64_MIN as an unsigned word)
    *s = (int64_t)((uint64_t)f - r);
    return true;
}

// what became of one record.  kPassed: it has a code and is written as it is, counted nowhere
constexpr uint32_t kPassed = 0, kBucketed = 1, kRange = 2, kNoBits = 3, kOther = 4;
MSJ_HD bool bad_bucket(int64_t width, uint32_t flags) { return width < 1 || flags != 0; }
// one record in, one record out (width >= 1)
template <class Field>
MSJ_HD uint32_t bucket_record(const Field &in, int64_t width, int64_t origin, Field &out) {
    if (in.code != 0) {
        out = in;
        return kPassed;
    }
    const uint32_t kind = value_kind(in);
    if (kind == kNoNumber) {
        out = msj::sel::error_field<Field>(kIncorrectType);
        return kOther;
    }
    out = msj::sel::error_field<Field>(kNumberError);
    if (kind == kSkipped) return kNoBits;
    int64_t f = (int64_t)in.bits, s;
    bool whole;
    if (in.type == 'd' && !floor_of_double(in.bits, &f, &whole)) return kRange;
    if (!bucket_floor(f, (uint64_t)width, origin, &s)) return kRange;
    out.bits = (uint64_t)s, out.token = in.token, out.type = 'l', out.flags = 0, out.code = 0;
    return kBucketed;
}

// ---- a key part's bytes -------------------------------------------------------------------------------------------------------
MSJ_HD uint32_t part_width(uint32_t kind) { return kind == kNumber ? kNumberBytes : kind == kCode ? kCodeBytes : 0; }
MSJ_HD bool bad_part(uint32_t kind, uint32_t flags) { return (kind != kNumber && kind != kCode) || (flags & ~kNullIsGroup) != 0; }
// a record as a NUMBER part: tag 0x00, sort_rows_math.h's ascending key big-endian, hi in 8 bytes and lo in 2; a record that
// is no number value: tag 0x01 and ten zero bytes -> true: the part is null
template <class Field>
MSJ_HD bool encode_number(const Field &f, uint8_t *out) {
    const msj::srows::Key k = msj::srows::make_key(value_kind(f) == kValue, f.type, f.bits, 0);
    out[0] = (uint8_t)k.null;
    for (int i = 0; i < 8; i++) out[1 + i] = (uint8_t)(k.hi >> (56 - 8 * i));
    out[9] = (uint8_t)(k.lo >> 8), out[10] = (uint8_t)k.lo;
    return k.null != 0;
}
// a code as a CODE part: tag 0x00 and the code big-endian; a code below 0: tag 0x01 and four zero bytes
MSJ_HD bool encode_code(int32_t code, uint8_t *out) {
    const bool null = code < 0;
    const uint32_t c = null ? 0 : (uint32_t)code;
    out[0] = null ? 1 : 0, out[1] = (uint8_t)(c >> 24), out[2] = (uint8_t)(c >> 16), out[3] = (uint8_t)(c >> 8), out[4] = (uint8_t)c;
    return null;
}
// A NUMBER part back to its canonical value: an integer inside int64 is that int64 ('l'), anything else the double ('d').
// -> false: the part is null (or its tag is none of the two).  Any eleven bytes are safe
MSJ_HD bool decode_number(const uint8_t *p, uint32_t *type, uint64_t *bits) {
    *type = 0, *bits = 0;
    if (p[0] != 0) return false;
    uint64_t hi = 0;
    for (int i = 0; i < 8; i++) hi = hi << 8 | p[1 + i];
    const uint32_t lo = (uint32_t)p[9] << 8 | p[10];
    const uint64_t d = (hi >> 63) ? hi ^ kSign : ~hi;  // (the inverse of srows::ordered)
    int64_t f;
    bool whole;
    if (msj::agg::is_finite_bits(d) && floor_of_double(d, &f, &whole) && whole) {
        *type = 'l', *bits = (uint64_t)f + lo;  // (an int64's key: d is its floor among the doubles, lo what lies above it)
        return true;
    }
    *type = 'd', *bits = d;
    return true;
}
MSJ_HD bool decode_code(const uint8_t *p, int32_t *code) {
    *code = (int32_t)((uint32_t)p[1] << 24 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 8 | p[4]);
    return p[0] == 0;
}

// ---- what the keys call says of itself ----------------------------------------------------------------------------------------
// the code: the select result's wins; then the sizes (R < 2^31 and W <= 88: R * W does not wrap)
MSJ_HD int32_t head_code(int32_t rows_code, uint64_t R, uint64_t stride, uint64_t capacity, uint64_t W, uint64_t bytes_capacity,
                         int32_t capacity_code) {
    if (rows_code != 0) return rows_code;
    return R > stride || R > capacity || R >= kMaxRows || R * W > bytes_capacity ? capacity_code : 0;
}

}  // namespace gkeys
}  // namespace msj
