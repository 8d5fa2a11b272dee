// cast_strings_math.h -- the arithmetic of msj_cast_strings_device (cast_strings_kernel.hip): the timestamp grammar and its
// arithmetic over a reader, the number wrapper around number_math.h's convert, and "one record in, one record and an
// outcome out".  Host + device like its siblings, so that tests/test_cast_strings_math.py runs the same code on the CPU
// (g++, tests/cast_strings_math_host.cpp).
//
// Definition (include/msj_stage1.h): a string row's value is by definition what
// msj_string_column_device writes for the record, so the row test is string_column_math.h's and the bytes of an escaped
// value are tape_math.h's unescape: nothing of either is restated here.  A value of the kind's grammar becomes an 'l' or 'd'
// record that keeps the input's token; any other string row the record of code 9 (NUMBER_ERROR); a row that is no string
// code 17 (INCORRECT_TYPE), or itself when it is a number and MSJ_CAST_KEEP_NUMBERS asks for that; a record with a code
// itself.
#pragma once
#include <stdint.h>

#include "number_math.h"
#include "select_math.h"
#include "string_column_math.h"
#include "validate_math.h"

namespace msj {
namespace cast {

using msj::scol::kMaxRows;
using msj::sel::kFieldNoBits;
using msj::sel::kIncorrectType;

constexpr uint32_t kTimestamp = 1, kNumber = 2;                   // MSJ_CAST_TIMESTAMP, MSJ_CAST_NUMBER
constexpr uint32_t kUnitS = 0, kUnitMs = 1, kUnitUs = 2, kUnitNs = 3;  // MSJ_CAST_UNIT_*
constexpr uint32_t kKeepNumbers = 1u;                             // MSJ_CAST_KEEP_NUMBERS
constexpr uint32_t kNumberError = 9;                              // the reference's errors.mojo: NUMBER_ERROR
constexpr uint32_t kMaxTimestampBytes = 35, kMinTimestampBytes = 10, kMaxNumberBytes = 128;
// what became of one record.  kPassed: it has a code and is written as it is, counted nowhere.  kPending is never an answer of
// cast_record: the kernel's lane path hands the row to the list (an escaped body, a number that needs the exact path)
constexpr uint32_t kPassed = 0, kCast = 1, kSyntax = 2, kRange = 3, kOther = 4, kPending = 5;

MSJ_HD uint32_t result_flags(uint32_t kind, uint32_t unit, uint32_t flags) { return kind | (unit << 8) | (flags << 16); }
// -> 0, or -1: an unknown kind, unit or flag, a unit with the number kind
MSJ_HD int check_kind(uint32_t kind, uint32_t unit, uint32_t flags) {
    if (kind != kTimestamp && kind != kNumber) return -1;
    if (unit > kUnitNs || (kind == kNumber && unit != 0) || (flags & ~kKeepNumbers) != 0) return -1;
    return 0;
}
MSJ_HD bool rows_over(uint64_t R, uint64_t capacity) { return R > capacity || R >= kMaxRows; }
// the most bytes of a value of the kind: a longer one is kSyntax, unread
MSJ_HD uint32_t max_value_bytes(uint32_t kind) { return kind == kTimestamp ? kMaxTimestampBytes : kMaxNumberBytes; }
// an escape of 6 raw bytes gives at least one byte: an escaped body of more raw bytes than this is longer than the kind allows
MSJ_HD uint64_t max_raw_bytes(uint32_t kind) { return 6ull * max_value_bytes(kind); }

// ---- readers ------------------------------------------------------------------------------------------------------------------
// the bytes of a value that lies in `base` at [.., e): blanks behind it, whatever the window holds there
template <class Base>
struct ValueReader {
    const Base &base;
    uint64_t e;
    MSJ_HM uint32_t at(uint64_t p) const { return p < e ? base.at(p) : 0x20u; }
};
// number_math.h's runs over a value that has to be a number WHOLE: the scan accepts a structural byte or a blank behind the
// number, so one of those inside the value reads as a byte no number holds, and the only place the scan can end well is e
template <class Base>
struct NumberRuns {
    const Base &base;
    uint64_t e;
    MSJ_HM uint32_t at(uint64_t p) const {
        if (p >= e) return 0x20u;
        const uint32_t c = base.at(p);
        return msj::num::ends_number(c) ? (uint32_t)'x' : c;
    }
    MSJ_HM uint64_t run_end(uint64_t p) const {
        while (msj::num::is_digit(at(p))) p++;
        return p;
    }
    MSJ_HM uint64_t first_nonzero(uint64_t b, uint64_t end) const {
        while (b < end && at(b) == '0') b++;
        return b;
    }
    MSJ_HM bool any_nonzero(uint64_t b, uint64_t end) const { return first_nonzero(b, end) < end; }
};
// tape_math.h's writer into a few bytes; what lies behind them is measured only
struct BoundedWriter {
    uint8_t *out;
    uint32_t cap;
    MSJ_HM void put(uint64_t o, uint32_t byte) const {
        if (o < cap) out[o] = (uint8_t)byte;
    }
};

// ---- the calendar -------------------------------------------------------------------------------------------------------------
MSJ_HD bool is_leap(uint32_t y) { return (y % 4 == 0 && y % 100 != 0) || y % 400 == 0; }
MSJ_HD uint32_t days_in_month(uint32_t y, uint32_t m) { return m == 2 ? 28u + (is_leap(y) ? 1u : 0u) : 30u + ((m + (m >> 3)) & 1u); }
// days since 1970-01-01 of a proleptic Gregorian date, year 0..9999 (Hinnant, "chrono-Compatible Low-Level Date Algorithms")
MSJ_HD int64_t days_from_civil(uint32_t year, uint32_t m, uint32_t d) {
    const int32_t y = (int32_t)year - (m <= 2 ? 1 : 0);
    const int32_t era = (y >= 0 ? y : y - 399) / 400;
    const uint32_t yoe = (uint32_t)(y - era * 400);
    const uint32_t doy = (153u * (m > 2 ? m - 3 : m + 9) + 2u) / 5u + d - 1u;
    const uint32_t doe = yoe * 365u + yoe / 4u - yoe / 100u + doy;
    return (int64_t)era * 146097 + (int64_t)doe - 719468;
}

// ---- the timestamp --------------------------------------------------------------------------------------------------------------
//   date      = YYYY "-" MM "-" DD
//   time      = hh ":" mm [ ":" ss [ ("." | ",") 1*9DIGIT ] ]
//   offset    = "Z" | "z" | ("+" | "-") hh [ [":"] mm ]
//   timestamp = date [ ("T" | "t" | " ") time [offset] ]
template <class R>
MSJ_HD bool two_digits(const R &r, uint64_t p, uint32_t &v) {
    const uint32_t a = r.at(p) - '0', b = r.at(p + 1) - '0';
    v = a * 10 + b;
    return a < 10u && b < 10u;
}
// seconds * U + fraction as an int64 or not at all: no product here wraps.  secs: within +-3 * 10^11; frac: below U
MSJ_HD uint32_t scale_seconds(int64_t secs, uint32_t unit, uint32_t frac_ns, uint64_t &bits) {
    const int64_t U = unit == kUnitS ? 1 : unit == kUnitMs ? 1000 : unit == kUnitUs ? 1000000 : 1000000000;
    const int64_t frac = (int64_t)(frac_ns / (uint32_t)(1000000000 / U));  // cut to the unit's digits: a floor
    if (unit == kUnitNs) {  // 2^63 - 1 = 9223372036 s + 854775807 ns; -2^63 = -9223372037 s + 145224192 ns
        if (secs > 9223372036ll || (secs == 9223372036ll && frac > 854775807)) return kRange;
        if (secs < -9223372037ll || (secs == -9223372037ll && frac < 145224192)) return kRange;
    }
    // below zero (secs + 1) * U >= -9223372036 * 10^9 fits, and frac - U brings it to -2^63 at the least
    const int64_t v = secs >= 0 ? secs * U + frac : (secs + 1) * U + (frac - U);
    bits = (uint64_t)v;
    return kCast;
}
// the value in r at [b, b + n), r reading blanks from b + n on
template <class R>
MSJ_HD uint32_t parse_timestamp(const R &r, uint64_t b, uint64_t n, uint32_t unit, uint64_t &bits) {
    bits = 0;
    if (n < kMinTimestampBytes || n > kMaxTimestampBytes) return kSyntax;
    uint32_t yh, yl, mo, dd, hh = 0, mi = 0, ss = 0, frac = 0;
    if (!two_digits(r, b, yh) || !two_digits(r, b + 2, yl) || r.at(b + 4) != '-' || !two_digits(r, b + 5, mo) || r.at(b + 7) != '-' ||
        !two_digits(r, b + 8, dd))
        return kSyntax;
    const uint32_t year = yh * 100 + yl;
    if (mo - 1 >= 12u || dd - 1 >= days_in_month(year, mo)) return kSyntax;
    int64_t offset = 0;
    uint64_t p = b + 10;
    const uint64_t e = b + n;
    if (p < e) {
        const uint32_t sep = r.at(p);
        if (sep != 'T' && sep != 't' && sep != ' ') return kSyntax;
        if (!two_digits(r, p + 1, hh) || r.at(p + 3) != ':' || !two_digits(r, p + 4, mi) || hh > 23 || mi > 59) return kSyntax;
        p += 6;
        if (r.at(p) == ':') {
            if (!two_digits(r, p + 1, ss) || ss > 59) return kSyntax;  // (a leap second 60 is no member)
            p += 3;
            const uint32_t mark = r.at(p);
            if (mark == '.' || mark == ',') {
                uint32_t digits = 0, scale = 100000000;
                p++;
                for (uint32_t d; digits < 9 && (d = r.at(p) - '0') < 10u; digits++, p++) frac += d * scale, scale /= 10;
                if (digits == 0) return kSyntax;  // (a tenth digit is no offset: refused below)
            }
        }
        const uint32_t z = r.at(p);
        if (z == 'Z' || z == 'z') {
            p++;
        } else if (z == '+' || z == '-') {
            uint32_t oh, om = 0;
            if (!two_digits(r, p + 1, oh) || oh > 23) return kSyntax;
            p += 3;
            if (r.at(p) == ':') {
                if (!two_digits(r, p + 1, om)) return kSyntax;
                p += 3;
            } else if (r.at(p) - '0' < 10u) {
                if (!two_digits(r, p, om)) return kSyntax;
                p += 2;
            }
            if (om > 59) return kSyntax;
            offset = (int64_t)(oh * 3600 + om * 60);
            if (z == '-') offset = -offset;
        }
        if (p != e) return kSyntax;
    }
    const int64_t secs = days_from_civil(year, mo, dd) * 86400 + (int64_t)(hh * 3600 + mi * 60 + ss) - offset;
    return scale_seconds(secs, unit, frac, bits);
}

// ---- the number -----------------------------------------------------------------------------------------------------------------
// the value in r at [b, b + n), whole, as msj_number_values_device gives it for the same text as a token.  kExact = false
// stops in front of the exact path (number_math.h: Big, 736 bytes of a lane's own memory) with kPending
template <bool kExact, class R>
MSJ_HD uint32_t parse_number(const R &r, uint64_t b, uint64_t n, uint64_t &bits, uint32_t &type) {
    bits = 0, type = 'l';
    if (n == 0 || n > kMaxNumberBytes) return kSyntax;
    const NumberRuns<R> runs{r, b + n};
    const msj::num::Scan sc = msj::num::scan_number(runs, b);
    msj::num::Result res = msj::num::convert_fast(runs, sc);
    if (res.kind == msj::num::kPending) {
        if (!kExact) return kPending;
        res = msj::num::convert_exact(runs, sc, res);
    }
    if (res.kind == msj::num::kErrSyntax) return kSyntax;
    if (res.kind == msj::num::kErrRange) return kRange;
    bits = res.bits, type = res.kind == msj::num::kDouble ? 'd' : 'l';
    return kCast;
}

// ---- one record ---------------------------------------------------------------------------------------------------------------
template <class Field>
MSJ_HD Field value_field(const Field &f, uint32_t type, uint64_t bits) {
    Field out;
    out.bits = bits, out.token = f.token, out.type = (uint8_t)type, out.flags = 0, out.code = 0;
    return out;
}
// what a string row became: the value's record, or the record of a value that is none
template <class Field>
MSJ_HD Field string_result(const Field &f, uint32_t outcome, uint32_t type, uint64_t bits) {
    return outcome == kCast ? value_field(f, type, bits) : msj::sel::error_field<Field>(kNumberError);
}
// The part that reads no byte of the window.  -> true: `out` and `outcome` are the record's; false: the record is a string
// row, y its body
template <class Field>
MSJ_HD bool cast_without_bytes(const Field &f, uint64_t len, uint32_t flags, msj::scol::Row &y, Field &out, uint32_t &outcome) {
    y = msj::scol::row_of(f, len);
    if (y.valid) return false;
    if (f.code != 0) {
        out = f, outcome = kPassed;
    } else if ((flags & kKeepNumbers) && (f.type == 'l' || f.type == 'd')) {
        out = f, outcome = kCast;
    } else {
        out = msj::sel::error_field<Field>(kIncorrectType), outcome = kOther;
    }
    return true;
}
// a string row whose body holds no escape; r: the window's bytes, or any reader that agrees with them on [y.b, y.b + y.r)
template <bool kExact, class Field, class R>
MSJ_HD uint32_t cast_plain(const Field &f, const msj::scol::Row &y, const R &r, uint32_t kind, uint32_t unit, Field &out) {
    uint64_t bits = 0;
    uint32_t type = 'l', outcome = kSyntax;
    if (y.r <= max_value_bytes(kind)) {
        const ValueReader<R> v{r, y.b + y.r};
        outcome = kind == kTimestamp ? parse_timestamp(v, y.b, y.r, unit, bits) : parse_number<kExact>(v, y.b, y.r, bits, type);
    }
    out = string_result(f, outcome, type, bits);
    return outcome;
}
// a string row with MSJ_SPAN_ESCAPED: its bytes by tape_math.h's unescape into a lane's own memory, then the same grammar.
// kRoom: the bytes of that memory, the kind's most at least (a kernel that knows its kind keeps a timestamp's in registers)
template <uint32_t kRoom, class Field, class R>
MSJ_HD uint32_t cast_escaped(const Field &f, const msj::scol::Row &y, const R &r, uint32_t kind, uint32_t unit, Field &out) {
    uint64_t bits = 0;
    uint32_t type = 'l', outcome = kSyntax;
    if (y.r <= max_raw_bytes(kind)) {
        uint8_t value[kRoom];
        const uint32_t cap = max_value_bytes(kind) < kRoom ? max_value_bytes(kind) : kRoom;
        const uint64_t n = msj::scol::unescape_serial(r, BoundedWriter{value, cap}, y.b, y.b + y.r);
        if (n <= cap) {
            const msj::val::ByteReader v{value, n};
            outcome = kind == kTimestamp ? parse_timestamp(v, 0, n, unit, bits) : parse_number<true>(v, 0, n, bits, type);
        }
    }
    out = string_result(f, outcome, type, bits);
    return outcome;
}
// one record in, one record and its outcome out; r: the window's bytes (r.len their number)
template <uint32_t kRoom, class Field, class R>
MSJ_HD uint32_t cast_record(const Field &f, const R &r, uint32_t kind, uint32_t unit, uint32_t flags, Field &out) {
    msj::scol::Row y;
    uint32_t outcome;
    if (cast_without_bytes(f, r.len, flags, y, out, outcome)) return outcome;
    return y.escaped ? cast_escaped<kRoom>(f, y, r, kind, unit, out) : cast_plain<true>(f, y, r, kind, unit, out);
}
template <class Field, class R>
MSJ_HD uint32_t cast_record(const Field &f, const R &r, uint32_t kind, uint32_t unit, uint32_t flags, Field &out) {
    return cast_record<kMaxNumberBytes>(f, r, kind, unit, flags, out);
}

}  // namespace cast
}  // namespace msj
