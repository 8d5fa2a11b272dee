// filter_rows_math.h -- the arithmetic of msj_predicates_create, msj_filter_rows_device and msj_take_rows_device
// (filter_rows_kernel.hip): the compiled form of the predicates, the exact compare of an int64 with a binary64, the string
// compares (equality through select_math.h's key compare, the prefix through tape_math.h's unescape ended early), one
// predicate on one record, a row's verdict, the gather that re-bases list offsets and the record of an index out of range.
// Host + device like its siblings, so that tests/test_filter_rows_math.py runs the same code on the CPU (g++,
// tests/filter_rows_math_host.cpp).
//
// Definition (include/msj_stage1.h): a predicate looks at ONE record and holds or does not; NOT
// inverts that, also for a record without a value (two-valued, not SQL's three); a row is kept when all (ANY: any) of its
// predicates hold.  A string row's value is by definition what msj_string_column_device writes for the record, so the row
// test is string_column_math.h's and the bytes are tape_math.h's unescape: nothing of either is restated here.
#pragma once
#include <stdint.h>

#include "select_math.h"
#include "string_column_math.h"
#include "validate_math.h"

namespace msj {
namespace frows {

using msj::scol::kMaxRows;
using msj::sel::kFieldNoBits;
using msj::sel::kNoSuchField;

constexpr uint32_t kMaxPredicates = 16, kMaxColumns = 16, kMaxOperandBytes = 255;
// msj_predicate.op (MSJ_PRED_*)
constexpr uint32_t kFound = 0, kType = 1, kNumEq = 2, kNumLt = 3, kNumLe = 4, kNumGt = 5, kNumGe = 6, kStrEq = 7, kStrPrefix = 8, kOps = 9;
constexpr uint32_t kNot = 1u, kOperandDouble = 2u;  // msj_predicate.flags: MSJ_PRED_NOT, MSJ_PRED_DOUBLE
constexpr uint32_t kAny = 1u;                       // MSJ_PREDICATES_ANY
// what one predicate says of one record
constexpr uint32_t kHolds = 1u, kMetCode = 2u, kMetNoBits = 4u;

// ---- the predicates, compiled (what msj_predicates keeps in device memory; the same bytes on the host) ----------------------
struct Pred {
    uint8_t column, op, flags, reserved;
    uint32_t n;     // bytes of a string operand
    uint64_t bits;  // a numeric operand (int64, or the binary64 pattern with kOperandDouble); TYPE: the mask
};
struct Predicates {
    uint32_t n, flags, max_column, reserved;
    Pred p[kMaxPredicates];
    uint8_t bytes[kMaxPredicates][256];
};

// the bit of a tape tag in TYPE's mask, in the order { [ " l d t f n; 0 for any other byte
MSJ_HD uint32_t tag_bit(uint32_t type) {
    switch (type) {
        case '{': return 1u;
        case '[': return 2u;
        case '"': return 4u;
        case 'l': return 8u;
        case 'd': return 16u;
        case 't': return 32u;
        case 'f': return 64u;
        case 'n': return 128u;
        default: return 0;
    }
}
MSJ_HD double double_of(uint64_t bits) {
    double d;
    __builtin_memcpy(&d, &bits, 8);
    return d;
}
MSJ_HD bool is_finite_bits(uint64_t bits) { return ((bits >> 52) & 0x7FFu) != 0x7FFu; }

// msj_predicates_create's host part.  Spec: msj_predicate.  -> 0, or -1 (NULL, a count outside 1..16, a column above 15, an
// unknown op or flag, an operand over 255 bytes or without its pointer, a TYPE mask of 0 or over 8 bits, a double operand that
// is not finite)
template <class Spec>
static inline int compile_predicates(const Spec *specs, uint32_t n, uint32_t flags, Predicates &out) {
    if (!specs || n == 0 || n > kMaxPredicates || (flags & ~kAny) != 0) return -1;
    out = Predicates{};
    out.n = n, out.flags = flags;
    for (uint32_t i = 0; i < n; i++) {
        const Spec &s = specs[i];
        if (s.column >= kMaxColumns || s.op >= kOps) return -1;
        const bool numeric = s.op >= kNumEq && s.op <= kNumGe, text = s.op == kStrEq || s.op == kStrPrefix;
        if ((s.flags & ~(kNot | (numeric ? kOperandDouble : 0u))) != 0) return -1;
        if (text && (s.operand_len > kMaxOperandBytes || (s.operand_len > 0 && !s.operand_bytes))) return -1;
        if (s.op == kType && (s.operand_bits == 0 || s.operand_bits > 0xFFu)) return -1;
        if (numeric && (s.flags & kOperandDouble) && !is_finite_bits(s.operand_bits)) return -1;
        Pred &p = out.p[i];
        p.column = (uint8_t)s.column, p.op = (uint8_t)s.op, p.flags = (uint8_t)s.flags;
        p.n = text ? s.operand_len : 0;
        p.bits = numeric || s.op == kType ? s.operand_bits : 0;
        for (uint32_t x = 0; x < p.n; x++) out.bytes[i][x] = s.operand_bytes[x];
        if (s.column > out.max_column) out.max_column = s.column;
    }
    return 0;
}

// ---- numbers: as real numbers, exactly ---------------------------------------------------------------------------------------
// i against d: -1 below, 0 equal, 1 above; 2 when d is a NaN (no record of a number call holds one; any array may).
// d >= 2^63 or d < -2^63: the sign decides (-2^63 itself is an int64).  Else trunc(d) is an int64 and d - trunc(d) is exact:
// the integers decide, and on equality the fraction against 0.  Neither side is ever cast to the other's type
MSJ_HD int cmp_int_double(int64_t i, double d) {
    if (d != d) return 2;
    if (d >= 9223372036854775808.0) return -1;
    if (d < -9223372036854775808.0) return 1;
    const double t = __builtin_trunc(d);
    const int64_t ti = (int64_t)t;
    if (i != ti) return i < ti ? -1 : 1;
    const double frac = d - t;
    return frac > 0 ? -1 : frac < 0 ? 1 : 0;
}
// the value of a number record (type 'l' or 'd', its bits) against the operand
MSJ_HD int cmp_number(uint32_t type, uint64_t bits, bool operand_double, uint64_t operand) {
    if (type == 'l' && !operand_double) {
        const int64_t a = (int64_t)bits, b = (int64_t)operand;
        return a < b ? -1 : a > b ? 1 : 0;
    }
    if (type == 'l') return cmp_int_double((int64_t)bits, double_of(operand));
    const double a = double_of(bits);
    if (!operand_double) {
        const int c = cmp_int_double((int64_t)operand, a);
        return c == 2 ? 2 : -c;
    }
    const double b = double_of(operand);
    return a < b ? -1 : a > b ? 1 : a == b ? 0 : 2;
}
MSJ_HD bool order_holds(uint32_t op, int c) {
    switch (op) {
        case kNumEq: return c == 0;
        case kNumLt: return c == -1;
        case kNumLe: return c == -1 || c == 0;
        case kNumGt: return c == 1;
        default: return c == 0 || c == 1;  // kNumGe
    }
}

// ---- strings -----------------------------------------------------------------------------------------------------------------
// tape_math.h's writer that compares the first n bytes and lets the rest pass (an escape's bytes may straddle n)
struct PrefixWriter {
    const uint8_t *seg;
    uint32_t n;
    bool *ok;
    MSJ_HM void put(uint64_t o, uint32_t byte) const {
        if (o < n && seg[o] != byte) *ok = false;
    }
};
// the value with the raw body [b, q) starts with the n bytes of seg; r: the window's bytes.  Escaped: unescape_serial's walk,
// left once n bytes are out or one differs -- at most 6 raw bytes per byte of the operand
template <class R>
MSJ_HD bool starts_with(const R &r, uint64_t b, uint64_t q, bool escaped, const uint8_t *seg, uint32_t n) {
    if (q < b || q > r.len || q - b < n) return false;  // (a byte of the value takes at least one raw byte)
    if (!escaped) {
        for (uint32_t x = 0; x < n; x++)
            if (r.at(b + x) != seg[x]) return false;
        return true;
    }
    bool ok = true, after_high = false;
    const PrefixWriter w{seg, n, &ok};
    uint64_t o = 0, p = b;
    while (p < q && o < n && ok) {
        const uint32_t c = r.at(p);
        if (c != '\\') {
            w.put(o++, c);
            p++;
            after_high = false;
            continue;
        }
        uint32_t len;
        o += msj::tape::escape_out(r, w, b, q, p, after_high, o, len);
        p += len;
        after_high = len == 6;
    }
    return ok && o >= n;
}

// ---- one predicate on one record ---------------------------------------------------------------------------------------------
// -> kHolds (NOT applied) | kMetCode (the record has a code) | kMetNoBits (a numeric op met a number without bits)
template <class Field, class R>
MSJ_HD uint32_t eval_pred(const Pred &p, const uint8_t *operand, const Field &f, const R &r) {
    bool holds = false;
    uint32_t met = f.code != 0 ? kMetCode : 0;
    const bool number = f.code == 0 && (f.type == 'l' || f.type == 'd');
    if (p.op == kFound) {
        holds = f.code == 0;
    } else if (p.op == kType) {
        holds = f.code == 0 && (tag_bit(f.type) & (uint32_t)p.bits) != 0;
    } else if (p.op <= kNumGe) {
        if (number && (f.flags & kFieldNoBits)) met |= kMetNoBits;
        else if (number) holds = order_holds(p.op, cmp_number(f.type, f.bits, (p.flags & kOperandDouble) != 0, p.bits));
    } else {
        const msj::scol::Row y = msj::scol::row_of(f, r.len);
        if (y.valid && p.op == kStrEq) holds = msj::sel::key_equals(r, y.b, y.b + y.r, y.escaped, operand, p.n);
        else if (y.valid) holds = starts_with(r, y.b, y.b + y.r, y.escaped, operand, p.n);
    }
    if (p.flags & kNot) holds = !holds;
    return (holds ? kHolds : 0u) | met;
}
// a row over all its predicates: `all` the AND of kHolds, `any` the OR, `met` the OR of the other bits
struct RowVerdict {
    bool all, any;
    uint32_t met;
};
MSJ_HD RowVerdict verdict_begin() { return RowVerdict{true, false, 0}; }
MSJ_HD void verdict_add(RowVerdict &v, uint32_t e) {
    v.all = v.all && (e & kHolds), v.any = v.any || (e & kHolds), v.met |= e & ~kHolds;
}
MSJ_HD bool row_kept(const RowVerdict &v, uint32_t flags) { return (flags & kAny) ? v.any : v.all; }

// ---- the calls' verdicts on themselves ---------------------------------------------------------------------------------------
MSJ_HD bool rows_over(uint64_t R, uint64_t capacity) { return R > capacity || R >= kMaxRows; }
// list offsets: the kept rows in front of row min(o, R) -- rank[k] the kept rows in front of row k, k < R
MSJ_HD uint64_t rebased_offset(uint64_t o, uint64_t R, const uint32_t *rank, uint64_t n_kept) { return o >= R ? n_kept : rank[o]; }
// take: K indices into R rows of `stride` records each, room for out_capacity
MSJ_HD bool take_over(uint64_t K, uint64_t out_capacity, uint64_t R, uint64_t stride) { return rows_over(K, out_capacity) || rows_over(R, stride); }
// the record of an index at or past R: a missing value
template <class Field>
MSJ_HD Field missing_field() { return msj::sel::error_field<Field>(kNoSuchField); }

}  // namespace frows
}  // namespace msj
