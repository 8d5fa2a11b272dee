// raw_column_math.h -- the arithmetic of msj_raw_column_device (raw_column_kernel.hip): where a token's text ends, the row
// test on one msj_field, a row's length in the verbatim and in the compact form, and the two searches the copy is organised
// by -- from an output byte to its row (string_column_math.h's row_of_byte) and, in the compact form, from a byte of a row
// to its token.  Host + device like its siblings, so that tests/test_raw_column_math.py runs the same code on the CPU (g++,
// tests/raw_column_math_host.cpp).
//
// Definition (include/msj_stage1.h): a selected value's JSON text as a column -- offsets[R + 1], the
// bytes back to back, a validity byte per row.  Verbatim: the window's bytes from the value's first byte to the end of its
// last token.  Compact: the texts of its tokens back to back, the blanks between them dropped; the length is a difference
// of one exclusive sum P over the window's token texts.
#pragma once
#include <stdint.h>

#include "string_column_math.h"

namespace msj {
namespace rcol {

using msj::scol::bytes_code;
using msj::scol::row_of_byte;
using msj::scol::rows_over;

constexpr uint32_t kSpanString = 1u, kSpanNumber = 4u, kSpanLong = 128u;  // MSJ_SPAN_STRING / _NUMBER / _LONG
constexpr uint32_t kCompact = 1u;                                         // MSJ_RAW_COMPACT

// what the call reads of a window (d_match is not among it: a container's closing token is its record's `bits`)
struct Tokens {
    const uint8_t *buf;
    uint64_t len;
    const uint32_t *idx;
    uint64_t n;
    const uint8_t *type;
    const uint32_t *end;
    const uint8_t *flags;
};

MSJ_HD bool is_blank(uint32_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

// ---- token text -----------------------------------------------------------------------------------------------------------
// lim(i): where token i's text has to end at the latest -- the next token's start, the window's end behind the last token,
// and never past len whatever d_idx holds.  i < n
MSJ_HD uint64_t lim(const Tokens &t, uint64_t i) {
    const uint64_t l = i + 1 < t.n ? (uint64_t)t.idx[i + 1] : t.len;
    return l < t.len ? l : t.len;
}
// te(i), clipped to lim(i).  A LONG number has no d_end: its text runs to the blanks in front of lim(i)
MSJ_HD uint64_t text_end(const Tokens &t, uint64_t i) {
    const uint64_t s = t.idx[i], l = lim(t, i);
    const uint32_t f = t.flags[i];
    uint64_t e;
    if (f & kSpanString) {
        e = (uint64_t)t.end[i] + 1;
    } else if (f & kSpanNumber) {
        if (f & kSpanLong) {
            e = l;
            while (e > s && is_blank(t.buf[e - 1])) e--;  // (s < e <= len: inside the window)
        } else {
            e = t.end[i];
        }
    } else {
        const uint32_t c = t.type[i];
        e = s + ((c == 't' || c == 'n') ? 4u : c == 'f' ? 5u : 1u);
    }
    return e < l ? e : l;
}
// tl(i): token i's text is [idx[i], idx[i] + tl(i)), inside [0, len) and in front of lim(i) on any arrays
MSJ_HD uint64_t text_len(const Tokens &t, uint64_t i) {
    const uint64_t s = t.idx[i], e = text_end(t, i);
    return e > s ? e - s : 0;
}

// ---- the row test ---------------------------------------------------------------------------------------------------------
// One record against the window's token count.  valid: the row is a value, its tokens are token .. last (a container's last
// is its record's bits, every other value's is the token itself).  other: the record has code 0 and fails the test (a token
// at or past n, a container whose closing token is not in (token, n)); it is never dereferenced.  Neither: the record has a
// code.
struct Row {
    uint32_t token, last;
    bool valid, container, other;
};
template <class Field>
MSJ_HD Row row_of(const Field &f, uint64_t n) {
    Row y;
    const bool box = f.type == '{' || f.type == '[';
    y.token = f.token, y.last = f.token;
    y.valid = f.code == 0 && (uint64_t)f.token < n;
    if (y.valid && box) {
        y.valid = f.bits > (uint64_t)f.token && f.bits < n;
        y.last = (uint32_t)f.bits;  // (< n < 2^31 when valid)
    }
    y.container = y.valid && box;
    y.other = f.code == 0 && !y.valid;
    if (!y.valid) y.token = y.last = 0;
    return y;
}

// ---- a row's bytes --------------------------------------------------------------------------------------------------------
// Verbatim: [idx[token], te(last)); nothing when the arrays put the end in front of the start
MSJ_HD uint64_t verbatim_len(const Tokens &t, const Row &y) {
    if (!y.valid) return 0;
    const uint64_t s = t.idx[y.token], e = text_end(t, y.last);
    return e > s ? e - s : 0;
}
// Compact: P(i) = the sum of tl over the tokens in front of i, for i in [0, n]
template <class PSum>
MSJ_HD uint64_t compact_len(const PSum &P, const Row &y) {
    return y.valid ? P((uint64_t)y.last + 1) - P(y.token) : 0;
}
// byte q of the concatenated token texts, P(token) <= q < P(last + 1): the LAST token i in [token, last] with P(i) <= q.
// Tokens without text in front of it have the same sum and own nothing
template <class PSum>
MSJ_HD uint64_t token_of_byte(const PSum &P, uint64_t token, uint64_t last, uint64_t q) {
    uint64_t lo = token, hi = last + 1;  // the answer is in [lo, hi)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (P(mid) <= q) lo = mid;
        else hi = mid;
    }
    return lo;
}
// the window offset of byte o of a row: src = idx[token] (verbatim), src = P(token) (compact)
MSJ_HD uint64_t verbatim_source(uint64_t src, uint64_t o) { return src + o; }
template <class PSum>
MSJ_HD uint64_t compact_source(const Tokens &t, const PSum &P, const Row &y, uint64_t src, uint64_t o) {
    const uint64_t q = src + o, i = token_of_byte(P, y.token, y.last, q);
    return (uint64_t)t.idx[i] + (q - P(i));  // (q < P(i + 1): inside token i's text)
}

}  // namespace rcol
}  // namespace msj
