// string_column_math.h -- the arithmetic of msj_string_column_device (string_column_kernel.hip): the row test on one
// msj_field of a selected path, a row's unescaped length, the rule for the result's code, and the mapping from an output
// byte back to its row that the copy is organised by.  Host + device like its siblings, so that
// tests/test_string_column_math.py runs the same code on the CPU (g++, tests/string_column_math_host.cpp).
//
// Definition (include/msj_stage1.h): the column's string values in the standard variable-length
// layout -- offsets[D + 1], the unescaped bytes back to back, a validity byte per row.  The bytes of an escaped value are
// what tape_math.h's unescape gives for its body: nothing of that is restated here.
#pragma once
#include <stdint.h>

#include "tape_math.h"

namespace msj {
namespace scol {

using msj::tape::kSpanEscaped;
using msj::tape::NoWrite;
using msj::tape::unescape_serial;

constexpr uint64_t kMaxRows = 1ull << 31;  // a window has fewer tokens than this, so fewer documents
constexpr int32_t kCapacity = 1;           // MSJ_CAPACITY

// ---- the row test ---------------------------------------------------------------------------------------------------------
// One record of the column against the window's length.  valid: the row is a string, [b, b + r) is its raw body inside the
// window.  other: the record has code 0 and is no string -- a number, a container, an atom, or a '"' record whose span does
// not lie inside the window (no call writes one; it is never dereferenced).  Neither: the record has a code.
struct Row {
    uint64_t b, r;
    bool valid, escaped, other;
};
template <class Field>
MSJ_HD Row row_of(const Field &f, uint64_t len) {
    Row y;
    y.b = f.bits & 0xFFFFFFFFull, y.r = f.bits >> 32;
    y.valid = f.code == 0 && f.type == '"' && y.b + y.r <= len;  // (b + r < 2^33: no overflow)
    y.escaped = y.valid && (f.flags & kSpanEscaped) != 0;
    y.other = f.code == 0 && !y.valid;
    if (!y.valid) y.b = y.r = 0;
    return y;
}
// a body of more than `lane_body` raw bytes that has to be unescaped is walked by a wave, not by its lane
MSJ_HD bool is_long(const Row &y, uint32_t lane_body) { return y.escaped && y.r > lane_body; }

// the row's length in the output; r: the window's bytes
template <class R>
MSJ_HD uint64_t ulen(const R &r, const Row &y) {
    if (!y.valid) return 0;
    return y.escaped ? unescape_serial(r, NoWrite{}, y.b, y.b + y.r) : y.r;
}

// ---- the call's verdict on itself -----------------------------------------------------------------------------------------
// D: d_select->n_documents.  over: nothing but the result is written
MSJ_HD bool rows_over(uint64_t D, uint64_t capacity) { return D > capacity || D >= kMaxRows; }
// the code behind the layout: the bytes were clipped (the layout-only form asks for no byte, so nothing is clipped in it)
MSJ_HD int32_t bytes_code(uint64_t total_bytes, bool have_bytes, uint64_t bytes_capacity) {
    return have_bytes && total_bytes > bytes_capacity ? kCapacity : 0;
}

// ---- output byte -> row ---------------------------------------------------------------------------------------------------
// off[0 .. n] ascending, off[n] the end of the range: the row that owns output byte pos, off[0] <= pos < off[n] -- the LAST
// row whose offset is <= pos.  Empty rows (off[k] == off[k + 1]) in front of it have the same offset and own nothing.
template <class Off>
MSJ_HD uint32_t row_of_byte(const Off *off, uint32_t n, uint64_t pos) {
    uint32_t lo = 0, hi = n;  // the answer is in [lo, hi)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)off[mid] <= pos) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace scol
}  // namespace msj
