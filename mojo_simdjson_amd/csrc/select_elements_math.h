// select_elements_math.h -- the arithmetic of msj_select_elements_device (select_elements_kernel.hip) that is not already
// select_math.h's: the call's verdict on its rows, the order test, the state a (path, row) starts from, the row a key token
// belongs to, and the member test without a global depth.  Host + device like its siblings, so that
// tests/test_select_elements_math.py runs the same code on the CPU (g++, tests/select_elements_math_host.cpp).
//
// Definition (include/msj_stage1.h): msj_select_documents_device's lookup with ELEMENTS as the rows.
// A row is one msj_field of an array column: its object starts at the record's token and ends at that token's partner, and
// the window's n stands where a document's end e_k stood.  Rows sit at whatever depth their array does, so a key is tested
// against the depth of the object it is looked up in (d_depth[lo] + 1), not against the level.  The rows' tokens ascend
// strictly -- checked, not believed -- so "the row of key i" is one search: the last row whose token lies below i.  The
// state words, the key compare, the unescape, the number search and the record are select_math.h's, unchanged.
#pragma once
#include <stdint.h>

#include "select_math.h"

namespace msj {
namespace selem {

using namespace msj::sel;

constexpr int32_t kCapacity = 1;      // MSJ_CAPACITY
constexpr int32_t kBadArgument = -1;  // MSJ_ERR_BAD_ARGUMENT

// ---- the call's verdict on its rows -----------------------------------------------------------------------------------------
// Behind d_rows_select: the code in front of the rows, 0 when they are looked at.  stop (code != 0): no record is written.
// n_rows / n_paths_out: what the result reports then -- a zero result behind a code of d_rows_select
MSJ_HD int32_t head_code(int32_t rows_code, uint64_t rows, uint64_t capacity, uint32_t n_paths, uint64_t &n_rows, uint64_t &n_paths_out) {
    n_rows = n_paths_out = 0;
    if (rows_code != 0) return rows_code;
    n_rows = rows, n_paths_out = n_paths;
    return rows > capacity ? kCapacity : 0;
}
// the rows that can have a state of their own: tokens ascend strictly, so row r's token is at least r, and a row at or
// past n names no token of the window
MSJ_HD uint64_t state_rows(uint64_t n, uint64_t capacity) {
    const uint64_t d = n < capacity ? n : capacity;
    return d ? d : 1;
}
// row r (token t) against its predecessor (token t_prev; r > 0): compared as uint32
MSJ_HD bool in_order(uint32_t t_prev, uint32_t t) { return t_prev < t; }

// ---- where a (path, row) starts -----------------------------------------------------------------------------------------------
// The record's code, copied; with no segment the row's own value, re-derived (v < n); else the row's object, or
// INCORRECT_TYPE for a row that is not usable: every clause re-checked on the arrays
MSJ_HD uint32_t row_state(uint32_t rec_code, uint32_t rec_type, uint32_t v, uint32_t levels, uint64_t n, const uint8_t *type,
                          const uint32_t *match) {
    if (rec_code != 0) return state_code(rec_code);
    if ((uint64_t)v >= n) return state_code(kIncorrectType);
    if (levels == 0) return v;
    if (rec_type != '{') return state_code(kIncorrectType);
    return container_state(type[v], match[v], v, n);
}

// ---- rows and keys ----------------------------------------------------------------------------------------------------------
// how many of the ascending start[0 .. count) lie below x: the row of key token i is rows_below(i) - 1, none when that is 0
MSJ_HD uint32_t rows_below(const uint32_t *start, uint32_t count, uint32_t x) {
    uint32_t lo = 0, hi = count;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (start[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// token (type t, the token behind it of type t_next) can be a key of SOME object
MSJ_HD bool is_key(uint32_t t, uint32_t t_next) { return t == '"' && t_next == ':'; }
// key i at depth d_i is a direct member of the object `lo` (depth d_lo, partner m)
MSJ_HD bool is_direct_member(uint64_t i, int32_t d_i, uint32_t lo, int32_t d_lo, uint32_t m) {
    return is_member_of(i, lo, m) && d_i == (int32_t)((uint32_t)d_lo + 1u);  // (no signed overflow on any depth)
}

}  // namespace selem
}  // namespace msj
