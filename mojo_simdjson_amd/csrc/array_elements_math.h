// array_elements_math.h -- the arithmetic of msj_array_elements_device (array_elements_kernel.hip) that is not already
// array_column_math.h's or select_elements_math.h's: the call's verdict on its rows, which rows are live, how many of them
// need a state of their own, the row test with the window's n in the place of a document's end, the word a row keeps for the
// last pass, and the offset of a row from the dense rows' offsets.  Host + device like its siblings, so that
// tests/test_array_elements_math.py runs the same code on the CPU (g++, tests/array_elements_math_host.cpp).
//
// Definition (include/msj_stage1.h): msj_array_column_device with ANY ascending msj_field records as
// the rows -- the elements of a list column (a list of lists) or one path of msj_select_elements_device (a list inside a
// list of structs).  Such a column holds records with a code, whose token is 0xFFFFFFFF: the rows with code 0, the LIVE rows,
// must ascend strictly -- checked, not believed -- and a token belongs to the last live row below it, which is
// select_elements_math.h's rows_below over the live rows alone.  The candidate test, the element test, the descriptor and the
// code behind the layout are array_column_math.h's, the record select_math.h's value_field: nothing of them is restated.
#pragma once
#include <stdint.h>

#include "array_column_math.h"
#include "select_elements_math.h"

namespace msj {
namespace aelem {

using msj::acol::Desc;
using msj::acol::elements_code;
using msj::acol::is_candidate;
using msj::acol::is_element_of;
using msj::acol::kBadArgument;
using msj::acol::kCapacity;
using msj::acol::kFieldNoBits;
using msj::acol::value_field;
using msj::selem::in_order;
using msj::selem::rows_below;

// ---- the call's verdict on its rows -----------------------------------------------------------------------------------------
// Behind d_rows_select: the code in front of the rows, 0 when they are looked at.  stop (code != 0): nothing but the results
// is written.  n_rows: what the result reports then -- a zero result behind a code of d_rows_select
MSJ_HD int32_t head_code(int32_t rows_code, uint64_t rows, uint64_t capacity, uint64_t &n_rows) {
    n_rows = 0;
    if (rows_code != 0) return rows_code;
    n_rows = rows;
    return rows > capacity ? kCapacity : 0;
}

// ---- live rows ----------------------------------------------------------------------------------------------------------------
// a row whose record has no code: only these name a token, only these are ordered
MSJ_HD bool is_live(uint32_t rec_code) { return rec_code == 0; }
// the live rows that can own a token: live tokens ascend strictly, so live row j's token is at least j, and one at or
// past n names no token of the window (0 for a window without a token: no row is valid then)
MSJ_HD uint64_t dense_rows(uint64_t n, uint64_t capacity) { return n < capacity ? n : capacity; }

// One record against the arrays: array_column_math.h's row test with [0, n) as the document.  Every clause is checked on the
// arrays: code 0, type '[', v < n, d_type[v] == '[', the partner in (v, n).  other: the record is live and the row is no array
template <class Field>
MSJ_HD Desc row_of(const Field &r, uint64_t n, const uint8_t *type, const int32_t *depth, const uint32_t *match, bool &other) {
    return msj::acol::row_of(r, true, 0, n, type, depth, match, other);
}

// ---- what a row keeps for the last pass ---------------------------------------------------------------------------------------
// The number of live rows in front of row r -- the dense number of r itself when it is live, of the next live row when it is
// not -- and whether r is live.  31 bits are enough: a dense number that matters is below dense_rows() < 2^31
constexpr uint32_t kRankLive = 0x80000000u, kRankMask = 0x7FFFFFFFu;
MSJ_HD uint32_t rank_word(uint64_t live_in_front, bool live) {
    return (uint32_t)(live_in_front < kRankMask ? live_in_front : kRankMask) | (live ? kRankLive : 0u);
}
// d_offsets[r] from row r's word: the offset the dense row left -- the element tokens up to and including its own token, all of
// them elements of rows in front of it -- or n_elements when no live row follows or that row's token names no token: the
// live rows behind it do not either.  dense: the dense rows that exist, min(live rows, dense_rows())
MSJ_HD uint64_t offset_of_row(uint32_t word, uint64_t dense, const uint32_t *start, const uint64_t *dense_offset, uint64_t n, uint64_t n_elements) {
    const uint64_t j = word & kRankMask;
    return j < dense && (uint64_t)start[j] < n ? dense_offset[j] : n_elements;
}
// d_valid[r]: a live row whose descriptor says so
MSJ_HD uint32_t valid_of_row(uint32_t word, uint64_t dense, const Desc *desc) {
    const uint64_t j = word & kRankMask;
    return (word & kRankLive) && j < dense ? desc[j].valid : 0u;
}

}  // namespace aelem
}  // namespace msj
