// object_entries_math.h -- the arithmetic of msj_object_entries_device (object_entries_kernel.hip) that is not already
// array_elements_math.h's, array_column_math.h's or select_math.h's: the row test with '{' in the place of '[', the
// candidate test that looks one token BEHIND itself, the entry test and the code behind the layout.  Host + device like its
// siblings, so that tests/test_object_entries_math.py runs the same code on the CPU (g++, tests/object_entries_math_host.cpp).
//
// Definition (include/msj_stage1.h): an object's members as a map column -- msj_array_elements_device
// with objects as the rows and two records per entry.  The members of an object v are the string tokens followed by ':' one
// level below it between v and its partner m (select_math.h's member test), the value of member i is token i + 2, and i + 2
// must lie in front of m.  The verdict on the rows, the live rows, the order test, the row search, the word a row keeps and
// a row's offset are array_elements_math.h's; the records are select_math.h's value_field: nothing of them is restated.
#pragma once
#include <stdint.h>

#include "array_elements_math.h"

namespace msj {
namespace oent {

using msj::acol::Desc;
using msj::acol::kBadArgument;
using msj::acol::kCapacity;
using msj::acol::kFieldNoBits;
using msj::acol::value_field;
using msj::aelem::dense_rows;
using msj::aelem::head_code;
using msj::aelem::is_live;
using msj::aelem::offset_of_row;
using msj::aelem::rank_word;
using msj::aelem::valid_of_row;
using msj::selem::in_order;
using msj::selem::rows_below;

constexpr uint32_t kContainer = '{';

// One record against the arrays, [0, n) as the document: code 0, type '{', v < n, d_type[v] == '{', the partner in (v, n).
// other: the record is live and the row is no object
template <class Field>
MSJ_HD Desc row_of(const Field &r, uint64_t n, const uint8_t *type, const int32_t *depth, const uint32_t *match, bool &other) {
    return msj::acol::row_of_kind(r, kContainer, true, 0, n, type, depth, match, other);
}

// token (type t, the token BEHIND it of type t_next; 0 at or past n) can be the key of an entry of SOME object
MSJ_HD bool is_key_candidate(uint32_t t, uint32_t t_next) { return msj::selem::is_key(t, t_next); }
// ... and is one of row d's object: strictly between the partners, one level below, its value in front of the partner
// (m < n: tokens i + 1 and i + 2 index the arrays)
MSJ_HD bool is_entry_of(uint64_t i, int32_t depth_i, const Desc &d) {
    return msj::acol::is_element_of(i, depth_i, d) && i + 2 < (uint64_t)d.m;
}

// the code behind the layout: the entries were clipped (the layout-only form asks for none, so nothing is clipped in it)
MSJ_HD int32_t entries_code(uint64_t n_entries, bool have_entries, uint64_t entries_capacity) {
    return msj::acol::elements_code(n_entries, have_entries, entries_capacity);
}

}  // namespace oent
}  // namespace msj
