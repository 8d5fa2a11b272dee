// array_column_math.h -- the arithmetic of msj_array_column_device (array_column_kernel.hip): the row test on one msj_field
// of a selected path, the descriptor a row leaves for its tokens, the element test and the rule for the result's code.
// Host + device like its siblings, so that tests/test_array_column_math.py runs the same code on the CPU (g++,
// tests/array_column_math_host.cpp).
//
// Definition (include/msj_stage1.h): the column's arrays as a list column -- offsets[D + 1], a
// validity byte per row, one msj_field per element back to back.  Nothing of it needs a walk: the elements of an array v
// are the tokens one level below it between v and its partner that start a value -- the token in front of them is '[' or
// ',' -- and the arrays of one column lie in document order, so an element's place in the output is the number of element
// tokens in front of it in the window.  The element's record is select_math.h's value_field: nothing of that is restated.
#pragma once
#include <stdint.h>

#include "select_math.h"

namespace msj {
namespace acol {

using msj::sel::document_bounds;
using msj::sel::kFieldNoBits;
using msj::sel::value_field;
using msj::tape::kNoPartner;
using msj::tdocs::Window;
using msj::tdocs::window_of;

constexpr int32_t kCapacity = 1;      // MSJ_CAPACITY
constexpr int32_t kBadArgument = -1;  // MSJ_ERR_BAD_ARGUMENT

// ---- the row test ---------------------------------------------------------------------------------------------------------
// What a row leaves for the tokens of its document: the array v, its partner m and the depth of its direct children.  A row
// that is no array has the empty range (v = 0xFFFFFFFF, m = 0): no token lies inside it.  16 bytes, one load per candidate.
struct Desc {
    uint32_t v, m;
    int32_t child_depth;
    uint32_t valid;
};
MSJ_HD Desc no_array() { return Desc{0xFFFFFFFFu, 0u, 0, 0u}; }
// One record of the column against the arrays; [f, e) is its document, bounds_ok what document_bounds said of it.  Every
// clause is checked on the arrays, none believed from the record: the token lies in the document, is a '[' and has its
// partner behind it inside the document.  other: the record has code 0 and the row is no array.  row_of_kind: the same
// test for a row that opens with `container` -- '[' here, '{' for msj_object_entries_device (object_entries_math.h)
template <class Field>
MSJ_HD Desc row_of_kind(const Field &r, uint32_t container, bool bounds_ok, uint64_t f, uint64_t e, const uint8_t *type, const int32_t *depth,
                        const uint32_t *match, bool &other) {
    Desc d = no_array();
    const uint64_t v = r.token;
    if (r.code == 0 && r.type == container && bounds_ok && v >= f && v < e && type[v] == container) {  // (e <= T <= n: v indexes the arrays)
        const uint32_t m = match[v];
        if (m != kNoPartner && (uint64_t)m > v && (uint64_t)m < e) {
            d.v = (uint32_t)v, d.m = m;
            d.child_depth = (int32_t)((uint32_t)depth[v] + 1u);  // (no signed overflow on any depth)
            d.valid = 1;
        }
    }
    other = r.code == 0 && !d.valid;
    return d;
}
template <class Field>
MSJ_HD Desc row_of(const Field &r, bool bounds_ok, uint64_t f, uint64_t e, const uint8_t *type, const int32_t *depth, const uint32_t *match,
                   bool &other) {
    return row_of_kind(r, '[', bounds_ok, f, e, type, depth, match, other);
}

// ---- the element test -----------------------------------------------------------------------------------------------------
// token i (type t, the token in front of it of type t_prev) starts a value behind '[' or ',': an element of SOME array.  The
// closer clause keeps the ']' of a nested [] out: its predecessor is '[' and it carries its container's depth
MSJ_HD bool is_candidate(uint32_t t_prev, uint32_t t) { return (t_prev == '[' || t_prev == ',') && t != ']' && t != '}'; }
// ... and is one of row d's array: strictly between the partners, one level below
MSJ_HD bool is_element_of(uint64_t i, int32_t depth_i, const Desc &d) {
    return i > (uint64_t)d.v && i < (uint64_t)d.m && depth_i == d.child_depth;
}

// ---- the call's verdict on itself -----------------------------------------------------------------------------------------
// Behind the window and d_select: the code in front of the layout, 0 when there is one.  stop (code != 0): nothing but the
// results is written.  n_rows: what the result reports then
MSJ_HD int32_t head_code(int32_t select_code, uint64_t select_documents, const Window &w, uint64_t &n_rows) {
    n_rows = 0;
    if (select_code != 0) return select_code;
    if (select_documents != w.D) return kBadArgument;  // d_select is of another window
    n_rows = w.D;
    return w.over ? kCapacity : 0;
}
// the code behind the layout: the elements were clipped (the layout-only form asks for none, so nothing is clipped in it)
MSJ_HD int32_t elements_code(uint64_t n_elements, bool have_elements, uint64_t elements_capacity) {
    return have_elements && n_elements > elements_capacity ? kCapacity : 0;
}

}  // namespace acol
}  // namespace msj
