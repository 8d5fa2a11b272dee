// dictionary_extend_math.h -- the arithmetic msj_dictionary_extend_device (dictionary_extend_kernel.hip) adds to
// dictionary_math.h: an ITEM in place of a row.  With P prior entries and R rows, item c < P is prior entry c, whose bytes lie
// in d_dict_bytes behind d_dict_offsets, and item P + k is row k of the column.  The hash, the byte compare, the table and
// insert_row are dictionary_math.h's, over item numbers: the walk lowers a slot towards its smallest item, so a prior entry
// wins over every row, the lower of two equal prior entries over the higher, and the new values keep the order of first
// appearance.  Here: the entry test, where an item's bytes lie, the four conditions under which nothing is written, the
// walk that only looks up (MSJ_DICTIONARY_FROZEN) and the rule for the result's code.  Host + device like its siblings;
// tests/test_dictionary_extend_math.py runs the same code on the CPU (g++, tests/dictionary_extend_math_host.cpp).
#pragma once
#include <stdint.h>

#include "dictionary_math.h"

namespace msj {
namespace dictx {

using namespace msj::dict;

constexpr uint32_t kFrozen = 2u;    // MSJ_DICTIONARY_FROZEN
constexpr int32_t kNoEntry = -2;    // the code of a row whose value the frozen dictionary does not hold

// ---- the items --------------------------------------------------------------------------------------------------------------
struct Item {
    const uint8_t *p;  // the value's bytes [p, p + len); null, 0 for an item without a value
    uint64_t len;
    bool has;
};
// what the call reads, as the header names it
struct Source {
    const uint64_t *offsets;
    const uint8_t *valid, *bytes;
    uint64_t bytes_len;
    const uint64_t *dict_offsets;
    const uint8_t *dict_bytes;
    uint64_t dict_bytes_capacity;
};
// prior entry c: a value iff dict_offsets[c] <= dict_offsets[c + 1] <= dict_bytes_capacity -- checked, never believed
MSJ_HD Item prior_of(const Source &s, uint64_t c) {
    const uint64_t a = s.dict_offsets[c], b = s.dict_offsets[c + 1];
    Item y;
    y.has = a <= b && b <= s.dict_bytes_capacity;
    y.p = y.has ? s.dict_bytes + a : nullptr, y.len = y.has ? b - a : 0;
    return y;
}
// item i of P prior entries and the rows behind them (i < P + R)
MSJ_HD Item item_of(const Source &s, uint64_t P, uint64_t i) {
    if (i < P) return prior_of(s, i);
    const Row r = row_of(s.offsets, s.valid, i - P, s.bytes_len);
    return Item{r.has ? s.bytes + r.at : nullptr, r.len, r.has};
}

// ---- the call's verdict on its counts -----------------------------------------------------------------------------------------
// over: R > rows, P > dict_capacity, base > dict_bytes_capacity or P + R >= 2^31 -- nothing but code, flags, n_rows and
// n_prior is written.  base = dict_offsets[P], read only where the array has that entry; 0 with P == 0
struct Counts {
    uint64_t base;
    bool over;
};
MSJ_HD Counts counts_of(uint64_t R, uint64_t rows, uint64_t P, const uint64_t *dict_offsets, uint64_t dict_capacity,
                        uint64_t dict_bytes_capacity) {
    Counts n{0, true};
    if (R > rows || R >= kMaxRows || P >= kMaxRows || P + R >= kMaxRows) return n;
    if (P > dict_capacity || (P > 0 && !dict_offsets)) return n;
    n.base = P ? dict_offsets[P] : 0;
    n.over = n.base > dict_bytes_capacity;
    if (n.over) n.base = 0;
    return n;
}
// the table's slots: for every item, or in the frozen form for the prior entries alone (the rows only look up)
MSJ_HD uint64_t extend_slots(uint64_t P, uint64_t R, uint32_t flags) { return table_slots(flags & kFrozen ? P : P + R); }

// ---- the walk that only looks up ----------------------------------------------------------------------------------------------
// From hash & (S - 1) linearly as insert_row walks: an empty slot says that no inserted item has the value (found false), a
// slot whose item has the value ends the walk.  Behind the inserts' kernel boundary the slot holds the smallest such item
template <class Table, class Same>
MSJ_HD Walk lookup_item(Table &t, uint64_t S, uint64_t hash, const Same &same) {
    uint64_t i = hash & (S - 1);
    for (uint64_t step = 1; step <= S; step++, i = (i + 1) & (S - 1)) {
        const uint32_t r = t.load(i);
        if (r == kEmpty) return Walk{i, step, false};
        if (same(r)) return Walk{i, step, true};
    }
    return Walk{hash & (S - 1), S, false};
}

// ---- the call's verdict on itself -----------------------------------------------------------------------------------------
// n_distinct = P + the new values, dict_bytes = base + their bytes.  The frozen form clips nothing
MSJ_HD int32_t extend_code(uint64_t n_distinct, uint64_t dict_bytes, bool layout_only, uint64_t dict_capacity, uint64_t dict_bytes_capacity,
                           uint32_t flags) {
    return flags & kFrozen ? 0 : dict_code(n_distinct, dict_bytes, layout_only, dict_capacity, dict_bytes_capacity);
}

}  // namespace dictx
}  // namespace msj
