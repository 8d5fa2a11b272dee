// dictionary_math.h -- the arithmetic of msj_dictionary_device (dictionary_kernel.hip): the row test on the (offsets, valid)
// arrays of a byte column, the 64-bit hash of a row's bytes, the byte compare that decides equality, the size of the
// open-addressing table and one row's walk through it, and the rule for the result's code.  Host + device like its
// siblings, so that tests/test_dictionary_math.py runs the same code on the CPU (g++, tests/dictionary_math_host.cpp).
//
// Definition (include/msj_stage1.h): row k has a value iff valid[k] != 0 and offsets[k] <=
// offsets[k + 1] <= bytes_len; two rows are equal iff their bytes are; a value's code is the number of distinct values
// whose first row lies in front of its own first row.
//
// The hash is a SUM: over the row's 8-byte little-endian words (the last one padded with zero bytes) of mix(word, its
// position), plus mix(length, kLengthSalt).  A sum can be taken in pieces in any order -- a lane over one word, a wave in
// 64-lane steps, the host front to back -- and gives the same word.  Nothing rests on its quality: equal hashes only earn
// a row the byte compare.
#pragma once
#include <stdint.h>

#include "string_column_math.h"

namespace msj {
namespace dict {

using msj::scol::kCapacity;
using msj::scol::kMaxRows;
using msj::scol::row_of_byte;

constexpr uint32_t kWeakHash = 1u;           // MSJ_DICTIONARY_WEAK_HASH
constexpr uint32_t kEmpty = 0xFFFFFFFFu;     // a table slot no row has taken (rows are below 2^31)
constexpr uint64_t kMinSlots = 1024;
constexpr uint64_t kLengthSalt = ~0ull;
constexpr int32_t kExhausted = 24;           // MSJ_UNEXPECTED_ERROR: a row walked the whole table (never, with S >= 2R)

// ---- the row test ---------------------------------------------------------------------------------------------------------
struct Row {
    uint64_t at, len;  // the value's bytes [at, at + len) inside [0, bytes_len); 0, 0 for a null row
    bool has;
};
MSJ_HD Row row_of(const uint64_t *offsets, const uint8_t *valid, uint64_t k, uint64_t bytes_len) {
    const uint64_t a = offsets[k], b = offsets[k + 1];
    Row y;
    y.has = valid[k] != 0 && a <= b && b <= bytes_len;
    y.at = y.has ? a : 0, y.len = y.has ? b - a : 0;
    return y;
}

// ---- the hash -------------------------------------------------------------------------------------------------------------
MSJ_HD uint64_t mix(uint64_t word, uint64_t salt) {
    uint64_t x = word ^ ((salt + 1) * 0x9E3779B97F4A7C15ull);
    x ^= x >> 30, x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27, x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
MSJ_HD uint64_t words_of(uint64_t len) { return (len + 7) / 8; }
// word j of the value p[0 .. len): bytes [8j, 8j + 8), those from len on read as 0.  Reads nothing outside [0, len)
MSJ_HD uint64_t load_word(const uint8_t *p, uint64_t j, uint64_t len) {
    uint64_t w = 0;
    if (8 * j + 8 <= len) {
        __builtin_memcpy(&w, p + 8 * j, 8);  // (any alignment)
        return w;
    }
    for (uint64_t b = 8 * j; b < len; b++) w |= (uint64_t)p[b] << (8 * (b - 8 * j));
    return w;
}
// the words j = first, first + step, ... of the value: a piece of the sum
MSJ_HD uint64_t hash_piece(const uint8_t *p, uint64_t len, uint64_t first, uint64_t step) {
    uint64_t sum = 0;
    for (uint64_t j = first, n = words_of(len); j < n; j += step) sum += mix(load_word(p, j, len), j);
    return sum;
}
// the pieces' sum and the length -> the row's hash
MSJ_HD uint64_t hash_finish(uint64_t sum, uint64_t len, uint32_t flags) {
    if (flags & kWeakHash) return 0xFFFFFFFFFFFFFFFFull - (len & 3);
    return sum + mix(len, kLengthSalt);
}

// ---- equality: always on the bytes ----------------------------------------------------------------------------------------
// the words j = first, first + step, ... of two values of the same length: all equal?
MSJ_HD bool equal_piece(const uint8_t *a, const uint8_t *b, uint64_t len, uint64_t first, uint64_t step) {
    for (uint64_t j = first, n = words_of(len); j < n; j += step)
        if (load_word(a, j, len) != load_word(b, j, len)) return false;
    return true;
}

// ---- the table ------------------------------------------------------------------------------------------------------------
// S: the power of two >= 2R, at least 1 024 (R < 2^31: at most 2^32)
MSJ_HD uint64_t table_slots(uint64_t R) {
    uint64_t s = kMinSlots;
    while (s < 2 * R) s <<= 1;
    return s;
}

// One row's walk: from hash & (S - 1) linearly with wrap-around, at most S steps.  An empty slot is claimed; a slot whose row
// has the same value ends the walk, and is lowered to k when k is the smaller row; any other slot is passed.  Slots never
// empty again and the value of a slot's row never changes, so every row of one value ends in the same slot, whatever the
// order, and the slot ends holding the smallest of them.  Table: load(i), claim(i, k) -> what the slot
// held (kEmpty: it is k's now), lower(i, k); same(r): row r has k's value.  found false: S steps and no slot (never)
struct Walk {
    uint64_t slot, probes;
    bool found;
};
template <class Table, class Same>
MSJ_HD Walk insert_row(Table &t, uint64_t S, uint64_t hash, uint32_t k, const Same &same) {
    uint64_t i = hash & (S - 1);
    for (uint64_t step = 1; step <= S; step++, i = (i + 1) & (S - 1)) {
        uint32_t r = t.load(i);
        if (r == kEmpty) {
            r = t.claim(i, k);
            if (r == kEmpty) return Walk{i, step, true};
        }
        if (same(r)) {
            if (k < r) t.lower(i, k);
            return Walk{i, step, true};
        }
    }
    return Walk{hash & (S - 1), S, false};
}

// ---- the call's verdict on itself -----------------------------------------------------------------------------------------
MSJ_HD bool rows_over(uint64_t R, uint64_t rows) { return R > rows || R >= kMaxRows; }
// layout_only: the three dictionary arrays are NULL
MSJ_HD int32_t dict_code(uint64_t n_distinct, uint64_t dict_bytes, bool layout_only, uint64_t dict_capacity, uint64_t dict_bytes_capacity) {
    return !layout_only && (n_distinct > dict_capacity || dict_bytes > dict_bytes_capacity) ? kCapacity : 0;
}

}  // namespace dict
}  // namespace msj
