// join_rows_math.h -- the arithmetic of msj_join_rows_device (join_rows_kernel.hip): which int32 is a key, how many radix
// digits order the right side for a G, how many pairs a left row emits per kind, which left row owns an output pair, the pair
// itself, and the code and counters of the result.  Host + device like its siblings, so that tests/test_join_rows_math.py
// runs the same code on the CPU (g++, tests/join_rows_math_host.cpp).
//
// The definition (include/msj_stage1.h).  A key is a key iff it lies in [0, G).  match(l) are the
// right rows r < R with the key of left row l, ascending; c(l) their number, 0 for a left row without a key.  Row l emits
// n(l) pairs -- INNER c, LEFT max(c, 1), SEMI c > 0, ANTI c == 0 -- and pair j belongs to the LAST row l with
// offsets[l] <= j, offsets being the running sum of n: rows that emit nothing never own a pair.
#pragma once
#include <stdint.h>

#include "string_column_math.h"

namespace msj {
namespace jrows {

using msj::scol::kMaxRows;

constexpr uint32_t kInner = 0, kLeft = 1, kSemi = 2, kAnti = 3;  // MSJ_JOIN_*: flags & 3
constexpr uint32_t kKnownFlags = 3u;
constexpr uint32_t kNoRow = 0xFFFFFFFFu;  // MSJ_JOIN_NO_ROW; also "no run" in the per-row word the emit reads
constexpr uint32_t kDigitBits = 8, kBuckets = 1u << kDigitBits;
constexpr uint64_t kMaxKeys = 1ull << 31;  // an int32 key lies below this whatever G says

// ---- keys -------------------------------------------------------------------------------------------------------------------
// the G a table is sized and a key tested by: no int32 reaches 2^31
MSJ_HD uint64_t most_keys(uint64_t n_keys) { return n_keys < kMaxKeys ? n_keys : kMaxKeys; }
MSJ_HD bool is_key(int32_t key, uint64_t G) { return key >= 0 && (uint64_t)key < G; }

// the eight-bit digits that tell the keys of [0, G) apart: bits(G - 1) in eights; 0 for G <= 1
MSJ_HD uint32_t key_digits(uint64_t G) {
    G = most_keys(G);
    uint32_t d = 0;
    for (uint64_t top = G ? G - 1 : 0; top != 0; top >>= kDigitBits) d++;
    return d;
}
// The passes over the right side.  The first pass leaves out the rows without a key, so it is also the compaction of the
// rows with one: there is always one pass, over digit 0 -- with G == 1 every key's digit is 0 and the pass keeps the order
MSJ_HD uint32_t key_passes(uint64_t G) {
    const uint32_t d = key_digits(G);
    return d ? d : 1u;
}
MSJ_HD uint32_t digit_of(uint32_t key, uint32_t pass) { return (key >> (kDigitBits * pass)) & (kBuckets - 1u); }

// ---- a left row -------------------------------------------------------------------------------------------------------------
// n(l) from c(l)
MSJ_HD uint64_t pairs_of_row(uint32_t kind, uint64_t c) {
    switch (kind) {
        case kInner: return c;
        case kLeft: return c ? c : 1;
        case kSemi: return c ? 1 : 0;
        default: return c ? 0 : 1;
    }
}
// the word the emit reads per left row: where the row's run starts among the right rows ordered by key, or kNoRow for a row
// whose pairs have no right side (c == 0, and every row of ANTI)
MSJ_HD uint32_t run_of_row(uint32_t kind, uint64_t c, uint32_t start) { return c == 0 || kind == kAnti ? kNoRow : start; }
// the place among the ordered right rows of the row's `within`-th pair, or kNoRow: MSJ_JOIN_NO_ROW is written
MSJ_HD uint32_t right_place(uint32_t kind, uint32_t run, uint64_t within) {
    if (run == kNoRow) return kNoRow;
    return kind == kSemi ? run : run + (uint32_t)within;
}

// ---- a pair -----------------------------------------------------------------------------------------------------------------
// the last row l in [lo, hi] with offsets[l] <= j.  (offsets[lo] <= j: the caller's.)  Rows that emit nothing share their
// successor's offset, so the last one is the row that emits
template <class Offsets>
MSJ_HD uint64_t row_of_pair(const Offsets &offsets, uint64_t lo, uint64_t hi, uint64_t j) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] <= j) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- what the call says of itself ---------------------------------------------------------------------------------------------
// the counts the device read do not fit the rooms: nothing but the result (code, flags, the three counts) is written
MSJ_HD bool counts_over(uint64_t L, uint64_t left_rows, uint64_t R, uint64_t right_rows, uint64_t G, uint64_t keys_capacity) {
    return L > left_rows || R > right_rows || G > keys_capacity || L >= kMaxRows || R >= kMaxRows;
}
// the pairs do not fit: every counter and the offsets are exact, no pair is written
MSJ_HD bool pairs_over(uint64_t M, uint64_t pairs_capacity) { return M > pairs_capacity; }

}  // namespace jrows
}  // namespace msj
