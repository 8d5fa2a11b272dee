// dictionary_order_math.h -- the arithmetic of msj_dictionary_order_device and msj_rank_rows_device
// (dictionary_order_kernel.hip): which entry has a value, the eight bytes of a value a round compares and how many of them
// the value has, the round's key and its radix digits, which entry is tied, the record of a row, the codes and the path
// choice.  Host + device like its siblings, so that tests/test_dictionary_order_math.py runs the same code on the CPU (g++,
// tests/dictionary_order_math_host.cpp) and tests/cpp/dictionary_order_sanitize.cpp runs the word fetch under ASan.
//
// The definition (include/msj_stage1.h).  Entry c < V has a value iff offsets[c] <= offsets[c + 1] <=
// bytes_capacity.  Values compare as unsigned bytes, a proper prefix first.  The order by depth B is that order with every
// value cut to its first B bytes: sorted[] = the entries with a value ascending by (v[:B], entry), then the others in entry
// order; rank[c] = the entries whose v[:B] is smaller, kNoRank without a value.  An entry is tied iff it shares its rank
// with another entry and its length is at least B.  A round takes the order by B to the order by B + 8: the tied entries
// stand at the positions [rank, rank + group size) of sorted[]; a stable sort of them by (rank, word, nvalid), written back
// to the same positions in position order, refines every group, and the new ranks are the positions of the new groups'
// first members.
#pragma once
#include <stdint.h>

#include "string_column_math.h"

// a member function on both sides (MSJ_HD is `static inline` on the host)
#if defined(__HIPCC__)
#define MSJ_HD_MEMBER __host__ __device__ __forceinline__
#else
#define MSJ_HD_MEMBER inline
#endif

namespace msj {
namespace dord {

constexpr uint32_t kNoRank = 0xFFFFFFFFu;  // MSJ_ORDER_NO_RANK
constexpr uint32_t kContinue = 1u;         // MSJ_ORDER_CONTINUE
constexpr uint32_t kKnownFlags = kContinue;
constexpr uint32_t kMaxRounds = 64;
constexpr uint64_t kMaxEntries = 1ull << 31;
constexpr uint32_t kWordBytes = 8;  // bytes a round compares
constexpr uint32_t kDigitBits = 8, kBuckets = 1u << kDigitBits;
constexpr uint32_t kModeAuto = 0, kModeGrid = 1, kModeGroup = 2;  // msj_debug_set_order_mode
constexpr uint64_t kGroupEntries = 1024;                          // the most entries the one-workgroup path keeps in LDS
// Rounds of a call with max_rounds == 0.  The one-workgroup path loops inside one kernel and leaves at the first round
// with nothing tied: the whole budget costs nothing.  Every round of the grid path is enqueued whether it runs or not
// (DESIGN.md section 5b has the cost of an idle round): four rounds order values that differ inside their first 32 bytes.
constexpr uint32_t kDefaultRoundsGroup = 64, kDefaultRoundsGrid = 4;

// ---- the call ---------------------------------------------------------------------------------------------------------------
MSJ_HD bool use_group_path(uint64_t capacity, uint32_t mode) { return capacity <= kGroupEntries && mode != kModeGrid; }
MSJ_HD uint32_t rounds_of(uint32_t max_rounds, bool group) { return max_rounds ? max_rounds : group ? kDefaultRoundsGroup : kDefaultRoundsGrid; }
// what the entry point refuses besides pointers: -> 0 or MSJ_ERR_BAD_ARGUMENT's reason
MSJ_HD bool bad_numbers(uint64_t depth, uint32_t max_rounds, uint32_t flags) {
    return (flags & ~kKnownFlags) || max_rounds > kMaxRounds || (depth % kWordBytes) != 0 || (!(flags & kContinue) && depth != 0);
}
// the entries the device read do not fit: nothing but the result is written
MSJ_HD bool entries_over(uint64_t V, uint64_t capacity) { return V > capacity || V >= kMaxEntries; }
MSJ_HD uint64_t most_entries(uint64_t capacity) { return capacity < kMaxEntries ? capacity : kMaxEntries; }

// ---- an entry ---------------------------------------------------------------------------------------------------------------
struct Value {
    uint64_t begin, len;
    bool has;
};
// entry c of a dictionary of V entries (c < V: offsets[c + 1] is read): checked, never believed
MSJ_HD Value value_of(const uint64_t *offsets, uint64_t bytes_capacity, uint64_t c) {
    const uint64_t a = offsets[c], b = offsets[c + 1];
    Value v;
    v.has = a <= b && b <= bytes_capacity;
    v.begin = a, v.len = v.has ? b - a : 0;
    return v;
}

// ---- the word ---------------------------------------------------------------------------------------------------------------
// A byte source over memory: byte(i) and, for an i whose ADDRESS is a multiple of eight, the eight bytes from there.
struct MemoryBytes {
    const uint8_t *p;
    MSJ_HD_MEMBER uint64_t misalign() const { return (uint64_t)(reinterpret_cast<uintptr_t>(p) & 7u); }
    MSJ_HD_MEMBER uint8_t byte(uint64_t i) const { return p[i]; }
    MSJ_HD_MEMBER uint64_t word(uint64_t i) const {  // little-endian: memory byte k is bits [8k, 8k + 8)
        uint64_t w;
        __builtin_memcpy(&w, __builtin_assume_aligned(p + i, 8), 8);
        return w;
    }
};
struct Word {
    uint64_t word;    // bytes [depth, depth + 8) of the value, the first one most significant, zero-padded
    uint32_t nvalid;  // how many of them the value has: 0 .. 8.  What orders "a" in front of "a\0"
};
// THE place that reads the dictionary's bytes.  (begin, len): a value that passed value_of, so begin + len <=
// bytes_capacity.  Reads aligned eight-byte words where they lie wholly inside [0, bytes_capacity) and single bytes at the
// two ragged ends; never a byte outside [begin + depth, begin + depth + nvalid) but through such a word.
template <class Bytes>
MSJ_HD Word fetch_word(const Bytes &src, uint64_t bytes_capacity, uint64_t begin, uint64_t len, uint64_t depth) {
    Word out;
    out.word = 0;
    out.nvalid = len <= depth ? 0u : len - depth < kWordBytes ? (uint32_t)(len - depth) : kWordBytes;
    const uint64_t s = begin + depth, e = s + out.nvalid, m = src.misalign();
    uint64_t i = s;
    while (i < e) {
        const uint64_t off = (i + m) & 7u;  // of byte i inside its aligned word
        if (off <= i && i - off + 8 <= bytes_capacity) {
            const uint64_t w = src.word(i - off);
            uint64_t take = 8 - off;
            if (take > e - i) take = e - i;
            for (uint64_t k = 0; k < take; k++) out.word |= ((w >> (8 * (off + k))) & 0xFFull) << (8 * (7 - (i + k - s)));
            i += take;
        } else {
            out.word |= (uint64_t)src.byte(i) << (8 * (7 - (i - s)));
            i++;
        }
    }
    return out;
}

// ---- the key of a round -----------------------------------------------------------------------------------------------------
// (rank, word, nvalid), the rank most significant.  rn = rank << 8 | nvalid
struct Key {
    uint64_t word, rn;
};
MSJ_HD Key key_of(uint32_t rank, const Word &w) {
    Key k;
    k.word = w.word, k.rn = ((uint64_t)rank << 8) | w.nvalid;
    return k;
}
MSJ_HD bool key_equal(const Key &a, const Key &b) { return a.word == b.word && a.rn == b.rn; }
MSJ_HD bool key_less(const Key &a, const Key &b) {
    const uint64_t ra = a.rn >> 8, rb = b.rn >> 8;
    if (ra != rb) return ra < rb;
    if (a.word != b.word) return a.word < b.word;
    return (a.rn & 0xFFu) < (b.rn & 0xFFu);
}

// The radix digits, least significant first: digit 0 nvalid, 1 .. 8 the word's bytes from its last, 9 .. the rank's.  Of
// the rank only the digits that tell [0, capacity) apart (join_rows_math.h: key_digits)
MSJ_HD uint32_t rank_digits(uint64_t capacity) {
    capacity = most_entries(capacity);
    uint32_t d = 0;
    for (uint64_t top = capacity ? capacity - 1 : 0; top != 0; top >>= kDigitBits) d++;
    return d;
}
constexpr uint32_t kMaxDigits = 1 + kWordBytes + 4;
MSJ_HD uint32_t key_digits(uint64_t capacity) { return 1 + kWordBytes + rank_digits(capacity); }
MSJ_HD uint32_t digit_of(const Key &k, uint32_t d) {
    if (d == 0) return (uint32_t)(k.rn & 0xFFu);
    if (d <= kWordBytes) return (uint32_t)(k.word >> (kDigitBits * (d - 1))) & 0xFFu;
    return (uint32_t)(k.rn >> (kDigitBits * (d - kWordBytes))) & 0xFFu;
}
// The passes a round runs: bit d set iff digit d differs among the tied entries, from the OR and the AND of their keys.  A
// shared prefix inside a word costs no pass
MSJ_HD uint32_t varying_digits(const Key &any, const Key &all, uint32_t digits) {
    Key x;
    x.word = any.word ^ all.word, x.rn = any.rn ^ all.rn;
    uint32_t mask = 0;
    for (uint32_t d = 0; d < digits; d++) mask |= (digit_of(x, d) != 0 ? 1u : 0u) << d;
    return mask;
}
MSJ_HD uint32_t passes_before(uint32_t mask, uint32_t d) { return (uint32_t)__builtin_popcount(mask & ((1u << d) - 1u)); }

// ---- tied ---------------------------------------------------------------------------------------------------------------------
// the entry at position p < V of sorted[]: a number at or past V is an entry without a value
struct Entry {
    uint32_t e;
    Value v;
};
template <class Sorted>
MSJ_HD Entry entry_at(const Sorted &sorted, const uint64_t *offsets, uint64_t bytes_capacity, uint64_t V, uint64_t p) {
    Entry x;
    x.e = sorted[p];
    if (x.e < V) x.v = value_of(offsets, bytes_capacity, x.e);
    else x.v.has = false, x.v.begin = 0, x.v.len = 0;
    return x;
}
// is the entry at position p tied at this depth: it has at least `depth` bytes and a neighbour of its rank
template <class Sorted, class Rank>
MSJ_HD bool tied_at(const Sorted &sorted, const Rank &rank, const uint64_t *offsets, uint64_t bytes_capacity, uint64_t V, uint64_t p,
                    uint64_t depth, Entry &x) {
    x = entry_at(sorted, offsets, bytes_capacity, V, p);
    if (!x.v.has || x.v.len < depth) return false;
    const uint32_t r = rank[x.e];
    if (p > 0) {
        const Entry n = entry_at(sorted, offsets, bytes_capacity, V, p - 1);
        if (n.v.has && rank[n.e] == r) return true;
    }
    if (p + 1 < V) {
        const Entry n = entry_at(sorted, offsets, bytes_capacity, V, p + 1);
        if (n.v.has && rank[n.e] == r) return true;
    }
    return false;
}
// an entry whose value an earlier entry also holds: not tied, and not the first of its rank (a group stands in entry order)
MSJ_HD bool is_repeat(bool has, bool tied, uint32_t rank, uint64_t p) { return has && !tied && (uint64_t)rank != p; }

// the code of a call that did not stop: complete, or the round budget ended with entries still tied
MSJ_HD int32_t order_code(uint64_t n_tied) { return n_tied ? 1 /* MSJ_CAPACITY */ : 0; }

// ---- msj_rank_rows_device ---------------------------------------------------------------------------------------------------
constexpr uint16_t kNoSuchField = 20;
struct RowRecord {  // msj_field's members
    uint64_t bits;
    uint32_t token;
    uint8_t type, flags;
    uint16_t code;
};
constexpr uint32_t kRanked = 0, kNull = 1, kUnknown = 2;  // what a row counts as
// the record of a row with code c: its value's rank as an 'l', or the record of a missing value msj_take_rows_device writes
template <class Rank>
MSJ_HD uint32_t row_record(int32_t c, uint64_t V, const Rank &rank, RowRecord &r) {
    r.bits = 0, r.token = 0xFFFFFFFFu, r.type = 0, r.flags = 0, r.code = kNoSuchField;
    if (c >= 0 && (uint64_t)c < V) {
        const uint32_t k = rank[c];
        if (k != kNoRank) {
            r.bits = k, r.type = 'l', r.code = 0;
            return kRanked;
        }
    }
    return c == -1 ? kNull : kUnknown;
}
MSJ_HD bool rank_rows_over(uint64_t R, uint64_t rows, uint64_t capacity, uint64_t V, uint64_t rank_capacity) {
    return R > rows || R > capacity || V > rank_capacity || R >= msj::scol::kMaxRows;
}

}  // namespace dord
}  // namespace msj
