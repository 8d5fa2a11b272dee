// match_strings_math.h -- the arithmetic of msj_patterns_create and msj_match_strings_device (match_strings_kernel.hip): the
// ASCII fold of a byte and of four bytes at once, the tiles of the byte array and the masked 16-byte word that stages them,
// the four bytes at any phase of two neighbouring words, the piece test, the row of a byte, the accept rule, the chain's
// cursor and the record of a row.  Host + device like its siblings, so that tests/test_match_strings_math.py runs the same
// code on the CPU (g++, tests/match_strings_math_host.cpp) and tests/cpp/match_strings_sanitize.cpp runs it under ASan.
//
// The definition (include/msj_stage1.h).  A pattern is 1 to 4 literal pieces s_0 .. s_(n-1).  A value
// v matches iff positions p_0 .. p_(n-1) exist with v[p_j : p_j + len(s_j)] == s_j, p_(j+1) >= p_j + len(s_j), p_0 == 0
// under AT_START and p_(n-1) + len(s_(n-1)) == len(v) under AT_END; the row's number is the smallest such p_0.  The kernels
// run the leftmost-greedy chain, which finds exactly that: q_0 = the first place of s_0, q_j = the first place of s_j at or
// behind q_(j-1) + len(s_(j-1)); an anchored piece is accepted at its one place only.  A level of the chain is one pass over
// the bytes: every place where the level's piece stands competes, by minimum, in the row that holds it.
#pragma once
#include <stdint.h>

#include "string_column_math.h"

#if !defined(MSJ_HD_MEMBER)
#if defined(__HIPCC__)
#define MSJ_HD_MEMBER __host__ __device__ __forceinline__
#else
#define MSJ_HD_MEMBER inline
#endif
#endif

namespace msj {
namespace mstr {

using msj::scol::kMaxRows;

constexpr uint32_t kMaxPatterns = 16, kMaxPieces = 4, kMaxPieceBytes = 255;
constexpr uint32_t kAtStart = 1u, kAtEnd = 2u, kNocase = 4u;  // MSJ_MATCH_AT_START / _AT_END / _NOCASE_ASCII
constexpr uint32_t kKnownFlags = kAtStart | kAtEnd | kNocase;
constexpr uint64_t kNone = ~0ull;      // a (pattern, row) word: no place yet; a cursor: the chain has failed
constexpr uint64_t kMaxBytes = 1ull << 40;
constexpr uint32_t kNoSuchField = 20;  // the record of a missing value (msj_take_rows_device's)

// ---- the geometry of the pass over the bytes ----------------------------------------------------------------------------------
// The byte array is cut by ADDRESS: with phase = the address of bytes[0] mod 16, byte b stands at the aligned coordinate
// a = b + phase, and tile t holds the start positions a in [t * kTile, (t + 1) * kTile).  A tile is staged as the aligned
// 16-byte words of [t * kTile, (t + 1) * kTile + kHalo): a piece that starts at the tile's last byte ends inside the halo.
constexpr uint32_t kThreads = 256;
constexpr uint32_t kRun = 32;                  // consecutive start positions of a lane
constexpr uint32_t kTile = kThreads * kRun;    // 8 192
constexpr uint32_t kHalo = 256;                // >= kMaxPieceBytes - 1, a multiple of 16
constexpr uint32_t kWord = 16;
constexpr uint32_t kTileWords = (kTile + kHalo) / kWord;
constexpr uint32_t kStageChunk = kThreads;     // offsets staged per step
constexpr uint32_t kStage = 4 * kStageChunk;   // the most offsets staged for a tile; more rows than that: the search runs on memory
constexpr uint32_t kByteBlocks = 2048;         // most blocks of the pass over the bytes: each takes a run of consecutive tiles
constexpr uint32_t kRowBlocks = 1024;          // most blocks (per pattern) of the kernels over the rows
static_assert(kHalo % kWord == 0 && kHalo + 1 >= kMaxPieceBytes && kTile % kWord == 0, "geometry");

MSJ_HD uint32_t phase_of(const void *bytes) { return (uint32_t)(reinterpret_cast<uintptr_t>(bytes) & (kWord - 1)); }
MSJ_HD uint64_t tiles_of(uint32_t phase, uint64_t bytes_len) { return bytes_len ? (phase + bytes_len + kTile - 1) / kTile : 0; }
// the start positions of tile t as bytes [b0, b1) -- clipped to the array -- and its first aligned coordinate
struct Tile {
    uint64_t a0, b0, b1;
};
MSJ_HD Tile tile_of(uint32_t phase, uint64_t bytes_len, uint64_t t) {
    Tile x;
    x.a0 = t * kTile;
    x.b0 = x.a0 > phase ? x.a0 - phase : 0;
    const uint64_t e = x.a0 + kTile - phase;  // (a0 + kTile > phase)
    x.b1 = e < bytes_len ? e : bytes_len;
    return x;
}
// the tiles [first, last) of block `block` of `blocks`: consecutive, so that a block carries its place among the rows along
MSJ_HD void block_tiles(uint64_t tiles, uint64_t blocks, uint64_t block, uint64_t &first, uint64_t &last) {
    const uint64_t per = blocks ? (tiles + blocks - 1) / blocks : 0;
    first = block * per < tiles ? block * per : tiles;
    last = first + per < tiles ? first + per : tiles;
}

// The aligned 16-byte word at coordinate a (a multiple of 16) as four little-endian words.  A word that lies inside the array
// is ONE aligned load; the array's first and last word are put together from the bytes that exist, the others read as 0 (no
// place there is ever accepted: the accept rule knows the rows' ends).  No byte outside [0, bytes_len) is read.
struct Word16 {
    uint32_t w[4];
};
MSJ_HD Word16 load_word16(const uint8_t *bytes, uint32_t phase, uint64_t bytes_len, uint64_t a) {
    Word16 r;
    const uint64_t lo = phase, hi = phase + bytes_len;  // the coordinates that exist
    if (a >= lo && a + kWord <= hi) {
        __builtin_memcpy(r.w, __builtin_assume_aligned(bytes + (a - phase), kWord), kWord);
        return r;
    }
    r.w[0] = r.w[1] = r.w[2] = r.w[3] = 0;
    for (uint32_t k = 0; k < kWord; k++) {
        const uint64_t c = a + k;
        if (c >= lo && c < hi) r.w[k >> 2] |= (uint32_t)bytes[c - phase] << (8 * (k & 3));
    }
    return r;
}

// ---- bytes --------------------------------------------------------------------------------------------------------------------
// A to Z as a to z; every other byte, 0x80 .. 0xFF included, as itself
MSJ_HD uint32_t fold1(uint32_t c) { return c - 'A' < 26u ? c | 0x20u : c; }
// the same on the four bytes of a word
MSJ_HD uint32_t fold4(uint32_t w) {
    const uint32_t low = w & 0x7F7F7F7Fu;
    const uint32_t ge_a = low + 0x3F3F3F3Fu;  // bit 7 of a byte: its low seven bits >= 'A'
    const uint32_t gt_z = low + 0x25252525u;  // ... > 'Z'
    const uint32_t upper = ge_a & ~gt_z & ~w & 0x80808080u;
    return w | (upper >> 2);
}
// the four bytes from byte `shift` (0 .. 3) of `lo` on, `hi` the aligned word behind it
MSJ_HD uint32_t fetch4(uint32_t lo, uint32_t hi, uint32_t shift) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * shift)); }

// ---- the patterns, compiled (what msj_patterns keeps in device memory; the same bytes on the host) ----------------------------
struct Piece {
    uint32_t first, mask;  // the piece's first four bytes as a word, and which of them exist; folded under kNocase
    uint16_t len, at;      // its bytes: Patterns::bytes[at, at + len), folded under kNocase
    uint32_t reserved;
};
struct Pattern {
    uint32_t n_pieces, flags;
    Piece piece[kMaxPieces];
};
struct Patterns {
    uint32_t n, max_pieces, reserved[2];
    Pattern pat[kMaxPatterns];
    uint8_t bytes[kMaxPatterns * kMaxPieces * 256];
};

// msj_patterns_create's host part.  Spec: msj_pattern.  -> 0, or -1 (NULL, a count outside 1..16, a pattern without its
// bytes, of 0 or more than 4 pieces, a piece of 0 or more than 255 bytes, an unknown flag)
template <class Spec>
static inline int compile_patterns(const Spec *specs, uint32_t n, uint32_t flags, Patterns &out) {
    if (!specs || n == 0 || n > kMaxPatterns || flags != 0) return -1;
    out = Patterns{};
    out.n = n;
    uint32_t at = 0;
    for (uint32_t i = 0; i < n; i++) {
        const Spec &s = specs[i];
        if (!s.bytes || s.n_pieces == 0 || s.n_pieces > kMaxPieces || (s.flags & ~kKnownFlags) != 0) return -1;
        Pattern &p = out.pat[i];
        p.n_pieces = s.n_pieces, p.flags = s.flags;
        uint32_t from = 0;
        for (uint32_t j = 0; j < s.n_pieces; j++) {
            const uint32_t len = s.piece_len[j];
            if (len == 0 || len > kMaxPieceBytes) return -1;
            Piece &pc = p.piece[j];
            pc.len = (uint16_t)len, pc.at = (uint16_t)at;
            for (uint32_t x = 0; x < len; x++) {
                const uint32_t c = s.bytes[from + x];
                out.bytes[at + x] = (uint8_t)((s.flags & kNocase) ? fold1(c) : c);
            }
            for (uint32_t x = 0; x < 4 && x < len; x++) pc.first |= (uint32_t)out.bytes[at + x] << (8 * x);
            pc.mask = len >= 4 ? 0xFFFFFFFFu : (1u << (8 * len)) - 1u;
            from += len, at += len;
        }
        for (uint32_t j = s.n_pieces; j < kMaxPieces; j++)
            if (s.piece_len[j] != 0) return -1;
        if (s.n_pieces > out.max_pieces) out.max_pieces = s.n_pieces;
    }
    return 0;
}

// does pattern `p` take part in level `level`, and is that its last one
MSJ_HD bool has_level(const Pattern &p, uint32_t level) { return level < p.n_pieces; }
MSJ_HD bool is_last_level(const Pattern &p, uint32_t level) { return level + 1 == p.n_pieces; }

// ---- the piece test -----------------------------------------------------------------------------------------------------------
// the piece's first four bytes against the text's: w as read, wf = fold4(w)
MSJ_HD bool first_word_hits(uint32_t first, uint32_t mask, bool nocase, uint32_t w, uint32_t wf) { return (((nocase ? wf : w) ^ first) & mask) == 0; }
// ... and on a hit the bytes behind them; text.byte(j): byte j of the place under test (inside the staged tile and its halo)
template <class Text>
MSJ_HD bool rest_hits(const Piece &pc, bool nocase, const uint8_t *pattern_bytes, const Text &text) {
    for (uint32_t j = 4; j < pc.len; j++) {
        const uint32_t c = text.byte(j);
        if ((nocase ? fold1(c) : c) != pattern_bytes[pc.at + j]) return false;
    }
    return true;
}

// ---- the row of a byte --------------------------------------------------------------------------------------------------------
// offsets[0 .. R] ascend (the check pass has seen to that, and every later step reads its verdict).  upper_bound: the first
// index in [lo, hi) whose offset lies behind b, else hi; the caller knows that every index in front of lo does not.  The row
// of byte b is that index minus one: of a run of empty rows in front of a row that starts at b, the row that holds b.
struct MemoryOffsets {
    const uint64_t *p;
    MSJ_HD_MEMBER uint64_t at(uint64_t i) const { return p[i]; }
};
struct StagedOffsets {  // offsets[first ...) in a buffer
    const uint64_t *s;
    uint64_t first;
    MSJ_HD_MEMBER uint64_t at(uint64_t i) const { return s[i - first]; }
};
template <class Off>
MSJ_HD uint64_t upper_bound(const Off &off, uint64_t lo, uint64_t hi, uint64_t b) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off.at(mid) <= b)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
// the first offset a tile stages: the one in front of index i_start, the first index the tile's searches can give
MSJ_HD uint64_t stage_first(uint64_t i_start) { return i_start ? i_start - 1 : 0; }
// index i = upper_bound of b among offsets[0 .. R]: row i - 1 holds b, unless b lies in front of the first row or behind the last
MSJ_HD bool index_has_row(uint64_t i, uint64_t R) { return i >= 1 && i <= R; }

// ---- the accept rule ----------------------------------------------------------------------------------------------------------
// the row test of the check pass: offsets[k] <= offsets[k + 1] <= bytes_len
MSJ_HD bool offsets_ok(uint64_t begin, uint64_t end, uint64_t bytes_len) { return begin <= end && end <= bytes_len; }
// A place b of a piece of `len` bytes in the row [begin, end) whose cursor stands at `from` (level 0: begin; kNone: the chain
// has failed).  first / last: the piece is the pattern's first / last one, which the anchors bind
MSJ_HD bool accept(uint64_t b, uint32_t len, uint64_t begin, uint64_t end, uint64_t from, uint32_t flags, bool first, bool last) {
    if (b < from || b > end || end - b < len) return false;  // (from >= begin)
    if (first && (flags & kAtStart) && b != begin) return false;
    if (last && (flags & kAtEnd) && end - b != len) return false;
    return true;
}
// the chain: behind a level, the cursor of the next one
MSJ_HD uint64_t next_cursor(uint64_t hit, uint32_t len) { return hit == kNone ? kNone : hit + len; }

// ---- the call -----------------------------------------------------------------------------------------------------------------
MSJ_HD bool rows_over(uint64_t R, uint64_t rows, uint64_t capacity) { return R > rows || R > capacity || R >= kMaxRows; }
MSJ_HD uint64_t most_rows(uint64_t rows, uint64_t capacity) {
    const uint64_t m = rows < capacity ? rows : capacity;
    return m < kMaxRows ? m : kMaxRows;
}
// the record of a row: a match at p_0 relative to the row's first byte, or the missing value
struct RowRecord {
    uint64_t bits;
    uint32_t token;
    uint8_t type, flags;
    uint16_t code;
};
MSJ_HD RowRecord row_record(bool matched, uint64_t place, uint64_t begin) {
    RowRecord r;
    r.bits = matched ? place - begin : 0, r.token = 0xFFFFFFFFu;
    r.type = matched ? (uint8_t)'l' : (uint8_t)0, r.flags = 0, r.code = matched ? (uint16_t)0 : (uint16_t)kNoSuchField;
    return r;
}

}  // namespace mstr
}  // namespace msj
