// select_math.h -- the arithmetic of msj_select_documents_device (select_kernel.hip): the JSON pointer parser and the
// compiled form of the paths, the member test, the key compare (plain and through tape_math.h's unescape), the state word a
// (path, document) carries from level to level, the record and the search for a number's record.  Host + device like its
// siblings, so that tests/test_select_math.py runs the same code on the CPU (g++, tests/select_math_host.cpp).
//
// Definition (include/msj_stage1.h): upstream simdjson's at_key / at_pointer restricted to object
// keys, for every (path, document) of a window.  Nothing of it needs a walk: the members of an object v are the string
// tokens followed by ':' one level below it between v and its partner, "first match wins" is the minimum of the matching
// token indices, and the value of member i is token i + 2.  A document starts at depth 0, so the object a path has reached
// behind l segments sits at depth l and its keys at depth l + 1: one pass over the window per level serves every path and
// every document at once.
#pragma once
#include <stdint.h>

#include "tape_docs_math.h"

namespace msj {
namespace sel {

using msj::tape::kNoPartner;
using msj::tape::kNumberDouble;
using msj::tape::kNumberInt64;
using msj::tape::kSpanEscaped;
using msj::tape::kSpanNumber;
using msj::tdocs::Window;
using msj::tdocs::window_of;

constexpr uint32_t kMaxPaths = 16, kMaxSegments = 8, kMaxSegmentBytes = 255;
constexpr uint32_t kIncorrectType = 17, kNoSuchField = 20, kInvalidJsonPointer = 22;  // the reference's errors.mojo
constexpr uint32_t kSpanFloat = 8u;     // MSJ_SPAN_FLOAT
constexpr uint32_t kFieldNoBits = 64u;  // MSJ_FIELD_NO_BITS
constexpr uint32_t kNoLevel = 0xFFFFu;  // Paths::len of a path that has no such segment

// ---- the paths, compiled (what msj_paths keeps in device memory; the same bytes on the host) ----------------------------
// Level-major, so that a pass over the window stages the segments of its level from one place.
struct Paths {
    uint32_t n_paths, max_levels;                         // max_levels: the longest path's segment count
    uint32_t levels[kMaxPaths];                           // segments of path p
    uint16_t len[kMaxSegments][kMaxPaths];                // bytes of segment l of path p, or kNoLevel
    uint8_t bytes[kMaxSegments][kMaxPaths][256];          // the segment, unescaped (~0 ~1 resolved)
};

// One RFC 6901 pointer into path p.  -> 0, kInvalidJsonPointer (a non-empty pointer without its leading '/', a '~' not
// followed by 0 or 1) or -1 (more than kMaxSegments segments, a segment of more than kMaxSegmentBytes bytes)
static inline int parse_pointer(const char *s, Paths &out, uint32_t p) {
    uint32_t levels = 0;
    for (uint32_t l = 0; l < kMaxSegments; l++) out.len[l][p] = (uint16_t)kNoLevel;
    if (*s != 0 && *s != '/') return (int)kInvalidJsonPointer;
    while (*s == '/') {
        s++;
        if (levels == kMaxSegments) return -1;
        uint32_t n = 0;
        while (*s != 0 && *s != '/') {
            uint32_t c = (uint8_t)*s++;
            if (c == '~') {
                if (*s != '0' && *s != '1') return (int)kInvalidJsonPointer;
                c = *s++ == '0' ? '~' : '/';
            }
            if (n == kMaxSegmentBytes) return -1;
            out.bytes[levels][p][n++] = (uint8_t)c;
        }
        out.len[levels++][p] = (uint16_t)n;
    }
    out.levels[p] = levels;
    return 0;
}
// msj_paths_create's host part: n_paths pointers into `out`.  -> 0, kInvalidJsonPointer, or -1 (no path or more than
// kMaxPaths, a NULL, a pointer beyond the limits)
static inline int compile_paths(const char *const *pointers, uint32_t n_paths, Paths &out) {
    if (!pointers || n_paths == 0 || n_paths > kMaxPaths) return -1;
    out = Paths{};
    out.n_paths = n_paths;
    for (uint32_t p = 0; p < n_paths; p++) {
        if (!pointers[p]) return -1;
        const int rc = parse_pointer(pointers[p], out, p);
        if (rc != 0) return rc;
        if (out.levels[p] > out.max_levels) out.max_levels = out.levels[p];
    }
    return 0;
}

// ---- the state word of a (path, document) ---------------------------------------------------------------------------------
// Below 2^31 (n < 2^31): a window token -- the object the path has reached, or behind the last segment the value.  Above: a
// code.  kNotFound is what a level starts from and what an atomicMin of a matching key's index lowers.
constexpr uint32_t kNotFound = 0xFFFFFFFFu;
MSJ_HD uint32_t state_code(uint32_t code) { return 0x80000000u | (code & 0xFFFFu); }
MSJ_HD bool state_is_token(uint32_t s) { return s < 0x80000000u; }
MSJ_HD uint32_t state_to_code(uint32_t s) { return s == kNotFound ? kNoSuchField : (s & 0xFFFFu); }

// document k of the window: [f, e); false when d_doc_first does not hold what the split writes (nothing is looked up)
MSJ_HD bool document_bounds(const uint32_t *first, const Window &w, uint64_t k, uint64_t &f, uint64_t &e) {
    f = first[k];
    e = w.T;
    if (k + 1 < w.D && first[k + 1] < w.T) e = first[k + 1];
    return f < e;
}
// token v of the document that ends at e as the object of the next segment: itself, or INCORRECT_TYPE
MSJ_HD uint32_t container_state(uint32_t type_v, uint32_t partner, uint64_t v, uint64_t e) {
    const bool ok = type_v == '{' && partner != kNoPartner && (uint64_t)partner > v && (uint64_t)partner < e;
    return ok ? (uint32_t)v : state_code(kIncorrectType);
}
// where document k starts for a path of `levels` segments
MSJ_HD uint32_t first_state(int32_t verdict_code, bool bounds_ok, uint32_t levels, uint32_t type_f, uint32_t partner, uint64_t f, uint64_t e) {
    if (verdict_code != 0) return state_code((uint32_t)verdict_code);
    if (!bounds_ok) return state_code(kIncorrectType);
    return levels == 0 ? (uint32_t)f : container_state(type_f, partner, f, e);
}
// behind the pass over level l: `found` (the smallest matching key, or kNotFound) of a path whose state at level l was
// `at`, into its state at level l + 1.  last: l + 1 is the path's last level, the value is taken as it is
MSJ_HD uint32_t next_state(uint32_t at, uint32_t found, bool last, uint64_t e, const uint8_t *type, const uint32_t *match) {
    if (!state_is_token(at)) return at;
    if (found == kNotFound) return kNotFound;
    const uint64_t v = (uint64_t)found + 2;
    if (!state_is_token(found) || v >= e) return state_code(kIncorrectType);  // (no token past the document is read)
    return last ? (uint32_t)v : container_state(type[v], match[v], v, e);
}

// ---- members and keys -----------------------------------------------------------------------------------------------------
// token i (type t, depth d, the token behind it of type t_next) can be a key of an object reached behind `level` segments
MSJ_HD bool is_key_at(uint32_t t, uint32_t t_next, int32_t d, uint32_t level) { return t == '"' && t_next == ':' && d == (int32_t)level + 1; }
// ... and is one of the object `lo` with the partner m
MSJ_HD bool is_member_of(uint64_t i, uint32_t lo, uint32_t m) { return i > (uint64_t)lo && m != kNoPartner && i < (uint64_t)m; }

// tape_math.h's writer that compares instead of stores: *ok goes false at the first byte that differs or lies past the segment
struct CompareWriter {
    const uint8_t *seg;
    uint32_t n;
    bool *ok;
    MSJ_HM void put(uint64_t o, uint32_t byte) const {
        if (o >= n || seg[o] != byte) *ok = false;
    }
};
// can a raw body of `raw` bytes be a key of n bytes at all (an escape gives at least 1 byte per 6 and at most 1 per byte)
MSJ_HD bool length_may_match(uint64_t raw, bool escaped, uint32_t n) { return escaped ? raw >= n && raw <= 6ull * n : raw == n; }
// the key with the raw body [b, q) against the segment; r: the window's bytes
template <class R>
MSJ_HD bool key_equals(const R &r, uint64_t b, uint64_t q, bool escaped, const uint8_t *seg, uint32_t n) {
    if (q < b || q > r.len || !length_may_match(q - b, escaped, n)) return false;  // (before a byte of the buffer is touched)
    if (!escaped) {
        for (uint32_t x = 0; x < n; x++)
            if (r.at(b + x) != seg[x]) return false;
        return true;
    }
    bool ok = true;
    const uint64_t ulen = msj::tape::unescape_serial(r, CompareWriter{seg, n, &ok}, b, q);  // (at most 6 * 255 bytes)
    return ok && ulen == n;
}

// ---- the record -----------------------------------------------------------------------------------------------------------
// the record of the number token `token` among the first n_records (token order), or -1
template <class Number>
MSJ_HD int64_t find_number(const Number *records, uint64_t n_records, uint32_t token) {
    uint64_t lo = 0, hi = n_records;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (records[mid].token < token) lo = mid + 1;
        else hi = mid;
    }
    return lo < n_records && records[lo].token == token ? (int64_t)lo : -1;
}

template <class Field>
MSJ_HD Field error_field(uint32_t code) {
    Field r;
    r.bits = 0;
    r.token = 0xFFFFFFFFu;
    r.type = 0;
    r.flags = 0;
    r.code = (uint16_t)code;
    return r;
}
// the value at token v (below T).  records: NULL or the first n_records records of the number call
template <class Field, class Number>
MSJ_HD Field value_field(uint64_t v, const uint32_t *idx, const uint8_t *type, const uint32_t *match, const uint32_t *end,
                         const uint8_t *flags, const Number *records, uint64_t n_records) {
    Field r;
    const uint32_t t = type[v], fl = flags[v];
    r.bits = 0;
    r.token = (uint32_t)v;
    r.type = (uint8_t)t;
    r.flags = 0;
    r.code = 0;
    if (fl & kSpanNumber) {
        const int64_t j = records ? find_number(records, n_records, (uint32_t)v) : -1;
        uint32_t kind = 0;
        if (j >= 0) kind = records[j].kind;
        if (kind == kNumberInt64 || kind == kNumberDouble) {
            r.type = kind == kNumberDouble ? 'd' : 'l';
            r.bits = records[j].bits;
        } else {
            r.type = (fl & kSpanFloat) ? 'd' : 'l';
            r.flags = (uint8_t)kFieldNoBits;
        }
    } else if (t == '"') {
        const uint32_t b = idx[v] + 1u;
        r.bits = (uint64_t)b | ((uint64_t)(uint32_t)(end[v] - b) << 32);
        r.flags = (uint8_t)(fl & kSpanEscaped);
    } else if (t == '{' || t == '[') {
        r.bits = match[v];
    }
    return r;
}
// a (path, document)'s final state into its record
template <class Field, class Number>
MSJ_HD Field field_of_state(uint32_t s, const uint32_t *idx, const uint8_t *type, const uint32_t *match, const uint32_t *end,
                            const uint8_t *flags, const Number *records, uint64_t n_records) {
    if (!state_is_token(s)) return error_field<Field>(state_to_code(s));
    return value_field<Field, Number>(s, idx, type, match, end, flags, records, n_records);
}

}  // namespace sel
}  // namespace msj
