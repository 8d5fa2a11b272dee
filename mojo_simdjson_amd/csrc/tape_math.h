// tape_math.h -- the per-token arithmetic of msj_tape_device (tape_kernel.hip): words per token, the tape words, the
// element-count rule and the unescaped bytes of a string body.  Host + device like validate_math.h, so that
// tests/test_tape_math.py runs the same code on the CPU (g++, tests/tape_math_host.cpp).
//
// Definition (include/msj_stage1.h): the tape and the string buffer the reference's TapeBuilder
// (generic/stage2/tape_builder.mojo) leaves behind for a valid document.  Nothing of it needs the walk:
//   pos(i)   = 1 + the words of the tokens in front of i            (a prefix sum of words_per_token)
//   bracket  = its partner's position                               (one gather through d_match)
//   number   = the next record of msj_number_values_device          (a prefix sum of the number tokens)
//   string   = the offset of its record in the string buffer        (a prefix sum of 4 + unescaped length)
//   count    = 1 + the commas directly inside the container         (is_direct_comma; every comma credits one container)
#pragma once
#include <stdint.h>

#include "validate_math.h"

namespace msj {
namespace tape {

using msj::val::escape_start_mask;
using msj::val::hex4;
using msj::val::is_close;
using msj::val::is_open;

constexpr uint32_t kSpanEscaped = 2u, kSpanNumber = 4u;  // MSJ_SPAN_ESCAPED, MSJ_SPAN_NUMBER
constexpr uint32_t kNumberInt64 = 1u, kNumberDouble = 2u;  // MSJ_NUMBER_INT64, MSJ_NUMBER_DOUBLE
constexpr uint32_t kMaxCount = 0xFFFFFFu;                // bits 32..55 of an opening bracket's word
constexpr uint32_t kNoPartner = 0xFFFFFFFFu;

// ---- words ---------------------------------------------------------------------------------------------------------
MSJ_HD bool is_string(uint32_t type) { return type == '"'; }
MSJ_HD bool is_number(uint32_t flags) { return (flags & kSpanNumber) != 0; }
MSJ_HD bool is_atom(uint32_t type) { return type == 't' || type == 'f' || type == 'n'; }
MSJ_HD uint32_t words_per_token(uint32_t type, uint32_t flags) {
    if (is_number(flags)) return 2;
    return (is_open(type) || is_close(type) || is_string(type) || is_atom(type)) ? 1u : 0u;
}

MSJ_HD uint64_t tagged(uint32_t tag, uint64_t payload) { return ((uint64_t)tag << 56) | payload; }
MSJ_HD uint64_t root_first_word(uint64_t tape_words) { return tagged('r', tape_words); }  // visit_document_end: E + 1
MSJ_HD uint64_t root_last_word() { return tagged('r', 0); }
// elements of a container: 0 when its closing bracket follows at once (empty_container), else 1 + its direct commas
MSJ_HD uint64_t elements(bool empty, uint64_t direct_commas) { return empty ? 0 : 1 + direct_commas; }
MSJ_HD uint64_t open_word(uint32_t type, uint64_t n_elements, uint64_t partner_pos) {
    const uint64_t c = n_elements < kMaxCount ? n_elements : kMaxCount;  // deviation 3: saturates
    return tagged(type, (c << 32) | (partner_pos + 1));
}
MSJ_HD uint64_t close_word(uint32_t type, uint64_t partner_pos) { return tagged(type, partner_pos); }
MSJ_HD uint64_t string_word(uint64_t offset) { return tagged('"', offset); }
MSJ_HD uint64_t atom_word(uint32_t type) { return tagged(type, 0); }
MSJ_HD uint64_t number_tag_word(uint32_t kind) { return tagged(kind == kNumberDouble ? 'd' : 'l', 0); }  // 'u' is never produced

// the count rule: token k, strictly between an opening bracket at depth `open_depth` and its partner, is one of the
// container's own commas (what increment_count counts, tape_builder.mojo:245-272)
MSJ_HD bool is_direct_comma(uint32_t type, int32_t depth, int32_t open_depth) { return type == ',' && depth == open_depth + 1; }

// ---- strings -------------------------------------------------------------------------------------------------------
// R: at(p) = the byte at offset p (bytes at or past len read as blanks).  W: put(o, byte) stores byte o of the body's
// output (the kernels and the twin check their capacity inside it); NoWrite only measures.
struct NoWrite {
    MSJ_HM void put(uint64_t, uint32_t) const {}
};

// UTF-8 of a code point below 0x110000 (handle_unicode_codepoint :267-327 -> codepoint_to_utf8)
template <class W>
MSJ_HD uint32_t put_utf8(const W &w, uint64_t o, uint32_t cp) {
    if (cp < 0x80u) {
        w.put(o, cp);
        return 1;
    }
    if (cp < 0x800u) {
        w.put(o, 0xC0u | (cp >> 6));
        w.put(o + 1, 0x80u | (cp & 0x3Fu));
        return 2;
    }
    if (cp < 0x10000u) {
        w.put(o, 0xE0u | (cp >> 12));
        w.put(o + 1, 0x80u | ((cp >> 6) & 0x3Fu));
        w.put(o + 2, 0x80u | (cp & 0x3Fu));
        return 3;
    }
    w.put(o, 0xF0u | (cp >> 18));
    w.put(o + 1, 0x80u | ((cp >> 12) & 0x3Fu));
    w.put(o + 2, 0x80u | ((cp >> 6) & 0x3Fu));
    w.put(o + 3, 0x80u | (cp & 0x3Fu));
    return 4;
}

MSJ_HD uint32_t simple_escape(uint32_t c) {  // the byte "\c" stands for (parse_string's escape_map)
    switch (c) {
        case 'b': return 8;
        case 'f': return 12;
        case 'n': return 10;
        case 'r': return 13;
        case 't': return 9;
        default: return c;  // " \ / (anything else is STRING_ERROR in msj_validate_device: never specified here)
    }
}

// The escape that starts at the backslash at p, body [b, e), judged on its own: its bytes go to w at o, their number is
// returned, `len` receives the input bytes it covers (2 or 6).  A high surrogate followed at once by a \u low surrogate
// writes the pair's 4 bytes; the low one, whose own start follows 6 bytes later, then writes nothing: `start6` says
// whether the byte 6 in front of p starts an escape.  (An escape validate would refuse gives some bytes; the tape is
// specified for valid documents only.)
template <class R, class W>
MSJ_HD uint32_t escape_out(const R &r, const W &w, uint64_t b, uint64_t e, uint64_t p, bool start6, uint64_t o, uint32_t &len) {
    len = 2;
    if (p + 1 >= e) return 0;
    const uint32_t c = r.at(p + 1);
    if (c != 'u' || p + 6 > e) {
        w.put(o, simple_escape(c));
        return 1;
    }
    const uint32_t cp = hex4(r, p + 2);
    if (cp > 0xFFFFu) {
        w.put(o, c);
        return 1;
    }
    len = 6;
    if (cp - 0xD800u < 0x400u && p + 12 <= e && r.at(p + 6) == '\\' && r.at(p + 7) == 'u') {
        const uint32_t lo = hex4(r, p + 8);
        if (lo - 0xDC00u < 0x400u) return put_utf8(w, o, 0x10000u + ((cp - 0xD800u) << 10) + (lo - 0xDC00u));
    }
    if (cp - 0xDC00u < 0x400u && start6 && p >= b + 6 && r.at(p - 5) == 'u' && hex4(r, p - 4) - 0xD800u < 0x400u) return 0;
    return put_utf8(w, o, cp);
}

// One body, serially (what a lane does for a body of at most kLaneBody bytes): the unescaped length.
template <class R, class W>
MSJ_HD uint64_t unescape_serial(const R &r, const W &w, uint64_t b, uint64_t e) {
    uint64_t o = 0, p = b;
    bool after_high = false;  // the escape 6 bytes in front was an escape start (only a \u escape asks)
    while (p < e) {
        const uint32_t c = r.at(p);
        if (c != '\\') {
            w.put(o++, c);
            p++;
            after_high = false;
            continue;
        }
        uint32_t len;
        o += escape_out(r, w, b, e, p, after_high, o, len);
        p += len;
        after_high = len == 6;
    }
    return o;
}

// The same `width` (1..64) bytes per step, every byte on its own -- what a wave does for a longer body, width = 64.
// Carried from step to step: the parity of a run of backslashes that ends at the step's end (escape_start_mask), the
// escape starts among the 6 bytes in front (for the low surrogate's look back), the bytes of the next step that an
// escape of this one covers, and the output offset.  Nothing walks back, so the cost is linear in the body whatever
// it holds, and the body may be cut into steps anywhere.
struct StepState {
    uint64_t carry;   // the first byte of the next step is escaped
    uint64_t last6;   // bit k: the byte at p0 - 6 + k starts an escape
    uint64_t cover;   // bit k: the byte at p0 + k belongs to an escape that started in front of p0
    uint64_t out;     // unescaped bytes so far
};
MSJ_HD StepState step_begin() { return StepState{0, 0, 0, 0}; }
// (hi:lo) >> w for w in 1..64
MSJ_HD uint64_t shift_pair(uint64_t lo, uint64_t hi, uint32_t w) { return w >= 64 ? hi : (lo >> w) | (hi << (64 - w)); }

// what lane l of the step at p0 contributes, once the step's `starts` are known: output bytes (written to w at
// `o`, its own offset: st.out + the contributions of the lanes below) and the input bytes its escape covers
struct LaneOut {
    uint32_t out, len;
};
template <class R, class W>
MSJ_HD LaneOut step_lane(const R &r, const W &w, uint64_t b, uint64_t e, uint64_t p0, uint32_t l, uint32_t width, uint64_t starts,
                         const StepState &st, uint64_t o, bool measure_only) {
    const uint64_t p = p0 + l;
    LaneOut res{0, 0};
    if (l >= width || p >= e) return res;
    if ((starts >> l) & 1u) {
        const bool start6 = (((starts << 6) | st.last6) >> l) & 1u;
        if (measure_only)
            res.out = escape_out(r, NoWrite{}, b, e, p, start6, o, res.len);
        else
            res.out = escape_out(r, w, b, e, p, start6, o, res.len);
        return res;
    }
    res.out = 1;  // a byte of its own, unless an escape covers it: the caller knows after the wave agreed on `cover`
    return res;
}
// the bytes an escape at lane l of length len covers behind its backslash, as (lo, hi) masks relative to p0
MSJ_HD void cover_of(uint32_t l, uint32_t len, uint64_t &lo, uint64_t &hi) {
    const uint64_t m = (len >= 2 ? (1ull << len) - 2ull : 0ull);  // bits 1 .. len - 1
    lo = m << l;
    hi = l ? m >> (64 - l) : 0;
}
MSJ_HD void step_end(StepState &st, uint32_t width, uint64_t starts, uint64_t cover_lo, uint64_t cover_hi, uint64_t out) {
    st.carry = (starts >> (width - 1)) & 1u;
    st.last6 = shift_pair((starts << 6) | st.last6, starts >> 58, width) & 63u;
    st.cover = shift_pair(cover_lo, cover_hi, width);
    st.out = out;
}

// the host's form of one step (the twin of tape_kernel.hip: wave_unescape): bytes [p0, p0 + width) of the body [b, e)
template <class R, class W>
MSJ_HD void unescape_step(const R &r, const W &w, uint64_t b, uint64_t e, uint64_t p0, uint32_t width, StepState &st) {
    uint64_t bs = 0;
    for (uint32_t l = 0; l < width; l++) bs |= (uint64_t)(p0 + l < e && r.at(p0 + l) == '\\') << l;
    uint64_t carry = st.carry;
    const uint64_t starts = escape_start_mask(bs, carry);
    // pass 1: lengths (what the wave's ballots give); pass 2: offsets and bytes
    uint64_t cover_lo = st.cover, cover_hi = 0;
    for (uint32_t l = 0; l < width; l++) {
        if (!((starts >> l) & 1u)) continue;
        const LaneOut lo = step_lane(r, w, b, e, p0, l, width, starts, st, 0, true);
        uint64_t a, c;
        cover_of(l, lo.len, a, c);
        cover_lo |= a, cover_hi |= c;
    }
    uint64_t o = st.out;
    for (uint32_t l = 0; l < width; l++) {
        const uint64_t p = p0 + l;
        if (p >= e) break;
        if ((starts >> l) & 1u) {
            o += step_lane(r, w, b, e, p0, l, width, starts, st, o, false).out;
        } else if (!((cover_lo >> l) & 1u)) {
            w.put(o++, r.at(p));
        }
    }
    step_end(st, width, starts, cover_lo, cover_hi, o);
}

}  // namespace tape
}  // namespace msj
