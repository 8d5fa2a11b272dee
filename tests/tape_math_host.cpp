// Test-only harness: compiles mojo_simdjson_amd/csrc/tape_math.h for the host (g++), so that the arithmetic of
// msj_tape_device (csrc/tape_kernel.hip) -- the same code the kernels run -- is checked against a serial tape builder on a
// CPU-only box, and so that the GPU tests have an expected value at any size.  NOT part of the product.
#include <string.h>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/tape_math.h"

using namespace msj::tape;
using msj::val::ByteReader;

namespace {
struct HostWriter {  // byte o of one record, checked against the capacity like the kernels' writer
    uint8_t *out;
    uint64_t base, cap;
    void put(uint64_t o, uint32_t byte) const {
        if (out && base + o < cap) out[base + o] = (uint8_t)byte;
    }
};
constexpr uint64_t kLaneBody = 1024;  // tape_kernel.hip: longer bodies go 64 bytes per step

template <class W>
uint64_t unescape_steps(const ByteReader &r, const W &w, uint64_t b, uint64_t e, uint64_t cut) {
    // 64 bytes per step from b; a cut (b < cut < e) ends a step early and the next one starts there
    StepState st = step_begin();
    uint64_t p = b;
    while (p < e) {
        uint64_t width = e - p < 64 ? e - p : 64;
        if (p < cut && p + width > cut) width = cut - p;
        unescape_step(r, w, b, e, p, (uint32_t)width, st);
        p += width;
    }
    return st.out;
}
}  // namespace

extern "C" {

// the whole call.  num_bits / num_kinds: the records of msj_number_values_device in token order.  pos / counts / ulen
// (optional, n entries each): per token, for the tests that look at one quantity.
void tm_build(const uint8_t *buf, uint64_t len, const uint32_t *idx, uint64_t n, const uint8_t *typ, const int32_t *dep,
              const uint32_t *mat, const uint32_t *end, const uint8_t *flags, const uint64_t *num_bits, const uint32_t *num_kinds,
              uint64_t numbers_capacity, uint64_t *tape, uint64_t tape_capacity, uint8_t *sbuf, uint64_t string_capacity,
              msj_tape_result *out, uint32_t *pos_out, uint32_t *counts_out, uint32_t *ulen_out) {
    const ByteReader r{buf, len};
    uint64_t words = 0, nums = 0, nstr = 0, soff = 0;
    auto store = [&](uint64_t at, uint64_t w) {
        if (at < tape_capacity) tape[at] = w;
    };
    // positions first: a bracket's word holds its partner's
    uint32_t *pos = new uint32_t[n + 1];
    for (uint64_t i = 0; i < n; i++) {
        pos[i] = (uint32_t)(1 + words);
        words += words_per_token(typ[i], flags[i]);
    }
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t t = typ[i], fl = flags[i];
        if (pos_out) pos_out[i] = pos[i];
        if (counts_out) counts_out[i] = 0;
        if (ulen_out) ulen_out[i] = 0;
        if (is_number(fl)) {
            uint64_t bits = 0;
            uint32_t kind = kNumberInt64;
            if (nums < numbers_capacity && (num_kinds[nums] == kNumberInt64 || num_kinds[nums] == kNumberDouble))
                bits = num_bits[nums], kind = num_kinds[nums];
            nums++;
            store(pos[i], number_tag_word(kind));
            store((uint64_t)pos[i] + 1, bits);
        } else if (is_open(t) || is_close(t)) {
            const uint32_t m = mat[i];
            const bool usable = m != kNoPartner && m < n;
            const uint64_t pm = usable ? pos[m] : 0;
            if (is_open(t)) {
                uint64_t commas = 0;
                if (usable && m > i)
                    for (uint64_t k = i + 1; k < m; k++) commas += is_direct_comma(typ[k], dep[k], dep[i]);
                if (counts_out) counts_out[i] = (uint32_t)commas;
                store(pos[i], open_word(t, elements(m == i + 1, commas), pm));
            } else {
                store(pos[i], close_word(t, pm));
            }
        } else if (is_string(t)) {
            const uint64_t b = (uint64_t)idx[i] + 1, q = end[i];
            const bool ok = q <= len && q >= b;
            const HostWriter body{sbuf, soff + 4, string_capacity};
            uint64_t ulen = 0;
            if (ok) {
                if (!(fl & kSpanEscaped)) {
                    ulen = q - b;
                    for (uint64_t x = 0; x < ulen; x++) body.put(x, r.at(b + x));
                } else if (q - b <= kLaneBody) {
                    ulen = unescape_serial(r, body, b, q);
                } else {
                    ulen = unescape_steps(r, body, b, q, 0);
                }
            }
            const HostWriter pre{sbuf, soff, string_capacity};
            for (int x = 0; x < 4; x++) pre.put(x, (uint32_t)(ulen >> (8 * x)) & 0xFFu);
            if (ulen_out) ulen_out[i] = (uint32_t)ulen;
            store(pos[i], string_word(soff));
            soff += 4 + ulen;
            nstr++;
        } else if (is_atom(t)) {
            store(pos[i], atom_word(t));
        }
    }
    delete[] pos;
    out->flags = 0;
    out->tape_words = words + 2;
    out->string_bytes = soff;
    out->n_strings = nstr;
    const bool fits = out->tape_words <= tape_capacity && (!sbuf || soff <= string_capacity) && nums <= numbers_capacity;
    out->code = fits ? MSJ_SUCCESS : MSJ_CAPACITY;
    store(0, root_first_word(out->tape_words));
    store(words + 1, root_last_word());
}

// one string body [b, e) into out (capacity cap; NULL measures): the unescaped length.  which = 0: the serial walk; 1: 64
// bytes per step; 2: the same with a step cut short at `cut`
uint64_t tm_unescape(const uint8_t *buf, uint64_t len, uint64_t b, uint64_t e, int32_t which, uint64_t cut, uint8_t *out, uint64_t cap) {
    const ByteReader r{buf, len};
    const HostWriter w{out, 0, cap};
    if (which == 0) return unescape_serial(r, w, b, e);
    return unescape_steps(r, w, b, e, which == 2 ? cut : 0);
}

uint32_t tm_words_per_token(uint32_t type, uint32_t flags) { return words_per_token(type, flags); }
uint64_t tm_open_word(uint32_t type, uint64_t n_elements, uint64_t partner_pos) { return open_word(type, n_elements, partner_pos); }
uint64_t tm_close_word(uint32_t type, uint64_t partner_pos) { return close_word(type, partner_pos); }
uint64_t tm_string_word(uint64_t off) { return string_word(off); }
uint64_t tm_atom_word(uint32_t type) { return atom_word(type); }
uint64_t tm_number_tag_word(uint32_t kind) { return number_tag_word(kind); }
uint64_t tm_root_word(int32_t last, uint64_t tape_words) { return last ? root_last_word() : root_first_word(tape_words); }
int32_t tm_is_direct_comma(uint32_t type, int32_t depth, int32_t open_depth) { return is_direct_comma(type, depth, open_depth); }

}  // extern "C"
