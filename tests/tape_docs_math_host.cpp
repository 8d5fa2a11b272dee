// Test-only harness: compiles mojo_simdjson_amd/csrc/tape_docs_math.h (and tape_math.h behind it) for the host (g++), so that
// the window form of the tape -- the same addresses, local offsets, partner rebase and records the kernels of
// msj_tape_documents_device compute (csrc/tape_docs_kernel.hip) -- is checked on a CPU-only box against the one-document
// twin on every document's sub-arrays (tests/tape_math_host.cpp), and so that the GPU tests have an expected value.  NOT
// part of the product.
#include <string.h>

#include <vector>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/tape_docs_math.h"

using namespace msj::tape;
using namespace msj::tdocs;
using msj::val::ByteReader;

namespace {
struct HostWriter {  // byte o of one record, checked against the capacity like the kernels' writer
    uint8_t *out;
    uint64_t base, cap;
    void put(uint64_t o, uint32_t byte) const {
        if (out && base + o < cap) out[base + o] = (uint8_t)byte;
    }
};
constexpr uint64_t kLaneBody = 1024;  // tape_block.h: longer bodies go 64 bytes per step, and are written whatever the verdict

template <class W>
uint64_t unescape_body(const ByteReader &r, const W &w, uint64_t b, uint64_t e) {
    if (e - b <= kLaneBody) return unescape_serial(r, w, b, e);
    StepState st = step_begin();
    for (uint64_t p = b; p < e; p += 64) unescape_step(r, w, b, e, p, (uint32_t)(e - p < 64 ? e - p : 64), st);
    return st.out;
}
}  // namespace

extern "C" {

// The whole call, the kernels' way: prefix sums over the window, then one loop over its tokens, every token with its
// document's number, f, W(f) and S(f).  docs: a host copy of the device struct; verdicts NULL as in the call.  counts_out
// (optional, n entries): the direct commas credited to each token.
void tdm_tape_documents(const uint8_t *buf, uint64_t len, const uint32_t *idx, uint64_t n, const uint8_t *typ, const int32_t *dep,
                        const uint32_t *mat, const uint32_t *end, const uint8_t *flags, const uint32_t *first,
                        const msj_documents_result *docs, const msj_number *numbers, uint64_t numbers_capacity,
                        const msj_document_verdict *verdicts, uint64_t *tape, uint64_t tape_capacity, uint8_t *sbuf,
                        uint64_t string_capacity, msj_document_tape *doc_tapes, uint64_t capacity, msj_tape_documents_result *out,
                        uint32_t *counts_out) {
    const ByteReader r{buf, len};
    const Window win = window_of(docs->n_complete, docs->tokens_complete, n, capacity, (docs->n_complete > 0 && n > 0) ? first[0] : 0);
    std::vector<uint64_t> W(n + 1, 0), S(n + 1, 0), N(n + 1, 0), ulen(n + 1, 0);
    uint64_t nstr = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t w = 0, s = 0, c = 0;
        if (i < win.T) c = is_number(flags[i]);
        if (in_documents(win, i)) {
            w = words_per_token(typ[i], flags[i]);
            if (is_string(typ[i]) && !is_number(flags[i])) {
                const uint64_t b = (uint64_t)idx[i] + 1, q = end[i];
                if (q <= len && q >= b) ulen[i] = (flags[i] & kSpanEscaped) ? unescape_body(r, NoWrite{}, b, q) : q - b;
                s = 4 + ulen[i];
                nstr++;
            }
        }
        W[i + 1] = W[i] + w, S[i + 1] = S[i] + s, N[i + 1] = N[i] + c;
    }
    memset(out, 0, sizeof *out);
    out->n_documents = win.D;
    out->tape_words = win.D ? window_words(W[win.T], win.D) : 0;
    out->string_bytes = S[win.T];
    out->n_strings = nstr;
    out->n_numbers = win.D ? N[win.T] : 0;
    const bool fits = !win.over && out->tape_words <= tape_capacity && (!sbuf || out->string_bytes <= string_capacity) &&
                      out->n_numbers <= numbers_capacity;
    out->code = fits ? MSJ_SUCCESS : MSJ_CAPACITY;
    if (counts_out) memset(counts_out, 0, 4 * n);
    if (win.over || win.D == 0) return;
    auto store = [&](uint64_t at, uint64_t w) {
        if (at < tape_capacity) tape[at] = w;
    };
    // every comma credits its container: the nearest token in front with a smaller depth, if that is the opening bracket one
    // level up (the kernels find it in a min tree over the block's depths; here a stack of the tokens not yet undercut)
    std::vector<uint32_t> cnt(n + 1, 0), stack;
    for (uint64_t i = win.f0; i < win.T; i++) {
        while (!stack.empty() && dep[stack.back()] >= dep[i]) stack.pop_back();
        if (typ[i] == ',' && !stack.empty()) {
            const uint32_t j = stack.back();
            if (dep[j] == dep[i] - 1 && is_open(typ[j])) cnt[j]++;
        }
        stack.push_back((uint32_t)i);
    }
    if (counts_out) memcpy(counts_out, cnt.data(), 4 * n);
    uint64_t k_next = 0, k = 0, f = 0, e = 0;
    bool dropped = false;
    for (uint64_t i = win.f0; i < win.T; i++) {
        if (k_next < win.D && first[k_next] == i) {  // a document starts: its record, the root words on both sides of the border
            k = k_next++;
            f = i;
            e = k_next < win.D && first[k_next] < win.T ? first[k_next] : win.T;
            const int32_t code = verdicts ? verdicts[k].code : 0;
            dropped = code != 0;
            doc_tapes[k] = document_record<msj_document_tape>(k, W[f], W[e], S[f], S[e], code);
            out->n_built += !dropped;
            if (k > 0) store(tape_first(W[f], k) - 1, root_last_word());
            store(tape_first(W[f], k), root_first_word(document_words(W[f], W[e])));
        }
        const uint32_t t = typ[i], fl = flags[i];
        const uint64_t at = token_word_at(W[i], k);
        if (is_number(fl)) {
            uint64_t bits = 0;
            uint32_t kind = kNumberInt64;
            if (N[i] < numbers_capacity && (numbers[N[i]].kind == kNumberInt64 || numbers[N[i]].kind == kNumberDouble))
                bits = numbers[N[i]].bits, kind = numbers[N[i]].kind;
            store(at, dropped ? 0 : number_tag_word(kind));
            store(at + 1, dropped ? 0 : bits);
        } else if (is_open(t) || is_close(t)) {
            const uint32_t m = mat[i];
            const uint64_t pm = partner_inside(m, f, e) ? local_pos(W[m], W[f]) : 0;
            uint64_t word = 0;
            if (!dropped) word = is_open(t) ? open_word(t, elements(m == i + 1, cnt[i]), pm) : close_word(t, pm);
            store(at, word);
        } else if (is_string(t)) {
            store(at, dropped ? 0 : string_word(local_offset(S[i], S[f])));
            const uint64_t b = (uint64_t)idx[i] + 1, q = end[i];
            const bool ok = q <= len && q >= b;
            // MIRRORED, NOT SPECIFIED: the kernels write a body of more than kLaneBody bytes from their list whatever its
            // document's verdict.  The header only says that a dropped document's slot is unspecified and stays in bounds; the
            // twin copies what the kernels do so that whole arrays can be compared.  A change of that behaviour changes this
            // line with it and breaks no contract.
            if (sbuf && (!dropped || (ok && q - b > kLaneBody))) {
                const HostWriter pre{sbuf, S[i], string_capacity}, body{sbuf, S[i] + 4, string_capacity};
                for (int x = 0; x < 4; x++) pre.put(x, (uint32_t)(ulen[i] >> (8 * x)) & 0xFFu);
                if (ok) {
                    if (fl & kSpanEscaped) {
                        (void)unescape_body(r, body, b, q);
                    } else {
                        for (uint64_t x = 0; x < ulen[i]; x++) body.put(x, r.at(b + x));
                    }
                }
            }
        } else if (is_atom(t)) {
            store(at, dropped ? 0 : atom_word(t));
        }
    }
    store(window_words(W[win.T], win.D) - 1, root_last_word());
}

// the pieces on their own
uint64_t tdm_token_word_at(uint64_t w_i, uint64_t k) { return token_word_at(w_i, k); }
uint64_t tdm_tape_first(uint64_t w_f, uint64_t k) { return tape_first(w_f, k); }
uint32_t tdm_rebased_partner(uint32_t m, uint64_t f, uint64_t e) { return rebased_partner(m, f, e); }
int64_t tdm_block_origin(uint64_t w_base, uint64_t k0) { return block_origin(w_base, k0); }
uint32_t tdm_block_slot(uint64_t w_i, uint64_t w_base, uint32_t j) { return block_slot(w_i, w_base, j); }
void tdm_window(uint64_t n_complete, uint64_t tokens_complete, uint64_t n, uint64_t capacity, uint64_t first0, uint64_t *out) {
    const Window w = window_of(n_complete, tokens_complete, n, capacity, first0);
    out[0] = w.D, out[1] = w.T, out[2] = w.f0, out[3] = w.over;
}

}  // extern "C"
