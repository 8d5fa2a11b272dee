// tape_docs_math.h -- what msj_tape_documents_device (tape_docs_kernel.hip) adds to the arithmetic of tape_math.h: where a
// token's word, a document's root words and its string records lie in the window's output arrays, what is local to the
// document (positions in bracket words, the word count of tape[0], string offsets), the partner rebase and the record.
// Host + device, so that tests/test_tape_documents_math.py runs the same code on the CPU (g++,
// tests/tape_docs_math_host.cpp).
//
// The layout is a closed form of three prefix sums over the window's tokens -- W words, S string bytes, N number tokens, all
// counted from the first document's first token f_0 (W and S; N from token 0: the number call's records are the window's):
//   token i of document k   word   W(i) + 2k + 1            (document k's tape starts at W(f_k) + 2k: two root words each)
//   its string record       byte   S(i)                     (the word holds S(i) - S(f_k))
//   its number              record N(i)
// so no scan over the documents is needed: a token only has to know its document's number, f_k, W(f_k) and S(f_k).
#pragma once
#include <stdint.h>

#include "tape_math.h"
#include "validate_docs_math.h"

namespace msj {
namespace tdocs {

using msj::tape::kNoPartner;
using msj::val::docs_starting_up_to;

// the window as every kernel reads it from the device structs: D complete documents over the tokens [f0, T)
struct Window {
    uint64_t D, T, f0;
    bool over;  // more documents than records: nothing is built (D keeps the true number)
};
// first0: d_doc_first[0] (read only when n_complete > 0)
MSJ_HD Window window_of(uint64_t n_complete, uint64_t tokens_complete, uint64_t n, uint64_t capacity, uint64_t first0) {
    Window w;
    w.T = tokens_complete < n ? tokens_complete : n;
    w.D = n_complete < w.T ? n_complete : w.T;  // (a document has a token)
    w.f0 = w.D > 0 && first0 < w.T ? first0 : w.T;
    if (w.f0 == w.T) w.D = 0;  // (no value from d_doc_first is used unchecked)
    w.over = w.D > capacity;
    return w;
}
MSJ_HD bool in_documents(const Window &w, uint64_t i) { return i >= w.f0 && i < w.T; }

// ---- addresses in d_tape (64-bit: W(T) + 2D can pass 2^32) -----------------------------------------------------------
MSJ_HD uint64_t tape_first(uint64_t w_f, uint64_t k) { return w_f + 2 * k; }
MSJ_HD uint64_t token_word_at(uint64_t w_i, uint64_t k) { return w_i + 2 * k + 1; }
MSJ_HD uint64_t document_words(uint64_t w_f, uint64_t w_e) { return w_e - w_f + 2; }
MSJ_HD uint64_t window_words(uint64_t w_T, uint64_t D) { return w_T + 2 * D; }
// ---- what is local to document k --------------------------------------------------------------------------------------
MSJ_HD uint64_t local_pos(uint64_t w_i, uint64_t w_f) { return w_i - w_f + 1; }   // msj_tape_device's pos(i - f_k)
MSJ_HD uint64_t local_offset(uint64_t s_i, uint64_t s_f) { return s_i - s_f; }
// the partner of a bracket of the document [f, e): itself, or none when it lies in another document
MSJ_HD bool partner_inside(uint32_t m, uint64_t f, uint64_t e) { return m != kNoPartner && (uint64_t)m >= f && (uint64_t)m < e; }
MSJ_HD uint32_t rebased_partner(uint32_t m, uint64_t f, uint64_t e) { return partner_inside(m, f, e) ? (uint32_t)(m - f) : kNoPartner; }

// ---- a workgroup's slice of d_tape ------------------------------------------------------------------------------------
// A block of tokens from `base` on, k0 documents starting in front of it, writes the words [origin, next block's origin):
// token i, the j-th document of the block (0: the one that began in front of it), at slot W(i) - W(base) + 2j; the root
// words of a document that starts at i in the two slots in front of that.  Slot 0 of the window's first block would be
// word -1: it is never stored.
MSJ_HD int64_t block_origin(uint64_t w_base, uint64_t k0) { return (int64_t)(w_base + 2 * k0) - 1; }
MSJ_HD uint32_t block_slot(uint64_t w_i, uint64_t w_base, uint32_t j) { return (uint32_t)(w_i - w_base) + 2 * j; }

// ---- the record ---------------------------------------------------------------------------------------------------------
template <class Rec>
MSJ_HD Rec document_record(uint64_t k, uint64_t w_f, uint64_t w_e, uint64_t s_f, uint64_t s_e, int32_t code) {
    Rec r;
    r.tape_first = tape_first(w_f, k);
    r.string_first = s_f;
    r.tape_words = code ? 0u : (uint32_t)document_words(w_f, w_e);
    r.code = code;
    r.string_bytes = code ? 0 : s_e - s_f;
    return r;
}

}  // namespace tdocs
}  // namespace msj
