// validate_docs_math.h -- what msj_validate_documents_device (validate_docs_kernel.hip) adds to the rule of
// validate_math.h: every document of a window judged by the unchanged token_rule / in_object, each token seeing its own
// document's [f, e) instead of [0, n).  Host + device, so that tests/test_validate_documents_math.py runs the same code on
// the CPU (g++, tests/validate_docs_math_host.cpp).
//
// Why nothing else is needed: the rule is local -- three tokens in front and one hop through the partners -- and the split
// starts a document at every depth-0 token that is not a closing bracket.  So the only thing a token of document k may
// not see is a token of another document: the accessor below shows the rule the sub-arrays [f, e) with rebased indices,
// a partner outside them as no partner, a token in front of f as nothing and token e as the end of the stream.  Depths
// need no rebase (f sits at depth 0); offsets and bytes are the window's.
#pragma once
#include "validate_math.h"

namespace msj {
namespace val {

// A: the window's accessor (type(j) = 0 and match(j) = kNoPartner outside the window's judged tokens, depth(j) for tokens
// inside).  Indices handed to and taken from the rule are relative to f.
template <class A>
struct DocTokens {
    const A &a;
    int64_t f, e;  // window indices; f <= e
    MSJ_HM uint32_t type(int64_t j) const { return (uint64_t)j < (uint64_t)(e - f) ? a.type(f + j) : 0u; }
    MSJ_HM uint32_t match(int64_t j) const {
        if ((uint64_t)j >= (uint64_t)(e - f)) return kNoPartner;
        const uint32_t m = a.match(f + j);
        if (m == kNoPartner || (int64_t)m < f || (int64_t)m >= e) return kNoPartner;  // another document's: no partner
        return (uint32_t)((int64_t)m - f);
    }
    MSJ_HM int32_t depth(int64_t j) const { return a.depth(f + j); }
};

// the structure / depth code of window token i in [f, e] as a token of the document [f, e)
template <class A>
MSJ_HD uint32_t doc_token_rule(const A &a, int64_t f, int64_t e, int64_t i, uint32_t max_depth, uint32_t &role) {
    const DocTokens<A> d{a, f, e};
    return token_rule(d, i - f, e - f, max_depth, role);
}

// Documents k < n_docs with first[k] <= token (an upper bound in the ascending first[]): the token belongs to document
// result - 1; 0: it lies in front of the first document.
MSJ_HD uint64_t docs_starting_up_to(const uint32_t *first, uint64_t n_docs, uint64_t token) {
    uint64_t lo = 0, hi = n_docs;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)first[mid] <= token) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace val
}  // namespace msj
