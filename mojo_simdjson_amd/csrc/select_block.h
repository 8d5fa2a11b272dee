// select_block.h -- the steps select_kernel.hip (rows = the documents of a window) and select_elements_kernel.hip (rows =
// the elements of a list column) share: a block's key candidates, the level's segments in LDS, a candidate's walk over
// the paths, and the bodies of the step and finish kernels.  How a token finds its row, what a (path, row) starts from
// and when a block can end early is each file's own.  Device code only; the arithmetic is select_math.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "docs_block.h"
#include "select_math.h"

namespace msj_selblock {

using namespace msj_tdocs;
using namespace msj::sel;

static_assert(sizeof(msj_field) == 16 && sizeof(msj_select_documents_result) == 48, "ABI");

// (Words, below: each file's struct of the two state words of (p, row), level l's in word[l & 1][p * stride + row].)

// a level's segments, staged once per block: len[p] is kNoLevel for a path without this level
struct Segments {
    uint8_t bytes[kMaxPaths][256];
    uint32_t len[kMaxPaths];
};

// A block's first step, in two halves so that a caller can put work of its own in front of the barrier, where the loads'
// latency hides it.  load_block: this lane's four tokens (tokens from `limit` on read as nothing), one token of halo
// behind the block for the ':', and the segments' lengths; s_type: kThreads + 1 words.  key_candidates: the barrier, then
// the candidates among the four -- bit k: token mine + k is below limit and is_key(i, type, type of the token behind,
// depth).  False in every lane: no candidate in the whole block
__device__ __forceinline__ TokenQuad load_block(const Paths *__restrict__ paths, uint32_t level, const uint8_t *__restrict__ type,
                                                const int32_t *__restrict__ depth, uint64_t base, uint64_t limit, uint32_t *s_type,
                                                Segments &seg) {
    const TokenQuad t = load_token_quad(type, depth, base + (uint64_t)threadIdx.x * kPer, limit);
    s_type[threadIdx.x] = t.tw;
    if (threadIdx.x == 0) s_type[kThreads] = load_byte_quad(type, base + kBlock, limit);  // the halo: one token is needed
    if (threadIdx.x < kMaxPaths) seg.len[threadIdx.x] = threadIdx.x < paths->n_paths ? paths->len[level][threadIdx.x] : kNoLevel;
    return t;
}
template <class IsKey>
__device__ __forceinline__ bool key_candidates(const TokenQuad &t, uint64_t base, uint64_t limit, const uint32_t *s_type, uint32_t &cand,
                                               IsKey is_key) {
    const uint64_t mine = base + (uint64_t)threadIdx.x * kPer;
    __syncthreads();
    const uint32_t behind = s_type[threadIdx.x + 1];
    cand = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint64_t i = mine + k;
        const uint32_t ty = (t.tw >> (8 * k)) & 0xFFu, t_next = k + 1 < kPer ? (t.tw >> (8 * (k + 1))) & 0xFFu : behind & 0xFFu;
        if (i < limit && is_key(i, ty, t_next, t.dk[k])) cand |= 1u << k;
    }
    return __syncthreads_or((int)cand) != 0;
}

// the level's segments into LDS (the caller's next barrier publishes them)
__device__ __forceinline__ void stage_segments(const Paths *__restrict__ paths, uint32_t level, Segments &seg) {
    const uint32_t n_paths = paths->n_paths;
    for (uint32_t p = 0; p < n_paths; p++) {
        const uint32_t sl = seg.len[p];
        if (sl != kNoLevel)
            for (uint32_t x = threadIdx.x; x < sl; x += kThreads) seg.bytes[p][x] = paths->bytes[level][p][x];
    }
}

// Candidate key token i of `row`: for every path whose segment can have the key's raw length, the state word, the member
// test -- is_member(lo, m): key i is a direct member of the object lo with partner m -- and the key compare.  A match issues
// one atomicMin of i on the next level's word: "the first match wins" is the minimum
template <class Words, class IsMember>
__device__ __forceinline__ void match_key(const ByteReader &r, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ match,
                                          const uint32_t *__restrict__ end, const uint8_t *__restrict__ flags, uint64_t i, uint64_t row,
                                          uint32_t n_paths, uint32_t level, const Segments &seg, const Words &ws, IsMember is_member) {
    const uint64_t b = (uint64_t)idx[i] + 1, q = end[i];
    const bool escaped = (flags[i] & kSpanEscaped) != 0;
    if (q < b || q > r.len) return;  // not what the span call writes: never read
    const uint32_t *at = ws.word[level & 1];
    uint32_t *found = ws.word[(level + 1) & 1];
    for (uint32_t p = 0; p < n_paths; p++) {
        const uint32_t sl = seg.len[p];
        if (sl == kNoLevel || !length_may_match(q - b, escaped, sl)) continue;
        const uint64_t w = p * ws.stride + row;
        const uint32_t lo = at[w];
        if (!state_is_token(lo) || !is_member(lo, match[lo])) continue;  // (a token state is below the window's n)
        if (key_equals(r, b, q, escaped, seg.bytes[p], sl)) atomicMin(found + w, (uint32_t)i);
    }
}

// Behind each level, per (p, row) with p = blockIdx.y: the minimum into the next level's state -- v = i + 2, checked for '{'
// and a partner below bound(row) unless it is the path's last level -- and the word of the level after it "not found" (the
// two word arrays alternate).  A path that ended at or in front of this level keeps its word
template <class Words, class Bound>
__device__ __forceinline__ void step_rows(const Paths *__restrict__ paths, uint32_t level, const uint8_t *__restrict__ type,
                                          const uint32_t *__restrict__ match, const Words &ws, uint64_t rows, Bound bound) {
    const uint32_t p = blockIdx.y, levels = paths->levels[p];
    if (levels <= level) return;
    uint32_t *at = ws.word[level & 1], *next = ws.word[(level + 1) & 1];
    const uint64_t lanes = (uint64_t)gridDim.x * kThreads;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < rows; k += lanes) {
        const uint64_t w = p * ws.stride + k;
        next[w] = next_state(at[w], next[w], levels == level + 1, bound(k), type, match);
        if (levels > level + 1) at[w] = kNotFound;  // the word of level + 2
    }
}

// Per (p, row) with p = blockIdx.y, coalesced along the rows: the record of state_of(row); n_found / n_no_bits by wave and
// block, one atomic per block and counter
template <class StateOf>
__device__ __forceinline__ void finish_rows(const uint32_t *__restrict__ idx, const uint8_t *__restrict__ type, const uint32_t *__restrict__ match,
                                            const uint32_t *__restrict__ end, const uint8_t *__restrict__ flags, const NumberRecords nr,
                                            uint64_t rows, msj_field *__restrict__ fields, uint64_t capacity,
                                            msj_select_documents_result *__restrict__ result, StateOf state_of) {
    __shared__ uint32_t w_found[kWaves], w_nobits[kWaves];
    const uint64_t lanes = (uint64_t)gridDim.x * kThreads;
    uint32_t n_found = 0, n_nobits = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < rows; k += lanes) {
        const msj_field f = field_of_state<msj_field, msj_number>(state_of(k), idx, type, match, end, flags, nr.records, nr.n);
        fields[blockIdx.y * capacity + k] = f;  // (k < rows <= capacity)
        n_found += f.code == 0;
        n_nobits += (f.flags & kFieldNoBits) != 0;
    }
    (void)block_counter_add(n_found, w_found, &result->n_found);
    (void)block_counter_add(n_nobits, w_nobits, &result->n_no_bits);
}

}  // namespace msj_selblock
