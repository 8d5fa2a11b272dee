// list_block.h -- what the list and map column calls share over a block of 1 024 tokens (array_column_kernel.hip, and through
// rows_block.h array_elements_kernel.hip and object_entries_kernel.hip): the blocks a window needs, a lane's four tokens with
// their candidate bits, the lane whose candidates look at the token in FRONT of them, and the msj_select_documents_result
// that goes with item records.  Device code but for the size; the candidate test is array_column_math.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "array_column_math.h"
#include "docs_block.h"

namespace msj_list {

using namespace msj_tdocs;

__host__ __device__ inline uint64_t token_blocks(uint64_t tokens) { return (tokens + kBlock - 1) / kBlock; }

// A lane's four tokens of the block at `base`: types, depths and the candidates among them (bit k: token mine + k)
struct Lane {
    TokenQuad t;
    uint32_t cand;
};

// Candidates behind '[' or ',' (array_column_math.h: is_candidate): one token of halo in front of the block.  Tokens from
// `limit` on read as nothing; in_range(i): token i can be a candidate at all.  s_type: kThreads words of LDS that nothing
// else uses (a lane reads its neighbour's word behind the barrier)
template <class InRange>
__device__ __forceinline__ Lane load_lane_front(uint64_t limit, uint64_t base, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                uint32_t *s_type, InRange in_range) {
    Lane l;
    const uint64_t mine = base + (uint64_t)threadIdx.x * kPer;
    l.t = load_token_quad(type, depth, mine, limit);
    s_type[threadIdx.x] = l.t.tw;
    __syncthreads();
    // the token in front of this lane's first: the lane before's last, or the halo, one token in front of the block
    uint32_t prev = threadIdx.x > 0 ? s_type[threadIdx.x - 1] >> 24 : (base > 0 ? (uint32_t)type[base - 1] : 0u);  // (base - 1 < limit)
    l.cand = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint32_t t = (l.t.tw >> (8 * k)) & 0xFFu;
        if (in_range(mine + k) && msj::acol::is_candidate(prev, t)) l.cand |= 1u << k;
        prev = t;
    }
    return l;
}

// The result that makes `items` item records the rows of a later call: one path, every record found.  n_no_bits is the emit
// kernel's
__device__ __forceinline__ msj_select_documents_result items_select(int32_t code, uint64_t items) {
    msj_select_documents_result e;
    e.code = code;
    e.flags = 0;
    e.n_documents = e.n_found = items;
    e.n_paths = 1;
    e.n_no_bits = e.reserved = 0;
    return e;
}

}  // namespace msj_list
