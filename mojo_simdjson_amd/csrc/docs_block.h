// docs_block.h -- what the window kernels over a block of tokens share (tape_docs_kernel.hip, select_kernel.hip): the window as
// every kernel reads it from the device structs, and the documents of a block's tokens.  Device code only; the arithmetic
// is tape_docs_math.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "tape_block.h"
#include "tape_docs_math.h"

namespace msj_tdocs {

using namespace msj_tape;
using namespace msj::tdocs;

__device__ __forceinline__ Window load_window(const msj_documents_result *__restrict__ docs, const uint32_t *__restrict__ first, uint64_t n,
                                              uint64_t capacity) {
    const uint64_t nc = docs->n_complete;
    return window_of(nc, docs->tokens_complete, n, capacity, (nc > 0 && n > 0) ? first[0] : 0);
}

// The documents of a block's tokens.  rank[k]: how many documents start in the block at or in front of this lane's token k
// (0: the token belongs to the document that began in front of the block, number k0 - 1, or to none when k0 == 0);
// starts: bit k = a document starts at token k; nd: starts in the block.  s_flag: kThreads words, s_k: 2, s_w: kWaves.
struct BlockDocs {
    uint32_t k0, nd, starts;
    uint32_t rank[kPer];
};
__device__ __forceinline__ BlockDocs block_docs(const uint32_t *__restrict__ first, const Window &w, uint64_t base, uint32_t *s_flag,
                                                uint32_t *s_k, uint32_t *s_w) {
    s_flag[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_k[0] = base > 0 ? (uint32_t)docs_starting_up_to(first, w.D, base - 1) : 0u;
    if (threadIdx.x == 64) s_k[1] = (uint32_t)docs_starting_up_to(first, w.D, base + kBlock - 1);
    __syncthreads();
    BlockDocs b;
    b.k0 = s_k[0];
    const uint32_t k1 = s_k[1];
    uint8_t *flag = reinterpret_cast<uint8_t *>(s_flag);
    for (uint64_t k = (uint64_t)b.k0 + threadIdx.x; k < k1; k += kThreads) {
        // (an ascending d_doc_first, as the split writes it, has at most kBlock starts here: 4 per lane.  On any other
        // contents k1 - k0 is bounded by D only: everything stays in bounds, the block's work is no longer linear)
        const uint64_t s = first[k], o = s - base;
        if (o < kBlock && s < w.T) flag[o] = 1;  // (no value from d_doc_first is used unchecked)
    }
    __syncthreads();
    const uint32_t fw = s_flag[threadIdx.x];
    uint32_t total;
    uint32_t r = block_scan((uint32_t)__popc(fw), s_w, total);
    b.nd = total;
    b.starts = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint32_t is = (fw >> (8 * k)) & 1u;
        r += is;
        b.starts |= is << k;
        b.rank[k] = r;
    }
    return b;
}

}  // namespace msj_tdocs
