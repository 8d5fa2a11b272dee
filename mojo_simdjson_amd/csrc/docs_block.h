// docs_block.h -- what the window kernels over a block of tokens or over rows share (tape_docs_kernel.hip,
// select_kernel.hip, select_elements_kernel.hip, array_column_kernel.hip, string_column_kernel.hip): the window as every
// kernel reads it from the device structs, the documents of a block's tokens, a lane's four tokens, a msj_field as one
// 16-byte access, the number records a kernel may search, and the sizes of the launches over rows.  Device code, but for
// those sizes; the arithmetic is tape_docs_math.h.
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

// Host code: the most rows of a window of n tokens when the caller has room for `capacity` (1 for none: no array is empty),
// and the grid of the kernels over rows, which loop over what the device finds
inline uint64_t most_documents(uint64_t n, uint64_t capacity) {
    const uint64_t d = n < capacity ? n : capacity;
    return d ? d : 1;
}
inline uint32_t row_grid_blocks(uint64_t rows) {
    const uint64_t gb = (rows + kThreads - 1) / kThreads;
    return (uint32_t)(gb > 1024 ? 1024 : gb);
}

// This lane's four tokens, mine .. mine + 3 (mine a multiple of 4): the types as one 4-byte load, the depths as one 16-byte
// load; tokens from `limit` on read as type 0 at depth 0.  (A halo is the caller's: behind the block, or in front of it.)
struct TokenQuad {
    uint32_t tw;
    int32_t dk[kPer];
};
__device__ __forceinline__ TokenQuad load_token_quad(const uint8_t *__restrict__ type, const int32_t *__restrict__ depth, uint64_t mine,
                                                     uint64_t limit) {
    TokenQuad t{load_byte_quad(type, mine, limit), {0, 0, 0, 0}};
    if (mine + kPer <= limit) {
        const int4 q = *reinterpret_cast<const int4 *>(depth + mine);
        t.dk[0] = q.x, t.dk[1] = q.y, t.dk[2] = q.z, t.dk[3] = q.w;
    } else {
        for (int k = 0; k < kPer && mine + k < limit; k++) t.dk[k] = depth[mine + k];
    }
    return t;
}

// a msj_field as one 16-byte access (aligned: the entry point checks): .x/.y the bits, .z the token, .w type | flags << 8 | code << 16
__device__ __forceinline__ uint4 load_field_words(const msj_field *__restrict__ column, uint64_t k) {
    return *reinterpret_cast<const uint4 *>(column + k);
}
__device__ __forceinline__ msj_field load_field(const msj_field *__restrict__ column, uint64_t k) {
    const uint4 q = load_field_words(column, k);
    msj_field f;
    f.bits = (uint64_t)q.x | ((uint64_t)q.y << 32);
    f.token = q.z;
    f.type = (uint8_t)(q.w & 0xFFu), f.flags = (uint8_t)((q.w >> 8) & 0xFFu), f.code = (uint16_t)(q.w >> 16);
    return f;
}
__device__ __forceinline__ void store_field(msj_field *__restrict__ out, uint64_t at, const msj_field &f) {
    uint4 q;
    q.x = (uint32_t)f.bits, q.y = (uint32_t)(f.bits >> 32), q.z = f.token;
    q.w = (uint32_t)f.type | ((uint32_t)f.flags << 8) | ((uint32_t)f.code << 16);
    *reinterpret_cast<uint4 *>(out + at) = q;
}

// The number records a kernel may search: those the number call wrote and the caller has room for; none without either
struct NumberRecords {
    const msj_number *records;
    uint64_t n;
};
__device__ __forceinline__ NumberRecords number_records(const msj_number *__restrict__ numbers, uint64_t numbers_capacity,
                                                        const msj_numbers_result *__restrict__ nr) {
    NumberRecords r{nullptr, 0};
    if (numbers && nr) r.n = umin64(nr->n_numbers, numbers_capacity);
    if (r.n) r.records = numbers;
    return r;
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
