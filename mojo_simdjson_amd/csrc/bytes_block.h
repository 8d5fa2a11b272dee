// bytes_block.h -- what the two calls that lay bytes out as a column share (string_column_kernel.hip, raw_column_kernel.hip):
// the rows a block owns and the grid over them, what every kernel reads of the select result that counts the rows, and how
// the lengths kernel hands on a block's sum and its three row counts.  Device code but for the size; the arithmetic is
// string_column_math.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "docs_block.h"
#include "string_column_math.h"

namespace msj_bytes {

using msj::wave::wave_sum, msj::wave::wave_sum64;
using msj_tape::kThreads, msj_tape::kWaves;

constexpr uint32_t kRows = kThreads;    // rows per block: one per lane
constexpr uint32_t kGridBlocks = 4096;  // most blocks of the kernels over the rows (they loop over what R needs)

__host__ __device__ inline uint64_t most_rows(uint64_t capacity) { return capacity < msj::scol::kMaxRows ? capacity : msj::scol::kMaxRows; }

// what every kernel reads of the select result: R rows (its n_documents; the string column's D) in `blocks` blocks.  stop:
// nothing but the result is written
struct Head {
    uint64_t R, blocks;
    int32_t code;
    bool skip, over, stop;
};
__device__ __forceinline__ Head load_head(const msj_select_documents_result *__restrict__ sel, uint64_t capacity) {
    Head h;
    h.code = sel->code;
    h.R = sel->n_documents;
    h.skip = h.code != 0;
    h.over = !h.skip && msj::scol::rows_over(h.R, capacity);
    h.stop = h.skip || h.over;
    h.blocks = h.stop ? 0 : (h.R + kRows - 1) / kRows;
    return h;
}

// A block's round of the lengths kernel ends: the sum of its rows' lengths to *bsum, and its rows of three kinds -- a lane
// has a, b, c in {0, 1}; at most 256 of each, 10 bits each in one word -- to three counters, an atomic each where there are
// any.  lane, wave: threadIdx.x & 63 and >> 6, which the kernels have at hand in front of their loop (computed here, the
// compiler lays the loop out differently); s_sum, s_cnt: kWaves words each, free again at the next round's first barrier
__device__ __forceinline__ void block_sums_out(uint32_t lane, uint32_t wave, uint64_t length, uint32_t a, uint32_t b, uint32_t c, uint64_t *s_sum,
                                               uint32_t *s_cnt, uint64_t *bsum, unsigned long long *n_a, unsigned long long *n_b,
                                               unsigned long long *n_c) {
    const uint32_t cnt = wave_sum(a | (b << 10) | (c << 20));
    const uint64_t sum = wave_sum64(length);
    __syncthreads();  // (the last round's words have been read)
    if (lane == 0) s_sum[wave] = sum, s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t all = 0;
        uint32_t k = 0;
        for (int x = 0; x < kWaves; x++) all += s_sum[x], k += s_cnt[x];
        *bsum = all;
        if (k & 0x3FFu) atomicAdd(n_a, (unsigned long long)(k & 0x3FFu));
        if ((k >> 10) & 0x3FFu) atomicAdd(n_b, (unsigned long long)((k >> 10) & 0x3FFu));
        if (k >> 20) atomicAdd(n_c, (unsigned long long)(k >> 20));
    }
}

}  // namespace msj_bytes
