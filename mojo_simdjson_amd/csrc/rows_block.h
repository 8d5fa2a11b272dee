// rows_block.h -- what the calls over ANY ascending msj_field records as rows share (array_elements_kernel.hip,
// object_entries_kernel.hip): the call's state and workspace, what every kernel reads of d_rows_select, the five kernels over
// rows -- the live rows counted, ranked, placed, their order checked, and at the end d_offsets / d_valid written --, and the
// search for the rows a block of tokens has to stage.  The kernels are templates over the byte a row's container opens with
// ('[' or '{'): only rows_place's row test reads it.  Device code but for the sizes; the arithmetic is array_elements_math.h.
//   rows_live    a lane per row, 256 rows per block of rows: the 16-byte record as one load, the live rows of the block counted
//   rows_ranks   one workgroup of 1 024: the exclusive sum over the blocks of rows, the number of live rows
//   rows_place   a lane per row: a live row's dense number j = the live rows in front of it; start[j] = its token for every
//                live row, the 16-byte descriptor {v, m, depth of v's children, valid} for j < min(n, capacity) -- a live row
//                past that names no token --, and for EVERY row the word {j, live} the last pass reads; n_containers / n_other
//                by wave and block, one atomic each per block
//   rows_order   start[j - 1] < start[j] over the live rows; a violation sets the state's flag, and every later kernel
//                returns at once when it is set
//   rows_finish  a lane per row, coalesced along r: d_offsets[r] and d_valid[r] from the row's word.  Last, so that an order
//                violation leaves both untouched
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "array_elements_math.h"
#include "docs_block.h"

namespace msj_rows {

using namespace msj_tdocs;
using namespace msj::aelem;

static_assert(sizeof(msj_field) == 16 && sizeof(Desc) == 16, "ABI");

constexpr uint32_t kRowBlock = kThreads;   // rows per block of rows: a lane each
constexpr uint32_t kStaged = kBlock + 1;   // rows a block of tokens stages: those that start in it and the one in front

struct RowsState {  // cleared by a memset per call
    uint64_t n_containers, n_other, n_live, n_items;  // rows that are a container, live rows that are none, live rows, elements / entries
    uint32_t bad_order, pad;
    uint64_t reserved[3];
};
struct RowsWork {
    RowsState *st;
    uint64_t *rsum;    // per block of rows: its live rows, then (rows_ranks) the live rows in front of the block
    uint32_t *rank;    // per row: rank_word
    uint32_t *start;   // per live row: its token
    Desc *desc;        // per dense row
    uint64_t *doff;    // per dense row: the items in front of it
    uint32_t *bsum;    // per block of tokens: its items, then (the call's scan) the items in front of the block
    uint64_t dense;    // dense_rows(n, capacity)
};

__host__ __device__ inline uint64_t row_blocks(uint64_t rows) { return (rows + kRowBlock - 1) / kRowBlock; }
__host__ __device__ inline uint64_t token_blocks(uint64_t tokens) { return (tokens + kBlock - 1) / kBlock; }
static inline uint64_t work_bytes(uint64_t n, uint64_t capacity) {
    return sizeof(RowsState) + up16(8 * row_blocks(capacity)) + 2 * up16(4 * capacity) + (sizeof(Desc) + 8) * dense_rows(n, capacity) +
           up16(4 * token_blocks(n)) + 64;
}
static inline RowsWork work_layout(void *ws, uint64_t n, uint64_t capacity) {
    uint8_t *p = static_cast<uint8_t *>(ws);
    auto take = [&](uint64_t bytes) {
        uint8_t *q = p;
        p += up16(bytes);
        return q;
    };
    RowsWork w;
    w.dense = dense_rows(n, capacity);
    w.st = reinterpret_cast<RowsState *>(take(sizeof(RowsState)));
    w.desc = reinterpret_cast<Desc *>(take(sizeof(Desc) * w.dense));
    w.doff = reinterpret_cast<uint64_t *>(take(8 * w.dense));
    w.rsum = reinterpret_cast<uint64_t *>(take(8 * row_blocks(capacity)));
    w.rank = reinterpret_cast<uint32_t *>(take(4 * capacity));
    w.start = reinterpret_cast<uint32_t *>(take(4 * capacity));
    w.bsum = reinterpret_cast<uint32_t *>(take(4 * token_blocks(n)));
    return w;
}

// what every kernel reads of d_rows_select.  stop: nothing but the results is written
struct Head {
    uint64_t R, n_rows;
    int32_t code;
    bool stop;
};
__device__ __forceinline__ Head load_head(const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity) {
    Head h;
    h.R = rows_select->n_documents;
    h.code = head_code(rows_select->code, h.R, capacity, h.n_rows);
    h.stop = h.code != 0;
    return h;
}
// ... and, behind rows_order, of the state: the dense rows that exist
__device__ __forceinline__ uint32_t dense_count(const RowsWork &w) { return (uint32_t)umin64(w.st->n_live, w.dense); }  // (< 2^31)

__device__ __forceinline__ bool live_record(const uint4 q) { return is_live(q.w >> 16); }

template <uint32_t kContainer>
__global__ __launch_bounds__(kThreads) void rows_live(const msj_field *__restrict__ rows, const msj_select_documents_result *__restrict__ rows_select,
                                                      uint64_t capacity, const RowsWork w) {
    __shared__ uint32_t s_w32[kWaves];
    const Head h = load_head(rows_select, capacity);
    if (h.stop) return;
    const uint64_t blocks = row_blocks(h.R);  // (R <= capacity)
    for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const uint64_t r = b * kRowBlock + threadIdx.x;
        const uint32_t live = r < h.R && live_record(load_field_words(rows, r));
        uint32_t total;
        (void)block_scan(live, s_w32, total);
        if (threadIdx.x == 0) w.rsum[b] = total;
    }
}

template <uint32_t kContainer>
__global__ __launch_bounds__(1024) void rows_ranks(const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity, const RowsWork w) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(rows_select, capacity);
    if (h.stop) return;
    const uint64_t live = scan_in_place(w.rsum, row_blocks(h.R), s_w);
    if (threadIdx.x == 0) w.st->n_live = live;
}

template <uint32_t kContainer>
__global__ __launch_bounds__(kThreads) void rows_place(uint64_t n, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                       const uint32_t *__restrict__ match, const msj_field *__restrict__ rows,
                                                       const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                       const RowsWork w) {
    __shared__ uint32_t s_w32[kWaves], s_containers[kWaves], s_other[kWaves];
    const Head h = load_head(rows_select, capacity);
    if (h.stop) return;
    const uint64_t blocks = row_blocks(h.R);
    uint32_t n_containers = 0, n_other = 0;
    for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const uint64_t r = b * kRowBlock + threadIdx.x;
        msj_field f;
        f.bits = 0, f.token = 0, f.type = 0, f.flags = 0, f.code = 1;
        if (r < h.R) f = load_field(rows, r);
        const bool live = r < h.R && is_live(f.code);
        uint32_t total;
        const uint64_t j = w.rsum[b] + block_scan((uint32_t)live, s_w32, total);
        if (r >= h.R) continue;  // (behind the scan's barriers: the whole block meets there)
        w.rank[r] = rank_word(j, live);  // (r < R <= capacity)
        if (!live) continue;
        w.start[j] = f.token;  // (j <= r)
        bool other;
        const Desc d = msj::acol::row_of_kind(f, kContainer, true, 0, n, type, depth, match, other);
        if (j < w.dense) *reinterpret_cast<uint4 *>(w.desc + j) = make_uint4(d.v, d.m, (uint32_t)d.child_depth, d.valid);
        n_containers += d.valid, n_other += other;
    }
    (void)block_counter_add(n_containers, s_containers, &w.st->n_containers);
    (void)block_counter_add(n_other, s_other, &w.st->n_other);
}

template <uint32_t kContainer>
__global__ __launch_bounds__(kThreads) void rows_order(const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                       const RowsWork w) {
    const Head h = load_head(rows_select, capacity);
    if (h.stop) return;
    const uint64_t live = w.st->n_live, lanes = (uint64_t)gridDim.x * kThreads;  // (<= R <= capacity)
    for (uint64_t j = 1 + (uint64_t)blockIdx.x * kThreads + threadIdx.x; j < live; j += lanes)
        if (!in_order(w.start[j - 1], w.start[j])) w.st->bad_order = 1;  // (every writer stores the same value)
}

template <uint32_t kContainer>
__global__ __launch_bounds__(kThreads) void rows_finish(uint64_t n, const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                        const RowsWork w, uint64_t *__restrict__ offsets, uint8_t *__restrict__ valid) {
    const Head h = load_head(rows_select, capacity);
    if (h.stop || w.st->bad_order) return;
    const uint64_t dense = dense_count(w), n_items = w.st->n_items;
    const uint64_t lanes = (uint64_t)gridDim.x * kThreads;
    for (uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x; r < h.R; r += lanes) {  // (R <= capacity)
        const uint32_t word = w.rank[r];
        offsets[r] = offset_of_row(word, dense, w.start, w.doff, n, n_items);
        valid[r] = (uint8_t)valid_of_row(word, dense, w.desc);
    }
}

// The dense rows that can own a token of the block or start in it: the last one below `base` through the last one below
// the block's end.  The tokens ascend strictly (rows_order has seen to it), so these are at most kStaged.  s_k: 2 words, read
// behind the caller's next barrier
struct BlockRows {
    uint32_t first, count;
};
__device__ __forceinline__ void search_rows(const RowsWork &w, uint32_t dense, uint64_t base, uint32_t *s_k) {
    if (threadIdx.x == 64) s_k[0] = rows_below(w.start, dense, (uint32_t)base);
    if (threadIdx.x == 128) s_k[1] = rows_below(w.start, dense, (uint32_t)(base + kBlock));  // (base < n < 2^31)
}
__device__ __forceinline__ BlockRows block_rows(const uint32_t *s_k) {
    BlockRows b;
    b.first = s_k[0] > 0 ? s_k[0] - 1 : 0;
    b.count = s_k[1] - b.first;  // (s_k[1] >= s_k[0]: the array ascends)
    if (b.count > kStaged) b.count = kStaged;
    return b;
}

}  // namespace msj_rows
