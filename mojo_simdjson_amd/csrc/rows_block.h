// rows_block.h -- the calls over ANY ascending msj_field records as rows (array_elements_kernel.hip,
// object_entries_kernel.hip), whole but for what tells an element from an entry: the call's state and workspace, what every
// kernel reads of d_rows_select, the five kernels over rows -- the live rows counted, ranked, placed, their order checked, and
// at the end d_offsets / d_valid written --, the search for the rows a block of tokens has to stage, the three kernels over
// blocks of tokens -- the items (elements or entries) counted, summed, written -- and the eight launches.  rows_place is a
// template over the byte a row's container opens with ('[' or '{'), the kernels over tokens over the call's policy (below);
// the other four are plain kernels, one copy in each of the two files.  Device code but for the sizes and the launches; the
// arithmetic is array_elements_math.h.
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
//   items_count, items_scan, items_emit   see below
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "array_elements_math.h"
#include "launch.h"
#include "list_block.h"

namespace msj_rows {

using namespace msj_list;
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
static inline RowsWork work_layout(msj_carver &c, uint64_t n, uint64_t capacity) {
    RowsWork w;
    w.dense = dense_rows(n, capacity);
    w.st = c.take<RowsState>(1);
    w.desc = c.take<Desc>(w.dense);
    w.doff = c.take<uint64_t>(w.dense);
    w.rsum = c.take<uint64_t>(row_blocks(capacity));
    w.rank = c.take<uint32_t>(capacity);
    w.start = c.take<uint32_t>(capacity);
    w.bsum = c.take<uint32_t>(token_blocks(n));
    return w;
}
// The size of both calls.  The sizes callers budget with have always counted doff unrounded: with an odd number of dense rows
// its 8 bytes of rounding come out of the slack
static inline uint64_t work_bytes(uint64_t n, uint64_t capacity) { return msj_measure(work_layout, n, capacity) + 64 - 8 * (dense_rows(n, capacity) & 1); }

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

static __global__ __launch_bounds__(kThreads) void rows_live(const msj_field *__restrict__ rows,
                                                             const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                             const RowsWork w) {
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

static __global__ __launch_bounds__(1024) void rows_ranks(const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                          const RowsWork w) {
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

static __global__ __launch_bounds__(kThreads) void rows_order(const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                              const RowsWork w) {
    const Head h = load_head(rows_select, capacity);
    if (h.stop) return;
    const uint64_t live = w.st->n_live, lanes = (uint64_t)gridDim.x * kThreads;  // (<= R <= capacity)
    for (uint64_t j = 1 + (uint64_t)blockIdx.x * kThreads + threadIdx.x; j < live; j += lanes)
        if (!in_order(w.start[j - 1], w.start[j])) w.st->bad_order = 1;  // (every writer stores the same value)
}

static __global__ __launch_bounds__(kThreads) void rows_finish(uint64_t n, const msj_select_documents_result *__restrict__ rows_select,
                                                               uint64_t capacity, const RowsWork w, uint64_t *__restrict__ offsets,
                                                               uint8_t *__restrict__ valid) {
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

// ---- the kernels over blocks of tokens ---------------------------------------------------------------------------------------
// No walk and no counter per row: the live rows ascend and each token belongs to one of them, so an item's place in the output
// is the number of items in front of it in the window, and a row's offset is that number just behind the row's own token.
//   items_count  a block of 1 024 tokens, 4 per lane, with the policy's one token of halo.  Two searches in start[] give the
//                rows that can own a token of the block or start in it -- at most 1 025 --, staged in LDS; a candidate finds its
//                row there by binary search and tests itself against that row's descriptor, one 16-byte gather.  Ends early: a
//                block without a candidate, a block no row reaches, a block inside ONE row whose partner lies in front of it
//   items_scan   one workgroup of 1 024: the exclusive sum over the blocks' counts, then the results and d_offsets[R]
//   items_emit   the same block shape.  An item's position is the block's prefix + the exclusive sum inside the block; its
//                record(s) leave when the position is below the capacity.  A staged row that starts in the block marks its
//                token in LDS; the lane that holds the token writes the dense row's offset, also in a block that holds no item
// What tells the two calls apart is their policy P:
//   P::kContainer                              the byte a row's container opens with
//   P::load_lane(n, base, type, depth, s_type) a lane's tokens and its candidate bits, the halo it needs included; it holds
//                                              the block's first barrier (s_type as in list_block.h)
//   P::is_item(i, depth_i, d)                  candidate i is an item of the row with descriptor d
//   P::Out                                     what the call writes besides d_offsets and d_valid, a kernel argument: the
//                                              record arrays with capacity, have() -- they are there --, the result (a
//                                              struct with n_no_bits) and no_bits_select(), the select result that counts
//                                              the records without bits too (or NULL)
//   P::store(out, pos, i, values)              the record(s) of the item at token i to position pos -> those without bits
//   P::results(out, totals)                    the call's result and the select results of its records, by items_scan
struct ItemTotals {
    int32_t stop_code;  // the code that stopped the call (d_rows_select's, or the order's); 0: none, and the policy's holds
    uint64_t n_rows, n_containers, n_items, n_other;
};
// where an item's record comes from (select_math.h: value_field)
struct ItemValues {
    const uint32_t *idx;
    const uint8_t *type;
    const uint32_t *match, *end;
    const uint8_t *flags;
    NumberRecords rec;
    __device__ __forceinline__ msj_field field(uint64_t i) const {
        return value_field<msj_field, msj_number>(i, idx, type, match, end, flags, rec.records, rec.n);
    }
};

// the candidates that are items of their row: the row by binary search in LDS, then one 16-byte gather
template <class P>
__device__ __forceinline__ uint32_t items_of(const Lane &l, const BlockRows &br, const uint32_t *s_start, uint64_t base,
                                             const Desc *__restrict__ desc) {
    const uint64_t mine = base + (uint64_t)threadIdx.x * kPer;
    uint32_t item = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        if (!((l.cand >> k) & 1u)) continue;
        const uint32_t below = rows_below(s_start, br.count, (uint32_t)(mine + k));
        if (below == 0) continue;  // in front of the first row
        const uint4 q = *reinterpret_cast<const uint4 *>(desc + ((uint64_t)br.first + below - 1));  // (a dense number)
        const Desc d{q.x, q.y, (int32_t)q.z, q.w};
        if (P::is_item(mine + k, l.t.dk[k], d)) item |= 1u << k;
    }
    return item;
}

template <class P>
__global__ __launch_bounds__(kThreads) void items_count(uint64_t n, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                        const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                        const RowsWork w) {
    __shared__ uint32_t s_type[kThreads], s_start[kStaged], s_k[2], s_w32[kWaves];
    const Head h = load_head(rows_select, capacity);
    const uint64_t base = (uint64_t)blockIdx.x * kBlock;
    if (h.stop || w.st->bad_order || base >= n) return;
    const uint32_t dense = dense_count(w);
    // (the searches' dependent loads run while the token loads are in flight: load_lane's barrier publishes s_k)
    search_rows(w, dense, base, s_k);
    const Lane l = P::load_lane(n, base, type, depth, s_type);
    const BlockRows br = block_rows(s_k);
    bool none = !__syncthreads_or((int)l.cand) || br.count == 0;  // no candidate in the block, or no row reaches it
    // the block lies inside ONE row (or behind the last one): does that row's container reach into it
    if (!none && br.count == 1) none = (uint64_t)w.desc[br.first].m <= base;  // (an item lies in front of m; no container: m = 0)
    if (none) {
        if (threadIdx.x == 0) w.bsum[blockIdx.x] = 0;
        return;
    }
    for (uint32_t x = threadIdx.x; x < br.count; x += kThreads) s_start[x] = w.start[br.first + x];
    __syncthreads();
    const uint32_t item = items_of<P>(l, br, s_start, base, w.desc);
    uint32_t total;
    (void)block_scan((uint32_t)__popc(item), s_w32, total);
    if (threadIdx.x == 0) w.bsum[blockIdx.x] = total;
}

template <class P>
__global__ __launch_bounds__(1024) void items_scan(uint64_t n, const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                   const RowsWork w, uint64_t *__restrict__ offsets, const typename P::Out out) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(rows_select, capacity);
    const bool bad = !h.stop && w.st->bad_order != 0, stop = h.stop || bad;
    const uint64_t run = scan_in_place(w.bsum, stop ? 0 : token_blocks(n), s_w);  // (fewer items than tokens: a prefix is below 2^31)
    if (threadIdx.x != 0) return;
    P::results(out, ItemTotals{h.stop ? h.code : bad ? kBadArgument : 0, h.n_rows, stop ? 0 : w.st->n_containers, run, stop ? 0 : w.st->n_other});
    w.st->n_items = run;
    if (!stop && offsets) offsets[h.R] = run;  // (NULL only with capacity 0: R is 0 then)
}

template <class P>
__global__ __launch_bounds__(kThreads) void items_emit(const uint32_t *__restrict__ idx, uint64_t n, const uint8_t *__restrict__ type,
                                                       const int32_t *__restrict__ depth, const uint32_t *__restrict__ match,
                                                       const uint32_t *__restrict__ end, const uint8_t *__restrict__ flags,
                                                       const msj_number *__restrict__ numbers, uint64_t numbers_capacity,
                                                       const msj_numbers_result *__restrict__ nr,
                                                       const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                       const RowsWork w, const typename P::Out out) {
    __shared__ uint32_t s_type[kThreads], s_start[kStaged], s_mark[kBlock], s_k[2], s_w32[kWaves];
    const Head h = load_head(rows_select, capacity);
    const uint64_t base = (uint64_t)blockIdx.x * kBlock;
    if (h.stop || w.st->bad_order || base >= n) return;
    const uint32_t dense = dense_count(w);
    search_rows(w, dense, base, s_k);
    *reinterpret_cast<uint4 *>(s_mark + threadIdx.x * kPer) = make_uint4(0, 0, 0, 0);
    const Lane l = P::load_lane(n, base, type, depth, s_type);
    const BlockRows br = block_rows(s_k);
    if (br.count == 0) return;  // no row reaches the block: no item, no row start
    // (no exit for a block without a candidate: the rows that start in it still need their offsets)
    for (uint32_t x = threadIdx.x; x < br.count; x += kThreads) {
        const uint32_t s = w.start[br.first + x];
        s_start[x] = s;
        const uint64_t o = (uint64_t)s - base;               // (the staged row in front of the block wraps: no mark)
        if (o < kBlock && (uint64_t)s < n) s_mark[o] = x + 1;  // 1 + the staged number of the row that starts at this token
    }
    __syncthreads();
    const uint32_t item = items_of<P>(l, br, s_start, base, w.desc);
    uint32_t total;
    uint64_t pos = (uint64_t)w.bsum[blockIdx.x] + block_scan((uint32_t)__popc(item), s_w32, total);
    const ItemValues values{idx, type, match, end, flags, number_records(numbers, numbers_capacity, nr)};
    const uint64_t mine = base + (uint64_t)threadIdx.x * kPer;
    const uint4 mark = *reinterpret_cast<const uint4 *>(s_mark + threadIdx.x * kPer);
    const uint32_t mk[kPer] = {mark.x, mark.y, mark.z, mark.w};
    uint32_t n_nobits = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        if ((item >> k) & 1u) {
            if (out.have() && pos < out.capacity) n_nobits += P::store(out, pos, mine + k, values);
            pos++;
        }
        // a row's own token can be an item of the row in front of it (a row inside a row, hostile records): counted in front
        // of the row
        if (mk[k]) w.doff[(uint64_t)br.first + mk[k] - 1] = pos;  // (a dense number)
    }
    if (!out.have() || !__syncthreads_or((int)n_nobits)) return;
    // (s_w32 is free: the scan's reads lie in front of that barrier)
    const uint32_t all = block_counter_add(n_nobits, s_w32, &out.result->n_no_bits);
    if (all && out.no_bits_select())
        atomicAdd(reinterpret_cast<unsigned long long *>(&out.no_bits_select()->n_no_bits), (unsigned long long)all);
}

// The call's eight launches on the caller's stream, behind a 64-byte memset of its state
template <class P>
int launch_items(const msj_token_view &t, const msj_number_view &nv, const msj_field *d_rows, const msj_select_documents_result *d_rows_select,
                 uint64_t *d_offsets, uint8_t *d_valid, uint64_t capacity, const typename P::Out &out, void *d_ws, void *stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t n = t.n;
    const RowsWork w = msj_place(work_layout, d_ws, n, capacity);
    const hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(RowsState), s);
    if (cleared != hipSuccess) return (int)cleared;
    const uint32_t rb = row_grid_blocks(capacity), nb = (uint32_t)token_blocks(n);
    if (rb) {
        hipLaunchKernelGGL(rows_live, dim3(rb), dim3(kThreads), 0, s, d_rows, d_rows_select, capacity, w);
        hipLaunchKernelGGL(rows_ranks, dim3(1), dim3(1024), 0, s, d_rows_select, capacity, w);
        hipLaunchKernelGGL(rows_place<P::kContainer>, dim3(rb), dim3(kThreads), 0, s, n, t.d_type, t.d_depth, t.d_match, d_rows, d_rows_select,
                           capacity, w);
        hipLaunchKernelGGL(rows_order, dim3(rb), dim3(kThreads), 0, s, d_rows_select, capacity, w);
    }
    if (nb && rb) hipLaunchKernelGGL(items_count<P>, dim3(nb), dim3(kThreads), 0, s, n, t.d_type, t.d_depth, d_rows_select, capacity, w);
    hipLaunchKernelGGL(items_scan<P>, dim3(1), dim3(1024), 0, s, rb ? n : 0, d_rows_select, capacity, w, d_offsets, out);
    if (nb && rb)
        hipLaunchKernelGGL(items_emit<P>, dim3(nb), dim3(kThreads), 0, s, t.d_idx, n, t.d_type, t.d_depth, t.d_match, t.d_end, t.d_flags, nv.d_numbers,
                           nv.numbers_capacity, nv.d_numbers_result, d_rows_select, capacity, w, out);
    if (rb) hipLaunchKernelGGL(rows_finish, dim3(rb), dim3(kThreads), 0, s, n, d_rows_select, capacity, w, d_offsets, d_valid);
    return (int)hipGetLastError();
}

}  // namespace msj_rows
