// The arrays inside list rows as a list column -- msj_array_elements_device (include/msj_stage1.h): msj_array_column_device
// with ANY ascending msj_field records as the rows, so that a list of lists ("coordinates":[[x,y],...]) and a list inside a
// list of structs (items[*].tags) are list columns too, and the call runs on its own output to any depth.  The arithmetic
// that is new -- the verdict on the rows, the live rows, the word a row keeps, a row's offset -- is array_elements_math.h,
// host + device and checked on the CPU by tests/test_array_elements_math.py; the candidate and element tests and the
// descriptor are array_column_math.h's, the row search and the order test select_elements_math.h's, an element's record
// select_math.h's value_field.  R = d_rows_select->n_documents is read on the device by every kernel: the host never learns it.
//
// No walk and no counter per row: the live rows (records with code 0) ascend and each token belongs to one of them, so an
// element's place in the output is the number of element tokens in front of it in the window, and a row's offset is that
// number just behind the row's own token.  Launches, all on the caller's stream, behind a 64-byte memset of the call's state:
//   ae_live    a lane per row, 256 rows per block of rows: the 16-byte record as one load, the live rows of the block counted
//   ae_ranks   one workgroup of 1 024: the exclusive sum over the blocks of rows, the number of live rows
//   ae_place   a lane per row: a live row's dense number j = the live rows in front of it; start[j] = its token for every
//              live row, the 16-byte descriptor {v, m, depth of v's children, valid} for j < min(n, capacity) -- a live row
//              past that names no token --, and for EVERY row the word {j, live} the last pass reads; n_arrays / n_other by
//              wave and block, one atomic each per block
//   ae_order   start[j - 1] < start[j] over the live rows; a violation sets the state's flag, and every later kernel
//              returns at once when it is set
//   ae_count   a block of 1 024 tokens, 4 per lane; the type word as one 4-byte load, the depths as one 16-byte load, one
//              token of halo in FRONT of the block.  Two searches in start[] give the rows that can own a token of the block
//              or start in it -- at most 1 025 --, staged in LDS; a candidate (behind '[' or ',', no closer) finds its row
//              there by binary search and tests itself against that row's descriptor, one 16-byte gather.  Ends early: a
//              block without a candidate, a block no row reaches, a block inside ONE row whose partner lies in front of it
//   ae_scan    one workgroup of 1 024: the exclusive sum over the blocks' counts, then the result, d_offsets[R] and
//              d_elements_select
//   ae_emit    the same block shape.  An element's position is the block's prefix + the exclusive sum inside the block; its
//              record leaves as one 16-byte store when the position is below elements_capacity.  A staged row that starts in
//              the block marks its token in LDS; the lane that holds the token writes the dense row's offset, also in a
//              block that holds no element
//   ae_rows    a lane per row, coalesced along r: d_offsets[r] and d_valid[r] from the row's word.  Last, so that an order
//              violation leaves both untouched
// Safety: a row's token is used only when it is below n; every index from d_match is checked before it is used; dense numbers
// are below min(live rows, n, capacity); rows are below R <= capacity; every store to d_elements is checked against
// elements_capacity.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "array_elements_math.h"
#include "docs_block.h"
#include "launch.h"

namespace msj_aelem {

using namespace msj_tdocs;
using namespace msj::aelem;

static_assert(sizeof(msj_field) == 16 && sizeof(msj_array_column_result) == 48 && sizeof(Desc) == 16, "ABI");

constexpr uint32_t kRowBlock = kThreads;   // rows per block of rows: a lane each
constexpr uint32_t kStaged = kBlock + 1;   // rows a block of tokens stages: those that start in it and the one in front

struct ElemState {  // cleared by a memset per call
    uint64_t n_arrays, n_other, n_live, n_elements;
    uint32_t bad_order, pad;
    uint64_t reserved[3];
};
struct ElemWork {
    ElemState *st;
    uint64_t *rsum;    // per block of rows: its live rows, then (ae_ranks) the live rows in front of the block
    uint32_t *rank;    // per row: rank_word
    uint32_t *start;   // per live row: its token
    Desc *desc;        // per dense row
    uint64_t *doff;    // per dense row: the elements in front of it
    uint32_t *bsum;    // per block of tokens: its elements, then (ae_scan) the elements in front of the block
    uint64_t dense;    // dense_rows(n, capacity)
};

__host__ __device__ inline uint64_t row_blocks(uint64_t rows) { return (rows + kRowBlock - 1) / kRowBlock; }
__host__ __device__ inline uint64_t token_blocks(uint64_t tokens) { return (tokens + kBlock - 1) / kBlock; }
static inline uint64_t work_bytes(uint64_t n, uint64_t capacity) {
    return sizeof(ElemState) + up16(8 * row_blocks(capacity)) + 2 * up16(4 * capacity) + (sizeof(Desc) + 8) * dense_rows(n, capacity) +
           up16(4 * token_blocks(n)) + 64;
}
static inline ElemWork work_layout(void *ws, uint64_t n, uint64_t capacity) {
    uint8_t *p = static_cast<uint8_t *>(ws);
    auto take = [&](uint64_t bytes) {
        uint8_t *q = p;
        p += up16(bytes);
        return q;
    };
    ElemWork w;
    w.dense = dense_rows(n, capacity);
    w.st = reinterpret_cast<ElemState *>(take(sizeof(ElemState)));
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
// ... and, behind ae_order, of the state: the dense rows that exist
__device__ __forceinline__ uint32_t dense_count(const ElemWork &w) { return (uint32_t)umin64(w.st->n_live, w.dense); }  // (< 2^31)

__device__ __forceinline__ bool live_record(const uint4 q) { return is_live(q.w >> 16); }

__global__ __launch_bounds__(kThreads) void ae_live(const msj_field *__restrict__ rows, const msj_select_documents_result *__restrict__ rows_select,
                                                    uint64_t capacity, const ElemWork w) {
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

__global__ __launch_bounds__(1024) void ae_ranks(const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity, const ElemWork w) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(rows_select, capacity);
    if (h.stop) return;
    const uint64_t live = scan_in_place(w.rsum, row_blocks(h.R), s_w);
    if (threadIdx.x == 0) w.st->n_live = live;
}

__global__ __launch_bounds__(kThreads) void ae_place(uint64_t n, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                     const uint32_t *__restrict__ match, const msj_field *__restrict__ rows,
                                                     const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                     const ElemWork w) {
    __shared__ uint32_t s_w32[kWaves], s_arrays[kWaves], s_other[kWaves];
    const Head h = load_head(rows_select, capacity);
    if (h.stop) return;
    const uint64_t blocks = row_blocks(h.R);
    uint32_t n_arrays = 0, n_other = 0;
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
        const Desc d = row_of(f, n, type, depth, match, other);
        if (j < w.dense) *reinterpret_cast<uint4 *>(w.desc + j) = make_uint4(d.v, d.m, (uint32_t)d.child_depth, d.valid);
        n_arrays += d.valid, n_other += other;
    }
    (void)block_counter_add(n_arrays, s_arrays, &w.st->n_arrays);
    (void)block_counter_add(n_other, s_other, &w.st->n_other);
}

__global__ __launch_bounds__(kThreads) void ae_order(const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                     const ElemWork w) {
    const Head h = load_head(rows_select, capacity);
    if (h.stop) return;
    const uint64_t live = w.st->n_live, lanes = (uint64_t)gridDim.x * kThreads;  // (<= R <= capacity)
    for (uint64_t j = 1 + (uint64_t)blockIdx.x * kThreads + threadIdx.x; j < live; j += lanes)
        if (!in_order(w.start[j - 1], w.start[j])) w.st->bad_order = 1;  // (every writer stores the same value)
}

// A lane's four tokens of the block at `base`: types, depths and the candidates among them (bit k: token mine + k)
struct Lane {
    TokenQuad t;
    uint32_t cand;
};
// s_type: kThreads words of LDS that nothing else uses (a lane reads its neighbour's word behind the barrier)
__device__ __forceinline__ Lane load_lane(uint64_t n, uint64_t base, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                          uint32_t *s_type) {
    Lane l;
    const uint64_t mine = base + (uint64_t)threadIdx.x * kPer;
    l.t = load_token_quad(type, depth, mine, n);
    s_type[threadIdx.x] = l.t.tw;
    __syncthreads();
    // the token in front of this lane's first: the lane before's last, or the halo, one token in front of the block
    uint32_t prev = threadIdx.x > 0 ? s_type[threadIdx.x - 1] >> 24 : (base > 0 ? (uint32_t)type[base - 1] : 0u);  // (base - 1 < n)
    l.cand = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint32_t t = (l.t.tw >> (8 * k)) & 0xFFu;
        if (mine + k < n && is_candidate(prev, t)) l.cand |= 1u << k;
        prev = t;
    }
    return l;
}

// The dense rows that can own a token of the block or start in it: the last one below `base` through the last one below
// the block's end.  The tokens ascend strictly (ae_order has seen to it), so these are at most kStaged.  s_k: 2 words, read
// behind the caller's next barrier
struct BlockRows {
    uint32_t first, count;
};
__device__ __forceinline__ void search_rows(const ElemWork &w, uint32_t dense, uint64_t base, uint32_t *s_k) {
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
// the candidates that are elements of their row: the row by binary search in LDS, then one 16-byte gather
__device__ __forceinline__ uint32_t elements_of(const Lane &l, const BlockRows &br, const uint32_t *s_start, uint64_t base,
                                                const Desc *__restrict__ desc) {
    const uint64_t mine = base + (uint64_t)threadIdx.x * kPer;
    uint32_t elem = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        if (!((l.cand >> k) & 1u)) continue;
        const uint32_t below = rows_below(s_start, br.count, (uint32_t)(mine + k));
        if (below == 0) continue;  // in front of the first row
        const uint4 q = *reinterpret_cast<const uint4 *>(desc + ((uint64_t)br.first + below - 1));  // (a dense number)
        const Desc d{q.x, q.y, (int32_t)q.z, q.w};
        if (is_element_of(mine + k, l.t.dk[k], d)) elem |= 1u << k;
    }
    return elem;
}

__global__ __launch_bounds__(kThreads) void ae_count(uint64_t n, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                     const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                     const ElemWork w) {
    __shared__ uint32_t s_type[kThreads], s_start[kStaged], s_k[2], s_w32[kWaves];
    const Head h = load_head(rows_select, capacity);
    const uint64_t base = (uint64_t)blockIdx.x * kBlock;
    if (h.stop || w.st->bad_order || base >= n) return;
    const uint32_t dense = dense_count(w);
    // (the searches' dependent loads run while the token loads are in flight: load_lane's barrier publishes s_k)
    search_rows(w, dense, base, s_k);
    const Lane l = load_lane(n, base, type, depth, s_type);
    const BlockRows br = block_rows(s_k);
    bool none = !__syncthreads_or((int)l.cand) || br.count == 0;  // no value behind '[' or ',' in the block, or no row reaches it
    // the block lies inside ONE row (or behind the last one): does that row's array reach into it
    if (!none && br.count == 1) none = (uint64_t)w.desc[br.first].m <= base;  // (an element lies in front of m; no array: m = 0)
    if (none) {
        if (threadIdx.x == 0) w.bsum[blockIdx.x] = 0;
        return;
    }
    for (uint32_t x = threadIdx.x; x < br.count; x += kThreads) s_start[x] = w.start[br.first + x];
    __syncthreads();
    const uint32_t elem = elements_of(l, br, s_start, base, w.desc);
    uint32_t total;
    (void)block_scan((uint32_t)__popc(elem), s_w32, total);
    if (threadIdx.x == 0) w.bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void ae_scan(uint64_t n, const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                const ElemWork w, uint64_t *__restrict__ offsets, bool have_elements, uint64_t elements_capacity,
                                                msj_array_column_result *__restrict__ result,
                                                msj_select_documents_result *__restrict__ elements_select) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(rows_select, capacity);
    const bool bad = !h.stop && w.st->bad_order != 0, stop = h.stop || bad;
    const uint64_t run = scan_in_place(w.bsum, stop ? 0 : token_blocks(n), s_w);  // (fewer elements than tokens: a prefix is below 2^31)
    if (threadIdx.x != 0) return;
    msj_array_column_result r;
    r.code = h.stop ? h.code : bad ? kBadArgument : elements_code(run, have_elements, elements_capacity);
    r.flags = 0;
    r.n_rows = h.n_rows;
    r.n_arrays = stop ? 0 : w.st->n_arrays;
    r.n_elements = run;
    r.n_other = stop ? 0 : w.st->n_other;
    r.n_no_bits = 0;  // (ae_emit's)
    *result = r;
    w.st->n_elements = run;
    if (!stop && offsets) offsets[h.R] = run;  // (NULL only with capacity 0: R is 0 then)
    if (elements_select) {
        msj_select_documents_result e;
        e.code = r.code;
        e.flags = 0;
        e.n_documents = e.n_found = run;
        e.n_paths = 1;
        e.n_no_bits = e.reserved = 0;
        *elements_select = e;
    }
}

__global__ __launch_bounds__(kThreads) void ae_emit(const uint32_t *__restrict__ idx, uint64_t n, const uint8_t *__restrict__ type,
                                                    const int32_t *__restrict__ depth, const uint32_t *__restrict__ match,
                                                    const uint32_t *__restrict__ end, const uint8_t *__restrict__ flags,
                                                    const msj_number *__restrict__ numbers, uint64_t numbers_capacity,
                                                    const msj_numbers_result *__restrict__ nr,
                                                    const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                    const ElemWork w, msj_field *__restrict__ elements, uint64_t elements_capacity,
                                                    msj_array_column_result *__restrict__ result,
                                                    msj_select_documents_result *__restrict__ elements_select) {
    __shared__ uint32_t s_type[kThreads], s_start[kStaged], s_mark[kBlock], s_k[2], s_w32[kWaves];
    const Head h = load_head(rows_select, capacity);
    const uint64_t base = (uint64_t)blockIdx.x * kBlock;
    if (h.stop || w.st->bad_order || base >= n) return;
    const uint32_t dense = dense_count(w);
    search_rows(w, dense, base, s_k);
    *reinterpret_cast<uint4 *>(s_mark + threadIdx.x * kPer) = make_uint4(0, 0, 0, 0);
    const Lane l = load_lane(n, base, type, depth, s_type);
    const BlockRows br = block_rows(s_k);
    if (br.count == 0) return;  // no row reaches the block: no element, no row start
    // (no exit for a block without a candidate: the rows that start in it still need their offsets)
    for (uint32_t x = threadIdx.x; x < br.count; x += kThreads) {
        const uint32_t s = w.start[br.first + x];
        s_start[x] = s;
        const uint64_t o = (uint64_t)s - base;               // (the staged row in front of the block wraps: no mark)
        if (o < kBlock && (uint64_t)s < n) s_mark[o] = x + 1;  // 1 + the staged number of the row that starts at this token
    }
    __syncthreads();
    const uint32_t elem = elements_of(l, br, s_start, base, w.desc);
    uint32_t total;
    uint64_t pos = (uint64_t)w.bsum[blockIdx.x] + block_scan((uint32_t)__popc(elem), s_w32, total);
    const NumberRecords rec = number_records(numbers, numbers_capacity, nr);
    const uint64_t mine = base + (uint64_t)threadIdx.x * kPer;
    const uint4 mark = *reinterpret_cast<const uint4 *>(s_mark + threadIdx.x * kPer);
    const uint32_t mk[kPer] = {mark.x, mark.y, mark.z, mark.w};
    uint32_t n_nobits = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        if ((elem >> k) & 1u) {
            if (elements && pos < elements_capacity) {
                const msj_field r = value_field<msj_field, msj_number>(mine + k, idx, type, match, end, flags, rec.records, rec.n);
                store_field(elements, pos, r);
                n_nobits += (r.flags & kFieldNoBits) != 0;
            }
            pos++;
        }
        // a row's own token can be an element of the row in front of it (a row inside a row): counted in front of the row
        if (mk[k]) w.doff[(uint64_t)br.first + mk[k] - 1] = pos;  // (a dense number)
    }
    if (!elements || !__syncthreads_or((int)n_nobits)) return;
    // (s_w32 is free: the scan's reads lie in front of that barrier)
    const uint32_t all = block_counter_add(n_nobits, s_w32, &result->n_no_bits);
    if (all && elements_select) atomicAdd(reinterpret_cast<unsigned long long *>(&elements_select->n_no_bits), (unsigned long long)all);
}

__global__ __launch_bounds__(kThreads) void ae_rows(uint64_t n, const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                    const ElemWork w, uint64_t *__restrict__ offsets, uint8_t *__restrict__ valid) {
    const Head h = load_head(rows_select, capacity);
    if (h.stop || w.st->bad_order) return;
    const uint64_t dense = dense_count(w), n_elements = w.st->n_elements;
    const uint64_t lanes = (uint64_t)gridDim.x * kThreads;
    for (uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x; r < h.R; r += lanes) {  // (R <= capacity)
        const uint32_t word = w.rank[r];
        offsets[r] = offset_of_row(word, dense, w.start, w.doff, n, n_elements);
        valid[r] = (uint8_t)valid_of_row(word, dense, w.desc);
    }
}

}  // namespace msj_aelem

extern "C" uint64_t msj_array_elements_workspace_bytes(uint64_t n, uint64_t capacity) { return msj_aelem::work_bytes(n, capacity); }

extern "C" int msj_launch_array_elements(const msj_token_view &t, const msj_number_view &nv, const msj_field *d_rows,
                                         const msj_select_documents_result *d_rows_select, uint64_t *d_offsets, uint8_t *d_valid,
                                         uint64_t capacity, msj_field *d_elements, uint64_t elements_capacity, msj_array_column_result *d_result,
                                         msj_select_documents_result *d_elements_select, void *d_ws, void *stream) {
    using namespace msj_aelem;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t n = t.n;
    const ElemWork w = work_layout(d_ws, n, capacity);
    const hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(ElemState), s);
    if (cleared != hipSuccess) return (int)cleared;
    const uint32_t rb = row_grid_blocks(capacity), nb = (uint32_t)token_blocks(n);
    if (rb) {
        hipLaunchKernelGGL(ae_live, dim3(rb), dim3(kThreads), 0, s, d_rows, d_rows_select, capacity, w);
        hipLaunchKernelGGL(ae_ranks, dim3(1), dim3(1024), 0, s, d_rows_select, capacity, w);
        hipLaunchKernelGGL(ae_place, dim3(rb), dim3(kThreads), 0, s, n, t.d_type, t.d_depth, t.d_match, d_rows, d_rows_select, capacity, w);
        hipLaunchKernelGGL(ae_order, dim3(rb), dim3(kThreads), 0, s, d_rows_select, capacity, w);
    }
    if (nb && rb) hipLaunchKernelGGL(ae_count, dim3(nb), dim3(kThreads), 0, s, n, t.d_type, t.d_depth, d_rows_select, capacity, w);
    hipLaunchKernelGGL(ae_scan, dim3(1), dim3(1024), 0, s, rb ? n : 0, d_rows_select, capacity, w, d_offsets, d_elements != nullptr,
                       elements_capacity, d_result, d_elements_select);
    if (nb && rb)
        hipLaunchKernelGGL(ae_emit, dim3(nb), dim3(kThreads), 0, s, t.d_idx, n, t.d_type, t.d_depth, t.d_match, t.d_end, t.d_flags, nv.d_numbers,
                           nv.numbers_capacity, nv.d_numbers_result, d_rows_select, capacity, w, d_elements, elements_capacity, d_result,
                           d_elements_select);
    if (rb) hipLaunchKernelGGL(ae_rows, dim3(rb), dim3(kThreads), 0, s, n, d_rows_select, capacity, w, d_offsets, d_valid);
    return (int)hipGetLastError();
}
