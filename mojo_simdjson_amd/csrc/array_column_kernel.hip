// One selected path's arrays as a list column -- msj_array_column_device (include/msj_stage1.h): from the msj_field records
// msj_select_documents_device wrote for a path, offsets[D + 1], a validity byte per row and one msj_field per element back
// to back.  The arithmetic -- the row test, the descriptor, the element test, the codes -- is array_column_math.h, host +
// device and checked on the CPU by tests/test_array_column_math.py; an element's record is select_math.h's value_field.
// D = d_docs->n_complete and T = d_docs->tokens_complete are read on the device by every kernel, d_select only to be
// checked against them: the host never learns them.
//
// No walk: the arrays of one column lie in document order, so an element's place in the output is the number of element
// tokens in front of it in the window, and offsets[k] is that number at document k's first token.  Launches, all on the
// caller's stream, behind a 64-byte memset of the call's counters:
//   ac_rows   a lane per row: the 16-byte record as one load, the row test, d_valid, and a 16-byte descriptor {v, m, depth of
//             v's children} to the workspace, so that a candidate token makes one gather; the counts by wave and block, two
//             atomics per block
//   ac_count  a block of 1 024 tokens, 4 per lane; the type word as one 4-byte load, the depths as one 16-byte load, one
//             token of halo in FRONT of the block for the predecessor.  A candidate (behind '[' or ',', no closer) finds its
//             document as td_emit does (docs_block.h) and tests itself against that document's descriptor.  The block's
//             element count goes to the workspace; a block without a candidate writes its 0 and ends there
//   ac_scan   one workgroup of 1 024: the exclusive sum over the blocks' counts in chunks of 1 024, then the result -- the
//             code, n_elements, the counts --, d_offsets[D] and d_elements_select
//   ac_emit   the same block shape.  An element's position is the block's prefix + the exclusive sum inside the block; its
//             record leaves as one 16-byte store when the position is below elements_capacity.  The lane that holds a
//             document's first token writes d_offsets[k], also in a block that holds no element.  n_no_bits: one atomic per
//             block that has any
// Safety: a row's token is used only when it lies in its document; every index from d_match or d_doc_first is checked before
// it is used; tokens are below T <= n; rows are below D <= capacity; every store to d_elements is checked against
// elements_capacity.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "array_column_math.h"
#include "launch.h"
#include "list_block.h"

namespace msj_acol {

using namespace msj_list;
using namespace msj::acol;

static_assert(sizeof(msj_field) == 16 && sizeof(msj_array_column_result) == 48 && sizeof(Desc) == 16, "ABI");

struct ColState {  // cleared by a memset per call
    uint64_t n_arrays, n_other;
    uint64_t reserved[6];
};
struct ColWork {
    ColState *st;
    Desc *desc;       // per row
    uint32_t *bsum;   // per block of tokens: its elements, then (ac_scan) the elements in front of the block
};

__host__ __device__ inline uint64_t most_rows(uint64_t n, uint64_t capacity) { return n < capacity ? n : capacity; }
static inline ColWork col_layout(msj_carver &c, uint64_t n, uint64_t capacity) {
    ColWork w;
    w.st = c.take<ColState>(1);
    w.desc = c.take<Desc>(most_rows(n, capacity));
    w.bsum = c.take<uint32_t>(token_blocks(n));
    return w;
}

// what every kernel reads of the window and of d_select.  stop: nothing but the results is written
struct Head {
    Window win;
    uint64_t n_rows;
    int32_t code;
    bool stop;
};
__device__ __forceinline__ Head load_head(const msj_documents_result *__restrict__ docs, const uint32_t *__restrict__ first, uint64_t n,
                                          uint64_t capacity, const msj_select_documents_result *__restrict__ sel) {
    Head h;
    h.win = load_window(docs, first, n, capacity);
    h.code = head_code(sel->code, sel->n_documents, h.win, h.n_rows);
    h.stop = h.code != 0;
    return h;
}

__global__ __launch_bounds__(kThreads) void ac_rows(uint64_t n, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                    const uint32_t *__restrict__ match, const uint32_t *__restrict__ first,
                                                    const msj_documents_result *__restrict__ docs, const msj_field *__restrict__ column,
                                                    const msj_select_documents_result *__restrict__ sel, uint64_t capacity, const ColWork w,
                                                    uint8_t *__restrict__ valid) {
    __shared__ uint32_t s_arrays[kWaves], s_other[kWaves];
    const Head h = load_head(docs, first, n, capacity, sel);
    if (h.stop) return;
    const uint64_t lanes = (uint64_t)gridDim.x * kThreads;
    uint32_t n_arrays = 0, n_other = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < h.win.D; k += lanes) {
        uint64_t f, e;
        const bool ok = document_bounds(first, h.win, k, f, e);
        bool other;
        const Desc d = row_of(load_field(column, k), ok, f, e, type, depth, match, other);
        valid[k] = (uint8_t)d.valid;  // (k < D <= capacity)
        *reinterpret_cast<uint4 *>(w.desc + k) = make_uint4(d.v, d.m, (uint32_t)d.child_depth, d.valid);
        n_arrays += d.valid, n_other += other;
    }
    (void)block_counter_add(n_arrays, s_arrays, &w.st->n_arrays);
    (void)block_counter_add(n_other, s_other, &w.st->n_other);
}

// a lane's tokens and its candidates (list_block.h): tokens at or past T read as nothing, they belong to the cut document
__device__ __forceinline__ Lane load_lane(const Window &win, uint64_t base, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                          uint32_t *s_type) {
    return load_lane_front(win.T, base, type, depth, s_type, [&win](uint64_t i) { return in_documents(win, i); });
}
// the candidates that are elements of their document's row: one 16-byte gather each
__device__ __forceinline__ uint32_t elements_of(const Lane &l, const BlockDocs &bd, const Window &win, uint64_t base, const Desc *__restrict__ desc) {
    const uint64_t mine = base + (uint64_t)threadIdx.x * kPer;
    uint32_t elem = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        if (!((l.cand >> k) & 1u)) continue;
        const uint64_t doc = (uint64_t)bd.k0 + bd.rank[k];  // 1 + the document's number
        if (doc == 0 || doc > win.D) continue;               // (<= capacity)
        const uint4 q = *reinterpret_cast<const uint4 *>(desc + (doc - 1));
        const Desc d{q.x, q.y, (int32_t)q.z, q.w};
        if (is_element_of(mine + k, l.t.dk[k], d)) elem |= 1u << k;
    }
    return elem;
}

__global__ __launch_bounds__(kThreads) void ac_count(uint64_t n, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                     const uint32_t *__restrict__ first, const msj_documents_result *__restrict__ docs,
                                                     const msj_select_documents_result *__restrict__ sel, uint64_t capacity, const ColWork w) {
    __shared__ uint32_t s_type[kThreads], s_flag[kThreads], s_k[2], s_w32[kWaves];
    const Head h = load_head(docs, first, n, capacity, sel);
    const uint64_t base = (uint64_t)blockIdx.x * kBlock;
    if (h.stop || base >= h.win.T) return;
    const Lane l = load_lane(h.win, base, type, depth, s_type);
    if (!__syncthreads_or((int)l.cand)) {  // (the whole block: no value behind '[' or ',' in it)
        if (threadIdx.x == 0) w.bsum[blockIdx.x] = 0;
        return;
    }
    const BlockDocs bd = block_docs(first, h.win, base, s_flag, s_k, s_w32);
    const uint32_t elem = elements_of(l, bd, h.win, base, w.desc);
    uint32_t total;
    (void)block_scan((uint32_t)__popc(elem), s_w32, total);
    if (threadIdx.x == 0) w.bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void ac_scan(uint64_t n, const uint32_t *__restrict__ first, const msj_documents_result *__restrict__ docs,
                                                const msj_select_documents_result *__restrict__ sel, uint64_t capacity, const ColWork w,
                                                uint64_t *__restrict__ offsets, bool have_elements, uint64_t elements_capacity,
                                                msj_array_column_result *__restrict__ result,
                                                msj_select_documents_result *__restrict__ elements_select) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(docs, first, n, capacity, sel);
    const uint64_t blocks = h.stop ? 0 : token_blocks(h.win.T);
    const uint64_t run = scan_in_place(w.bsum, blocks, s_w);  // (fewer elements than tokens: a prefix is below 2^31)
    if (threadIdx.x != 0) return;
    msj_array_column_result r;
    r.code = h.stop ? h.code : elements_code(run, have_elements, elements_capacity);
    r.flags = 0;
    r.n_rows = h.n_rows;
    r.n_arrays = h.stop ? 0 : w.st->n_arrays;
    r.n_elements = run;
    r.n_other = h.stop ? 0 : w.st->n_other;
    r.n_no_bits = 0;  // (ac_emit's)
    *result = r;
    if (!h.stop && offsets) offsets[h.win.D] = run;  // (NULL only with capacity 0: D is 0 then)
    if (elements_select) *elements_select = items_select(r.code, run);
}

__global__ __launch_bounds__(kThreads) void ac_emit(const uint32_t *__restrict__ idx, uint64_t n, const uint8_t *__restrict__ type,
                                                    const int32_t *__restrict__ depth, const uint32_t *__restrict__ match,
                                                    const uint32_t *__restrict__ end, const uint8_t *__restrict__ flags,
                                                    const uint32_t *__restrict__ first, const msj_documents_result *__restrict__ docs,
                                                    const msj_number *__restrict__ numbers, uint64_t numbers_capacity,
                                                    const msj_numbers_result *__restrict__ nr, const msj_select_documents_result *__restrict__ sel,
                                                    uint64_t capacity, const ColWork w, uint64_t *__restrict__ offsets,
                                                    msj_field *__restrict__ elements, uint64_t elements_capacity,
                                                    msj_array_column_result *__restrict__ result,
                                                    msj_select_documents_result *__restrict__ elements_select) {
    __shared__ uint32_t s_type[kThreads], s_flag[kThreads], s_k[2], s_w32[kWaves];
    const Head h = load_head(docs, first, n, capacity, sel);
    const uint64_t base = (uint64_t)blockIdx.x * kBlock;
    if (h.stop || base >= h.win.T) return;
    const Lane l = load_lane(h.win, base, type, depth, s_type);
    // (no exit for a block without a candidate: the documents that start in it still need their offsets)
    const BlockDocs bd = block_docs(first, h.win, base, s_flag, s_k, s_w32);
    const uint32_t elem = elements_of(l, bd, h.win, base, w.desc);
    uint32_t total;
    uint64_t pos = (uint64_t)w.bsum[blockIdx.x] + block_scan((uint32_t)__popc(elem), s_w32, total);
    const NumberRecords rec = number_records(numbers, numbers_capacity, nr);
    const uint64_t mine = base + (uint64_t)threadIdx.x * kPer;
    uint32_t n_nobits = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        if ((bd.starts >> k) & 1u) {
            const uint64_t doc = (uint64_t)bd.k0 + bd.rank[k];
            if (doc >= 1 && doc <= h.win.D) offsets[doc - 1] = pos;  // (D <= capacity; a first token is no element)
        }
        if (!((elem >> k) & 1u)) continue;
        if (elements && pos < elements_capacity) {
            const msj_field r = value_field<msj_field, msj_number>(mine + k, idx, type, match, end, flags, rec.records, rec.n);
            store_field(elements, pos, r);
            n_nobits += (r.flags & kFieldNoBits) != 0;
        }
        pos++;
    }
    if (!elements || !__syncthreads_or((int)n_nobits)) return;
    // (s_w32 is free: the scan's reads lie in front of that barrier)
    const uint32_t all = block_counter_add(n_nobits, s_w32, &result->n_no_bits);
    if (all && elements_select) atomicAdd(reinterpret_cast<unsigned long long *>(&elements_select->n_no_bits), (unsigned long long)all);
}

}  // namespace msj_acol

extern "C" uint64_t msj_array_column_workspace_bytes(uint64_t n, uint64_t capacity) { return msj_measure(msj_acol::col_layout, n, capacity) + 64; }

extern "C" int msj_launch_array_column(const msj_token_view &t, const msj_split_view &sp, const msj_number_view &nv, const msj_field *d_column,
                                       const msj_select_documents_result *d_select, uint64_t *d_offsets, uint8_t *d_valid, uint64_t capacity,
                                       msj_field *d_elements, uint64_t elements_capacity, msj_array_column_result *d_result,
                                       msj_select_documents_result *d_elements_select, void *d_ws, void *stream) {
    using namespace msj_acol;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t n = t.n;
    const ColWork w = msj_place(col_layout, d_ws, n, capacity);
    const hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(ColState), s);
    if (cleared != hipSuccess) return (int)cleared;
    const uint32_t rb = row_grid_blocks(most_rows(n, capacity)), nb = (uint32_t)token_blocks(n);
    if (rb)
        hipLaunchKernelGGL(ac_rows, dim3(rb), dim3(kThreads), 0, s, n, t.d_type, t.d_depth, t.d_match, sp.d_doc_first, sp.d_docs, d_column, d_select,
                           capacity, w, d_valid);
    if (nb) hipLaunchKernelGGL(ac_count, dim3(nb), dim3(kThreads), 0, s, n, t.d_type, t.d_depth, sp.d_doc_first, sp.d_docs, d_select, capacity, w);
    hipLaunchKernelGGL(ac_scan, dim3(1), dim3(1024), 0, s, n, sp.d_doc_first, sp.d_docs, d_select, capacity, w, d_offsets, d_elements != nullptr,
                       elements_capacity, d_result, d_elements_select);
    if (nb)
        hipLaunchKernelGGL(ac_emit, dim3(nb), dim3(kThreads), 0, s, t.d_idx, n, t.d_type, t.d_depth, t.d_match, t.d_end, t.d_flags, sp.d_doc_first,
                           sp.d_docs, nv.d_numbers, nv.numbers_capacity, nv.d_numbers_result, d_select, capacity, w, d_offsets, d_elements,
                           elements_capacity, d_result, d_elements_select);
    return (int)hipGetLastError();
}
