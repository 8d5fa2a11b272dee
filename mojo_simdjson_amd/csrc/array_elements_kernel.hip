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
//   ae_live, ae_ranks, ae_place, ae_order   the kernels over rows of rows_block.h with '[' as the container (shared with
//              object_entries_kernel.hip): the live rows counted and ranked, start[j] and the 16-byte descriptor per dense
//              row, the word {j, live} per row, n_arrays / n_other; a violation of the order sets the state's flag, and every
//              later kernel returns at once when it is set
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
//   ae_rows    rows_block.h's rows_finish: d_offsets[r] and d_valid[r] from the row's word.  Last, so that an order
//              violation leaves both untouched
// Safety: a row's token is used only when it is below n; every index from d_match is checked before it is used; dense numbers
// are below min(live rows, n, capacity); rows are below R <= capacity; every store to d_elements is checked against
// elements_capacity.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "array_elements_math.h"
#include "launch.h"
#include "rows_block.h"

namespace msj_aelem {

using namespace msj_rows;

static_assert(sizeof(msj_array_column_result) == 48, "ABI");

// the kernels over rows (rows_block.h) with '[' as the container, under the names this file's launches have always had
constexpr auto ae_live = rows_live<'['>;
constexpr auto ae_ranks = rows_ranks<'['>;
constexpr auto ae_place = rows_place<'['>;
constexpr auto ae_order = rows_order<'['>;
constexpr auto ae_rows = rows_finish<'['>;

using ElemWork = RowsWork;

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
    r.n_arrays = stop ? 0 : w.st->n_containers;
    r.n_elements = run;
    r.n_other = stop ? 0 : w.st->n_other;
    r.n_no_bits = 0;  // (ae_emit's)
    *result = r;
    w.st->n_items = run;
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
    const hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(RowsState), s);
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
