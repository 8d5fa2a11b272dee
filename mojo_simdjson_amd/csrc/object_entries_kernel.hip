// An object's members as a map column -- msj_object_entries_device (include/msj_stage1.h): msj_array_elements_device with
// objects as the rows and two records per entry, the key's and the value's, so that an object whose keys are data
// ("attrs":{"color":"red","size":"L"}, a map of maps) is a column too.  The arithmetic that is new -- the row test with '{',
// the candidate test, the entry test -- is object_entries_math.h, host + device and checked on the CPU by
// tests/test_object_entries_math.py; everything else is array_elements_math.h's and select_math.h's.  R =
// d_rows_select->n_documents is read on the device by every kernel: the host never learns it.
//
// As in array_elements_kernel.hip there is no walk and no counter per row: an entry's place in the output is the number of
// key tokens of entries in front of it in the window, a row's offset that number just behind the row's own token.  Launches,
// all on the caller's stream, behind a 64-byte memset of the call's state:
//   oe_live, oe_ranks, oe_place, oe_order   the kernels over rows of rows_block.h with '{' as the container
//   oe_count   a block of 1 024 tokens, 4 per lane; the type word as one 4-byte load, the depths as one 16-byte load, one
//              token of halo BEHIND the block (type[base + 1 024], 0 at or past n): a lane takes its successor's first type
//              byte from LDS.  A candidate is a '"' with ':' behind it; it finds its row among the staged ones by binary
//              search and tests itself against that row's descriptor, one 16-byte gather.  Ends early: a block without a
//              candidate, a block no row reaches, a block inside ONE row whose partner lies in front of it
//   oe_scan    one workgroup of 1 024: the exclusive sum over the blocks' counts, then the result, d_offsets[R] and the two
//              select results
//   oe_emit    the same block shape.  An entry's position is the block's prefix + the exclusive sum inside the block; the
//              key's record (token i) and the value's (token i + 2, gathered: it may lie in the next block) leave as one
//              16-byte store each when the position is below entries_capacity.  A staged row that starts in the block marks
//              its token in LDS; the lane that holds the token writes the dense row's offset
//   oe_rows    rows_block.h's rows_finish
// Safety: a row's token is used only when it is below n; every index from d_match is checked before it is used; an entry has
// i + 2 < m < n, so tokens i + 1 and i + 2 index the arrays; the type behind a token is read only below n; every store to
// d_keys / d_values is checked against entries_capacity.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "launch.h"
#include "object_entries_math.h"
#include "rows_block.h"

namespace msj_oent {

using namespace msj_rows;
namespace oent = msj::oent;

static_assert(sizeof(msj_object_entries_result) == 48, "ABI");

constexpr auto oe_live = rows_live<oent::kContainer>;
constexpr auto oe_ranks = rows_ranks<oent::kContainer>;
constexpr auto oe_place = rows_place<oent::kContainer>;
constexpr auto oe_order = rows_order<oent::kContainer>;
constexpr auto oe_rows = rows_finish<oent::kContainer>;

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
    l.t = load_token_quad(type, depth, mine, n);  // (tokens at or past n read as type 0)
    s_type[threadIdx.x] = l.t.tw;
    // the halo, one token behind the block: the last lane's successor
    uint32_t halo = 0;
    if (threadIdx.x == kThreads - 1 && base + kBlock < n) halo = type[base + kBlock];
    __syncthreads();
    const uint32_t behind = threadIdx.x + 1 < kThreads ? s_type[threadIdx.x + 1] & 0xFFu : halo;
    l.cand = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint32_t t = (l.t.tw >> (8 * k)) & 0xFFu;
        const uint32_t t_next = k + 1 < kPer ? (l.t.tw >> (8 * (k + 1))) & 0xFFu : behind;
        if (mine + k < n && oent::is_key_candidate(t, t_next)) l.cand |= 1u << k;
    }
    return l;
}

// the candidates that are keys of entries of their row: the row by binary search in LDS, then one 16-byte gather
__device__ __forceinline__ uint32_t entries_of(const Lane &l, const BlockRows &br, const uint32_t *s_start, uint64_t base,
                                               const Desc *__restrict__ desc) {
    const uint64_t mine = base + (uint64_t)threadIdx.x * kPer;
    uint32_t entry = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        if (!((l.cand >> k) & 1u)) continue;
        const uint32_t below = rows_below(s_start, br.count, (uint32_t)(mine + k));
        if (below == 0) continue;  // in front of the first row
        const uint4 q = *reinterpret_cast<const uint4 *>(desc + ((uint64_t)br.first + below - 1));  // (a dense number)
        const Desc d{q.x, q.y, (int32_t)q.z, q.w};
        if (oent::is_entry_of(mine + k, l.t.dk[k], d)) entry |= 1u << k;
    }
    return entry;
}

__global__ __launch_bounds__(kThreads) void oe_count(uint64_t n, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                     const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                     const RowsWork w) {
    __shared__ uint32_t s_type[kThreads], s_start[kStaged], s_k[2], s_w32[kWaves];
    const Head h = load_head(rows_select, capacity);
    const uint64_t base = (uint64_t)blockIdx.x * kBlock;
    if (h.stop || w.st->bad_order || base >= n) return;
    const uint32_t dense = dense_count(w);
    // (the searches' dependent loads run while the token loads are in flight: load_lane's barrier publishes s_k)
    search_rows(w, dense, base, s_k);
    const Lane l = load_lane(n, base, type, depth, s_type);
    const BlockRows br = block_rows(s_k);
    bool none = !__syncthreads_or((int)l.cand) || br.count == 0;  // no '"' with ':' behind it in the block, or no row reaches it
    // the block lies inside ONE row (or behind the last one): does that row's object reach into it
    if (!none && br.count == 1) none = (uint64_t)w.desc[br.first].m <= base;  // (an entry lies in front of m; no object: m = 0)
    if (none) {
        if (threadIdx.x == 0) w.bsum[blockIdx.x] = 0;
        return;
    }
    for (uint32_t x = threadIdx.x; x < br.count; x += kThreads) s_start[x] = w.start[br.first + x];
    __syncthreads();
    const uint32_t entry = entries_of(l, br, s_start, base, w.desc);
    uint32_t total;
    (void)block_scan((uint32_t)__popc(entry), s_w32, total);
    if (threadIdx.x == 0) w.bsum[blockIdx.x] = total;
}

__device__ __forceinline__ msj_select_documents_result entries_select(int32_t code, uint64_t n_entries) {
    msj_select_documents_result e;
    e.code = code;
    e.flags = 0;
    e.n_documents = e.n_found = n_entries;
    e.n_paths = 1;
    e.n_no_bits = e.reserved = 0;  // (the values': oe_emit's)
    return e;
}

__global__ __launch_bounds__(1024) void oe_scan(uint64_t n, const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                const RowsWork w, uint64_t *__restrict__ offsets, bool have_entries, uint64_t entries_capacity,
                                                msj_object_entries_result *__restrict__ result, msj_select_documents_result *__restrict__ keys_select,
                                                msj_select_documents_result *__restrict__ values_select) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(rows_select, capacity);
    const bool bad = !h.stop && w.st->bad_order != 0, stop = h.stop || bad;
    const uint64_t run = scan_in_place(w.bsum, stop ? 0 : token_blocks(n), s_w);  // (fewer entries than tokens: a prefix is below 2^31)
    if (threadIdx.x != 0) return;
    msj_object_entries_result r;
    r.code = h.stop ? h.code : bad ? kBadArgument : oent::entries_code(run, have_entries, entries_capacity);
    r.flags = 0;
    r.n_rows = h.n_rows;
    r.n_objects = stop ? 0 : w.st->n_containers;
    r.n_entries = run;
    r.n_other = stop ? 0 : w.st->n_other;
    r.n_no_bits = 0;  // (oe_emit's)
    *result = r;
    w.st->n_items = run;
    if (!stop && offsets) offsets[h.R] = run;  // (NULL only with capacity 0: R is 0 then)
    if (keys_select) *keys_select = entries_select(r.code, run);
    if (values_select) *values_select = entries_select(r.code, run);
}

__global__ __launch_bounds__(kThreads) void oe_emit(const uint32_t *__restrict__ idx, uint64_t n, const uint8_t *__restrict__ type,
                                                    const int32_t *__restrict__ depth, const uint32_t *__restrict__ match,
                                                    const uint32_t *__restrict__ end, const uint8_t *__restrict__ flags,
                                                    const msj_number *__restrict__ numbers, uint64_t numbers_capacity,
                                                    const msj_numbers_result *__restrict__ nr,
                                                    const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                    const RowsWork w, msj_field *__restrict__ keys, msj_field *__restrict__ values,
                                                    uint64_t entries_capacity, msj_object_entries_result *__restrict__ result,
                                                    msj_select_documents_result *__restrict__ values_select) {
    __shared__ uint32_t s_type[kThreads], s_start[kStaged], s_mark[kBlock], s_k[2], s_w32[kWaves];
    const Head h = load_head(rows_select, capacity);
    const uint64_t base = (uint64_t)blockIdx.x * kBlock;
    if (h.stop || w.st->bad_order || base >= n) return;
    const uint32_t dense = dense_count(w);
    search_rows(w, dense, base, s_k);
    *reinterpret_cast<uint4 *>(s_mark + threadIdx.x * kPer) = make_uint4(0, 0, 0, 0);
    const Lane l = load_lane(n, base, type, depth, s_type);
    const BlockRows br = block_rows(s_k);
    if (br.count == 0) return;  // no row reaches the block: no entry, no row start
    // (no exit for a block without a candidate: the rows that start in it still need their offsets)
    for (uint32_t x = threadIdx.x; x < br.count; x += kThreads) {
        const uint32_t s = w.start[br.first + x];
        s_start[x] = s;
        const uint64_t o = (uint64_t)s - base;               // (the staged row in front of the block wraps: no mark)
        if (o < kBlock && (uint64_t)s < n) s_mark[o] = x + 1;  // 1 + the staged number of the row that starts at this token
    }
    __syncthreads();
    const uint32_t entry = entries_of(l, br, s_start, base, w.desc);
    uint32_t total;
    uint64_t pos = (uint64_t)w.bsum[blockIdx.x] + block_scan((uint32_t)__popc(entry), s_w32, total);
    const NumberRecords rec = number_records(numbers, numbers_capacity, nr);
    const uint64_t mine = base + (uint64_t)threadIdx.x * kPer;
    const uint4 mark = *reinterpret_cast<const uint4 *>(s_mark + threadIdx.x * kPer);
    const uint32_t mk[kPer] = {mark.x, mark.y, mark.z, mark.w};
    uint32_t n_nobits = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        if ((entry >> k) & 1u) {
            if (keys && pos < entries_capacity) {  // (keys and values come together: the entry point checks)
                const uint64_t i = mine + k;       // (an entry: i + 2 < m < n)
                store_field(keys, pos, value_field<msj_field, msj_number>(i, idx, type, match, end, flags, rec.records, rec.n));
                const msj_field v = value_field<msj_field, msj_number>(i + 2, idx, type, match, end, flags, rec.records, rec.n);
                store_field(values, pos, v);
                n_nobits += (v.flags & kFieldNoBits) != 0;
            }
            pos++;
        }
        // a row's own token can be the key of an entry of the row in front of it (hostile records): counted in front of the row
        if (mk[k]) w.doff[(uint64_t)br.first + mk[k] - 1] = pos;  // (a dense number)
    }
    if (!keys || !__syncthreads_or((int)n_nobits)) return;
    // (s_w32 is free: the scan's reads lie in front of that barrier)
    const uint32_t all = block_counter_add(n_nobits, s_w32, &result->n_no_bits);
    if (all && values_select) atomicAdd(reinterpret_cast<unsigned long long *>(&values_select->n_no_bits), (unsigned long long)all);
}

}  // namespace msj_oent

extern "C" uint64_t msj_object_entries_workspace_bytes(uint64_t n, uint64_t capacity) { return msj_rows::work_bytes(n, capacity); }

extern "C" int msj_launch_object_entries(const msj_token_view &t, const msj_number_view &nv, const msj_field *d_rows,
                                         const msj_select_documents_result *d_rows_select, uint64_t *d_offsets, uint8_t *d_valid,
                                         uint64_t capacity, msj_field *d_keys, msj_field *d_values, uint64_t entries_capacity,
                                         msj_object_entries_result *d_result, msj_select_documents_result *d_keys_select,
                                         msj_select_documents_result *d_values_select, void *d_ws, void *stream) {
    using namespace msj_oent;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t n = t.n;
    const RowsWork w = work_layout(d_ws, n, capacity);
    const hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(RowsState), s);
    if (cleared != hipSuccess) return (int)cleared;
    const uint32_t rb = row_grid_blocks(capacity), nb = (uint32_t)token_blocks(n);
    if (rb) {
        hipLaunchKernelGGL(oe_live, dim3(rb), dim3(kThreads), 0, s, d_rows, d_rows_select, capacity, w);
        hipLaunchKernelGGL(oe_ranks, dim3(1), dim3(1024), 0, s, d_rows_select, capacity, w);
        hipLaunchKernelGGL(oe_place, dim3(rb), dim3(kThreads), 0, s, n, t.d_type, t.d_depth, t.d_match, d_rows, d_rows_select, capacity, w);
        hipLaunchKernelGGL(oe_order, dim3(rb), dim3(kThreads), 0, s, d_rows_select, capacity, w);
    }
    if (nb && rb) hipLaunchKernelGGL(oe_count, dim3(nb), dim3(kThreads), 0, s, n, t.d_type, t.d_depth, d_rows_select, capacity, w);
    hipLaunchKernelGGL(oe_scan, dim3(1), dim3(1024), 0, s, rb ? n : 0, d_rows_select, capacity, w, d_offsets, d_keys != nullptr,
                       entries_capacity, d_result, d_keys_select, d_values_select);
    if (nb && rb)
        hipLaunchKernelGGL(oe_emit, dim3(nb), dim3(kThreads), 0, s, t.d_idx, n, t.d_type, t.d_depth, t.d_match, t.d_end, t.d_flags, nv.d_numbers,
                           nv.numbers_capacity, nv.d_numbers_result, d_rows_select, capacity, w, d_keys, d_values, entries_capacity, d_result,
                           d_values_select);
    if (rb) hipLaunchKernelGGL(oe_rows, dim3(rb), dim3(kThreads), 0, s, n, d_rows_select, capacity, w, d_offsets, d_valid);
    return (int)hipGetLastError();
}
