// Fields by path inside the elements of a list column -- msj_select_elements_device (include/msj_stage1.h):
// msj_select_documents_device's lookup with the element records of msj_array_column_device as the rows, so that
// items[*].sku is a column aligned with the list column's offsets.  The arithmetic that is new -- the call's verdict on its
// rows, the order test, the state a row starts from, the row of a key, the member test against the object's own depth -- is
// select_elements_math.h, host + device and checked on the CPU by tests/test_select_elements_math.py; the state words, the
// key compare, the unescape, the number search and the record are select_math.h's.  R = d_rows_select->n_documents is read on
// the device by every kernel: the host never learns it.
//
// select_kernel.hip's shape, the shared steps in select_block.h: one pass over the window per path LEVEL, one uint32 of
// state per (path, row), atomicMin for "the first match wins".  What differs: a row starts anywhere and at any depth, so
// there is no depth filter over the window, and a key finds its row among the rows' start tokens instead of among the
// documents' first tokens.  Launches, all on the caller's stream, behind a memset of d_result:
//   se_init    per (p, r): state 0 -- the record's code, the row's own token for "", its object, or 17 -- and the next
//              level's word "not found"; for p == 0 also the row's start token into a dense uint32 array (a search then does
//              not stride through 16-byte records) and the order test against the predecessor, which writes
//              MSJ_ERR_BAD_ARGUMENT into d_result->code.  One lane writes the result's fixed part.  Every later kernel reads
//              d_result->code and returns at once when it is not 0
//   se_level   the hot path, once per level: a block of 1 024 tokens, 4 per lane, loaded as sel_level loads them.  A
//              candidate is a string with ':' behind it.  Two searches in the dense array give the rows that can own a token
//              of the block -- the last row below `base` through the last row below the block's last token; the tokens ascend
//              strictly, so these are at most 1 024 -- and their start tokens are staged in LDS, where each candidate finds
//              its row by binary search.  A block no row reaches ends there, and so does a block that lies inside ONE row
//              when no path's object of that row reaches into it.  Then as sel_level: the state word, the member test (with
//              the depth of the object, d_depth[lo] + 1), the key compare against the level's segments staged in LDS, one
//              atomicMin per match
//   se_step    per (p, r), behind each level: sel_step with n as the bound
//   se_finish  per (p, r), coalesced along r: the record; n_found / n_no_bits by wave and block, one atomic per block
// Safety: a state word that is a token is below n; every index from a record, d_match or d_end is checked before it is used;
// rows are below R <= capacity; the window is read through ByteReader only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "launch.h"
#include "select_block.h"
#include "select_elements_math.h"

namespace msj_selem {

using namespace msj_selblock;
using namespace msj::selem;

// the two state words of (p, r): level l's in word[l & 1]; the rows' start tokens
struct Words {
    uint32_t *word[2];
    uint32_t *start;
    uint64_t stride;  // rows per path that have a state (select_elements_math.h: state_rows)
};

// the state a (path, row) starts from, from the row's record as load_field_words gives it
__device__ __forceinline__ uint32_t state_of_row(const uint4 q, uint32_t levels, uint64_t n, const uint8_t *__restrict__ type,
                                                 const uint32_t *__restrict__ match) {
    return row_state(q.w >> 16, q.w & 0xFFu, q.z, levels, n, type, match);
}

__global__ __launch_bounds__(kThreads) void se_init(const Paths *__restrict__ paths, const uint8_t *__restrict__ type,
                                                    const uint32_t *__restrict__ match, uint64_t n, const msj_field *__restrict__ rows,
                                                    const msj_select_documents_result *__restrict__ rows_select, uint64_t capacity,
                                                    const Words ws, msj_select_documents_result *__restrict__ result) {
    const uint64_t R = rows_select->n_documents;
    const uint32_t p = blockIdx.y;
    uint64_t n_rows, n_paths;
    const int32_t code = head_code(rows_select->code, R, capacity, paths->n_paths, n_rows, n_paths);
    if (blockIdx.x == 0 && p == 0 && threadIdx.x == 0) {  // (the rest of the result is the memset's)
        result->n_documents = n_rows;
        result->n_paths = n_paths;
        if (code != 0) result->code = code;
    }
    if (code != 0) return;
    const uint32_t levels = paths->levels[p];
    const uint64_t lanes = (uint64_t)gridDim.x * kThreads;
    for (uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x; r < R; r += lanes) {  // (R <= capacity)
        const uint4 q = load_field_words(rows, r);
        if (p == 0) {
            if (r > 0 && !in_order(rows[r - 1].token, q.z)) result->code = kBadArgument;  // (every writer stores the same value)
            if (r < ws.stride) ws.start[r] = q.z;
        }
        if (r >= ws.stride) continue;  // (its token is at or past n: se_finish derives its record from the row alone)
        ws.word[0][p * ws.stride + r] = state_of_row(q, levels, n, type, match);
        ws.word[1][p * ws.stride + r] = kNotFound;
    }
}

__global__ __launch_bounds__(kThreads) void se_level(const Paths *__restrict__ paths, uint32_t level, const uint8_t *__restrict__ buf,
                                                     uint64_t len, const uint32_t *__restrict__ idx, uint64_t n,
                                                     const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                     const uint32_t *__restrict__ match, const uint32_t *__restrict__ end,
                                                     const uint8_t *__restrict__ flags,
                                                     const msj_select_documents_result *__restrict__ rows_select, const Words ws,
                                                     const msj_select_documents_result *__restrict__ result) {
    __shared__ Segments s_seg;
    __shared__ uint32_t s_type[kThreads + 1];
    __shared__ uint32_t s_start[kBlock];
    __shared__ uint32_t s_k[2];
    const uint64_t base = (uint64_t)blockIdx.x * kBlock, mine = base + (uint64_t)threadIdx.x * kPer;
    const uint32_t R = (uint32_t)umin64(rows_select->n_documents, ws.stride);  // (stride <= max(n, 1) < 2^31)
    if (result->code != 0 || R == 0 || base >= n) return;
    const TokenQuad t = load_block(paths, level, type, depth, base, n, s_type, s_seg);
    // the rows that can own a token of the block: the last one below `base` through the last one below its last token
    // (behind the token loads, in front of their barrier: the searches' dependent loads run while those are in flight)
    if (threadIdx.x == 64) s_k[0] = rows_below(ws.start, R, (uint32_t)base);
    if (threadIdx.x == 128) s_k[1] = rows_below(ws.start, R, (uint32_t)(base + kBlock - 1));  // (base < n < 2^31)
    uint32_t cand;  // a candidate: a string with ':' behind it
    if (!key_candidates(t, base, n, s_type, cand, [](uint64_t, uint32_t ty, uint32_t t_next, int32_t) { return is_key(ty, t_next); })) return;
    const uint32_t first = s_k[0] > 0 ? s_k[0] - 1 : 0;
    uint32_t count = s_k[1] - first;  // (s_k[1] >= s_k[0]: the array ascends, se_init has seen to it)
    if (count == 0) return;           // no row starts in front of the block's last token
    if (count > kBlock) count = kBlock;  // (strictly ascending tokens: at most 1 023 start inside the block, and one in front)
    const uint32_t n_paths = paths->n_paths;
    if (count == 1) {  // the block lies inside one row (or behind the last one): does any path's object reach into it
        int live = 0;
        if (threadIdx.x < n_paths && s_seg.len[threadIdx.x] != kNoLevel) {
            const uint32_t lo = ws.word[level & 1][threadIdx.x * ws.stride + first];
            if (state_is_token(lo)) {
                const uint32_t m = match[lo];  // (a token state is below n)
                live = m != kNoPartner && (uint64_t)m > base && (uint64_t)m > (uint64_t)lo;
            }
        }
        if (!__syncthreads_or(live)) return;
    }
    for (uint32_t x = threadIdx.x; x < count; x += kThreads) s_start[x] = ws.start[first + x];
    stage_segments(paths, level, s_seg);
    __syncthreads();
    const ByteReader r{buf, len};
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        if (!((cand >> k) & 1u)) continue;
        const uint64_t i = mine + k;
        const uint32_t below = rows_below(s_start, count, (uint32_t)i);
        if (below == 0) continue;  // in front of the first row
        match_key(r, idx, match, end, flags, i, (uint64_t)first + below - 1, n_paths, level, s_seg, ws,
                  [&](uint32_t lo, uint32_t m) { return is_direct_member(i, t.dk[k], lo, depth[lo], m); });
    }
}

__global__ __launch_bounds__(kThreads) void se_step(const Paths *__restrict__ paths, uint32_t level, const uint8_t *__restrict__ type,
                                                    const uint32_t *__restrict__ match, uint64_t n,
                                                    const msj_select_documents_result *__restrict__ rows_select, const Words ws,
                                                    const msj_select_documents_result *__restrict__ result) {
    if (result->code != 0) return;
    step_rows(paths, level, type, match, ws, umin64(rows_select->n_documents, ws.stride), [&](uint64_t) { return n; });
}

__global__ __launch_bounds__(kThreads) void se_finish(const Paths *__restrict__ paths, const uint32_t *__restrict__ idx, uint64_t n,
                                                      const uint8_t *__restrict__ type, const uint32_t *__restrict__ match,
                                                      const uint32_t *__restrict__ end, const uint8_t *__restrict__ flags,
                                                      const msj_number *__restrict__ numbers, uint64_t numbers_capacity,
                                                      const msj_numbers_result *__restrict__ nr, const msj_field *__restrict__ rows,
                                                      const msj_select_documents_result *__restrict__ rows_select, const Words ws,
                                                      msj_field *__restrict__ fields, uint64_t capacity,
                                                      msj_select_documents_result *__restrict__ result) {
    const uint64_t R = rows_select->n_documents;
    if (result->code != 0 || R == 0) return;
    const uint32_t levels = paths->levels[blockIdx.y];
    const uint32_t *word = ws.word[levels & 1] + blockIdx.y * ws.stride;
    // (a row at or past the stride names no token of the window: the record's code, or 17)
    finish_rows(idx, type, match, end, flags, number_records(numbers, numbers_capacity, nr), R, fields, capacity, result, [&](uint64_t r) {
        return r < ws.stride ? word[r] : state_of_row(load_field_words(rows, r), levels, n, type, match);
    });
}

static inline Words words_layout(msj_carver &c, uint64_t n, uint64_t capacity, uint32_t n_paths) {
    Words ws;
    ws.stride = state_rows(n, capacity);
    for (int b = 0; b < 2; b++) ws.word[b] = c.take<uint32_t>((uint64_t)n_paths * ws.stride, 4);
    ws.start = c.take<uint32_t>(ws.stride, 4);
    return ws;
}

}  // namespace msj_selem

extern "C" uint64_t msj_select_elements_workspace_bytes(uint64_t n, uint64_t capacity, uint32_t n_paths) {
    return msj_measure(msj_selem::words_layout, n, capacity, n_paths) + 64;
}

extern "C" int msj_launch_select_elements(const void *d_paths, uint32_t n_paths, uint32_t max_levels, const msj_token_view &t,
                                          const msj_number_view &nv, const msj_field *d_rows, const msj_select_documents_result *d_rows_select,
                                          msj_field *d_fields, uint64_t capacity, msj_select_documents_result *d_result, void *d_ws,
                                          void *stream) {
    using namespace msj_selem;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Paths *paths = static_cast<const Paths *>(d_paths);
    const hipError_t cleared = hipMemsetAsync(d_result, 0, sizeof(msj_select_documents_result), s);
    if (cleared != hipSuccess) return (int)cleared;
    const Words ws = msj_place(words_layout, d_ws, t.n, capacity, n_paths);
    const dim3 row_grid(row_grid_blocks(ws.stride), n_paths);  // (the kernels over rows loop: rows past n need no larger grid)
    hipLaunchKernelGGL(se_init, row_grid, dim3(kThreads), 0, s, paths, t.d_type, t.d_match, t.n, d_rows, d_rows_select, capacity, ws, d_result);
    const uint32_t nb = (uint32_t)((t.n + kBlock - 1) / kBlock);
    for (uint32_t l = 0; l < max_levels; l++) {
        if (nb)  // (no token: no key, and the states -- every row's is a code then -- still step to the word se_finish reads)
            hipLaunchKernelGGL(se_level, dim3(nb), dim3(kThreads), 0, s, paths, l, t.d_buf, t.len, t.d_idx, t.n, t.d_type, t.d_depth, t.d_match,
                               t.d_end, t.d_flags, d_rows_select, ws, d_result);
        hipLaunchKernelGGL(se_step, row_grid, dim3(kThreads), 0, s, paths, l, t.d_type, t.d_match, t.n, d_rows_select, ws, d_result);
    }
    hipLaunchKernelGGL(se_finish, row_grid, dim3(kThreads), 0, s, paths, t.d_idx, t.n, t.d_type, t.d_match, t.d_end, t.d_flags, nv.d_numbers,
                       nv.numbers_capacity, nv.d_numbers_result, d_rows, d_rows_select, ws, d_fields, capacity, d_result);
    return (int)hipGetLastError();
}
