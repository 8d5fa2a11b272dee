// Fields by path inside the elements of a list column -- msj_select_elements_device (include/msj_stage1.h):
// msj_select_documents_device's lookup with the element records of msj_array_column_device as the rows, so that
// items[*].sku is a column aligned with the list column's offsets.  The arithmetic that is new -- the call's verdict on its
// rows, the order test, the state a row starts from, the row of a key, the member test against the object's own depth -- is
// select_elements_math.h, host + device and checked on the CPU by tests/test_select_elements_math.py; the state words, the
// key compare, the unescape, the number search and the record are select_math.h's.  R = d_rows_select->n_documents is read on
// the device by every kernel: the host never learns it.
//
// select_kernel.hip's shape: one pass over the window per path LEVEL, one uint32 of state per (path, row), atomicMin for
// "the first match wins".  What differs: a row starts anywhere and at any depth, so there is no depth filter over the
// window, and a key finds its row among the rows' start tokens instead of among the documents' first tokens.  Launches, all
// on the caller's stream, behind a memset of d_result:
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
#include "docs_block.h"
#include "launch.h"
#include "select_elements_math.h"
#include "tape_block.h"
#include "wave_ops.h"

namespace msj_selem {

using namespace msj_tdocs;
using namespace msj::selem;

constexpr int kGridBlocks = 1024;  // most blocks along r of the kernels over (p, r)

static_assert(sizeof(msj_field) == 16 && sizeof(msj_select_documents_result) == 48, "ABI");

// the two state words of (p, r): level l's in word[l & 1]; the rows' start tokens
struct Words {
    uint32_t *word[2];
    uint32_t *start;
    uint64_t stride;  // rows per path that have a state (select_elements_math.h: state_rows)
};

// a row's record as one 16-byte load: .x/.y the bits, .z the token, .w type | flags << 8 | code << 16
__device__ __forceinline__ uint4 load_row(const msj_field *__restrict__ rows, uint64_t r) {
    return *reinterpret_cast<const uint4 *>(rows + r);  // (16-byte aligned: checked by the entry point)
}
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
        const uint4 q = load_row(rows, r);
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
    __shared__ uint8_t s_seg[kMaxPaths][256];
    __shared__ uint32_t s_len[kMaxPaths];
    __shared__ uint32_t s_type[kThreads + 1];
    __shared__ uint32_t s_start[kBlock];
    __shared__ uint32_t s_k[2];
    const uint64_t base = (uint64_t)blockIdx.x * kBlock, mine = base + (uint64_t)threadIdx.x * kPer;
    const uint32_t R = (uint32_t)umin64(rows_select->n_documents, ws.stride);  // (stride <= max(n, 1) < 2^31)
    if (result->code != 0 || R == 0 || base >= n) return;
    const uint32_t tw = load_byte_quad(type, mine, n);
    s_type[threadIdx.x] = tw;
    if (threadIdx.x == 0) s_type[kThreads] = load_byte_quad(type, base + kBlock, n);  // the halo: one token is needed
    int32_t dk[kPer] = {0, 0, 0, 0};
    if (mine + kPer <= n) {
        const int4 q = *reinterpret_cast<const int4 *>(depth + mine);
        dk[0] = q.x, dk[1] = q.y, dk[2] = q.z, dk[3] = q.w;
    } else {
        for (int k = 0; k < kPer && mine + k < n; k++) dk[k] = depth[mine + k];
    }
    if (threadIdx.x < kMaxPaths) s_len[threadIdx.x] = threadIdx.x < paths->n_paths ? paths->len[level][threadIdx.x] : kNoLevel;
    // the rows that can own a token of the block: the last one below `base` through the last one below its last token
    if (threadIdx.x == 64) s_k[0] = rows_below(ws.start, R, (uint32_t)base);
    if (threadIdx.x == 128) s_k[1] = rows_below(ws.start, R, (uint32_t)(base + kBlock - 1));  // (base < n < 2^31)
    __syncthreads();
    const uint32_t behind = s_type[threadIdx.x + 1];
    uint32_t cand = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint64_t i = mine + k;
        const uint32_t t = (tw >> (8 * k)) & 0xFFu, t_next = k + 1 < kPer ? (tw >> (8 * (k + 1))) & 0xFFu : behind & 0xFFu;
        if (i < n && is_key(t, t_next)) cand |= 1u << k;
    }
    if (!__syncthreads_or((int)cand)) return;  // (the whole block: no key in it)
    const uint32_t first = s_k[0] > 0 ? s_k[0] - 1 : 0;
    uint32_t count = s_k[1] - first;  // (s_k[1] >= s_k[0]: the array ascends, se_init has seen to it)
    if (count == 0) return;           // no row starts in front of the block's last token
    if (count > kBlock) count = kBlock;  // (strictly ascending tokens: at most 1 023 start inside the block, and one in front)
    const uint32_t n_paths = paths->n_paths;
    const uint32_t *at = ws.word[level & 1];
    uint32_t *found = ws.word[(level + 1) & 1];
    if (count == 1) {  // the block lies inside one row (or behind the last one): does any path's object reach into it
        int live = 0;
        if (threadIdx.x < n_paths && s_len[threadIdx.x] != kNoLevel) {
            const uint32_t lo = at[threadIdx.x * ws.stride + first];
            if (state_is_token(lo)) {
                const uint32_t m = match[lo];  // (a token state is below n)
                live = m != kNoPartner && (uint64_t)m > base && (uint64_t)m > (uint64_t)lo;
            }
        }
        if (!__syncthreads_or(live)) return;
    }
    for (uint32_t x = threadIdx.x; x < count; x += kThreads) s_start[x] = ws.start[first + x];
    for (uint32_t p = 0; p < n_paths; p++) {
        const uint32_t sl = s_len[p];
        if (sl != kNoLevel)
            for (uint32_t x = threadIdx.x; x < sl; x += kThreads) s_seg[p][x] = paths->bytes[level][p][x];
    }
    __syncthreads();
    const ByteReader r{buf, len};
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        if (!((cand >> k) & 1u)) continue;
        const uint64_t i = mine + k;
        const uint32_t below = rows_below(s_start, count, (uint32_t)i);
        if (below == 0) continue;  // in front of the first row
        const uint64_t row = (uint64_t)first + below - 1;
        const uint64_t b = (uint64_t)idx[i] + 1, q = end[i];
        const bool escaped = (flags[i] & kSpanEscaped) != 0;
        if (q < b || q > len) continue;  // not what the span call writes: never read
        for (uint32_t p = 0; p < n_paths; p++) {
            const uint32_t sl = s_len[p];
            if (sl == kNoLevel || !length_may_match(q - b, escaped, sl)) continue;
            const uint64_t w = p * ws.stride + row;
            const uint32_t lo = at[w];
            if (!state_is_token(lo) || !is_direct_member(i, dk[k], lo, depth[lo], match[lo])) continue;  // (a token state is below n)
            if (key_equals(r, b, q, escaped, s_seg[p], sl)) atomicMin(found + w, (uint32_t)i);
        }
    }
}

__global__ __launch_bounds__(kThreads) void se_step(const Paths *__restrict__ paths, uint32_t level, const uint8_t *__restrict__ type,
                                                    const uint32_t *__restrict__ match, uint64_t n,
                                                    const msj_select_documents_result *__restrict__ rows_select, const Words ws,
                                                    const msj_select_documents_result *__restrict__ result) {
    const uint32_t p = blockIdx.y, levels = paths->levels[p];
    if (result->code != 0 || levels <= level) return;  // (the path ended at or in front of this level: its word stays)
    const uint64_t R = umin64(rows_select->n_documents, ws.stride);
    uint32_t *at = ws.word[level & 1], *next = ws.word[(level + 1) & 1];
    const uint64_t lanes = (uint64_t)gridDim.x * kThreads;
    for (uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x; r < R; r += lanes) {
        const uint64_t w = p * ws.stride + r;
        next[w] = next_state(at[w], next[w], levels == level + 1, n, type, match);
        if (levels > level + 1) at[w] = kNotFound;  // the word of level + 2
    }
}

__global__ __launch_bounds__(kThreads) void se_finish(const Paths *__restrict__ paths, const uint32_t *__restrict__ idx, uint64_t n,
                                                      const uint8_t *__restrict__ type, const uint32_t *__restrict__ match,
                                                      const uint32_t *__restrict__ end, const uint8_t *__restrict__ flags,
                                                      const msj_number *__restrict__ numbers, uint64_t numbers_capacity,
                                                      const msj_numbers_result *__restrict__ nr, const msj_field *__restrict__ rows,
                                                      const msj_select_documents_result *__restrict__ rows_select, const Words ws,
                                                      msj_field *__restrict__ fields, uint64_t capacity,
                                                      msj_select_documents_result *__restrict__ result) {
    __shared__ uint32_t w_found[kWaves], w_nobits[kWaves];
    const uint64_t R = rows_select->n_documents;
    if (result->code != 0 || R == 0) return;
    const uint32_t p = blockIdx.y, levels = paths->levels[p];
    const uint32_t *word = ws.word[levels & 1];
    uint64_t n_records = 0;
    if (numbers && nr) n_records = umin64(nr->n_numbers, numbers_capacity);
    const msj_number *records = n_records ? numbers : nullptr;
    const uint64_t lanes = (uint64_t)gridDim.x * kThreads;
    uint32_t n_found = 0, n_nobits = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x; r < R; r += lanes) {
        // (a row at or past the stride names no token of the window: the record's code, or 17)
        const uint32_t s = r < ws.stride ? word[p * ws.stride + r] : state_of_row(load_row(rows, r), levels, n, type, match);
        const msj_field f = field_of_state<msj_field, msj_number>(s, idx, type, match, end, flags, records, n_records);
        fields[p * capacity + r] = f;  // (r < R <= capacity)
        n_found += f.code == 0;
        n_nobits += (f.flags & kFieldNoBits) != 0;
    }
    n_found = wave_sum(n_found), n_nobits = wave_sum(n_nobits);
    if ((threadIdx.x & 63) == 0) w_found[threadIdx.x >> 6] = n_found, w_nobits[threadIdx.x >> 6] = n_nobits;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int v = 1; v < kWaves; v++) n_found += w_found[v], n_nobits += w_nobits[v];
    if (n_found) atomicAdd(reinterpret_cast<unsigned long long *>(&result->n_found), (unsigned long long)n_found);
    if (n_nobits) atomicAdd(reinterpret_cast<unsigned long long *>(&result->n_no_bits), (unsigned long long)n_nobits);
}

}  // namespace msj_selem

extern "C" uint64_t msj_select_elements_workspace_bytes(uint64_t n, uint64_t capacity, uint32_t n_paths) {
    return (2ull * 4ull * n_paths + 4ull) * msj::selem::state_rows(n, capacity) + 64;
}

extern "C" int msj_launch_select_elements(const void *d_paths, uint32_t n_paths, uint32_t max_levels, const uint8_t *d_buf, uint64_t len,
                                          const uint32_t *d_idx, uint64_t n, const uint8_t *d_type, const int32_t *d_depth,
                                          const uint32_t *d_match, const uint32_t *d_end, const uint8_t *d_flags, const msj_number *d_numbers,
                                          uint64_t numbers_capacity, const msj_numbers_result *d_numbers_result, const msj_field *d_rows,
                                          const msj_select_documents_result *d_rows_select, msj_field *d_fields, uint64_t capacity,
                                          msj_select_documents_result *d_result, void *d_ws, void *stream) {
    using namespace msj_selem;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Paths *paths = static_cast<const Paths *>(d_paths);
    const hipError_t cleared = hipMemsetAsync(d_result, 0, sizeof(msj_select_documents_result), s);
    if (cleared != hipSuccess) return (int)cleared;
    const uint64_t most = state_rows(n, capacity);
    Words ws;
    ws.word[0] = static_cast<uint32_t *>(d_ws);
    ws.word[1] = ws.word[0] + (uint64_t)n_paths * most;
    ws.start = ws.word[1] + (uint64_t)n_paths * most;
    ws.stride = most;
    const uint64_t gb = (most + kThreads - 1) / kThreads;  // (the kernels over rows loop: rows past n need no larger grid)
    const dim3 row_grid((uint32_t)(gb > (uint64_t)kGridBlocks ? (uint64_t)kGridBlocks : gb), n_paths);
    hipLaunchKernelGGL(se_init, row_grid, dim3(kThreads), 0, s, paths, d_type, d_match, n, d_rows, d_rows_select, capacity, ws, d_result);
    const uint32_t nb = (uint32_t)((n + kBlock - 1) / kBlock);
    for (uint32_t l = 0; l < max_levels; l++) {
        if (nb)  // (no token: no key, and the states -- every row's is a code then -- still step to the word se_finish reads)
            hipLaunchKernelGGL(se_level, dim3(nb), dim3(kThreads), 0, s, paths, l, d_buf, len, d_idx, n, d_type, d_depth, d_match, d_end, d_flags,
                               d_rows_select, ws, d_result);
        hipLaunchKernelGGL(se_step, row_grid, dim3(kThreads), 0, s, paths, l, d_type, d_match, n, d_rows_select, ws, d_result);
    }
    hipLaunchKernelGGL(se_finish, row_grid, dim3(kThreads), 0, s, paths, d_idx, n, d_type, d_match, d_end, d_flags, d_numbers, numbers_capacity,
                       d_numbers_result, d_rows, d_rows_select, ws, d_fields, capacity, d_result);
    return (int)hipGetLastError();
}
