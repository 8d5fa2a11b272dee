// Rows grouped by numbers, time buckets and several keys at once -- msj_bucket_rows_device and msj_group_keys_device
// (include/msj_stage1.h).  The first floors a column of number records to multiples of a width; the second lays 1 to 8
// columns -- number records, int32 codes -- out as one fixed-width, order-preserving byte key per row in the (offsets, valid,
// bytes) layout that msj_dictionary_device and msj_dictionary_extend_device read, so that the codes, the distinct keys and
// the aggregate behind them are the calls that exist.  The arithmetic -- the bucket, the parts' bytes, the codes -- is
// group_keys_math.h, host + device and checked on the CPU by tests/test_group_keys_math.py.  R is read on the device by
// every kernel: the host sizes the launches by the capacity.
//
// A block owns kRows consecutive rows -- block v the rows [v * kRows, + kRows), the grid loops over the blocks R needs.
// Launches, all on the caller's stream, behind a memset of the call's counters; no lane ever waits for another block:
//   gk_bucket  a lane per row: one 16-byte record load, the floor, one 16-byte record store (a wave's stores consecutive),
//              the five counts by a wave sum and an atomic per block where non-zero -- cast_strings_kernel.hip's cs_cast
//              without a body to read
//   gk_keys    a lane per row builds the row's W bytes in the block's LDS tile at tid * W (W is odd for most part lists, so a
//              wave's byte stores spread over the banks; an even W costs conflicts in the build and nothing in the copy); then
//              the block writes its kRows * W contiguous bytes -- its first one a multiple of 16 -- with aligned 16-byte
//              stores, lane t the 16 bytes at 16 * t, + 16 * kThreads, ...: consecutive in LDS and in memory.  The last block's
//              tail of 1 to 15 bytes leaves as byte stores, so no byte at or past R * W is touched.  The offsets (8 bytes per
//              lane) and the valid bytes are written by the row's lane, consecutive within a wave.  The two counts by a wave
//              ballot, kept per wave over the grid loop: one atomic per wave and count at the end
//   *_finish   one lane: the result (and d_out_select, d_offsets[R])
// Safety: a record or a code is read only at k < R <= stride, capacity; the bytes are written only below R * W <=
// bytes_capacity, the offsets at or below R <= capacity, the valid bytes below R.  In place (d_out == d_rows): row k is read by
// the one lane that writes it, before it writes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "bytes_block.h"
#include "group_keys_math.h"
#include "launch.h"

namespace msj_gkeys {

using namespace msj::gkeys;
using namespace msj::wave;
using msj_bytes::Head, msj_bytes::load_head;
using msj_bytes::kRows, msj_bytes::most_rows;
using msj_tape::kThreads, msj_tape::kWaves;
using msj_tdocs::load_field, msj_tdocs::store_field;

static_assert(sizeof(msj_bucket_rows_result) == 48 && sizeof(msj_group_keys_result) == 48 && sizeof(msj_field) == 16, "ABI");
static_assert(kRows == (uint32_t)kThreads && kWaves == 4, "geometry");
static_assert(MSJ_KEY_NUMBER == kNumber && MSJ_KEY_CODE == kCode && MSJ_KEY_NULL_IS_GROUP == kNullIsGroup && MSJ_KEY_MAX_PARTS == kMaxParts, "ABI");

constexpr uint32_t kGridBlocks = 1024;  // most blocks of both kernels (they loop over what R needs)

struct State {  // cleared by a memset per call; both calls carve the same one
    unsigned long long n_a, n_b, n_c, n_d, n_no_bits;  // bucket: bucketed, range, skipped, other; keys: keys, null rows
    uint64_t reserved[3];
};
static_assert(sizeof(State) == 64, "layout");
struct Work {
    State *st;
};
static inline Work layout(msj_carver &c, uint64_t) {
    Work w;
    w.st = c.take<State>(1);
    return w;
}

struct Rows {
    const msj_field *fields;
    const msj_select_documents_result *sel;
    uint64_t capacity;
};

// ---- msj_bucket_rows_device ---------------------------------------------------------------------------------------------------
// a lane's five counts, at most 256 of each in a block: 10 bits each in one word
__device__ __forceinline__ uint64_t counts_word(uint32_t outcome, uint32_t out_flags) {
    uint64_t w = (out_flags & kFieldNoBits) ? 1ull << 40 : 0;
    if (outcome != kPassed) w |= 1ull << (10 * (outcome - kBucketed));
    return w;
}

__global__ __launch_bounds__(kThreads) void gk_bucket(const Rows rows, const int64_t width, const int64_t origin, const Work w, msj_field *out) {
    __shared__ uint64_t s_cnt[kWaves];
    const Head h = load_head(rows.sel, rows.capacity);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t k = v * kRows + threadIdx.x;
        uint64_t cnt = 0;
        if (k < h.R) {
            const msj_field f = load_field(rows.fields, k);
            msj_field o;
            const uint32_t outcome = bucket_record(f, width, origin, o);
            store_field(out, k, o);
            cnt = counts_word(outcome, o.flags);
        }
        const uint64_t sum = wave_sum64(cnt);
        __syncthreads();  // (the last round's words have been read)
        if (lane == 0) s_cnt[wave] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t n = 0;
            for (int x = 0; x < kWaves; x++) n += s_cnt[x];
            if (n & 0x3FFu) atomicAdd(&w.st->n_a, (unsigned long long)(n & 0x3FFu));
            if ((n >> 10) & 0x3FFu) atomicAdd(&w.st->n_b, (unsigned long long)((n >> 10) & 0x3FFu));
            if ((n >> 20) & 0x3FFu) atomicAdd(&w.st->n_c, (unsigned long long)((n >> 20) & 0x3FFu));
            if ((n >> 30) & 0x3FFu) atomicAdd(&w.st->n_d, (unsigned long long)((n >> 30) & 0x3FFu));
            if ((n >> 40) & 0x3FFu) atomicAdd(&w.st->n_no_bits, (unsigned long long)((n >> 40) & 0x3FFu));
        }
    }
}

__global__ void gk_bucket_finish(const Rows rows, const Work w, msj_bucket_rows_result *__restrict__ result,
                                 msj_select_documents_result *__restrict__ out_select) {
    const Head h = load_head(rows.sel, rows.capacity);
    msj_bucket_rows_result r;
    r.code = h.skip ? h.code : h.over ? MSJ_CAPACITY : 0;
    r.flags = 0;
    r.n_rows = h.skip ? 0 : h.R;
    r.n_bucketed = h.stop ? 0 : w.st->n_a;
    r.n_range = h.stop ? 0 : w.st->n_b;
    r.n_skipped = h.stop ? 0 : w.st->n_c;
    r.n_other = h.stop ? 0 : w.st->n_d;
    *result = r;
    if (!out_select) return;
    msj_select_documents_result s;
    s.code = r.code, s.flags = 0;
    s.n_documents = h.stop ? 0 : h.R, s.n_paths = 1, s.n_found = r.n_bucketed, s.n_no_bits = h.stop ? 0 : w.st->n_no_bits, s.reserved = 0;
    *out_select = s;
}

// ---- msj_group_keys_device ----------------------------------------------------------------------------------------------------
struct Parts {
    const void *column[kMaxParts];
    uint8_t kind[kMaxParts], flags[kMaxParts];
    uint32_t n, W;
};
struct KeysHead {
    uint64_t R, blocks;
    int32_t code;
    bool skip, stop;
};
struct KeysOut {
    uint64_t *offsets;
    uint8_t *valid, *bytes;
    uint64_t stride, capacity, bytes_capacity;
};
__device__ __forceinline__ KeysHead load_keys_head(const msj_select_documents_result *__restrict__ sel, const KeysOut &o, uint32_t W) {
    KeysHead h;
    const int32_t rows_code = sel->code;
    h.R = sel->n_documents;
    h.code = head_code(rows_code, h.R, o.stride, o.capacity, W, o.bytes_capacity, MSJ_CAPACITY);
    h.skip = rows_code != 0;
    h.stop = h.code != 0;
    h.blocks = h.stop ? 0 : (h.R + kRows - 1) / kRows;
    return h;
}

__global__ __launch_bounds__(kThreads) void gk_keys(const Parts parts, const msj_select_documents_result *__restrict__ sel, const KeysOut o,
                                                    const Work w) {
    __shared__ __attribute__((aligned(16))) uint8_t s_key[kRows * kMaxWidth];  // 22 KiB: a block's keys, row t at t * W
    const KeysHead h = load_keys_head(sel, o, parts.W);
    const uint32_t W = parts.W, lane = threadIdx.x & 63;
    uint32_t n_keys = 0, n_null = 0;  // (wave-uniform; fewer than 2^31 rows)
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t k = v * kRows + threadIdx.x;
        const bool live = k < h.R;
        bool any_null = false, valid = true;
        if (live) {
            uint8_t *p = s_key + threadIdx.x * W;
            for (uint32_t j = 0; j < parts.n; j++) {
                bool null;
                if (parts.kind[j] == kNumber) {
                    null = encode_number(load_field(static_cast<const msj_field *>(parts.column[j]), k), p);
                    p += kNumberBytes;
                } else {
                    null = encode_code(static_cast<const int32_t *>(parts.column[j])[k], p);
                    p += kCodeBytes;
                }
                any_null |= null;
                valid &= !null || (parts.flags[j] & kNullIsGroup) != 0;
            }
            o.offsets[k] = k * W;
            o.valid[k] = valid ? 1 : 0;
        }
        n_keys += (uint32_t)__popcll((unsigned long long)__ballot(live && valid));
        n_null += (uint32_t)__popcll((unsigned long long)__ballot(live && any_null));
        __syncthreads();
        // the block's bytes: [v * kRows * W, + rows * W), the first a multiple of 16 and d_bytes 16-byte aligned
        const uint64_t first = v * kRows * W;
        const uint32_t rows_here = h.R - v * kRows < kRows ? (uint32_t)(h.R - v * kRows) : kRows;
        const uint32_t count = rows_here * W;
        for (uint32_t at = threadIdx.x * 16u; at < count; at += kThreads * 16u) {
            if (at + 16u <= count) {
                *reinterpret_cast<uint4 *>(o.bytes + first + at) = *reinterpret_cast<const uint4 *>(s_key + at);
            } else {
                for (uint32_t i = at; i < count; i++) o.bytes[first + i] = s_key[i];
            }
        }
        __syncthreads();  // (the tile has been read: the next round builds over it)
    }
    if (lane == 0) {
        if (n_keys) atomicAdd(&w.st->n_a, (unsigned long long)n_keys);
        if (n_null) atomicAdd(&w.st->n_b, (unsigned long long)n_null);
    }
}

__global__ void gk_keys_finish(const Parts parts, const msj_select_documents_result *__restrict__ sel, const KeysOut o, const Work w,
                               msj_group_keys_result *__restrict__ result) {
    const KeysHead h = load_keys_head(sel, o, parts.W);
    msj_group_keys_result r;
    r.code = h.code;
    r.flags = 0;
    r.n_rows = h.skip ? 0 : h.R;
    r.n_keys = h.stop ? 0 : w.st->n_a;
    r.n_null_rows = h.stop ? 0 : w.st->n_b;
    r.key_width = parts.W;
    r.bytes_len = h.stop ? 0 : h.R * parts.W;
    *result = r;
    if (!h.stop && o.offsets) o.offsets[h.R] = h.R * parts.W;  // (R <= capacity: the array has capacity + 1 entries)
}

}  // namespace msj_gkeys

extern "C" uint64_t msj_bucket_rows_workspace_bytes(uint64_t capacity) { return msj_measure(msj_gkeys::layout, capacity) + 64; }
extern "C" uint64_t msj_group_keys_workspace_bytes(uint64_t capacity) { return msj_measure(msj_gkeys::layout, capacity) + 64; }

extern "C" int msj_launch_bucket_rows(const msj_field *d_rows, const msj_select_documents_result *d_rows_select, int64_t width, int64_t origin,
                                      msj_field *d_out, uint64_t capacity, msj_bucket_rows_result *d_result,
                                      msj_select_documents_result *d_out_select, void *d_ws, void *stream) {
    using namespace msj_gkeys;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Rows rows{d_rows, d_rows_select, capacity};
    const Work w = msj_place(layout, d_ws, capacity);
    const hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(State), s);
    if (cleared != hipSuccess) return (int)cleared;
    const uint64_t most = most_rows(capacity), nb = (most + kRows - 1) / kRows;
    if (most) hipLaunchKernelGGL(gk_bucket, dim3((uint32_t)(nb > kGridBlocks ? kGridBlocks : nb)), dim3(kThreads), 0, s, rows, width, origin, w, d_out);
    hipLaunchKernelGGL(gk_bucket_finish, dim3(1), dim3(1), 0, s, rows, w, d_result, d_out_select);
    return (int)hipGetLastError();
}

extern "C" int msj_launch_group_keys(const msj_key_part *parts, uint32_t n_parts, uint64_t stride, const msj_select_documents_result *d_rows_select,
                                     uint64_t *d_offsets, uint8_t *d_valid, uint8_t *d_bytes, uint64_t capacity, uint64_t bytes_capacity,
                                     msj_group_keys_result *d_result, void *d_ws, void *stream) {
    using namespace msj_gkeys;
    hipStream_t s = static_cast<hipStream_t>(stream);
    Parts p{};
    p.n = n_parts;
    for (uint32_t j = 0; j < n_parts; j++) {
        p.column[j] = parts[j].d_column, p.kind[j] = (uint8_t)parts[j].kind, p.flags[j] = (uint8_t)parts[j].flags;
        p.W += part_width(parts[j].kind);
    }
    const KeysOut o{d_offsets, d_valid, d_bytes, stride, capacity, bytes_capacity};
    const Work w = msj_place(layout, d_ws, capacity);
    const hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(State), s);
    if (cleared != hipSuccess) return (int)cleared;
    uint64_t most = most_rows(capacity < stride ? capacity : stride);
    if (most * p.W > bytes_capacity) most = bytes_capacity / p.W;  // (more rows than that write nothing)
    const uint64_t nb = (most + kRows - 1) / kRows;
    if (most) hipLaunchKernelGGL(gk_keys, dim3((uint32_t)(nb > kGridBlocks ? kGridBlocks : nb)), dim3(kThreads), 0, s, p, d_rows_select, o, w);
    hipLaunchKernelGGL(gk_keys_finish, dim3(1), dim3(1), 0, s, p, d_rows_select, o, w, d_result);
    return (int)hipGetLastError();
}
