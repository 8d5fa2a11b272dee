// Timestamps and numbers written as strings -- msj_cast_strings_device (include/msj_stage1.h): from any msj_field records
// with their msj_select_documents_result, a record per row that holds the string's value as an int64 or a binary64, so that
// the filter, the take and the number columns run on it as on a number a select call found.  The arithmetic -- the timestamp
// grammar, the calendar, the number wrapper, one record in and one record out -- is cast_strings_math.h, host + device and
// checked on the CPU by tests/test_cast_strings_math.py.  R is read on the device by every kernel: the host sizes the
// launches by the capacity.
//
// A block owns kRows consecutive rows -- block v the rows [v * kRows, + kRows), the grid loops over the blocks R needs.
// Launches, all on the caller's stream, behind a memset of the call's counters; no lane ever waits for another lane:
//   cs_cast    a lane per row: one 16-byte record load, the body's bytes, one 16-byte record store (a wave's stores
//              consecutive), the five counts by a wave sum and an atomic per block where non-zero.  A row whose body is
//              escaped, and a number the fast paths of number_math.h cannot decide, is not written here: its row number goes
//              to the list (a ballot and one atomic per wave that has any)
//   cs_list    a lane per entry of the list, the grid sized by the capacity: cast_strings_math.h's cast_record whole --
//              the unescape into a lane's own memory and, for the number kind, the exact big-integer path: the only two
//              users of scratch memory (the kind is a template argument: a timestamp's instance has no big integer)
//   cs_finish  one lane: the result and d_out_select
// The body's bytes, two forms (kWindow; DESIGN.md section 5b has both rates): byte loads from the window as fr_eval does
// them, or the aligned 16-byte words that cover the body loaded into the lane's slot of LDS and read from there, as
// numbers_kernel.hip's lane path does.  Both read the same bytes and give the same records.
// Safety: a record is read and written only at k < R <= capacity; the window only inside [0, len) and only after
// string_column_math.h's row test said that the body lies inside it; the list holds at most R entries, every one below R.
// In place (d_out == d_rows): row k is read by the one lane that writes it, before it writes; a listed row is not written
// by cs_cast, so cs_list reads the input record.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "bytes_block.h"
#include "cast_strings_math.h"
#include "launch.h"

namespace msj_cast {

using namespace msj::cast;
using namespace msj::wave;
using msj::val::ByteReader;
using msj_bytes::Head, msj_bytes::load_head;
using msj_bytes::kGridBlocks, msj_bytes::kRows, msj_bytes::most_rows;
using msj_tape::kThreads, msj_tape::kWaves;
using msj_tdocs::load_field, msj_tdocs::store_field;

static_assert(sizeof(msj_cast_strings_result) == 48 && sizeof(msj_field) == 16, "ABI");
static_assert(kRows == (uint32_t)kThreads && kWaves == 4, "geometry");

struct State {  // cleared by a memset per call
    unsigned long long n_cast, n_syntax, n_range, n_other, n_no_bits;
    uint32_t n_list, reserved[5];
};
static_assert(sizeof(State) == 64, "layout");
struct Work {
    State *st;
    uint32_t *list;  // the rows cs_cast left to cs_list, in any order
};
struct Rows {
    const msj_field *fields;
    const msj_select_documents_result *sel;
    uint64_t capacity;
};
struct Call {
    uint32_t kind, unit, flags;
};

static inline Work layout(msj_carver &c, uint64_t capacity) {
    Work w;
    w.st = c.take<State>(1);
    w.list = c.take<uint32_t>(most_rows(capacity));
    return w;
}

constexpr uint32_t kWin = 64;              // bytes of a body's window in LDS, from its 16-byte line on: 15 + 35 fit
constexpr uint32_t kWinStride = kWin + 4;  // per lane; 17 dwords: lanes spread over the banks

// The window form's reader: the aligned 16-byte words that cover [b, b + r) -- at most four, clipped to [0, len) -- loaded
// with independent 16-byte loads into this lane's slot, so that the grammar's byte-by-byte reads wait for LDS and not for
// memory.  A body that leaves the window (a number of more than 49 bytes may) reads its rest from memory.  Same answers as
// ByteReader on [b, b + r), which is all cast_plain asks
struct WindowReader {
    const uint8_t *buf;
    uint64_t len;
    int64_t a;           // the window's first byte as a window offset: its ADDRESS is 16-byte aligned, so it may lie in front of 0
    const uint8_t *win;  // this lane's LDS slot
    __device__ __forceinline__ void load(uint8_t *slot, uint64_t b, uint64_t r) {
        const uint64_t mis = reinterpret_cast<uintptr_t>(buf) & 15u;
        a = (int64_t)((b + mis) & ~15ull) - (int64_t)mis;
        win = slot;
        uint4 q[kWin / 16];
#pragma unroll
        for (uint32_t c = 0; c < kWin / 16; c++) {
            const int64_t w0 = a + 16 * (int64_t)c;
            q[c] = make_uint4(0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u);
            if (w0 >= (int64_t)(b + r)) continue;  // (no byte of the body)
            if (w0 >= 0 && (uint64_t)w0 + 16 <= len) {
                q[c] = *reinterpret_cast<const uint4 *>(buf + w0);
            } else {
                uint32_t v[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    v[k] = 0;
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int64_t p = w0 + 4 * k + i;
                        v[k] |= (p >= 0 && (uint64_t)p < len ? (uint32_t)buf[p] : 0x20u) << (8 * i);
                    }
                }
                q[c] = make_uint4(v[0], v[1], v[2], v[3]);
            }
        }
        uint32_t *d = reinterpret_cast<uint32_t *>(slot);
#pragma unroll
        for (uint32_t c = 0; c < kWin / 16; c++) d[4 * c] = q[c].x, d[4 * c + 1] = q[c].y, d[4 * c + 2] = q[c].z, d[4 * c + 3] = q[c].w;
    }
    __device__ __forceinline__ uint32_t at(uint64_t p) const {
        const uint64_t o = p - (uint64_t)a;  // (p >= b >= a)
        if (o < (uint64_t)kWin) return win[o];
        return p < len ? buf[p] : 0x20u;
    }
};

// a lane's five counts, at most 256 of each in a block: 10 bits each in one word
__device__ __forceinline__ uint64_t counts_word(uint32_t outcome, uint32_t out_flags) {
    uint64_t w = (out_flags & kFieldNoBits) ? 1ull << 40 : 0;
    if (outcome != kPassed) w |= 1ull << (10 * (outcome - kCast));
    return w;
}

template <uint32_t kKind, bool kWindow>
__global__ __launch_bounds__(kThreads) void cs_cast(const uint8_t *__restrict__ buf, uint64_t len, const Rows rows, const Call call, const Work w,
                                                    msj_field *out) {
    __shared__ uint64_t s_cnt[kWaves];
    __shared__ uint32_t s_win[kWindow ? kThreads * kWinStride / 4 : 1];
    const Head h = load_head(rows.sel, rows.capacity);
    const ByteReader rd{buf, len};
    WindowReader wr{buf, len, 0, nullptr};
    uint8_t *slot = reinterpret_cast<uint8_t *>(s_win) + (kWindow ? threadIdx.x * kWinStride : 0);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t k = v * kRows + threadIdx.x;
        uint64_t cnt = 0;
        bool listed = false;
        if (k < h.R) {
            const msj_field f = load_field(rows.fields, k);
            msj::scol::Row y;
            msj_field o;
            uint32_t outcome;
            if (!cast_without_bytes(f, len, call.flags, y, o, outcome)) {
                if (y.escaped) {
                    outcome = kPending;
                } else if (kWindow) {
                    if (y.r <= max_value_bytes(kKind)) wr.load(slot, y.b, y.r);
                    outcome = cast_plain<false>(f, y, wr, kKind, call.unit, o);
                } else {
                    outcome = cast_plain<false>(f, y, rd, kKind, call.unit, o);
                }
            }
            listed = outcome == kPending;
            if (!listed) {
                store_field(out, k, o);
                cnt = counts_word(outcome, o.flags);
            }
        }
        const uint64_t m = __ballot(listed);
        if (m) {  // (wave-uniform) one atomic for the wave's rows; their order in the list means nothing
            const uint32_t leader = (uint32_t)__ffsll((unsigned long long)m) - 1u;
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(&w.st->n_list, (uint32_t)__popcll((unsigned long long)m));
            base = (uint32_t)__shfl((int)base, (int)leader);
            const uint32_t below = lanes_below(m);
            if (listed) w.list[base + below] = (uint32_t)k;  // (base + below < the listed rows <= R <= capacity)
        }
        const uint64_t sum = wave_sum64(cnt);
        __syncthreads();  // (the last round's words have been read)
        if (lane == 0) s_cnt[wave] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t n = 0;
            for (int x = 0; x < kWaves; x++) n += s_cnt[x];
            if (n & 0x3FFu) atomicAdd(&w.st->n_cast, (unsigned long long)(n & 0x3FFu));
            if ((n >> 10) & 0x3FFu) atomicAdd(&w.st->n_syntax, (unsigned long long)((n >> 10) & 0x3FFu));
            if ((n >> 20) & 0x3FFu) atomicAdd(&w.st->n_range, (unsigned long long)((n >> 20) & 0x3FFu));
            if ((n >> 30) & 0x3FFu) atomicAdd(&w.st->n_other, (unsigned long long)((n >> 30) & 0x3FFu));
            if ((n >> 40) & 0x3FFu) atomicAdd(&w.st->n_no_bits, (unsigned long long)((n >> 40) & 0x3FFu));
        }
    }
}

template <uint32_t kKind>
__global__ __launch_bounds__(kThreads) void cs_list(const uint8_t *__restrict__ buf, uint64_t len, const Rows rows, const Call call, const Work w,
                                                    msj_field *out) {
    __shared__ uint32_t s_a[kWaves], s_b[kWaves], s_c[kWaves];
    const Head h = load_head(rows.sel, rows.capacity);
    const ByteReader rd{buf, len};
    const uint64_t listed = h.stop ? 0 : w.st->n_list;  // (<= R)
    uint32_t n_cast = 0, n_syntax = 0, n_range = 0;     // (a listed row is a string row: nothing else comes of it)
    for (uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x; j < listed && j < h.R; j += (uint64_t)gridDim.x * kThreads) {
        const uint64_t k = w.list[j];
        if (k >= h.R) continue;  // (never: cs_cast lists rows below R)
        const msj_field f = load_field(rows.fields, k);
        msj_field o;
        const uint32_t outcome = cast_record<kKind == kTimestamp ? kMaxTimestampBytes + 1 : kMaxNumberBytes>(f, rd, kKind, call.unit, call.flags, o);  // (the kind a constant: a timestamp needs no big integer)
        store_field(out, k, o);
        n_cast += outcome == kCast, n_syntax += outcome == kSyntax, n_range += outcome == kRange;
    }
    (void)block_counter_add(n_cast, s_a, reinterpret_cast<uint64_t *>(&w.st->n_cast));
    (void)block_counter_add(n_syntax, s_b, reinterpret_cast<uint64_t *>(&w.st->n_syntax));
    (void)block_counter_add(n_range, s_c, reinterpret_cast<uint64_t *>(&w.st->n_range));
}

__global__ void cs_finish(const Rows rows, const Call call, const Work w, msj_cast_strings_result *__restrict__ result,
                          msj_select_documents_result *__restrict__ out_select) {
    const Head h = load_head(rows.sel, rows.capacity);
    msj_cast_strings_result r;
    r.code = h.skip ? h.code : h.over ? MSJ_CAPACITY : 0;
    r.flags = result_flags(call.kind, call.unit, call.flags);
    r.n_rows = h.skip ? 0 : h.R;
    r.n_cast = h.stop ? 0 : w.st->n_cast;
    r.n_syntax = h.stop ? 0 : w.st->n_syntax;
    r.n_range = h.stop ? 0 : w.st->n_range;
    r.n_other = h.stop ? 0 : w.st->n_other;
    *result = r;
    if (!out_select) return;
    msj_select_documents_result s;
    s.code = r.code, s.flags = 0;
    s.n_documents = h.stop ? 0 : h.R, s.n_paths = 1, s.n_found = r.n_cast, s.n_no_bits = h.stop ? 0 : w.st->n_no_bits, s.reserved = 0;
    *out_select = s;
}

template <uint32_t kKind>
static inline void launch_cast(bool window, dim3 grid, hipStream_t s, const uint8_t *d_buf, uint64_t len, const Rows &rows, const Call &call,
                               const Work &w, msj_field *d_out) {
    if (window) hipLaunchKernelGGL((cs_cast<kKind, true>), grid, dim3(kThreads), 0, s, d_buf, len, rows, call, w, d_out);
    else hipLaunchKernelGGL((cs_cast<kKind, false>), grid, dim3(kThreads), 0, s, d_buf, len, rows, call, w, d_out);
}

}  // namespace msj_cast

extern "C" uint64_t msj_cast_strings_workspace_bytes(uint64_t capacity) { return msj_measure(msj_cast::layout, capacity) + 64; }

extern "C" int msj_launch_cast_strings(const uint8_t *d_buf, uint64_t len, const msj_field *d_rows, const msj_select_documents_result *d_rows_select,
                                       uint32_t kind, uint32_t unit, uint32_t flags, uint32_t fetch, msj_field *d_out, uint64_t capacity,
                                       msj_cast_strings_result *d_result, msj_select_documents_result *d_out_select, void *d_ws, void *stream) {
    using namespace msj_cast;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Rows rows{d_rows, d_rows_select, capacity};
    const Call call{kind, unit, flags};
    const Work w = msj_place(layout, d_ws, capacity);
    const hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(State), s);
    if (cleared != hipSuccess) return (int)cleared;
    const uint64_t most = most_rows(capacity), nb = (most + kRows - 1) / kRows;
    const dim3 grid((uint32_t)(nb > kGridBlocks ? kGridBlocks : nb));
    if (most) {
        const bool window = fetch == MSJ_CAST_FETCH_WINDOW;
        if (kind == kTimestamp) {
            launch_cast<kTimestamp>(window, grid, s, d_buf, len, rows, call, w, d_out);
            hipLaunchKernelGGL(cs_list<kTimestamp>, grid, dim3(kThreads), 0, s, d_buf, len, rows, call, w, d_out);
        } else {
            launch_cast<kNumber>(window, grid, s, d_buf, len, rows, call, w, d_out);
            hipLaunchKernelGGL(cs_list<kNumber>, grid, dim3(kThreads), 0, s, d_buf, len, rows, call, w, d_out);
        }
    }
    hipLaunchKernelGGL(cs_finish, dim3(1), dim3(1), 0, s, rows, call, w, d_result, d_out_select);
    return (int)hipGetLastError();
}
