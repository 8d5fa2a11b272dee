// One selected path's strings as a column -- msj_string_column_device (include/msj_stage1.h): from the msj_field records
// msj_select_documents_device wrote for a path, offsets[D + 1], the unescaped bytes back to back and a validity byte per
// row.  The arithmetic -- the row test, a row's length, the code, the mapping from an output byte to its row -- is
// string_column_math.h, host + device and checked on the CPU by tests/test_string_column_math.py; the bytes of an escaped
// value are tape_math.h's, a long one walked by a wave as in the tape calls (wave_unescape.h).  D = d_select->n_documents
// is read on the device by every kernel: the host never learns it, and sizes the launches by the capacity.
//
// A block owns kRows consecutive rows -- block v the rows [v * kRows, + kRows), the grid loops over the blocks D needs.
// Launches, all on the caller's stream, behind a 64-byte memset of the call's counters:
//   sc_lengths  a lane per row: the 16-byte record as one load, the row test, d_valid.  A plain row's length is its span's;
//               an escaped one up to kLaneBody raw bytes is measured by its lane, a longer one by its wave, 64 bytes per
//               step, where it stands (no list: records from anywhere may name the same long span any number of times).
//               The lengths go to the workspace, their sum per block beside them; the counts by wave and block, three
//               atomics per block
//   sc_scan     one workgroup: the exclusive sum over the blocks' sums, offsets[0], and the result -- d_select's code,
//               MSJ_CAPACITY for D > capacity or for more bytes than d_bytes holds
//   sc_copy     the hot path.  The exclusive sum over the block's lengths gives its rows' offsets (d_offsets leaves here)
//               and the block's contiguous range of output bytes; offsets and source starts are staged in LDS and the lanes
//               take CONSECUTIVE OUTPUT BYTES of the range, find each byte's row by binary search in LDS (row_of_byte) and
//               copy buf[b_row + (pos - off_row)]: stores are coalesced whatever the rows' lengths -- a lane per row would
//               store single bytes 20 apart -- and loads nearly sequential.  The loop runs until the range is done, so a
//               1 MiB body between short ones is nothing special.  A byte of an escaped row is skipped there: those rows are
//               written by their own lane, or by their wave when long, through the checked writer.  The layout-only form
//               (d_bytes NULL) stops behind the offsets
// Safety: a record is dereferenced only when b + r <= len, and every read of the window goes through ByteReader; every
// store to d_bytes is checked against bytes_capacity; rows are below D <= capacity.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "bytes_block.h"
#include "launch.h"
#include "string_column_math.h"

namespace msj_scol {

using namespace msj::scol;
using namespace msj::wave;
using namespace msj_bytes;
using msj::val::ByteReader;
using msj_tape::block_scan, msj_tape::BufWriter, msj_tape::kLaneBody, msj_tape::kThreads, msj_tape::kWaves, msj_tape::wave_unescape;
using msj_tdocs::load_field;

static_assert(sizeof(msj_string_column_result) == 48 && sizeof(msj_field) == 16, "ABI");

struct State {  // cleared by a memset per call
    unsigned long long n_strings, n_escaped, n_other;
    uint64_t reserved[5];
};
struct Work {
    State *st;
    uint64_t *bsum;  // per block: the sum of its rows' lengths, then (sc_scan) the bytes in front of the block
    uint32_t *lens;  // per row: its length in the output
};

static inline Work layout(msj_carver &c, uint64_t capacity) {
    const uint64_t rows = most_rows(capacity);
    Work w;
    w.st = c.take<State>(1);
    w.bsum = c.take<uint64_t>(rows / kRows + 1);
    w.lens = c.take<uint32_t>(rows);
    return w;
}

__global__ __launch_bounds__(kThreads) void sc_lengths(const uint8_t *__restrict__ buf, uint64_t len, const msj_field *__restrict__ column,
                                                       const msj_select_documents_result *__restrict__ sel, uint64_t capacity,
                                                       const Work w, uint8_t *__restrict__ valid) {
    __shared__ uint64_t s_sum[kWaves];
    __shared__ uint32_t s_cnt[kWaves];
    const Head h = load_head(sel, capacity);
    const ByteReader rd{buf, len};
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t k = v * kRows + threadIdx.x;
        Row y = row_of(msj_field{0, 0, 0, 0, 1}, len);  // (a row past D: a record with a code)
        if (k < h.R) y = row_of(load_field(column, k), len);
        const bool far = is_long(y, kLaneBody);
        uint64_t ul = far ? 0 : ulen(rd, y);
        for (uint64_t m = __ballot(far); m; m &= m - 1) {  // (the same in every lane of the wave)
            const int src = __ffsll((unsigned long long)m) - 1;
            const uint64_t b = __shfl((unsigned long long)y.b, src), r = __shfl((unsigned long long)y.r, src);
            const uint64_t u = wave_unescape(rd, BufWriter{nullptr, 0, 0}, b, b + r, true);
            if ((int)lane == src) ul = u;
        }
        if (k < h.R) {
            valid[k] = y.valid;
            w.lens[k] = (uint32_t)ul;  // (<= r < 2^32)
        }
        block_sums_out(lane, wave, ul, y.valid, y.escaped, y.other, s_sum, s_cnt, &w.bsum[v], &w.st->n_strings, &w.st->n_escaped, &w.st->n_other);
    }
}

__global__ __launch_bounds__(1024) void sc_scan(const msj_select_documents_result *__restrict__ sel, uint64_t capacity, const Work w,
                                                uint64_t *__restrict__ offsets, bool have_bytes, uint64_t bytes_capacity,
                                                msj_string_column_result *__restrict__ result) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(sel, capacity);
    const uint64_t run = scan_in_place(w.bsum, h.blocks, s_w);
    if (threadIdx.x != 0) return;
    msj_string_column_result r;
    r.code = h.skip ? h.code : h.over ? MSJ_CAPACITY : bytes_code(run, have_bytes, bytes_capacity);
    r.flags = 0;
    r.n_rows = h.skip ? 0 : h.R;
    r.n_strings = h.stop ? 0 : w.st->n_strings;
    r.n_escaped = h.stop ? 0 : w.st->n_escaped;
    r.total_bytes = run;
    r.n_other = h.stop ? 0 : w.st->n_other;
    *result = r;
    if (!h.stop && offsets) offsets[0] = 0;  // (NULL only with capacity 0: D is 0 then)
}

__global__ __launch_bounds__(kThreads) void sc_copy(const uint8_t *__restrict__ buf, uint64_t len, const msj_field *__restrict__ column,
                                                    const msj_select_documents_result *__restrict__ sel, uint64_t capacity, const Work w,
                                                    uint64_t *__restrict__ offsets, uint8_t *__restrict__ bytes, uint64_t bytes_capacity) {
    __shared__ uint64_t s_off[kRows + 1];
    __shared__ uint32_t s_src[kRows];
    __shared__ uint8_t s_esc[kRows];
    __shared__ uint64_t s_w[kWaves];
    const Head h = load_head(sel, capacity);
    const ByteReader rd{buf, len};
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t k = v * kRows + threadIdx.x;
        Row y = row_of(msj_field{0, 0, 0, 0, 1}, len);
        uint64_t ul = 0;
        if (k < h.R) y = row_of(load_field(column, k), len), ul = w.lens[k];
        uint64_t total;
        const uint64_t base = w.bsum[v], off = base + block_scan(ul, s_w, total);
        if (k < h.R) offsets[k + 1] = off + ul;  // (k + 1 <= D <= capacity)
        if (!bytes || total == 0) continue;      // (the whole block: the layout-only form, or rows without a byte)
        __syncthreads();                         // (the last round's mapping has been read)
        s_off[threadIdx.x] = off, s_src[threadIdx.x] = (uint32_t)y.b, s_esc[threadIdx.x] = y.escaped;
        if (threadIdx.x == 0) s_off[kRows] = base + total;
        __syncthreads();
        const uint64_t end = base + total < bytes_capacity ? base + total : bytes_capacity;
        for (uint64_t pos = base + threadIdx.x; pos < end; pos += kThreads) {
            const uint32_t row = row_of_byte(s_off, kRows, pos);
            if (!s_esc[row]) bytes[pos] = (uint8_t)rd.at((uint64_t)s_src[row] + (pos - s_off[row]));
        }
        const bool far = is_long(y, kLaneBody);
        if (y.escaped && !far) (void)unescape_serial(rd, BufWriter{bytes, off, bytes_capacity}, y.b, y.b + y.r);
        for (uint64_t m = __ballot(far); m; m &= m - 1) {
            const int src = __ffsll((unsigned long long)m) - 1;
            const uint64_t b = __shfl((unsigned long long)y.b, src), r = __shfl((unsigned long long)y.r, src);
            const uint64_t o = __shfl((unsigned long long)off, src);
            (void)wave_unescape(rd, BufWriter{bytes, o, bytes_capacity}, b, b + r, false);
        }
    }
}

}  // namespace msj_scol

extern "C" uint64_t msj_string_column_workspace_bytes(uint64_t capacity) { return msj_measure(msj_scol::layout, capacity) + 64; }

extern "C" int msj_launch_string_column(const uint8_t *d_buf, uint64_t len, const msj_field *d_column, const msj_select_documents_result *d_select,
                                        uint64_t *d_offsets, uint8_t *d_valid, uint64_t capacity, uint8_t *d_bytes, uint64_t bytes_capacity,
                                        msj_string_column_result *d_result, void *d_ws, void *stream) {
    using namespace msj_scol;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Work w = msj_place(layout, d_ws, capacity);
    const hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(State), s);
    if (cleared != hipSuccess) return (int)cleared;
    const uint64_t nb = (most_rows(capacity) + kRows - 1) / kRows;
    const dim3 grid((uint32_t)(nb > kGridBlocks ? kGridBlocks : nb));
    if (nb) hipLaunchKernelGGL(sc_lengths, grid, dim3(kThreads), 0, s, d_buf, len, d_column, d_select, capacity, w, d_valid);
    hipLaunchKernelGGL(sc_scan, dim3(1), dim3(1024), 0, s, d_select, capacity, w, d_offsets, d_bytes != nullptr, bytes_capacity, d_result);
    if (nb) hipLaunchKernelGGL(sc_copy, grid, dim3(kThreads), 0, s, d_buf, len, d_column, d_select, capacity, w, d_offsets, d_bytes, bytes_capacity);
    return (int)hipGetLastError();
}
