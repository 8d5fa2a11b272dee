// Rows by predicate -- msj_filter_rows_device and msj_take_rows_device (include/msj_stage1.h): from any msj_field records
// with their msj_select_documents_result, a keep byte per row, the kept row numbers ascending, re-based list offsets, and the
// records of a selection vector gathered into a new set of records with a select result of its own, so that every column
// call runs on filtered rows as it does on a select call's output.  The arithmetic -- the exact number compare, the string
// compares, a predicate on a record, a row's verdict -- is filter_rows_math.h, host + device and checked on the CPU by
// tests/test_filter_rows_math.py.  R, P and K are read on the device by every kernel: the host sizes the launches by the
// capacities.
//
// A block owns kRows consecutive rows -- block v the rows [v * kRows, + kRows), the grid loops over the blocks R needs.
// Launches of the filter, all on the caller's stream, behind a memset of the call's counters; the passes are separated by
// kernel boundaries only, and no lane ever waits for another lane or workgroup:
//   fr_eval    a lane per row: every predicate on its column's record, one 16-byte load each; the keep byte, the block's
//              count, and the rows that met a code / a number without bits to two counters (an atomic per block where any)
//   fr_scan    one workgroup: the exclusive sum over the block counts, the result, d_kept_select
//   fr_place   the rank inside the block from a ballot per wave (v_mbcnt: the kept lanes below) and the four wave totals in
//              LDS: the row number to d_kept[base + rank]; the exclusive rank of every row to the workspace when list offsets
//              are to be re-based
//   fr_list    a lane per list offset: the rank at min(offset, R) -- a gather, defined on any array
// The take is tk_gather, a lane per output row and a loop over the columns -- one 16-byte load and one 16-byte store per
// record, the stores of a wave consecutive -- and tk_finish for the result.
// Safety: a record is read only at k < R <= capacity (take: at an index below R <= stride); the window only through
// ByteReader, inside [0, len), after string_column_math.h's row test; d_kept[base + rank] has base + rank < n_kept <= R;
// list entries only at r <= P <= list_rows, the rank array only at an index below R; take stores only at j < K <=
// out_capacity.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "bytes_block.h"
#include "filter_rows_math.h"
#include "launch.h"

namespace msj_frows {

using namespace msj::frows;
using namespace msj::wave;
using msj::val::ByteReader;
using msj_bytes::kGridBlocks, msj_bytes::kRows, msj_bytes::most_rows;
using msj_tape::kThreads, msj_tape::kWaves;
using msj_tdocs::load_field, msj_tdocs::store_field;

static_assert(sizeof(msj_filter_rows_result) == 48 && sizeof(msj_take_rows_result) == 48 && sizeof(msj_field) == 16, "ABI");
static_assert(sizeof(msj_predicate) == 32 && sizeof(Pred) == 16, "ABI");
static_assert(kRows == (uint32_t)kThreads && kWaves == 4, "geometry");

struct State {  // cleared by a memset per call
    unsigned long long n_missing, n_no_bits;         // filter: rows that met a code / a number without bits
    unsigned long long n_found, n_out_of_range;      // take (with n_no_bits)
    uint64_t n_kept;                                 // (fr_scan)
    uint64_t reserved[3];
};
struct Work {
    State *st;
    uint64_t *bcnt;  // per block of rows: its kept rows, then (fr_scan) the kept rows in front of the block
    uint32_t *rank;  // per row: the kept rows in front of it
};
// the records and the call
struct Rows {
    const msj_field *fields;
    uint64_t stride;
    const msj_select_documents_result *sel;
    uint64_t capacity;
};
struct List {
    const uint64_t *offsets;
    uint64_t rows;
    const uint64_t *n_rows;
    uint64_t *out;
};

static inline Work layout(msj_carver &c, uint64_t capacity) {
    const uint64_t rows = most_rows(capacity);
    Work w;
    w.st = c.take<State>(1);
    w.bcnt = c.take<uint64_t>(rows / kRows + 1);
    w.rank = c.take<uint32_t>(rows);
    return w;
}

using msj_bytes::Head, msj_bytes::load_head;

// P list rows; over: more than the caller's arrays hold, no list offset is written
struct ListHead {
    uint64_t P;
    bool over;
};
__device__ __forceinline__ ListHead load_list_head(const List &l) {
    ListHead h;
    h.P = l.n_rows ? *l.n_rows : l.rows;
    h.over = l.offsets != nullptr && msj::frows::rows_over(h.P, l.rows);
    return h;
}

// ---- the filter -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void fr_eval(const Predicates *__restrict__ preds, const uint8_t *__restrict__ buf, uint64_t len,
                                                    const Rows rows, const Work w, uint8_t *__restrict__ keep) {
    __shared__ uint32_t s_cnt[kWaves];
    const Head h = load_head(rows.sel, rows.capacity);
    const ByteReader rd{buf, len};
    const uint32_t n_preds = preds->n, flags = preds->flags;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t k = v * kRows + threadIdx.x;
        bool kept = false;
        uint32_t met = 0;
        if (k < h.R) {
            RowVerdict rv = verdict_begin();
            for (uint32_t i = 0; i < n_preds; i++) {
                const Pred p = preds->p[i];
                verdict_add(rv, eval_pred(p, preds->bytes[i], load_field(rows.fields + (uint64_t)p.column * rows.stride, k), rd));
            }
            kept = row_kept(rv, flags), met = rv.met;
            keep[k] = kept;
        }
        // at most 256 of each: 10 bits each in one word
        const uint32_t cnt = wave_sum((kept ? 1u : 0u) | ((met & kMetCode) ? 1u << 10 : 0u) | ((met & kMetNoBits) ? 1u << 20 : 0u));
        __syncthreads();  // (the last round's words have been read)
        if (lane == 0) s_cnt[wave] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t n = 0;
            for (int x = 0; x < kWaves; x++) n += s_cnt[x];
            w.bcnt[v] = n & 0x3FFu;
            if ((n >> 10) & 0x3FFu) atomicAdd(&w.st->n_missing, (unsigned long long)((n >> 10) & 0x3FFu));
            if (n >> 20) atomicAdd(&w.st->n_no_bits, (unsigned long long)(n >> 20));
        }
    }
}

__global__ __launch_bounds__(1024) void fr_scan(const Predicates *__restrict__ preds, const Rows rows, const Work w, const List list,
                                                msj_filter_rows_result *__restrict__ result,
                                                msj_select_documents_result *__restrict__ kept_select) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(rows.sel, rows.capacity);
    const uint64_t n_kept = scan_in_place(w.bcnt, h.blocks, s_w);
    if (threadIdx.x != 0) return;
    w.st->n_kept = n_kept;
    const bool list_over = !h.stop && load_list_head(list).over;
    msj_filter_rows_result r;
    r.code = h.skip ? h.code : h.over || list_over ? MSJ_CAPACITY : 0;
    r.flags = h.skip ? 0 : preds->flags;
    r.n_rows = h.skip ? 0 : h.R;
    r.n_kept = n_kept;
    r.n_no_bits = h.stop ? 0 : w.st->n_no_bits;
    r.n_missing = h.stop ? 0 : w.st->n_missing;
    r.reserved = 0;
    *result = r;
    if (!kept_select) return;
    msj_select_documents_result s;
    s.code = r.code, s.flags = 0;
    s.n_documents = n_kept, s.n_paths = 1, s.n_found = n_kept, s.n_no_bits = 0, s.reserved = 0;
    *kept_select = s;
}

__global__ __launch_bounds__(kThreads) void fr_place(const Rows rows, const Work w, const uint8_t *__restrict__ keep, uint32_t *__restrict__ kept,
                                                     bool want_rank) {
    __shared__ uint32_t s_tot[kWaves];
    const Head h = load_head(rows.sel, rows.capacity);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t k = v * kRows + threadIdx.x;
        const bool is_kept = k < h.R && keep[k] != 0;
        const uint64_t m = __ballot(is_kept);
        const uint32_t below = lanes_below(m);
        __syncthreads();  // (the last round's totals have been read)
        if (lane == 0) s_tot[wave] = (uint32_t)__popcll((unsigned long long)m);
        __syncthreads();
        uint32_t before = 0;
        for (uint32_t x = 0; x < wave; x++) before += s_tot[x];
        const uint64_t at = w.bcnt[v] + before + below;  // the kept rows in front of row k
        if (k >= h.R) continue;                          // (behind the barriers: the whole block meets there)
        if (want_rank) w.rank[k] = (uint32_t)at;         // (at <= k < 2^31)
        if (is_kept && kept) kept[at] = (uint32_t)k;     // (at < n_kept <= R <= capacity)
    }
}

__global__ __launch_bounds__(kThreads) void fr_list(const Rows rows, const Work w, const List list) {
    const Head h = load_head(rows.sel, rows.capacity);
    const ListHead lh = load_list_head(list);
    if (h.stop || lh.over) return;
    const uint64_t n_kept = w.st->n_kept;
    for (uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x; r <= lh.P; r += (uint64_t)gridDim.x * kThreads)
        list.out[r] = rebased_offset(list.offsets[r], h.R, w.rank, n_kept);
}

// ---- the take ---------------------------------------------------------------------------------------------------------------
struct Take {
    const uint32_t *take;
    const msj_select_documents_result *take_sel;
    msj_field *out;
    uint64_t out_stride, out_capacity;
    uint32_t n_columns;
};
struct TakeHead {
    uint64_t K, R, blocks;
    int32_t code;
    bool skip, over, stop;
};
__device__ __forceinline__ TakeHead load_take_head(const Take &t, const Rows &rows) {
    TakeHead h;
    h.code = t.take_sel->code != 0 ? t.take_sel->code : rows.sel->code;
    h.K = t.take_sel->n_documents, h.R = rows.sel->n_documents;
    h.skip = h.code != 0;
    h.over = !h.skip && take_over(h.K, t.out_capacity, h.R, rows.stride);
    h.stop = h.skip || h.over;
    h.blocks = h.stop ? 0 : (h.K + kRows - 1) / kRows;
    return h;
}

__global__ __launch_bounds__(kThreads) void tk_gather(const Take t, const Rows rows, const Work w) {
    __shared__ uint32_t s_a[kWaves], s_b[kWaves], s_c[kWaves];
    const TakeHead h = load_take_head(t, rows);
    uint32_t found = 0, no_bits = 0, out_of_range = 0;  // (a lane meets at most 2^31 / 256 / gridDim.x * 16 records)
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t j = v * kRows + threadIdx.x;
        if (j >= h.K) continue;
        const uint64_t src = t.take[j];
        out_of_range += src >= h.R;
        for (uint32_t c = 0; c < t.n_columns; c++) {
            msj_field f = missing_field<msj_field>();
            if (src < h.R) f = load_field(rows.fields + (uint64_t)c * rows.stride, src);  // (src < R <= stride)
            found += f.code == 0, no_bits += (f.flags & kFieldNoBits) != 0;
            store_field(t.out + (uint64_t)c * t.out_stride, j, f);  // (j < K <= out_capacity)
        }
    }
    (void)block_counter_add(found, s_a, reinterpret_cast<uint64_t *>(&w.st->n_found));
    (void)block_counter_add(no_bits, s_b, reinterpret_cast<uint64_t *>(&w.st->n_no_bits));
    (void)block_counter_add(out_of_range, s_c, reinterpret_cast<uint64_t *>(&w.st->n_out_of_range));
}

__global__ void tk_finish(const Take t, const Rows rows, const Work w, msj_take_rows_result *__restrict__ result,
                          msj_select_documents_result *__restrict__ out_select) {
    const TakeHead h = load_take_head(t, rows);
    msj_take_rows_result r;
    r.code = h.skip ? h.code : h.over ? MSJ_CAPACITY : 0;
    r.flags = 0;
    r.n_rows = h.skip ? 0 : h.K;
    r.n_out_of_range = h.stop ? 0 : w.st->n_out_of_range;
    r.n_found = h.stop ? 0 : w.st->n_found;
    r.n_no_bits = h.stop ? 0 : w.st->n_no_bits;
    r.reserved = 0;
    *result = r;
    if (!out_select) return;
    msj_select_documents_result s;
    s.code = r.code, s.flags = 0;
    s.n_documents = h.stop ? 0 : h.K, s.n_paths = t.n_columns, s.n_found = r.n_found, s.n_no_bits = r.n_no_bits, s.reserved = 0;
    *out_select = s;
}

static inline dim3 grid_over(uint64_t items) {
    const uint64_t nb = (items + kRows - 1) / kRows;
    return dim3((uint32_t)(nb > kGridBlocks ? kGridBlocks : nb));
}

}  // namespace msj_frows

extern "C" uint64_t msj_filter_rows_workspace_bytes(uint64_t capacity) { return msj_measure(msj_frows::layout, capacity) + 64; }

extern "C" int msj_launch_filter_rows(const void *d_predicates, const uint8_t *d_buf, uint64_t len, const msj_field *d_fields, uint64_t stride,
                                      const msj_select_documents_result *d_rows_select, uint8_t *d_keep, uint32_t *d_kept, uint64_t capacity,
                                      const uint64_t *d_list_offsets, uint64_t list_rows, const uint64_t *d_list_n_rows,
                                      uint64_t *d_list_offsets_out, msj_filter_rows_result *d_result,
                                      msj_select_documents_result *d_kept_select, void *d_ws, void *stream) {
    using namespace msj_frows;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Predicates *preds = static_cast<const Predicates *>(d_predicates);
    const Rows rows{d_fields, stride, d_rows_select, capacity};
    const List list{d_list_offsets, list_rows, d_list_n_rows, d_list_offsets_out};
    const Work w = msj_place(layout, d_ws, capacity);
    const hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(State), s);
    if (cleared != hipSuccess) return (int)cleared;
    const uint64_t most = most_rows(capacity);
    const dim3 grid = grid_over(most), block(kThreads);
    if (most) hipLaunchKernelGGL(fr_eval, grid, block, 0, s, preds, d_buf, len, rows, w, d_keep);
    hipLaunchKernelGGL(fr_scan, dim3(1), dim3(1024), 0, s, preds, rows, w, list, d_result, d_kept_select);
    if (most && (d_kept || d_list_offsets)) hipLaunchKernelGGL(fr_place, grid, block, 0, s, rows, w, d_keep, d_kept, d_list_offsets != nullptr);
    if (d_list_offsets) hipLaunchKernelGGL(fr_list, grid_over(most_rows(list_rows) + 1), block, 0, s, rows, w, list);
    return (int)hipGetLastError();
}

extern "C" int msj_launch_take_rows(const uint32_t *d_take, const msj_select_documents_result *d_take_select, const msj_field *d_fields,
                                    uint64_t stride, uint32_t n_columns, const msj_select_documents_result *d_rows_select, msj_field *d_out,
                                    uint64_t out_stride, uint64_t out_capacity, msj_take_rows_result *d_result,
                                    msj_select_documents_result *d_out_select, void *d_ws, void *stream) {
    using namespace msj_frows;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Take t{d_take, d_take_select, d_out, out_stride, out_capacity, n_columns};
    const Rows rows{d_fields, stride, d_rows_select, stride};
    const Work w = msj_place(layout, d_ws, 0);  // (the counters alone)
    const hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(State), s);
    if (cleared != hipSuccess) return (int)cleared;
    const uint64_t most = most_rows(out_capacity);
    if (most) hipLaunchKernelGGL(tk_gather, grid_over(most), dim3(kThreads), 0, s, t, rows, w);
    hipLaunchKernelGGL(tk_finish, dim3(1), dim3(1), 0, s, t, rows, w, d_result, d_out_select);
    return (int)hipGetLastError();
}
