// Rows by exact numeric order -- msj_sort_rows_device (include/msj_stage1.h): from ONE column of msj_field records with its
// msj_select_documents_result, and optionally a list of row numbers, the row numbers in ascending (or descending) order of
// their values as real numbers, stable, rows without a value last, the first K of them.  The arithmetic -- the value test,
// the key, its digits, the code, K, the choice between the two paths -- is sort_rows_math.h, host + device and checked on
// the CPU by tests/test_sort_rows_math.py.  N, R and K are read on the device by every kernel: the host sizes the launches
// by the capacity.
//
// A row becomes two words (sort_rows_math.h): hi, and aux = position | lo << 32 | null << 42.  Two buffers of each in the
// workspace; every pass reads one and writes the other, and which is which is a word of the plan.  Launches, all on the
// caller's stream, behind a memset of the call's state; the passes are separated by kernel boundaries only, and no lane
// ever waits for another lane or workgroup:
//   sr_keys     a lane per input position: the row number (d_rows_in or the position), one 16-byte record load, the key
//               into buffer 0, n_values / n_skipped / n_out_of_range, and the histogram of each of the 11 digits (a block
//               counts in LDS and adds what it touched once)
//   the selection, only where sort_rows_math.h's takes_selection says so -- THE CUT-OVER: limit > 0, N >= 16 384 and
//   limit <= N / 8; below that the full sort's passes cost less than the selection's launches -- (every kernel works that
//   out from N itself and returns at once otherwise):
//   sl_hist(d), sl_pick(d)  from the null digit down: the histogram of digit d over the rows whose digits above d are the
//               prefix fixed so far -- while every digit above was constant that is sr_keys' own histogram and sl_hist
//               returns at once --, then one workgroup finds the bucket that holds the K-th row.  Ends when the rows at or
//               below the prefix are few (select_enough) or at the last digit: T is then the K-th row's whole key
//   sl_count, sl_scan, sl_place   the rows below the prefix and the first take_eq rows that equal it, compacted in input
//               order into buffer 1 (block counts, one workgroup's running sum, ballot ranks), with their digit histograms
//   sr_plan     one workgroup: the rows to sort (all N in buffer 0, or the survivors in buffer 1), per digit whether it is
//               constant over them -- its pass is skipped -- and the buffer each pass reads, and the start of every bucket
//   sr_count(d), sr_scan(d), sr_scatter(d)   one stable least-significant-digit pass, radix_block.h's: counts per (bucket,
//               tile of 1 024 rows), 256 workgroups scan a bucket each, the scatter ranks by ballots and LDS counters.  The
//               bucket starts are the plan's; sr_count reads the one word that holds the digit.  All three return at once
//               for a constant digit
//   sr_finish   d_order[i] = the row number at the i-th position for i < K, the result, d_order_select
// Every count is an integer sum and every place a function of the counts: the same bytes from run to run, on both paths.
// Safety: a record is read only at a row below R <= stride; d_rows_in only below N <= capacity; the buffers only below the
// rows to sort <= N (a scatter's place is tested against that once more); d_order only below K <= min(N, limit).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "bytes_block.h"
#include "launch.h"
#include "radix_block.h"
#include "sort_rows_math.h"

namespace msj_srows {

using namespace msj::srows;
using namespace msj::wave;
using msj_bytes::kRows, msj_bytes::most_rows;
using msj_radix::kScan, msj_radix::kTileBlocks, msj_radix::tiles_of;
using msj_tape::kThreads, msj_tape::kWaves;
using msj_tdocs::load_field;

static_assert(sizeof(msj_sort_rows_result) == 48 && sizeof(msj_field) == 16, "ABI");
static_assert(kRows == (uint32_t)kThreads && kWaves == 4 && kBuckets == (uint32_t)kThreads, "geometry");
static_assert(kBuckets == msj_radix::kBuckets, "the radix pass takes sort_rows_math.h's digits");

constexpr uint32_t kRowBlocks = 4096;  // most blocks of the kernels with a lane per row (they loop over what N needs)

struct Select {  // the selection's progress
    uint32_t pd[kDigits];  // the prefix: the digits fixed so far
    uint32_t low;          // the lowest digit fixed
    uint32_t own_hist;     // a digit above was not constant: sl_hist counts
    uint32_t done;
    uint64_t below, match;  // rows below the prefix, rows that equal it
    uint64_t take_eq;       // of the latter the first so many survive
};
struct Plan {
    uint64_t n;  // the rows to sort
    uint32_t skip[kDigits], src[kDigits];  // per pass: the digit is constant; the buffer it reads
    uint32_t last;                         // the buffer the order ends in
    uint32_t base[kDigits][kBuckets];      // the rows in the buckets in front
};
struct State {  // cleared by a memset per call
    unsigned long long n_values, n_skipped, n_out_of_range;
    uint32_t hist[kDigits][kBuckets];     // sr_keys: every row
    uint32_t hist_sl[kDigits][kBuckets];  // sl_hist: the rows that match the prefix above the digit
    uint32_t hist_sv[kDigits][kBuckets];  // sl_place: the survivors
    Select sl;
    Plan plan;
};
struct Work {
    State *st;
    uint64_t *hi[2], *aux[2];
    uint32_t *cnt;   // [bucket * tiles + tile]
    uint64_t *bcnt;  // sl_count: per block of rows, the rows below the prefix | the rows that equal it << 32
};
struct Call {
    const msj_field *fields;
    uint64_t stride;
    const msj_select_documents_result *sel;
    const uint32_t *rows_in;
    const msj_select_documents_result *in_sel;
    uint32_t flags, mode;
    uint64_t limit, capacity;
};

static inline Work layout(msj_carver &c, uint64_t capacity) {
    const uint64_t rows = most_rows(capacity);
    Work w;
    w.st = c.take<State>(1);
    for (int b = 0; b < 2; b++) w.hi[b] = c.take<uint64_t>(rows), w.aux[b] = c.take<uint64_t>(rows);
    w.cnt = c.take<uint32_t>(kBuckets * tiles_of(rows));
    w.bcnt = c.take<uint64_t>(rows / kRows + 1);
    return w;
}

// what every kernel reads of the call: N input rows over R records.  stop: nothing but the results is written
struct Head {
    uint64_t R, N, blocks;
    int32_t code;
    bool skip, stop, select;
};
__device__ __forceinline__ Head load_head(const Call &call) {
    Head h;
    const int32_t in_code = call.in_sel ? call.in_sel->code : 0, rows_code = call.sel->code;
    h.R = call.sel->n_documents;
    h.N = call.rows_in ? call.in_sel->n_documents : h.R;
    h.code = head_code(in_code, rows_code, h.R, call.stride, h.N, call.capacity, MSJ_CAPACITY);
    h.skip = in_code != 0 || rows_code != 0;
    h.stop = h.code != 0;
    h.blocks = h.stop ? 0 : (h.N + kRows - 1) / kRows;
    h.select = !h.stop && takes_selection(call.mode, call.limit, h.N);
    return h;
}
__device__ __forceinline__ uint64_t select_k(const Call &call, const Head &h) { return call.limit < h.N ? call.limit : h.N; }

// a block's LDS histograms of all the digits, zeroed / added to the global ones (lanes = kBuckets)
__device__ __forceinline__ void hist_zero(uint32_t (*s_hist)[kBuckets]) {
    for (uint32_t d = 0; d < kDigits; d++) s_hist[d][threadIdx.x] = 0;
    __syncthreads();
}
__device__ __forceinline__ void hist_flush(uint32_t (*s_hist)[kBuckets], uint32_t (*hist)[kBuckets]) {
    __syncthreads();
    for (uint32_t d = 0; d < kDigits; d++) {
        const uint32_t v = s_hist[d][threadIdx.x];
        if (v) atomicAdd(&hist[d][threadIdx.x], v);
    }
}

__global__ __launch_bounds__(kThreads) void sr_keys(const Call call, const Work w) {
    __shared__ uint32_t s_hist[kDigits][kBuckets];
    __shared__ uint32_t s_a[kWaves], s_b[kWaves], s_c[kWaves];
    const Head h = load_head(call);
    if (h.stop) return;
    hist_zero(s_hist);
    uint32_t values = 0, skipped = 0, out_of_range = 0;
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t j = v * kRows + threadIdx.x;
        const bool active = j < h.N;
        Key key{0, 0, 1};
        if (active) {
            const uint64_t row = call.rows_in ? call.rows_in[j] : j;  // (j < N <= capacity)
            out_of_range += row >= h.R;
            if (row < h.R) {
                const msj_field f = load_field(call.fields, row);  // (row < R <= stride)
                const uint32_t kind = value_kind(f);
                values += kind == kValue, skipped += kind == kSkipped;
                key = make_key(kind == kValue, f.type, f.bits, call.flags);
            }
            const uint64_t aux = aux_word(key, j);
            w.hi[0][j] = key.hi, w.aux[0][j] = aux;
        }
        const uint64_t aux = aux_word(key, 0);
#pragma unroll
        for (uint32_t d = 0; d < kDigits; d++) wave_hist_add(s_hist[d], digit_of(key.hi, aux, d), active);
    }
    hist_flush(s_hist, w.st->hist);
    (void)block_counter_add(values, s_a, reinterpret_cast<uint64_t *>(&w.st->n_values));
    (void)block_counter_add(skipped, s_b, reinterpret_cast<uint64_t *>(&w.st->n_skipped));
    (void)block_counter_add(out_of_range, s_c, reinterpret_cast<uint64_t *>(&w.st->n_out_of_range));
}

// ---- the selection ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void sl_hist(const Call call, const Work w, uint32_t d) {
    __shared__ uint32_t s_h[kBuckets], s_pd[kDigits];
    const Head h = load_head(call);
    if (!h.select || w.st->sl.done || !w.st->sl.own_hist) return;
    if (threadIdx.x < kDigits) s_pd[threadIdx.x] = w.st->sl.pd[threadIdx.x];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t j = v * kRows + threadIdx.x;
        uint64_t hi = 0, aux = 0;
        bool active = j < h.N;
        if (active) hi = w.hi[0][j], aux = w.aux[0][j];
        active = active && cmp_digits(hi, aux, s_pd, d + 1) == 0;
        wave_hist_add(s_h, digit_of(hi, aux, d), active);
    }
    __syncthreads();
    if (s_h[threadIdx.x]) atomicAdd(&w.st->hist_sl[d][threadIdx.x], s_h[threadIdx.x]);
}

__global__ __launch_bounds__(kThreads) void sl_pick(const Call call, const Work w, uint32_t d) {
    __shared__ uint32_t s_w[kWaves];
    const Head h = load_head(call);
    Select &sl = w.st->sl;
    if (!h.select || sl.done) return;
    const bool own = sl.own_hist != 0;
    const uint64_t K = select_k(call, h), below = sl.below, need = K - below;  // (1 <= need <= the rows that match)
    const uint32_t mine = own ? w.st->hist_sl[d][threadIdx.x] : w.st->hist[d][threadIdx.x];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = wave_scan32(mine, (int)lane);
    if (lane == 63) s_w[wave] = (uint32_t)inc;
    __syncthreads();
    inc = add_waves_before(inc, s_w, (int)wave);
    if (!(inc >= need && inc - mine < need)) return;  // one lane: the bucket of the K-th row
    const uint64_t new_below = below + (inc - mine), match = mine;
    sl.pd[d] = threadIdx.x, sl.low = d;
    sl.below = new_below, sl.match = match;
    if (!own && match != h.N) sl.own_hist = 1;
    const bool few = new_below + match <= select_enough(call.mode, K);
    if (few || d == 0) sl.done = 1, sl.take_eq = few ? match : K - new_below;
}

// 0: the row does not survive on its own count; 1: below the prefix; 2: equal to it
__device__ __forceinline__ uint32_t survivor_class(uint64_t hi, uint64_t aux, const uint32_t *pd, uint32_t low) {
    const int c = cmp_digits(hi, aux, pd, low);
    return c < 0 ? 1u : c == 0 ? 2u : 0u;
}

__global__ __launch_bounds__(kThreads) void sl_count(const Call call, const Work w) {
    __shared__ uint32_t s_pd[kDigits], s_cnt[kWaves];
    const Head h = load_head(call);
    if (!h.select) return;
    if (threadIdx.x < kDigits) s_pd[threadIdx.x] = w.st->sl.pd[threadIdx.x];
    const uint32_t low = w.st->sl.low;
    __syncthreads();
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t j = v * kRows + threadIdx.x;
        const uint32_t c = j < h.N ? survivor_class(w.hi[0][j], w.aux[0][j], s_pd, low) : 0u;
        const uint32_t cnt = wave_sum((c == 1 ? 1u : 0u) | (c == 2 ? 1u << 16 : 0u));  // (at most 64 of each)
        __syncthreads();  // (the last round's words have been read)
        if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t n = 0;
            for (int x = 0; x < kWaves; x++) n += s_cnt[x];
            w.bcnt[v] = (uint64_t)(n & 0xFFFFu) | (uint64_t)(n >> 16) << 32;
        }
    }
}

__global__ __launch_bounds__(1024) void sl_scan(const Call call, const Work w) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(call);
    if (!h.select) return;
    (void)scan_in_place(w.bcnt, h.blocks, s_w);  // (both halves stay below 2^31: no carry from one into the other)
}

__global__ __launch_bounds__(kThreads) void sl_place(const Call call, const Work w) {
    __shared__ uint32_t s_hist[kDigits][kBuckets];
    __shared__ uint32_t s_pd[kDigits], s_lt[kWaves], s_eq[kWaves];
    const Head h = load_head(call);
    if (!h.select) return;
    if (threadIdx.x < kDigits) s_pd[threadIdx.x] = w.st->sl.pd[threadIdx.x];
    const uint32_t low = w.st->sl.low, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t take_eq = w.st->sl.take_eq, n_surv = w.st->sl.below + take_eq;
    hist_zero(s_hist);
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t j = v * kRows + threadIdx.x;
        uint64_t hi = 0, aux = 0;
        uint32_t c = 0;
        if (j < h.N) hi = w.hi[0][j], aux = w.aux[0][j], c = survivor_class(hi, aux, s_pd, low);
        const uint64_t m_lt = __ballot(c == 1), m_eq = __ballot(c == 2);
        __syncthreads();  // (the last round's totals have been read)
        if (lane == 0) s_lt[wave] = (uint32_t)__popcll((unsigned long long)m_lt), s_eq[wave] = (uint32_t)__popcll((unsigned long long)m_eq);
        __syncthreads();
        const uint64_t before = w.bcnt[v];
        uint64_t lt = (before & 0xFFFFFFFFu) + lanes_below(m_lt), eq = (before >> 32) + lanes_below(m_eq);
        for (uint32_t x = 0; x < wave; x++) lt += s_lt[x], eq += s_eq[x];
        // the rows below the prefix in front of this one, and of those that equal it the ones that survive
        const bool keep = c == 1 || (c == 2 && eq < take_eq);
        const uint64_t at = lt + (eq < take_eq ? eq : take_eq);
        if (keep && at < n_surv) w.hi[1][at] = hi, w.aux[1][at] = aux;  // (at < n_surv <= N)
#pragma unroll
        for (uint32_t d = 0; d < kDigits; d++) wave_hist_add(s_hist[d], digit_of(hi, aux, d), keep);
    }
    hist_flush(s_hist, w.st->hist_sv);
}

// ---- the plan and the passes ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void sr_plan(const Call call, const Work w) {
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint32_t s_skip[kDigits];
    const Head h = load_head(call);
    if (h.stop) return;
    const uint64_t n = h.select ? w.st->sl.below + w.st->sl.take_eq : h.N;
    const uint32_t(*hist)[kBuckets] = h.select ? w.st->hist_sv : w.st->hist;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t d = 0; d < kDigits; d++) {
        const uint32_t mine = hist[d][threadIdx.x];
        uint32_t inc = wave_scan32(mine, (int)lane);
        __syncthreads();  // (the last digit's totals have been read)
        if (lane == 63) s_w[wave] = inc;
        if (threadIdx.x == 0) s_skip[d] = 0;
        __syncthreads();
        inc = add_waves_before(inc, s_w, (int)wave);
        w.st->plan.base[d][threadIdx.x] = inc - mine;
        if (n != 0 && mine == n) s_skip[d] = 1;  // (at most one bucket holds every row)
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t buffer = h.select ? 1u : 0u;
    for (uint32_t d = 0; d < kDigits; d++) {
        const uint32_t skip = n == 0 || s_skip[d];
        w.st->plan.skip[d] = skip, w.st->plan.src[d] = buffer;
        if (!skip) buffer ^= 1u;
    }
    w.st->plan.last = buffer;
    w.st->plan.n = n;
}

struct Pass {
    uint64_t n, tiles;
    uint32_t src;
    bool skip;
};
__device__ __forceinline__ Pass load_pass(const Work &w, uint32_t d) {
    Pass p;
    p.n = w.st->plan.n;  // (0 while the call stops: the memset's)
    p.skip = p.n == 0 || w.st->plan.skip[d] != 0;
    p.src = w.st->plan.src[d] & 1u;
    p.tiles = tiles_of(p.n);
    return p;
}

__global__ __launch_bounds__(kThreads) void sr_count(const Work w, uint32_t d) {
    __shared__ uint32_t s_h[kBuckets];
    const Pass p = load_pass(w, d);
    if (p.skip) return;
    const uint64_t *words = digit_in_hi(d) ? w.hi[p.src] : w.aux[p.src];
    const auto digit_at = [&](uint64_t j, uint32_t &digit) {
        const bool active = j < p.n;
        digit = active ? digit_of_word(words[j], d) : 0u;
        return active;
    };
    for (uint64_t v = blockIdx.x; v < p.tiles; v += gridDim.x) (void)msj_radix::count_tile(s_h, w.cnt, p.tiles, v, digit_at);
}

__global__ __launch_bounds__(kScan) void sr_scan(const Work w, uint32_t d) {
    __shared__ uint64_t s_w[16];
    const Pass p = load_pass(w, d);
    if (p.skip) return;
    (void)msj_radix::scan_bucket(w.cnt, p.tiles, s_w);
}

// a row of the scatter: its two words, from one pair of buffers to the other
struct Rows {
    struct Record {
        uint64_t hi, aux;
    };
    const uint64_t *src_hi, *src_aux;
    uint64_t *dst_hi, *dst_aux;
    uint64_t n;
    uint32_t d;
    __device__ __forceinline__ bool load(uint64_t j, Record &x) const {
        const bool active = j < n;
        x.hi = 0, x.aux = 0;
        if (active) x.hi = src_hi[j], x.aux = src_aux[j];
        return active;
    }
    __device__ __forceinline__ uint32_t digit(const Record &x) const { return digit_of(x.hi, x.aux, d); }
    __device__ __forceinline__ uint64_t bound() const { return n; }
    __device__ __forceinline__ void store(uint32_t at, const Record &x) const { dst_hi[at] = x.hi, dst_aux[at] = x.aux; }
};

__global__ __launch_bounds__(kThreads) void sr_scatter(const Work w, uint32_t d) {
    __shared__ uint32_t s_run[kBuckets], s_wcnt[kWaves][kBuckets];
    const Pass p = load_pass(w, d);
    if (p.skip) return;
    const Rows rows{w.hi[p.src], w.aux[p.src], w.hi[p.src ^ 1u], w.aux[p.src ^ 1u], p.n, d};
    const uint32_t base = w.st->plan.base[d][threadIdx.x];
    for (uint64_t v = blockIdx.x; v < p.tiles; v += gridDim.x) msj_radix::scatter_tile(s_run, s_wcnt, base, w.cnt, p.tiles, v, rows);
}

__global__ __launch_bounds__(kThreads) void sr_finish(const Call call, const Work w, uint32_t *__restrict__ order, msj_sort_rows_result *__restrict__ result,
                                                      msj_select_documents_result *__restrict__ order_select) {
    const Head h = load_head(call);
    const uint64_t n_values = h.stop ? 0 : w.st->n_values;
    const uint64_t K = h.stop ? 0 : rows_written(call.flags, call.limit, h.N, n_values);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        msj_sort_rows_result r;
        r.code = h.code;
        r.flags = h.skip ? 0 : call.flags;
        r.n_rows = h.skip ? 0 : h.N;
        r.n_values = n_values;
        r.n_written = K;
        r.n_skipped = h.stop ? 0 : w.st->n_skipped;
        r.n_out_of_range = h.stop ? 0 : w.st->n_out_of_range;
        *result = r;
        if (order_select) {
            msj_select_documents_result s;
            s.code = r.code, s.flags = 0;
            s.n_documents = K, s.n_paths = 1, s.n_found = K, s.n_no_bits = 0, s.reserved = 0;
            *order_select = s;
        }
    }
    if (K == 0) return;
    const uint64_t n = w.st->plan.n;  // (K <= n: the selection keeps at least min(limit, N) rows)
    const uint64_t *aux = w.aux[w.st->plan.last & 1u];
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < K && i < n; i += (uint64_t)gridDim.x * kThreads) {
        const uint32_t j = position_of(aux[i]);
        order[i] = call.rows_in && j < h.N ? call.rows_in[j] : j;  // (i < K; j < N <= capacity always: the buffers hold the call's own words)
    }
}

}  // namespace msj_srows

extern "C" uint64_t msj_sort_rows_workspace_bytes(uint64_t capacity) { return msj_measure(msj_srows::layout, capacity) + 64; }

extern "C" int msj_launch_sort_rows(const msj_field *d_fields, uint64_t stride, const msj_select_documents_result *d_rows_select,
                                    const uint32_t *d_rows_in, const msj_select_documents_result *d_rows_in_select, uint32_t flags, uint64_t limit,
                                    uint32_t mode, uint32_t *d_order, uint64_t capacity, msj_sort_rows_result *d_result,
                                    msj_select_documents_result *d_order_select, void *d_ws, void *stream) {
    using namespace msj_srows;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Call call{d_fields, stride, d_rows_select, d_rows_in, d_rows_in_select, flags, mode, limit, capacity};
    const Work w = msj_place(layout, d_ws, capacity);
    const hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(State), s);
    if (cleared != hipSuccess) return (int)cleared;
    const uint64_t most = most_rows(capacity), nb = (most + kRows - 1) / kRows, nt = tiles_of(most);
    const dim3 rows_grid((uint32_t)(nb > kRowBlocks ? kRowBlocks : nb)), tiles_grid((uint32_t)(nt > kTileBlocks ? kTileBlocks : nt)), block(kThreads);
    if (most) {
        hipLaunchKernelGGL(sr_keys, rows_grid, block, 0, s, call, w);
        if (limit != 0 && mode != kModeFull) {  // (whether the selection runs is decided on the device, from N)
            for (uint32_t d = kDigits; d-- > 0;) {
                hipLaunchKernelGGL(sl_hist, rows_grid, block, 0, s, call, w, d);
                hipLaunchKernelGGL(sl_pick, dim3(1), block, 0, s, call, w, d);
            }
            hipLaunchKernelGGL(sl_count, rows_grid, block, 0, s, call, w);
            hipLaunchKernelGGL(sl_scan, dim3(1), dim3(1024), 0, s, call, w);
            hipLaunchKernelGGL(sl_place, rows_grid, block, 0, s, call, w);
        }
        hipLaunchKernelGGL(sr_plan, dim3(1), block, 0, s, call, w);
        for (uint32_t d = 0; d < kDigits; d++) {
            hipLaunchKernelGGL(sr_count, tiles_grid, block, 0, s, w, d);
            hipLaunchKernelGGL(sr_scan, dim3(kBuckets), dim3(kScan), 0, s, w, d);
            hipLaunchKernelGGL(sr_scatter, tiles_grid, block, 0, s, w, d);
        }
    }
    hipLaunchKernelGGL(sr_finish, most ? rows_grid : dim3(1), block, 0, s, call, w, d_order, d_result, d_order_select);
    return (int)hipGetLastError();
}
