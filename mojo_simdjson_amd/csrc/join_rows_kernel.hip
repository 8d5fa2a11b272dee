// Equi-join of two code columns, as row pairs -- msj_join_rows_device (include/msj_stage1.h): from the int32 keys of L left
// rows and R right rows, codes of one dictionary of G entries, the pairs (l, r) of the INNER / LEFT / SEMI / ANTI join in
// ascending l and, inside a row, ascending r, with the running sum of the pairs per left row.  The arithmetic -- the key test,
// the digits for a G, the pairs a row emits, the row that owns a pair, the pair -- is join_rows_math.h, host + device and
// checked on the CPU by tests/test_join_rows_math.py.  L, R and G are read on the device by every kernel: the host sizes the
// launches by the rooms.
//
// Launches, all on the caller's stream, behind a memset of the call's state; the steps are separated by kernel boundaries
// only, and no lane ever waits for another lane or workgroup:
//   jn_clear    count[0 .. G] = 0
//   jn_count(p), jn_scan(p), jn_scatter(p)   one stable least-significant-digit pass over the right rows, radix_block.h's,
//               key_passes(G) of them (the launches behind that return at once): counts per (bucket, tile of 1 024 rows),
//               256 workgroups scan a bucket each and leave its total, the scatter ranks by ballots and LDS counters.
//               Stable is "ascending r inside a key".  Pass 0 reads the caller's keys, leaves out the rows without a key
//               (n_right_null) and counts count[key]: through the block's LDS histogram when G <= 256 -- the digit is the
//               key --, else by one integer atomic per row (one per wave where the wave's rows share the key).  The words
//               are (key, row number), four bytes each, in two buffers; the last pass stores no key
//   jn_start_sums, jn_start_scan, jn_start_apply   count[0 .. G] becomes its running sum: start[key], and start[G] = the rows
//               with a key
//   jn_left     a lane per left row: c(l) = start[key + 1] - start[key], n(l) into offsets[l], where the row's run starts
//               (or that it has none) into run[l], a tile's sum of n, n_left_null, n_left_matched
//   jn_total    one workgroup: the tiles' sums become running sums, M; the result, the two select results, offsets[L]
//   jn_offsets  offsets[l] = the tile's running sum + the sum of n in front inside the tile
//   jn_emit     organised by OUTPUT PAIR: a block takes kTile consecutive pair positions, finds the left rows of its first
//               and last pair by a search all its lanes share (256 probes a step), stages the offsets in between in LDS where
//               they fit (kStage; else the lanes search the global array: a stretch of rows that emit nothing), and every
//               lane finds its row by binary search and writes (l, sorted_right[run[l] + j - offsets[l]]): coalesced stores,
//               and a hot key whose one left row owns millions of pairs is spread over the grid like any other range
// Every count is an integer sum and every place a function of the counts: the same bytes from run to run.
// Safety: a key is read only below L / R; count / start only at a key below G <= keys_capacity, or at G; the buffers only
// below the rows with a key <= R (a scatter's place is tested against that once more); offsets only at or below L; the pairs
// only below M <= pairs_capacity.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "bytes_block.h"
#include "join_rows_math.h"
#include "launch.h"
#include "radix_block.h"

namespace msj_jrows {

using namespace msj::jrows;
using namespace msj::wave;
using msj_bytes::kRows, msj_bytes::most_rows;
using msj_radix::kRounds, msj_radix::kScan, msj_radix::kTile, msj_radix::kTileBlocks, msj_radix::tiles_of;  // also of keys and pairs
using msj_tape::block_scan, msj_tape::kThreads, msj_tape::kWaves;

static_assert(sizeof(msj_join_rows_result) == 64 && sizeof(msj_select_documents_result) == 48, "ABI");
static_assert(kRows == (uint32_t)kThreads && kWaves == 4 && kBuckets == (uint32_t)kThreads, "geometry");
static_assert(kBuckets == msj_radix::kBuckets && kDigitBits == msj_radix::kDigitBits, "the radix pass takes join_rows_math.h's digits");

constexpr uint32_t kEmitBlocks = 4096;       // most blocks of jn_emit
constexpr uint32_t kClearBlocks = 4096;      // most blocks of jn_clear
constexpr uint32_t kStage = kTile + 1;       // offsets jn_emit stages in LDS
constexpr uint32_t kMaxPasses = 4;           // key_passes(2^31)

struct State {  // cleared by a memset per call
    unsigned long long n_right_null, n_left_null, n_left_matched, n_pairs;
    uint32_t tot[kMaxPasses][kBuckets];  // jn_scan: the rows of every bucket of a pass
};
struct Work {
    State *st;
    uint32_t *start;            // [G + 1]: count[key], then its running sum
    uint32_t *csum;             // a sum per tile of keys
    uint32_t *key[2], *row[2];  // the right rows with a key; a pass reads one pair and writes the other
    uint32_t *cnt;              // [bucket * tiles + tile]
    uint32_t *run;              // per left row: the start of its run among the ordered right rows, or kNoRow
    uint64_t *off;              // [L + 1], where the caller gives no d_offsets
    uint64_t *bsum;             // a sum of n per tile of left rows
};
struct Call {
    const int32_t *left_keys;
    uint64_t left_rows;
    const uint64_t *n_left;
    const int32_t *right_keys;
    uint64_t right_rows;
    const uint64_t *n_right;
    uint64_t n_keys;
    const uint64_t *d_n_keys;
    uint64_t keys_capacity;
    uint32_t flags;
    uint64_t pairs_capacity;
};

static inline Work layout(msj_carver &c, uint64_t left_rows, uint64_t right_rows, uint64_t keys_capacity) {
    const uint64_t l = most_rows(left_rows), r = most_rows(right_rows), g = most_keys(keys_capacity) + 1;
    Work w;
    w.st = c.take<State>(1);
    w.start = c.take<uint32_t>(g);
    w.csum = c.take<uint32_t>(tiles_of(g));
    for (int b = 0; b < 2; b++) w.key[b] = c.take<uint32_t>(r), w.row[b] = c.take<uint32_t>(r);
    w.cnt = c.take<uint32_t>(kBuckets * tiles_of(r));
    w.run = c.take<uint32_t>(l);
    w.off = c.take<uint64_t>(l + 1);
    w.bsum = c.take<uint64_t>(tiles_of(l) + 1);
    return w;
}

// what every kernel reads of the call.  stop: nothing but the result is written
struct Head {
    uint64_t L, R, G, keys;  // keys: G as the tables and the key test take it (most_keys)
    uint32_t kind, passes;
    bool stop;
};
__device__ __forceinline__ Head load_head(const Call &call) {
    Head h;
    h.L = call.n_left ? *call.n_left : call.left_rows;
    h.R = call.n_right ? *call.n_right : call.right_rows;
    h.G = call.d_n_keys ? *call.d_n_keys : call.n_keys;
    h.stop = counts_over(h.L, call.left_rows, h.R, call.right_rows, h.G, call.keys_capacity);
    h.keys = most_keys(h.G);
    h.kind = call.flags & 3u;
    h.passes = key_passes(h.G);
    return h;
}

__global__ __launch_bounds__(kThreads) void jn_clear(const Call call, const Work w) {
    const Head h = load_head(call);
    if (h.stop) return;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i <= h.keys; i += (uint64_t)gridDim.x * kThreads) w.start[i] = 0;  // (keys <= most_keys(keys_capacity))
}

// ---- the right rows in the order of their keys --------------------------------------------------------------------------------
// a pass, and as radix_block.h's policy a right row of its scatter: (key, row number)
struct Pass {
    struct Record {
        uint32_t key, row;
    };
    uint64_t n, valid, tiles;  // the rows the pass reads; the rows with a key (pass 0: not known yet)
    uint64_t keys;
    uint32_t p;
    const uint32_t *src_key, *src_row;
    uint32_t *dst_key, *dst_row;
    bool skip, first, last;
    // pass 0 reads the caller's keys: the row number is the position, and a row without a key stays behind
    __device__ __forceinline__ bool load(uint64_t j, Record &x) const {
        bool active = j < n;
        x.key = 0, x.row = (uint32_t)j;
        if (active) {
            x.key = src_key[j];
            if (first) active = is_key((int32_t)x.key, keys);
            else x.row = src_row[j];
        }
        return active;
    }
    __device__ __forceinline__ uint32_t digit(const Record &x) const { return digit_of(x.key, p); }
    __device__ __forceinline__ uint64_t bound() const { return valid; }
    __device__ __forceinline__ void store(uint32_t at, const Record &x) const {
        dst_row[at] = x.row;
        if (!last) dst_key[at] = x.key;
    }
};
__device__ __forceinline__ Pass load_pass(const Call &call, const Work &w, const Head &h, uint32_t p) {
    Pass s;
    s.keys = h.keys, s.p = p;
    s.skip = h.stop || p >= h.passes;
    s.first = p == 0, s.last = p + 1 == h.passes;
    const uint64_t nulls = w.st->n_right_null;  // (complete behind pass 0's count)
    s.valid = h.R >= nulls ? h.R - nulls : 0;
    s.n = s.skip ? 0 : s.first ? h.R : s.valid;
    s.tiles = tiles_of(s.n);
    s.src_key = s.first ? reinterpret_cast<const uint32_t *>(call.right_keys) : w.key[(p - 1) & 1u];
    s.src_row = s.first ? nullptr : w.row[(p - 1) & 1u];
    s.dst_key = w.key[p & 1u], s.dst_row = w.row[p & 1u];
    return s;
}

__global__ __launch_bounds__(kThreads) void jn_count(const Call call, const Work w, uint32_t p) {
    __shared__ uint32_t s_h[kBuckets], s_tot[kBuckets], s_n[kWaves];
    const Head h = load_head(call);
    const Pass s = load_pass(call, w, h, p);
    if (s.skip) return;
    const bool small = h.keys <= kBuckets;  // the digit is the key: count[key] through s_tot
    s_tot[threadIdx.x] = 0;
    uint32_t nulls = 0;
    const auto digit_at = [&](uint64_t j, uint32_t &digit) {
        bool active = j < s.n;
        const uint32_t key = active ? s.src_key[j] : 0u;  // (j < R <= right_rows; j < valid <= R)
        if (s.first) {
            const bool valid = active && is_key((int32_t)key, h.keys);
            nulls += active && !valid;
            active = valid;
            if (!small) wave_hist_add(w.start, key, active);  // (key < keys)
        }
        digit = digit_of(key, p);
        return active;
    };
    for (uint64_t v = blockIdx.x; v < s.tiles; v += gridDim.x) s_tot[threadIdx.x] += msj_radix::count_tile(s_h, w.cnt, s.tiles, v, digit_at);
    if (!s.first) return;
    if (small && threadIdx.x < h.keys && s_tot[threadIdx.x]) atomicAdd(&w.start[threadIdx.x], s_tot[threadIdx.x]);
    (void)block_counter_add(nulls, s_n, reinterpret_cast<uint64_t *>(&w.st->n_right_null));
}

__global__ __launch_bounds__(kScan) void jn_scan(const Call call, const Work w, uint32_t p) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(call);
    const Pass s = load_pass(call, w, h, p);
    if (s.skip) return;
    const uint64_t total = msj_radix::scan_bucket(w.cnt, s.tiles, s_w);
    if (threadIdx.x == 0) w.st->tot[p][blockIdx.x] = (uint32_t)total;
}

__global__ __launch_bounds__(kThreads) void jn_scatter(const Call call, const Work w, uint32_t p) {
    __shared__ uint32_t s_run[kBuckets], s_wcnt[kWaves][kBuckets], s_w[kWaves];
    const Head h = load_head(call);
    const Pass s = load_pass(call, w, h, p);
    if (s.skip) return;
    const uint32_t base = msj_radix::bucket_base(w.st->tot[p], s_w);  // the rows in the buckets in front
    for (uint64_t v = blockIdx.x; v < s.tiles; v += gridDim.x) msj_radix::scatter_tile(s_run, s_wcnt, base, w.cnt, s.tiles, v, s);
}

// ---- count[0 .. G] becomes start[0 .. G] --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void jn_start_sums(const Call call, const Work w) {
    __shared__ uint32_t s_w[kWaves];
    const Head h = load_head(call);
    if (h.stop) return;
    const uint64_t n = h.keys + 1, tiles = tiles_of(n);
    for (uint64_t v = blockIdx.x; v < tiles; v += gridDim.x) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t r = 0; r < kRounds; r++) {
            const uint64_t i = v * kTile + r * kRows + threadIdx.x;
            sum += i < n ? w.start[i] : 0u;
        }
        uint32_t total;
        (void)block_scan(sum, s_w, total);
        if (threadIdx.x == 0) w.csum[v] = total;  // (below R < 2^31)
    }
}
__global__ __launch_bounds__(kScan) void jn_start_scan(const Call call, const Work w) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(call);
    if (h.stop) return;
    (void)scan_in_place(w.csum, tiles_of(h.keys + 1), s_w);
}
__global__ __launch_bounds__(kThreads) void jn_start_apply(const Call call, const Work w) {
    __shared__ uint32_t s_w[kWaves];
    const Head h = load_head(call);
    if (h.stop) return;
    const uint64_t n = h.keys + 1, tiles = tiles_of(n);
    for (uint64_t v = blockIdx.x; v < tiles; v += gridDim.x) {
        uint32_t run = w.csum[v];
        for (uint32_t r = 0; r < kRounds; r++) {
            const uint64_t i = v * kTile + r * kRows + threadIdx.x;
            const uint32_t x = i < n ? w.start[i] : 0u;
            uint32_t total;
            const uint32_t before = block_scan(x, s_w, total);
            if (i < n) w.start[i] = run + before;
            run += total;
        }
    }
}

// ---- the left rows ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void jn_left(const Call call, const Work w, uint64_t *__restrict__ off) {
    __shared__ uint64_t s_sum[kWaves];
    __shared__ uint32_t s_a[kWaves], s_b[kWaves];
    const Head h = load_head(call);
    if (h.stop) return;
    const uint64_t tiles = tiles_of(h.L);
    uint32_t nulls = 0, matched = 0;
    for (uint64_t v = blockIdx.x; v < tiles; v += gridDim.x) {
        uint64_t sum = 0;
#pragma unroll
        for (uint32_t r = 0; r < kRounds; r++) {
            const uint64_t l = v * kTile + r * kRows + threadIdx.x;
            if (l >= h.L) continue;
            const int32_t key = call.left_keys[l];  // (l < L <= left_rows)
            uint32_t c = 0, start = 0;
            if (is_key(key, h.keys)) start = w.start[key], c = w.start[(uint64_t)key + 1] - start;  // (key + 1 <= keys)
            else nulls++;
            matched += c != 0;
            const uint64_t n = pairs_of_row(h.kind, c);
            w.run[l] = run_of_row(h.kind, c, start);
            off[l] = n;
            sum += n;
        }
        uint64_t total;
        (void)block_scan(sum, s_sum, total);
        if (threadIdx.x == 0) w.bsum[v] = total;
    }
    (void)block_counter_add(nulls, s_a, reinterpret_cast<uint64_t *>(&w.st->n_left_null));
    (void)block_counter_add(matched, s_b, reinterpret_cast<uint64_t *>(&w.st->n_left_matched));
}

__global__ __launch_bounds__(kScan) void jn_total(const Call call, const Work w, uint64_t *__restrict__ off, msj_join_rows_result *__restrict__ result,
                                                  msj_select_documents_result *__restrict__ left_select,
                                                  msj_select_documents_result *__restrict__ right_select) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(call);
    uint64_t M = 0;
    if (!h.stop) M = scan_in_place(w.bsum, tiles_of(h.L), s_w);
    if (threadIdx.x != 0) return;
    msj_join_rows_result r;
    r.code = h.stop || pairs_over(M, call.pairs_capacity) ? MSJ_CAPACITY : 0;
    r.flags = call.flags;
    r.n_left = h.L, r.n_right = h.R, r.n_keys = h.G;
    r.n_pairs = M;
    r.n_left_matched = h.stop ? 0 : w.st->n_left_matched;
    r.n_left_null = h.stop ? 0 : w.st->n_left_null;
    r.n_right_null = h.stop ? 0 : w.st->n_right_null;
    *result = r;
    msj_select_documents_result s;
    s.code = r.code, s.flags = 0;
    s.n_documents = M, s.n_paths = 1, s.n_found = M, s.n_no_bits = 0, s.reserved = 0;
    if (left_select) *left_select = s;
    if (right_select) *right_select = s;
    if (h.stop) return;
    w.st->n_pairs = M;
    off[h.L] = M;
}

__global__ __launch_bounds__(kThreads) void jn_offsets(const Call call, const Work w, uint64_t *__restrict__ off) {
    __shared__ uint64_t s_w[kWaves];
    const Head h = load_head(call);
    if (h.stop) return;
    const uint64_t tiles = tiles_of(h.L);
    for (uint64_t v = blockIdx.x; v < tiles; v += gridDim.x) {
        uint64_t run = w.bsum[v];
        for (uint32_t r = 0; r < kRounds; r++) {
            const uint64_t l = v * kTile + r * kRows + threadIdx.x;
            const uint64_t x = l < h.L ? off[l] : 0;
            uint64_t total;
            const uint64_t before = block_scan(x, s_w, total);
            if (l < h.L) off[l] = run + before;
            run += total;
        }
    }
}

// ---- the pairs --------------------------------------------------------------------------------------------------------------
// the last row l in [lo, hi) with off[l] <= j, for the whole workgroup (off[lo] <= j < off[hi]): 256 probes a step
__device__ __forceinline__ uint64_t block_row_of_pair(const uint64_t *__restrict__ off, uint64_t lo, uint64_t hi, uint64_t j) {
    while (hi - lo > 1) {
        const uint64_t step = (hi - lo + kThreads - 1) / kThreads;
        const uint64_t p = lo + (threadIdx.x + 1) * step;
        const uint32_t below = (uint32_t)__syncthreads_count(p < hi && off[p] <= j);  // (the probes in front of the first one above j)
        const uint64_t up = lo + (below + 1) * step;
        lo += below * step;
        hi = up < hi ? up : hi;
    }
    return lo;
}
struct StagedOffsets {
    const uint64_t *s;
    __device__ __forceinline__ uint64_t operator[](uint64_t i) const { return s[i]; }
};

__global__ __launch_bounds__(kThreads) void jn_emit(const Call call, const Work w, const uint64_t *__restrict__ off, uint32_t *__restrict__ left_rows,
                                                    uint32_t *__restrict__ right_rows) {
    __shared__ uint64_t s_off[kStage];
    const Head h = load_head(call);
    if (h.stop) return;
    const uint64_t M = w.st->n_pairs;
    if (M == 0 || pairs_over(M, call.pairs_capacity)) return;
    const uint64_t nulls = w.st->n_right_null, valid = h.R >= nulls ? h.R - nulls : 0;
    const uint32_t *sorted = w.row[(h.passes - 1) & 1u];
    const uint64_t tiles = tiles_of(M);
    for (uint64_t v = blockIdx.x; v < tiles; v += gridDim.x) {
        const uint64_t j0 = v * kTile, j1 = (j0 + kTile < M ? j0 + kTile : M) - 1;
        const uint64_t lo = block_row_of_pair(off, 0, h.L, j0);  // (off[0] = 0 <= j0 < M = off[L])
        const uint64_t hi = block_row_of_pair(off, lo, h.L, j1);
        const uint64_t span = hi - lo + 1;
        const bool staged = span <= kStage;  // else: a stretch of rows that emit nothing
        __syncthreads();                     // (the last tile's offsets have been read)
        if (staged)
            for (uint64_t i = threadIdx.x; i < span; i += kThreads) s_off[i] = off[lo + i];
        __syncthreads();
        for (uint32_t r = 0; r < kRounds; r++) {
            const uint64_t j = j0 + r * kRows + threadIdx.x;
            if (j > j1) continue;
            uint64_t l, first;
            if (staged) {
                const uint64_t i = row_of_pair(StagedOffsets{s_off}, 0, span - 1, j);
                l = lo + i, first = s_off[i];
            } else {
                l = row_of_pair(off, lo, hi, j), first = off[l];
            }
            left_rows[j] = (uint32_t)l;  // (j < M <= pairs_capacity; l < L < 2^31)
            if (!right_rows) continue;
            const uint32_t place = right_place(h.kind, w.run[l], j - first);
            right_rows[j] = place != kNoRow && place < valid ? sorted[place] : kNoRow;
        }
    }
}

}  // namespace msj_jrows

extern "C" uint64_t msj_join_rows_workspace_bytes(uint64_t left_rows, uint64_t right_rows, uint64_t keys_capacity) {
    return msj_measure(msj_jrows::layout, left_rows, right_rows, keys_capacity) + 64;
}

extern "C" int msj_launch_join_rows(const int32_t *d_left_keys, uint64_t left_rows, const uint64_t *d_n_left, const int32_t *d_right_keys,
                                    uint64_t right_rows, const uint64_t *d_n_right, uint64_t n_keys, const uint64_t *d_n_keys,
                                    uint64_t keys_capacity, uint32_t flags, uint32_t *d_left_rows, uint32_t *d_right_rows, uint64_t pairs_capacity,
                                    uint64_t *d_offsets, msj_join_rows_result *d_result, msj_select_documents_result *d_left_select,
                                    msj_select_documents_result *d_right_select, void *d_ws, void *stream) {
    using namespace msj_jrows;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Call call{d_left_keys, left_rows, d_n_left, d_right_keys, right_rows, d_n_right, n_keys, d_n_keys, keys_capacity, flags, pairs_capacity};
    const Work w = msj_place(layout, d_ws, left_rows, right_rows, keys_capacity);
    uint64_t *off = d_offsets ? d_offsets : w.off;
    const hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(State), s);
    if (cleared != hipSuccess) return (int)cleared;
    const uint64_t l = most_rows(left_rows), r = most_rows(right_rows), g = most_keys(keys_capacity) + 1;
    auto grid_of = [](uint64_t blocks, uint32_t most) { return dim3((uint32_t)(blocks > most ? most : blocks ? blocks : 1)); };
    const dim3 block(kThreads), keys_grid = grid_of(tiles_of(g), kTileBlocks), left_grid = grid_of(tiles_of(l), kTileBlocks),
               right_grid = grid_of(tiles_of(r), kTileBlocks);
    hipLaunchKernelGGL(jn_clear, grid_of((g + kThreads - 1) / kThreads, kClearBlocks), block, 0, s, call, w);
    if (r) {
        const uint32_t passes = key_passes(keys_capacity);  // (how many of them run is decided on the device, from G)
        for (uint32_t p = 0; p < passes; p++) {
            hipLaunchKernelGGL(jn_count, right_grid, block, 0, s, call, w, p);
            hipLaunchKernelGGL(jn_scan, dim3(kBuckets), dim3(kScan), 0, s, call, w, p);
            hipLaunchKernelGGL(jn_scatter, right_grid, block, 0, s, call, w, p);
        }
        hipLaunchKernelGGL(jn_start_sums, keys_grid, block, 0, s, call, w);
        hipLaunchKernelGGL(jn_start_scan, dim3(1), dim3(kScan), 0, s, call, w);
        hipLaunchKernelGGL(jn_start_apply, keys_grid, block, 0, s, call, w);
    }
    if (l) hipLaunchKernelGGL(jn_left, left_grid, block, 0, s, call, w, off);
    hipLaunchKernelGGL(jn_total, dim3(1), dim3(kScan), 0, s, call, w, off, d_result, d_left_select, d_right_select);
    if (l) hipLaunchKernelGGL(jn_offsets, left_grid, block, 0, s, call, w, off);
    if (l && pairs_capacity) hipLaunchKernelGGL(jn_emit, grid_of(tiles_of(pairs_capacity), kEmitBlocks), block, 0, s, call, w, off, d_left_rows, d_right_rows);
    return (int)hipGetLastError();
}
