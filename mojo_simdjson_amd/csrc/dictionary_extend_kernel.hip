// One dictionary across windows -- msj_dictionary_extend_device (include/msj_stage1.h): a byte column encoded against the P
// entries the dictionary arrays already hold, its new values appended behind them, or (MSJ_DICTIONARY_FROZEN) looked up
// only.  The design is dictionary_kernel.hip's over ITEMS instead of rows (dictionary_extend_math.h): item c < P is prior
// entry c, item P + k is row k, and the table of S uint32 holds item numbers, S the power of two >= 2 (P + R).  insert_row's
// atomicMin towards the smallest item makes a prior entry win over every row and the lower of two equal prior entries over
// the higher; the new values keep the order of first appearance.  The arithmetic is dictionary_math.h's and
// dictionary_extend_math.h's, host + device, checked on the CPU by tests/test_dictionary_extend_math.py.  R and P are read
// on the device by every kernel: the host sizes the launches by `rows` and `dict_capacity`.
//
// A block owns kRows consecutive items -- block v the items [v * kRows, + kRows), the grid loops over the blocks P + R
// needs; the kernels over the rows alone start at the block that holds item P.  Launches, all on the caller's stream, behind
// a memset of the call's counters and one of the table to "empty"; the passes are separated by kernel boundaries only, and no
// lane ever waits for another lane or workgroup:
//   dx_hash     a lane per item: the entry test or the row test, and the length.  The words of the block's items are numbered
//               through an exclusive sum in LDS and the lanes take CONSECUTIVE words of the block, as dc_hash does -- prior
//               entries lie back to back in d_dict_bytes, rows in d_bytes.  An item LONGER THAN kLongItem = 512 bytes goes on
//               the list of long items (kLongCap = 1 024 entries); one that finds the list full is hashed by its own wave
//   dx_long_hash   a wave per listed item, in 64-lane steps
//   dx_insert   a lane per item that has a value and is not long: insert_row.  Frozen: the prior entries only.  Long items
//               that are not listed: the same walk by the item's wave, the compare in 64-lane steps
//   dx_long_insert   a wave per listed item
//  then, unless frozen:
//   dx_count    row item i is a first occurrence iff table[slot[i]] == i, and matches a prior entry iff table[slot[i]] < P:
//               per block the first rows and their bytes
//   dx_scan     one workgroup: the exclusive sums over both block arrays, d_dict_offsets[0] when P == 0, the result
//   dx_place    the first rows: their code (P + block base + sum inside the block), d_dict_first, d_dict_offsets (base + ...);
//               null rows: -1
//   dx_codes    every other row: the prior entry in its slot, or d_codes[that first row]
//   dx_copy     dc_copy's organisation by OUTPUT bytes, from `base` on: the first piece starts at base itself and goes byte
//               by byte up to the next 16-byte boundary, so no byte below base is written
//  and when frozen:
//   dx_lookup   a lane per row (a wave per long row): lookup_item -- the prior entry in the slot, or -2; the counts
//   dx_scan     the result
// Atomics on the table are relaxed, device scope, as in dictionary_kernel.hip: "empty" is settled by the CAS, and an item
// once seen in a slot is of the slot's value for good.
// Safety: prior offsets are used only after the entry test (inside [0, dict_bytes_capacity), ascending), row offsets only
// after the row test; items are below P + R <= dict_capacity + rows, which sizes the workspace; table values are items this
// call inserted; every dictionary store is at or past P / base and below its capacity.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "bytes_block.h"
#include "dictionary_extend_math.h"
#include "launch.h"

namespace msj_dictx {

using namespace msj::dictx;
using namespace msj::wave;
using msj_bytes::kGridBlocks, msj_bytes::kRows, msj_bytes::most_rows;
using msj_tape::block_scan, msj_tape::kThreads, msj_tape::kWaves;

constexpr uint64_t kLongItem = 512;   // an item of more bytes than this is hashed and compared by a wave, not by a lane
constexpr uint32_t kLongCap = 1024;   // entries of the list of long items
constexpr uint32_t kLongGrid = 256;   // blocks of the two list kernels: a wave per listed item
constexpr uint32_t kPiece = 16384;    // bytes of aligned output a block of dx_copy takes at a time
constexpr uint32_t kCopyGrid = 2048;  // most blocks of dx_copy

static_assert(sizeof(msj_dictionary_extend_result) == 64, "ABI");
static_assert(kPiece % (16 * kThreads) == 0 && kRows == (uint32_t)kThreads, "geometry");

struct State {  // cleared by a memset per call
    unsigned long long n_values, n_matched, max_probe;
    uint64_t n_distinct, dict_bytes;  // (dx_scan)
    uint32_t n_long, exhausted;       // long items met (those past kLongCap are not on the list); a walk found no slot
    uint64_t reserved[2];
};
struct Work {
    State *st;
    uint64_t *hash;   // per item
    uint32_t *slot;   // per item: between dx_hash and the inserts 1 for a listed item, then the item's slot
    uint32_t *table;  // S slots: kEmpty, or an item
    uint64_t *bcnt;   // per block of rows: its first rows, then (dx_scan) the first rows in front of the block
    uint64_t *blen;   // per block of rows: the bytes of its first rows, then the bytes in front
    uint32_t *list;   // the long items
};
// the column, the dictionary and the call
struct Call {
    Source src;
    uint64_t rows;
    const uint64_t *n_rows;
    uint64_t n_prior;
    const uint64_t *d_n_prior;
    uint64_t *dict_offsets;
    uint32_t *dict_first;
    uint64_t dict_capacity;
    uint8_t *dict_bytes;
    uint32_t flags;
};

// the most items a call of these sizes can have
__host__ __device__ inline uint64_t most_items(uint64_t rows, uint64_t dict_capacity) {
    return most_rows(rows + dict_capacity < rows ? ~0ull : rows + dict_capacity);
}
static inline Work layout(msj_carver &c, uint64_t rows, uint64_t dict_capacity) {
    const uint64_t items = most_items(rows, dict_capacity);
    Work w;
    w.st = c.take<State>(1);
    w.hash = c.take<uint64_t>(items);
    w.slot = c.take<uint32_t>(items);
    w.table = c.take<uint32_t>(table_slots(items));
    w.bcnt = c.take<uint64_t>(items / kRows + 1);
    w.blen = c.take<uint64_t>(items / kRows + 1);
    w.list = c.take<uint32_t>(kLongCap);
    return w;
}

// what every kernel reads first: P prior entries and R rows, N items in `blocks` blocks of which `row_block` is the first that
// holds a row, the table's S slots.  over: nothing but the result is written
struct Head {
    uint64_t R, P, base, N, blocks, row_block, S;
    bool over, frozen;
};
__device__ __forceinline__ Head load_head(const Call &c) {
    Head h;
    h.R = c.n_rows ? *c.n_rows : c.rows;
    h.P = c.d_n_prior ? *c.d_n_prior : c.n_prior;
    const Counts n = counts_of(h.R, c.rows, h.P, c.dict_offsets, c.dict_capacity, c.src.dict_bytes_capacity);
    h.over = n.over, h.base = n.base;
    h.frozen = (c.flags & kFrozen) != 0;
    h.N = h.over ? 0 : h.P + h.R;
    h.blocks = (h.N + kRows - 1) / kRows;
    h.row_block = h.over ? 0 : h.P / kRows;
    h.S = extend_slots(h.over ? 0 : h.P, h.over ? 0 : h.R, c.flags);
    return h;
}
__device__ __forceinline__ Item item_at(const Call &c, const Head &h, uint64_t i) {
    return i < h.N ? item_of(c.src, h.P, i) : Item{nullptr, 0, false};
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) { return (uint64_t)__shfl((unsigned long long)v, src); }
__device__ __forceinline__ Item shfl_item(const Item &y, int src) {
    return Item{reinterpret_cast<const uint8_t *>(shfl64(reinterpret_cast<uintptr_t>(y.p), src)), shfl64(y.len, src), true};
}

// ---- the hash ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t wave_hash(const Item &y, uint32_t lane, uint32_t flags) {
    return hash_finish(wave_sum64(hash_piece(y.p, y.len, lane, 64)), y.len, flags);
}

__global__ __launch_bounds__(kThreads) void dx_hash(const Call c, const Work w) {
    __shared__ uint64_t s_ws[kRows + 1], s_len[kRows], s_w[kWaves];
    __shared__ const uint8_t *s_p[kRows];
    __shared__ unsigned long long s_acc[kRows];
    const Head h = load_head(c);
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t i = v * kRows + threadIdx.x;
        const Item y = item_at(c, h, i);
        const bool is_long = y.len > kLongItem;
        bool listed = false;
        if (is_long) {
            const uint32_t e = atomicAdd(&w.st->n_long, 1u);
            if (e < kLongCap) w.list[e] = (uint32_t)i, listed = true;  // (i < N < 2^31)
        }
        uint64_t total;
        const uint64_t ws = block_scan(is_long ? 0 : words_of(y.len), s_w, total);  // (its barrier: the last round's words have been read)
        s_ws[threadIdx.x] = ws, s_p[threadIdx.x] = y.p, s_len[threadIdx.x] = is_long ? 0 : y.len, s_acc[threadIdx.x] = 0;
        if (threadIdx.x == 0) s_ws[kRows] = total;
        __syncthreads();
        for (uint64_t u = threadIdx.x; u < total; u += kThreads) {
            const uint32_t it = row_of_byte(s_ws, kRows, u);  // (items without a word own nothing)
            const uint64_t j = u - s_ws[it];
            atomicAdd(&s_acc[it], (unsigned long long)mix(load_word(s_p[it], j, s_len[it]), j));
        }
        __syncthreads();
        if (i < h.N) {
            if (!is_long) w.hash[i] = hash_finish(s_acc[threadIdx.x], y.len, c.flags);
            w.slot[i] = listed ? 1u : 0u;
        }
        for (uint64_t m = __ballot(is_long && !listed); m; m &= m - 1) {  // the list was full: by the item's own wave
            const int src = __ffsll((unsigned long long)m) - 1;
            const uint64_t hz = wave_hash(shfl_item(y, src), lane, c.flags);
            if ((int)lane == src) w.hash[i] = hz;
        }
    }
}

__global__ __launch_bounds__(kThreads) void dx_long_hash(const Call c, const Work w) {
    const Head h = load_head(c);
    if (h.over) return;
    const uint32_t met = w.st->n_long, nl = met < kLongCap ? met : kLongCap;
    const uint32_t waves = gridDim.x * kWaves, wave = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (uint32_t e = wave; e < nl; e += waves) {
        const uint64_t i = w.list[e];
        const Item y = item_at(c, h, i);
        if (!y.has) continue;  // (never: dx_hash listed it)
        const uint64_t hy = wave_hash(y, lane, c.flags);
        if (lane == 0) w.hash[i] = hy;
    }
}

// ---- the table --------------------------------------------------------------------------------------------------------------
// insert_row's and lookup_item's Table for one lane, and for a wave that walks together (lane 0 has the atomics, every lane
// the answer)
struct LaneTable {
    uint32_t *t;
    __device__ __forceinline__ uint32_t load(uint64_t i) const { return __hip_atomic_load(t + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint32_t claim(uint64_t i, uint32_t k) const {
        uint32_t seen = kEmpty;
        (void)__hip_atomic_compare_exchange_strong(t + i, &seen, k, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return seen;  // (kEmpty: exchanged)
    }
    __device__ __forceinline__ void lower(uint64_t i, uint32_t k) const { (void)__hip_atomic_fetch_min(t + i, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
struct WaveTable {
    LaneTable lt;
    uint32_t lane;
    __device__ __forceinline__ uint32_t load(uint64_t i) const { return (uint32_t)__shfl((int)lt.load(i), 0); }  // (one answer for the wave)
    __device__ __forceinline__ uint32_t claim(uint64_t i, uint32_t k) const {
        uint32_t seen = 0;
        if (lane == 0) seen = lt.claim(i, k);
        return (uint32_t)__shfl((int)seen, 0);
    }
    __device__ __forceinline__ void lower(uint64_t i, uint32_t k) const {
        if (lane == 0) lt.lower(i, k);
    }
};
// same(r): item r has the value of the item y with hash hy.  r is an item some walk put into the table: it has a value
struct Same {
    const Call &c;
    const Work &w;
    const Head &h;
    uint64_t hy;
    Item y;
    uint32_t first, step;  // 0, 1: a lane alone; lane, 64: a wave together
    __device__ __forceinline__ bool operator()(uint32_t r) const {
        if (w.hash[r] != hy) return false;
        const Item z = item_at(c, h, r);
        if (!z.has || z.len != y.len) return false;
        const bool eq = equal_piece(y.p, z.p, y.len, first, step);
        return step == 1 ? eq : __ballot(!eq) == 0;
    }
};
// an item's walk by its wave: insert_row, or for a row of the frozen form lookup_item
__device__ __forceinline__ Walk wave_walk(const Call &c, const Work &w, const Head &h, uint64_t i, const Item &y, uint32_t lane, bool insert) {
    WaveTable t{LaneTable{w.table}, lane};
    const uint64_t hy = w.hash[i];
    const Same same{c, w, h, hy, y, lane, 64};
    return insert ? insert_row(t, h.S, hy, (uint32_t)i, same) : lookup_item(t, h.S, hy, same);
}
// the walk's end, every lane of the wave calls (probes 0: no walk): the longest walk to the state
__device__ __forceinline__ void probes_out(const Work &w, const Walk &wk, bool keeps) {
    const unsigned long long longest = wave_reduce((unsigned long long)(keeps ? wk.probes : 0), [](auto a, auto b) { return a > b ? a : b; });
    if ((threadIdx.x & 63) == 0 && longest > w.st->max_probe) atomicMax(&w.st->max_probe, longest);
}
// ... and behind an insert the slot kept by `keeps`
__device__ __forceinline__ void walk_out(const Work &w, uint64_t i, const Walk &wk, bool keeps) {
    if (keeps) {
        w.slot[i] = (uint32_t)wk.slot;  // (S <= 2^32)
        if (!wk.found) w.st->exhausted = 1;
    }
    probes_out(w, wk, keeps);
}

__global__ __launch_bounds__(kThreads) void dx_insert(const Call c, const Work w) {
    const Head h = load_head(c);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t N = h.frozen && !h.over ? h.P : h.N, blocks = (N + kRows - 1) / kRows;  // frozen: the prior entries only
    for (uint64_t v = blockIdx.x; v < blocks; v += gridDim.x) {
        const uint64_t i = v * kRows + threadIdx.x;
        const Item y = i < N ? item_at(c, h, i) : Item{nullptr, 0, false};
        const bool is_long = y.len > kLongItem, listed = is_long && w.slot[i] != 0;
        Walk wk{0, 0, true};
        const bool alone = y.has && !is_long;
        if (alone) {
            LaneTable t{w.table};
            const uint64_t hy = w.hash[i];
            wk = insert_row(t, h.S, hy, (uint32_t)i, Same{c, w, h, hy, y, 0, 1});
        }
        walk_out(w, i, wk, alone);
        for (uint64_t m = __ballot(is_long && !listed); m; m &= m - 1) {  // the list was full: by the item's own wave
            const int src = __ffsll((unsigned long long)m) - 1;
            const uint64_t iz = shfl64(i, src);
            const Walk wz = wave_walk(c, w, h, iz, shfl_item(y, src), lane, true);
            walk_out(w, iz, wz, (int)lane == src);
        }
    }
}

__global__ __launch_bounds__(kThreads) void dx_long_insert(const Call c, const Work w) {
    const Head h = load_head(c);
    if (h.over) return;
    const uint32_t met = w.st->n_long, nl = met < kLongCap ? met : kLongCap;
    const uint32_t waves = gridDim.x * kWaves, wave = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (uint32_t e = wave; e < nl; e += waves) {
        const uint64_t i = w.list[e];
        if (h.frozen && i >= h.P) continue;  // (a row of the frozen form: dx_lookup)
        const Item y = item_at(c, h, i);
        if (!y.has) continue;  // (never)
        const Walk wk = wave_walk(c, w, h, i, y, lane, true);
        walk_out(w, i, wk, lane == 0);
    }
}

// ---- the frozen form: the rows look up ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void dx_lookup(const Call c, const Work w, int32_t *__restrict__ codes) {
    const Head h = load_head(c);
    const uint32_t lane = threadIdx.x & 63;
    uint32_t n_values = 0, n_matched = 0;  // this lane's, over its rounds (at most 2^31 / kRows of them)
    for (uint64_t v = h.row_block + blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t i = v * kRows + threadIdx.x;
        const bool is_row = i >= h.P && i < h.N;
        const Item y = is_row ? item_at(c, h, i) : Item{nullptr, 0, false};
        const bool is_long = y.len > kLongItem, alone = y.has && !is_long;
        Walk wk{0, 0, false};
        if (alone) {
            LaneTable t{w.table};
            const uint64_t hy = w.hash[i];
            wk = lookup_item(t, h.S, hy, Same{c, w, h, hy, y, 0, 1});
        }
        probes_out(w, wk, alone);
        for (uint64_t m = __ballot(is_long); m; m &= m - 1) {  // a long row: by its own wave
            const int src = __ffsll((unsigned long long)m) - 1;
            const Walk wz = wave_walk(c, w, h, shfl64(i, src), shfl_item(y, src), lane, false);
            probes_out(w, wz, (int)lane == src);
            if ((int)lane == src) wk = wz;
        }
        // (the inserts are behind a kernel boundary: the slot holds the lowest prior entry of the value)
        if (is_row) codes[i - h.P] = !y.has ? -1 : wk.found ? (int32_t)w.table[wk.slot] : kNoEntry;
        n_values += y.has ? 1u : 0u, n_matched += y.has && wk.found ? 1u : 0u;
    }
    // one pair of atomics per wave, not per round: every wave of the grid adds to the same two words
    const uint64_t values = wave_sum64(n_values), matched = wave_sum64(n_matched);
    if (lane == 0 && values) atomicAdd(&w.st->n_values, (unsigned long long)values);
    if (lane == 0 && matched) atomicAdd(&w.st->n_matched, (unsigned long long)matched);
}

// ---- the rank ---------------------------------------------------------------------------------------------------------------
// of the row item i with a value: the item its slot ended with -- i itself for a first occurrence, below P for a prior entry
__device__ __forceinline__ uint32_t holder(const Work &w, uint64_t i) { return w.table[w.slot[i]]; }

__global__ __launch_bounds__(kThreads) void dx_count(const Call c, const Work w) {
    __shared__ uint64_t s_sum[kWaves];
    __shared__ uint32_t s_cnt[kWaves];
    const Head h = load_head(c);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t n_values = 0, n_matched = 0;  // the block's, over its rounds (thread 0)
    for (uint64_t v = h.row_block + blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t i = v * kRows + threadIdx.x;
        const Item y = i >= h.P ? item_at(c, h, i) : Item{nullptr, 0, false};
        const uint32_t r = y.has ? holder(w, i) : kEmpty;
        const bool first = y.has && r == (uint32_t)i, matched = y.has && r < h.P;
        const uint32_t cnt = wave_sum((y.has ? 1u : 0u) | (first ? 1u << 10 : 0u) | (matched ? 1u << 20 : 0u));  // (at most 256 of each)
        const uint64_t sum = wave_sum64(first ? y.len : 0);
        __syncthreads();  // (the last round's words have been read)
        if (lane == 0) s_sum[wave] = sum, s_cnt[wave] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t all = 0;
            uint32_t n = 0;
            for (int x = 0; x < kWaves; x++) all += s_sum[x], n += s_cnt[x];
            w.bcnt[v - h.row_block] = (n >> 10) & 0x3FFu, w.blen[v - h.row_block] = all;
            n_values += n & 0x3FFu, n_matched += n >> 20;
        }
    }
    // one pair of atomics per block, not per round: every block of the grid adds to the same two words
    if (threadIdx.x == 0 && n_values) atomicAdd(&w.st->n_values, (unsigned long long)n_values);
    if (threadIdx.x == 0 && n_matched) atomicAdd(&w.st->n_matched, (unsigned long long)n_matched);
}

__global__ __launch_bounds__(1024) void dx_scan(const Call c, const Work w, msj_dictionary_extend_result *__restrict__ result) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(c);
    const uint64_t row_blocks = h.frozen || h.over || h.R == 0 ? 0 : h.blocks - h.row_block;  // (the blocks dx_count wrote)
    const uint64_t n_new = scan_in_place(w.bcnt, row_blocks, s_w);
    const uint64_t new_bytes = scan_in_place(w.blen, row_blocks, s_w);
    if (threadIdx.x != 0) return;
    const uint64_t n_distinct = h.over ? 0 : h.P + n_new, dict_bytes = h.over ? 0 : h.base + new_bytes;
    w.st->n_distinct = n_distinct, w.st->dict_bytes = dict_bytes;
    const bool layout_only = !c.dict_offsets && !c.dict_first && !c.dict_bytes;
    msj_dictionary_extend_result r;
    r.code = h.over ? MSJ_CAPACITY
                    : w.st->exhausted ? kExhausted : extend_code(n_distinct, dict_bytes, layout_only, c.dict_capacity, c.src.dict_bytes_capacity, c.flags);
    r.flags = c.flags;
    r.n_rows = h.R;
    r.n_values = h.over ? 0 : w.st->n_values;
    r.n_distinct = n_distinct;
    r.dict_bytes = dict_bytes;
    r.max_probe = h.over ? 0 : w.st->max_probe;
    r.n_prior = h.P;
    r.n_matched = h.over ? 0 : w.st->n_matched;
    *result = r;
    if (!h.over && !h.frozen && h.P == 0 && c.dict_offsets) c.dict_offsets[0] = 0;
}

__global__ __launch_bounds__(kThreads) void dx_place(const Call c, const Work w, int32_t *__restrict__ codes) {
    __shared__ uint64_t s_w[kWaves];
    const Head h = load_head(c);
    for (uint64_t v = h.row_block + blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t i = v * kRows + threadIdx.x;
        const bool is_row = i >= h.P && i < h.N;
        const Item y = is_row ? item_at(c, h, i) : Item{nullptr, 0, false};
        const bool first = y.has && holder(w, i) == (uint32_t)i;
        uint64_t total;
        const uint64_t code = h.P + w.bcnt[v - h.row_block] + block_scan<uint64_t>(first ? 1 : 0, s_w, total);
        const uint64_t off = h.base + w.blen[v - h.row_block] + block_scan<uint64_t>(first ? y.len : 0, s_w, total);
        if (!is_row) continue;
        const uint64_t k = i - h.P;
        if (!y.has) codes[k] = -1;
        if (!first) continue;
        codes[k] = (int32_t)code;  // (code < P + R < 2^31)
        if (code < c.dict_capacity) c.dict_first[code] = (uint32_t)k, c.dict_offsets[code + 1] = off + y.len;
    }
}

__global__ __launch_bounds__(kThreads) void dx_codes(const Call c, const Work w, int32_t *__restrict__ codes) {
    const Head h = load_head(c);
    for (uint64_t v = h.row_block + blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t i = v * kRows + threadIdx.x;
        if (i < h.P) continue;
        const Item y = item_at(c, h, i);
        if (!y.has) continue;
        const uint32_t r = holder(w, i);
        if (r < h.P) codes[i - h.P] = (int32_t)r;
        else if (r != (uint32_t)i) codes[i - h.P] = codes[r - h.P];  // (r is a first row: dx_place wrote its code, this kernel does not)
    }
}

// ---- the copy ---------------------------------------------------------------------------------------------------------------
// the new entries [P, nd) into the output bytes [base, lim): dc_copy with its entries and its bytes counted from there
__global__ __launch_bounds__(kThreads) void dx_copy(const Call c, const Work w) {
    __shared__ uint64_t s_off[kRows + 1], s_src[kRows];
    const Head h = load_head(c);
    if (h.over) return;
    const uint64_t nd = w.st->n_distinct < c.dict_capacity ? w.st->n_distinct : c.dict_capacity;
    if (nd <= h.P) return;
    const uint64_t *offsets = c.dict_offsets + h.P;  // (offsets[0] = base; [1 ..] are dx_place's, ascending)
    const uint32_t *firsts = c.dict_first + h.P;
    const uint64_t ne = nd - h.P;
    const uint64_t all = offsets[ne], lim = all < c.src.dict_bytes_capacity ? all : c.src.dict_bytes_capacity;
    if (lim <= h.base) return;
    const uint64_t mis = reinterpret_cast<uintptr_t>(c.dict_bytes) & 15;  // (output byte p sits at an aligned address when p + mis does)
    const uint64_t piece0 = (h.base + mis) / kPiece, pieces = (lim + mis + kPiece - 1) / kPiece;
    for (uint64_t piece = piece0 + blockIdx.x; piece < pieces; piece += gridDim.x) {
        const uint64_t lo = (piece * kPiece > h.base + mis ? piece * kPiece : h.base + mis) - mis;
        const uint64_t hi = ((piece + 1) * kPiece < lim + mis ? (piece + 1) * kPiece : lim + mis) - mis;
        uint64_t e = row_of_byte(offsets, (uint32_t)ne, lo);  // the entry of the piece's first byte (the same in every lane)
        for (uint64_t p = lo; p < hi;) {                       // (p < hi <= offsets[ne]: e < ne)
            const uint32_t cnt = (uint32_t)(ne - e < kRows ? ne - e : kRows);
            __syncthreads();  // (the last round's entries have been read)
            if (threadIdx.x < cnt) s_off[threadIdx.x] = offsets[e + threadIdx.x];
            if (threadIdx.x == 0) s_off[cnt] = offsets[e + cnt];  // (e + cnt <= ne)
            if (threadIdx.x < cnt) s_src[threadIdx.x] = c.src.offsets[firsts[e + threadIdx.x]];  // (a first row: it has a value)
            __syncthreads();
            const uint64_t stop = hi < s_off[cnt] ? hi : s_off[cnt];
            for (uint64_t a = ((p + mis) & ~15ull) + 16ull * threadIdx.x; a < stop + mis; a += 16ull * kThreads) {
                const uint64_t p0 = (a > p + mis ? a : p + mis) - mis, p1 = (a + 16 < stop + mis ? a + 16 : stop + mis) - mis;
                uint32_t row = row_of_byte(s_off, cnt, p0);
                if (p1 - p0 != 16) {  // an end of the stretch: the first one starts at base itself
                    for (uint64_t q = p0; q < p1; q++) {
                        while (q >= s_off[row + 1]) row++;  // (q < stop <= s_off[cnt])
                        c.dict_bytes[q] = c.src.bytes[s_src[row] + (q - s_off[row])];
                    }
                    continue;
                }
                uint4 out;
                if (p1 <= s_off[row + 1]) {  // inside one entry
                    __builtin_memcpy(&out, c.src.bytes + s_src[row] + (p0 - s_off[row]), 16);  // (any alignment; inside the value)
                } else {
                    uint32_t word[4] = {0, 0, 0, 0};
#pragma unroll
                    for (uint32_t j = 0; j < 16; j++) {
                        while (p0 + j >= s_off[row + 1]) row++;
                        word[j / 4] |= (uint32_t)c.src.bytes[s_src[row] + (p0 + j - s_off[row])] << (8 * (j % 4));
                    }
                    out = make_uint4(word[0], word[1], word[2], word[3]);
                }
                *reinterpret_cast<uint4 *>(c.dict_bytes + p0) = out;
            }
            p = stop, e += cnt;
        }
    }
}

}  // namespace msj_dictx

extern "C" uint64_t msj_dictionary_extend_workspace_bytes(uint64_t rows, uint64_t dict_capacity) {
    return msj_measure(msj_dictx::layout, rows, dict_capacity) + 64;
}

extern "C" int msj_launch_dictionary_extend(const uint64_t *d_offsets, const uint8_t *d_valid, uint64_t rows, const uint64_t *d_n_rows,
                                            const uint8_t *d_bytes, uint64_t bytes_len, uint64_t n_prior, const uint64_t *d_n_prior,
                                            int32_t *d_codes, uint64_t *d_dict_offsets, uint32_t *d_dict_first, uint64_t dict_capacity,
                                            uint8_t *d_dict_bytes, uint64_t dict_bytes_capacity, uint32_t flags,
                                            msj_dictionary_extend_result *d_result, void *d_ws, void *stream) {
    using namespace msj_dictx;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Call c{Source{d_offsets, d_valid, d_bytes, bytes_len, d_dict_offsets, d_dict_bytes, dict_bytes_capacity},
                 rows, d_n_rows, n_prior, d_n_prior, d_dict_offsets, d_dict_first, dict_capacity, d_dict_bytes, flags};
    const Work w = msj_place(layout, d_ws, rows, dict_capacity);
    const bool frozen = (flags & kFrozen) != 0;
    hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(State), s);
    if (cleared != hipSuccess) return (int)cleared;
    const uint64_t items = most_items(rows, dict_capacity);  // (P + R < 2^31 whatever the counts say)
    const uint64_t nb = (items + kRows - 1) / kRows, nbr = (most_rows(rows) + kRows - 1) / kRows + (rows ? 1 : 0);  // (P may cut a block)
    const dim3 grid((uint32_t)(nb > kGridBlocks ? kGridBlocks : nb)), row_grid((uint32_t)(nbr > kGridBlocks ? kGridBlocks : nbr)), block(kThreads);
    if (nb) {
        const uint64_t slots = table_slots(frozen ? most_rows(dict_capacity) : items);  // (at least the S the device finds)
        cleared = hipMemsetAsync(w.table, 0xFF, 4 * slots, s);  // kEmpty in every slot
        if (cleared != hipSuccess) return (int)cleared;
        hipLaunchKernelGGL(dx_hash, grid, block, 0, s, c, w);
        hipLaunchKernelGGL(dx_long_hash, dim3(kLongGrid), block, 0, s, c, w);
        hipLaunchKernelGGL(dx_insert, grid, block, 0, s, c, w);
        hipLaunchKernelGGL(dx_long_insert, dim3(kLongGrid), block, 0, s, c, w);
        if (nbr && frozen) hipLaunchKernelGGL(dx_lookup, row_grid, block, 0, s, c, w, d_codes);
        if (nbr && !frozen) hipLaunchKernelGGL(dx_count, row_grid, block, 0, s, c, w);
    }
    hipLaunchKernelGGL(dx_scan, dim3(1), dim3(1024), 0, s, c, w, d_result);
    if (nbr && !frozen) {
        hipLaunchKernelGGL(dx_place, row_grid, block, 0, s, c, w, d_codes);
        hipLaunchKernelGGL(dx_codes, row_grid, block, 0, s, c, w, d_codes);
    }
    if (nbr && !frozen && d_dict_bytes && d_dict_offsets && d_dict_first && dict_capacity && dict_bytes_capacity)
        hipLaunchKernelGGL(dx_copy, dim3(kCopyGrid), block, 0, s, c, w);
    return (int)hipGetLastError();
}
