// A byte column as codes plus distinct values -- msj_dictionary_device (include/msj_stage1.h): from the (offsets, valid,
// bytes) layout the string and raw column calls write, an int32 code per row in the order of first appearance and the
// distinct values back to back.  The arithmetic -- the row test, the hash as a sum of mixed words, the byte compare, a
// row's walk through the table -- is dictionary_math.h, host + device and checked on the CPU by
// tests/test_dictionary_math.py.  R is read on the device by every kernel: the host sizes the launches by `rows`.
//
// The core is an open-addressing table of S uint32 row numbers in the workspace, S the power of two >= 2R.  A block owns
// kRows consecutive rows -- block v the rows [v * kRows, + kRows), the grid loops over the blocks R needs.  Launches, all
// on the caller's stream, behind a memset of the call's counters and one of the table to "empty"; the passes are
// separated by kernel boundaries only, and no lane ever waits for another lane or workgroup:
//   dc_hash     a lane per row: the row test and the length.  The words of the block's rows are numbered through an
//               exclusive sum in LDS, and the lanes take CONSECUTIVE words of the block -- for a column whose rows lie back to
//               back, consecutive 8 bytes of d_bytes -- find the word's row by binary search in LDS and add mix(word,
//               position) to the row's sum with an LDS atomic: the hash is a sum, so the order does not matter.  A row
//               LONGER THAN kLongRow = 512 bytes takes no part: it goes on the list of long rows (kLongCap = 1 024 entries,
//               marked beside the row), and one that finds the list full is hashed by its own wave in 64-lane steps
//   dc_long_hash   a wave per listed row, in 64-lane steps
//   dc_insert   a lane per row that has a value and is not long: insert_row -- atomicCAS(empty -> k) on an empty slot; on
//               a slot whose row has the same hash AND the same bytes the walk ends, with an atomicMin only when a plain
//               read shows k below the holder; else the next slot.  The row's slot goes to the workspace.  Long rows that
//               are not listed: the same walk by the row's wave, the compare in 64-lane steps
//   dc_long_insert   a wave per listed row
//   dc_count    row k is a first occurrence iff table[slot[k]] == k: per block the first rows and their bytes
//   dc_scan     one workgroup: the exclusive sums over both block arrays, d_dict_offsets[0], the result
//   dc_place    the first rows: their code (block base + sum inside the block), d_dict_first, d_dict_offsets (block base +
//               the sum of the lengths in front, so no second pass over the entries and no dependence on their capacity);
//               null rows: -1
//   dc_codes    every other row: d_codes[table[slot[k]]]
//   dc_copy     organised by OUTPUT bytes: a block takes kPiece = 16 KiB of aligned output at a time, finds the entry of its
//               first byte by binary search over d_dict_offsets and stages 256 entries' offsets and sources in LDS at a time;
//               lanes take consecutive 16-byte pieces aligned to d_dict_bytes' address, each finds its entry by binary search
//               in LDS.  A piece inside one entry is one 16-byte load and store, a piece over several is gathered into
//               registers and leaves as one store; only the two ends go byte by byte.  A long entry is thereby cut into
//               pieces the grid shares
// Atomics on the table are relaxed, device scope.  A stale read of a slot is harmless: "empty" is settled by the CAS,
// and a row once seen in a slot is of the slot's value for good.
// Safety: offsets are used only after the row test (inside [0, bytes_len), ascending); rows are below R <= rows; table
// values are rows this call inserted; every dictionary store is below its capacity.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "bytes_block.h"
#include "dictionary_math.h"
#include "launch.h"

namespace msj_dict {

using namespace msj::dict;
using namespace msj::wave;
using msj_bytes::kGridBlocks, msj_bytes::kRows, msj_bytes::most_rows;
using msj_tape::block_scan, msj_tape::kThreads, msj_tape::kWaves;

constexpr uint64_t kLongRow = 512;    // a row of more bytes than this is hashed and compared by a wave, not by a lane
constexpr uint32_t kLongCap = 1024;   // entries of the list of long rows
constexpr uint32_t kLongGrid = 256;   // blocks of the two list kernels: a wave per listed row
constexpr uint32_t kPiece = 16384;    // bytes of aligned output a block of dc_copy takes at a time
constexpr uint32_t kCopyGrid = 2048;  // most blocks of dc_copy

static_assert(sizeof(msj_dictionary_result) == 48, "ABI");
static_assert(kPiece % (16 * kThreads) == 0 && kRows == (uint32_t)kThreads, "geometry");

struct State {  // cleared by a memset per call
    unsigned long long n_values, max_probe;
    uint64_t n_distinct, dict_bytes;  // (dc_scan)
    uint32_t n_long, exhausted;       // long rows met (those past kLongCap are not on the list); a walk found no slot
    uint64_t reserved[3];
};
struct Work {
    State *st;
    uint64_t *hash;   // per row
    uint32_t *slot;   // per row: between dc_hash and the inserts 1 for a listed row, then the row's slot
    uint32_t *table;  // S slots: kEmpty, or a row
    uint64_t *bcnt;   // per block of rows: its first rows, then (dc_scan) the first rows in front of the block
    uint64_t *blen;   // per block of rows: the bytes of its first rows, then the bytes in front
    uint32_t *list;   // the long rows
};
// the column and the call
struct Col {
    const uint64_t *offsets;
    const uint8_t *valid;
    uint64_t rows;
    const uint64_t *n_rows;
    const uint8_t *bytes;
    uint64_t bytes_len;
    uint32_t flags;
};
struct Dict {
    uint64_t *offsets;
    uint32_t *first;
    uint64_t capacity;
    uint8_t *bytes;
    uint64_t bytes_capacity;
};

static inline Work layout(msj_carver &c, uint64_t rows_in) {
    const uint64_t rows = most_rows(rows_in);
    Work w;
    w.st = c.take<State>(1);
    w.hash = c.take<uint64_t>(rows);
    w.slot = c.take<uint32_t>(rows);
    w.table = c.take<uint32_t>(table_slots(rows));
    w.bcnt = c.take<uint64_t>(rows / kRows + 1);
    w.blen = c.take<uint64_t>(rows / kRows + 1);
    w.list = c.take<uint32_t>(kLongCap);
    return w;
}

// what every kernel reads first: R rows in `blocks` blocks, the table's S slots.  over: nothing but the result is written
struct Head {
    uint64_t R, blocks, S;
    bool over;
};
__device__ __forceinline__ Head load_head(const Col &c) {
    Head h;
    h.R = c.n_rows ? *c.n_rows : c.rows;
    h.over = rows_over(h.R, c.rows);
    h.blocks = h.over ? 0 : (h.R + kRows - 1) / kRows;
    h.S = table_slots(h.over ? 0 : h.R);
    return h;
}
__device__ __forceinline__ Row row_at(const Col &c, const Head &h, uint64_t k) {
    return k < h.R ? row_of(c.offsets, c.valid, k, c.bytes_len) : Row{0, 0, false};
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) { return (uint64_t)__shfl((unsigned long long)v, src); }

// ---- the hash ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t wave_hash(const Col &c, const Row &y, uint32_t lane) {
    return hash_finish(wave_sum64(hash_piece(c.bytes + y.at, y.len, lane, 64)), y.len, c.flags);
}

__global__ __launch_bounds__(kThreads) void dc_hash(const Col c, const Work w) {
    __shared__ uint64_t s_ws[kRows + 1], s_at[kRows], s_len[kRows], s_w[kWaves];
    __shared__ unsigned long long s_acc[kRows];
    const Head h = load_head(c);
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t k = v * kRows + threadIdx.x;
        const Row y = row_at(c, h, k);
        const bool is_long = y.len > kLongRow;
        bool listed = false;
        if (is_long) {
            const uint32_t e = atomicAdd(&w.st->n_long, 1u);
            if (e < kLongCap) w.list[e] = (uint32_t)k, listed = true;  // (k < R < 2^31)
        }
        uint64_t total;
        const uint64_t ws = block_scan(is_long ? 0 : words_of(y.len), s_w, total);  // (its barrier: the last round's words have been read)
        s_ws[threadIdx.x] = ws, s_at[threadIdx.x] = y.at, s_len[threadIdx.x] = is_long ? 0 : y.len, s_acc[threadIdx.x] = 0;
        if (threadIdx.x == 0) s_ws[kRows] = total;
        __syncthreads();
        for (uint64_t u = threadIdx.x; u < total; u += kThreads) {
            const uint32_t row = row_of_byte(s_ws, kRows, u);  // (rows without a word own nothing)
            const uint64_t j = u - s_ws[row];
            atomicAdd(&s_acc[row], (unsigned long long)mix(load_word(c.bytes + s_at[row], j, s_len[row]), j));
        }
        __syncthreads();
        if (k < h.R) {
            if (!is_long) w.hash[k] = hash_finish(s_acc[threadIdx.x], y.len, c.flags);
            w.slot[k] = listed ? 1u : 0u;
        }
        for (uint64_t m = __ballot(is_long && !listed); m; m &= m - 1) {  // the list was full: by the row's own wave
            const int src = __ffsll((unsigned long long)m) - 1;
            const Row z{shfl64(y.at, src), shfl64(y.len, src), true};
            const uint64_t hz = wave_hash(c, z, lane);
            if ((int)lane == src) w.hash[k] = hz;
        }
    }
}

__global__ __launch_bounds__(kThreads) void dc_long_hash(const Col c, const Work w) {
    const Head h = load_head(c);
    if (h.over) return;
    const uint32_t met = w.st->n_long, nl = met < kLongCap ? met : kLongCap;
    const uint32_t waves = gridDim.x * kWaves, wave = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (uint32_t e = wave; e < nl; e += waves) {
        const uint64_t k = w.list[e];
        const Row y = row_at(c, h, k);
        if (!y.has) continue;  // (never: dc_hash listed it)
        const uint64_t hy = wave_hash(c, y, lane);
        if (lane == 0) w.hash[k] = hy;
    }
}

// ---- the table --------------------------------------------------------------------------------------------------------------
// insert_row's Table for one lane, and for a wave that walks together (lane 0 has the atomics, every lane the answer)
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
    __device__ __forceinline__ uint32_t load(uint64_t i) const { return lt.load(i); }
    __device__ __forceinline__ uint32_t claim(uint64_t i, uint32_t k) const {
        uint32_t seen = 0;
        if (lane == 0) seen = lt.claim(i, k);
        return (uint32_t)__shfl((int)seen, 0);
    }
    __device__ __forceinline__ void lower(uint64_t i, uint32_t k) const {
        if (lane == 0) lt.lower(i, k);
    }
};
// same(r): row r has the value of the row y with hash hy.  r is a row some walk put into the table: it has a value
struct Same {
    const Col &c;
    const Work &w;
    const Head &h;
    uint64_t hy;
    Row y;
    uint32_t first, step;  // 0, 1: a lane alone; lane, 64: a wave together
    __device__ __forceinline__ bool operator()(uint32_t r) const {
        if (w.hash[r] != hy) return false;
        const Row z = row_at(c, h, r);
        if (!z.has || z.len != y.len) return false;
        const bool eq = equal_piece(c.bytes + y.at, c.bytes + z.at, y.len, first, step);
        return step == 1 ? eq : __ballot(!eq) == 0;
    }
};
__device__ __forceinline__ Walk wave_insert(const Col &c, const Work &w, const Head &h, uint64_t k, const Row &y, uint32_t lane) {
    WaveTable t{LaneTable{w.table}, lane};
    const uint64_t hy = w.hash[k];
    return insert_row(t, h.S, hy, (uint32_t)k, Same{c, w, h, hy, y, lane, 64});
}
// the walk's end, every lane of the wave calls (probes 0: no walk): the slot kept by `keeps`, the longest walk to the state
__device__ __forceinline__ void walk_out(const Work &w, uint64_t k, const Walk &wk, bool keeps) {
    if (keeps) {
        w.slot[k] = (uint32_t)wk.slot;  // (S <= 2^32)
        if (!wk.found) w.st->exhausted = 1;
    }
    const unsigned long long longest = wave_reduce((unsigned long long)(keeps ? wk.probes : 0), [](auto a, auto b) { return a > b ? a : b; });
    if ((threadIdx.x & 63) == 0 && longest > w.st->max_probe) atomicMax(&w.st->max_probe, longest);
}

__global__ __launch_bounds__(kThreads) void dc_insert(const Col c, const Work w) {
    const Head h = load_head(c);
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t k = v * kRows + threadIdx.x;
        const Row y = row_at(c, h, k);
        const bool is_long = y.len > kLongRow, listed = is_long && w.slot[k] != 0;
        Walk wk{0, 0, true};
        const bool alone = y.has && !is_long;
        if (alone) {
            LaneTable t{w.table};
            const uint64_t hy = w.hash[k];
            wk = insert_row(t, h.S, hy, (uint32_t)k, Same{c, w, h, hy, y, 0, 1});
        }
        walk_out(w, k, wk, alone);
        for (uint64_t m = __ballot(is_long && !listed); m; m &= m - 1) {  // the list was full: by the row's own wave
            const int src = __ffsll((unsigned long long)m) - 1;
            const Row z{shfl64(y.at, src), shfl64(y.len, src), true};
            const uint64_t kz = shfl64(k, src);
            const Walk wz = wave_insert(c, w, h, kz, z, lane);
            walk_out(w, kz, wz, (int)lane == src);
        }
    }
}

__global__ __launch_bounds__(kThreads) void dc_long_insert(const Col c, const Work w) {
    const Head h = load_head(c);
    if (h.over) return;
    const uint32_t met = w.st->n_long, nl = met < kLongCap ? met : kLongCap;
    const uint32_t waves = gridDim.x * kWaves, wave = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (uint32_t e = wave; e < nl; e += waves) {
        const uint64_t k = w.list[e];
        const Row y = row_at(c, h, k);
        if (!y.has) continue;  // (never)
        const Walk wk = wave_insert(c, w, h, k, y, lane);
        walk_out(w, k, wk, lane == 0);
    }
}

// ---- the rank ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_first(const Work &w, const Row &y, uint64_t k) { return y.has && w.table[w.slot[k]] == (uint32_t)k; }

__global__ __launch_bounds__(kThreads) void dc_count(const Col c, const Work w) {
    __shared__ uint64_t s_sum[kWaves];
    __shared__ uint32_t s_cnt[kWaves];
    const Head h = load_head(c);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t k = v * kRows + threadIdx.x;
        const Row y = row_at(c, h, k);
        const bool first = is_first(w, y, k);
        const uint32_t cnt = wave_sum((y.has ? 1u : 0u) | (first ? 1u << 10 : 0u));  // (at most 256 of each)
        const uint64_t sum = wave_sum64(first ? y.len : 0);
        __syncthreads();  // (the last round's words have been read)
        if (lane == 0) s_sum[wave] = sum, s_cnt[wave] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t all = 0;
            uint32_t n = 0;
            for (int x = 0; x < kWaves; x++) all += s_sum[x], n += s_cnt[x];
            w.bcnt[v] = n >> 10, w.blen[v] = all;
            if (n & 0x3FFu) atomicAdd(&w.st->n_values, (unsigned long long)(n & 0x3FFu));
        }
    }
}

__global__ __launch_bounds__(1024) void dc_scan(const Col c, const Work w, const Dict d, msj_dictionary_result *__restrict__ result) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(c);
    const uint64_t n_distinct = scan_in_place(w.bcnt, h.blocks, s_w);
    const uint64_t dict_bytes = scan_in_place(w.blen, h.blocks, s_w);
    if (threadIdx.x != 0) return;
    w.st->n_distinct = n_distinct, w.st->dict_bytes = dict_bytes;
    const bool layout_only = !d.offsets && !d.first && !d.bytes;
    msj_dictionary_result r;
    r.code = h.over ? MSJ_CAPACITY : w.st->exhausted ? kExhausted : dict_code(n_distinct, dict_bytes, layout_only, d.capacity, d.bytes_capacity);
    r.flags = c.flags;
    r.n_rows = h.R;
    r.n_values = h.over ? 0 : w.st->n_values;
    r.n_distinct = n_distinct;
    r.dict_bytes = dict_bytes;
    r.max_probe = h.over ? 0 : w.st->max_probe;
    *result = r;
    if (!h.over && d.offsets) d.offsets[0] = 0;
}

__global__ __launch_bounds__(kThreads) void dc_place(const Col c, const Work w, const Dict d, int32_t *__restrict__ codes) {
    __shared__ uint64_t s_w[kWaves];
    const Head h = load_head(c);
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t k = v * kRows + threadIdx.x;
        const Row y = row_at(c, h, k);
        const bool first = is_first(w, y, k);
        uint64_t total;
        const uint64_t code = w.bcnt[v] + block_scan<uint64_t>(first ? 1 : 0, s_w, total);
        const uint64_t off = w.blen[v] + block_scan<uint64_t>(first ? y.len : 0, s_w, total);
        if (k >= h.R) continue;
        if (!y.has) codes[k] = -1;
        if (!first) continue;
        codes[k] = (int32_t)code;  // (code < R < 2^31)
        if (code < d.capacity) d.first[code] = (uint32_t)k, d.offsets[code + 1] = off + y.len;
    }
}

__global__ __launch_bounds__(kThreads) void dc_codes(const Col c, const Work w, int32_t *__restrict__ codes) {
    const Head h = load_head(c);
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t k = v * kRows + threadIdx.x;
        const Row y = row_at(c, h, k);
        if (!y.has) continue;
        const uint32_t r = w.table[w.slot[k]];
        if (r != (uint32_t)k) codes[k] = codes[r];  // (r is a first row: dc_place wrote its code, this kernel does not)
    }
}

// ---- the copy ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void dc_copy(const Col c, const Work w, const Dict d) {
    __shared__ uint64_t s_off[kRows + 1], s_src[kRows];
    const Head h = load_head(c);
    if (h.over) return;
    const uint64_t nd = w.st->n_distinct < d.capacity ? w.st->n_distinct : d.capacity;
    if (nd == 0) return;
    const uint64_t all = d.offsets[nd], lim = all < d.bytes_capacity ? all : d.bytes_capacity;
    if (lim == 0) return;
    const uint64_t mis = reinterpret_cast<uintptr_t>(d.bytes) & 15;  // (output byte p sits at an aligned address when p + mis does)
    const uint64_t pieces = (lim + mis + kPiece - 1) / kPiece;
    for (uint64_t piece = blockIdx.x; piece < pieces; piece += gridDim.x) {
        const uint64_t lo = (piece * kPiece > mis ? piece * kPiece : mis) - mis;
        const uint64_t hi = ((piece + 1) * kPiece < lim + mis ? (piece + 1) * kPiece : lim + mis) - mis;
        uint64_t e = row_of_byte(d.offsets, (uint32_t)nd, lo);  // the entry of the piece's first byte (the same in every lane)
        for (uint64_t p = lo; p < hi;) {                          // (p < hi <= offsets[nd]: e < nd)
            const uint32_t cnt = (uint32_t)(nd - e < kRows ? nd - e : kRows);
            __syncthreads();  // (the last round's entries have been read)
            if (threadIdx.x < cnt) s_off[threadIdx.x] = d.offsets[e + threadIdx.x];
            if (threadIdx.x == 0) s_off[cnt] = d.offsets[e + cnt];  // (e + cnt <= nd)
            if (threadIdx.x < cnt) s_src[threadIdx.x] = c.offsets[d.first[e + threadIdx.x]];  // (a first row: it has a value)
            __syncthreads();
            const uint64_t stop = hi < s_off[cnt] ? hi : s_off[cnt];
            for (uint64_t a = ((p + mis) & ~15ull) + 16ull * threadIdx.x; a < stop + mis; a += 16ull * kThreads) {
                const uint64_t p0 = (a > p + mis ? a : p + mis) - mis, p1 = (a + 16 < stop + mis ? a + 16 : stop + mis) - mis;
                uint32_t row = row_of_byte(s_off, cnt, p0);
                if (p1 - p0 != 16) {  // an end of the stretch
                    for (uint64_t q = p0; q < p1; q++) {
                        while (q >= s_off[row + 1]) row++;  // (q < stop <= s_off[cnt])
                        d.bytes[q] = c.bytes[s_src[row] + (q - s_off[row])];
                    }
                    continue;
                }
                uint4 out;
                if (p1 <= s_off[row + 1]) {  // inside one entry
                    __builtin_memcpy(&out, c.bytes + s_src[row] + (p0 - s_off[row]), 16);  // (any alignment; inside the value)
                } else {
                    uint32_t word[4] = {0, 0, 0, 0};
#pragma unroll
                    for (uint32_t j = 0; j < 16; j++) {
                        while (p0 + j >= s_off[row + 1]) row++;
                        word[j / 4] |= (uint32_t)c.bytes[s_src[row] + (p0 + j - s_off[row])] << (8 * (j % 4));
                    }
                    out = make_uint4(word[0], word[1], word[2], word[3]);
                }
                *reinterpret_cast<uint4 *>(d.bytes + p0) = out;
            }
            p = stop, e += cnt;
        }
    }
}

}  // namespace msj_dict

extern "C" uint64_t msj_dictionary_workspace_bytes(uint64_t rows) { return msj_measure(msj_dict::layout, rows) + 64; }

extern "C" int msj_launch_dictionary(const uint64_t *d_offsets, const uint8_t *d_valid, uint64_t rows, const uint64_t *d_n_rows,
                                     const uint8_t *d_bytes, uint64_t bytes_len, int32_t *d_codes, uint64_t *d_dict_offsets,
                                     uint32_t *d_dict_first, uint64_t dict_capacity, uint8_t *d_dict_bytes, uint64_t dict_bytes_capacity,
                                     uint32_t flags, msj_dictionary_result *d_result, void *d_ws, void *stream) {
    using namespace msj_dict;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Col c{d_offsets, d_valid, rows, d_n_rows, d_bytes, bytes_len, flags};
    const Dict d{d_dict_offsets, d_dict_first, dict_capacity, d_dict_bytes, dict_bytes_capacity};
    const Work w = msj_place(layout, d_ws, rows);
    hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(State), s);
    if (cleared != hipSuccess) return (int)cleared;
    const uint64_t nb = (most_rows(rows) + kRows - 1) / kRows;  // (R < 2^31 whatever `rows` says)
    const dim3 grid((uint32_t)(nb > kGridBlocks ? kGridBlocks : nb)), block(kThreads);
    if (nb) {
        cleared = hipMemsetAsync(w.table, 0xFF, 4 * table_slots(most_rows(rows)), s);  // kEmpty in every slot
        if (cleared != hipSuccess) return (int)cleared;
        hipLaunchKernelGGL(dc_hash, grid, block, 0, s, c, w);
        hipLaunchKernelGGL(dc_long_hash, dim3(kLongGrid), block, 0, s, c, w);
        hipLaunchKernelGGL(dc_insert, grid, block, 0, s, c, w);
        hipLaunchKernelGGL(dc_long_insert, dim3(kLongGrid), block, 0, s, c, w);
        hipLaunchKernelGGL(dc_count, grid, block, 0, s, c, w);
    }
    hipLaunchKernelGGL(dc_scan, dim3(1), dim3(1024), 0, s, c, w, d, d_result);
    if (nb) {
        hipLaunchKernelGGL(dc_place, grid, block, 0, s, c, w, d, d_codes);
        hipLaunchKernelGGL(dc_codes, grid, block, 0, s, c, w, d_codes);
    }
    if (nb && d_dict_bytes && d_dict_offsets && d_dict_first && dict_capacity && dict_bytes_capacity)
        hipLaunchKernelGGL(dc_copy, dim3(kCopyGrid), block, 0, s, c, w, d);
    return (int)hipGetLastError();
}
