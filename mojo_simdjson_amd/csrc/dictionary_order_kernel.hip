// A dictionary's values in byte order -- msj_dictionary_order_device and msj_rank_rows_device (include/msj_stage1.h): the
// entry numbers of V variable-length byte strings in memcmp-then-length order with every entry's rank, and the gather that
// turns a column of codes into rank records.  The arithmetic -- the entry test, the word fetch (the ONLY reader of the
// dictionary's bytes), the key and its digits, the tied test, the record of a row -- is dictionary_order_math.h, host +
// device and checked on the CPU by tests/test_dictionary_order_math.py.  V is read on the device by every kernel: the host
// sizes the launches by `capacity`.
//
// The order by depth B (every value cut to B bytes) becomes the order by B + 8 in a round: the tied entries stand at the
// positions [rank, rank + group size) of sorted[]; a stable sort of them by (rank, word, nvalid), written back to the same
// positions in position order, refines every group; the new ranks are the positions of the new groups' first members.
//
// The one-workgroup path (capacity <= 1 024): do_group, ONE kernel of 1 024 lanes, sorted[] and rank[] in LDS, a lane per
// position.  Per round: the tied lanes take a place by ballot ranks, fetch their word, every tied lane counts the keys in
// front of its own (smaller, or equal with a smaller place: stable), and a running maximum over the heads gives the ranks.
// The loop ends at the first round with nothing tied.
//
// The grid path, all launches on the caller's stream behind a memset of the call's state; the steps are separated by kernel
// boundaries only, no lane ever waits for another lane or workgroup, and atomics only add counts:
//   do_init_count, do_init_scan, do_init_write   (not with MSJ_ORDER_CONTINUE) the order by depth 0: the entries with a
//               value in entry order, rank 0, then the others, MSJ_ORDER_NO_RANK
//   per round t (every kernel behind do_tied_scan returns at once where nothing is tied):
//   do_tied_count, do_tied_scan   the tied positions of every tile of kTile = 1 024 positions, their running sum, the total
//   do_compact   the tied entries in position order: place, entry, key (the word fetched here) into buffer 0; the OR and AND
//               of a tile's keys
//   do_plan      one workgroup: the OR and AND over the tiles -> the digits that differ, the passes of this round
//   do_count(d), do_scan(d), do_scatter(d)   one stable least-significant-digit pass, radix_block.h's: counts per (bucket,
//               tile), 256 workgroups scan a bucket each and leave its total, the scatter ranks by ballots and LDS
//               counters.  A pass reads the buffer the passes in front of it left (their number's parity)
//   do_heads     writes the entries back to their places; a head is a tied entry whose key differs from the one in front;
//               the largest head place of a tile
//   do_heads_scan, do_rank   the running maximum of the head places over the tiles, then inside a tile: an entry's rank
//   do_finish_count, do_result   n_values, n_tied, n_equal at the final depth; the result
// Safety: an offset is read only at c <= V <= capacity; a byte only through fetch_word; sorted[] / rank[] only below V; the
// buffers only below the round's tied count <= V (a scatter's place is tested against it once more).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "bytes_block.h"
#include "dictionary_order_math.h"
#include "launch.h"
#include "radix_block.h"

namespace msj_dord {

using namespace msj::dord;
using namespace msj::wave;
using msj_bytes::kRows, msj_bytes::most_rows;
using msj_radix::kRounds, msj_radix::kScan, msj_radix::kTile, msj_radix::kTileBlocks, msj_radix::tiles_of;  // also of positions
using msj_tape::kThreads, msj_tape::kWaves;

static_assert(sizeof(msj_dictionary_order_result) == 48 && sizeof(msj_rank_rows_result) == 48 && sizeof(msj_field) == 16 &&
                  sizeof(msj_select_documents_result) == 48,
              "ABI");
static_assert(kRows == (uint32_t)kThreads && kWaves == 4 && kBuckets == (uint32_t)kThreads, "geometry");
static_assert(MSJ_ORDER_NO_RANK == kNoRank && MSJ_ORDER_CONTINUE == kContinue, "ABI");
static_assert(kBuckets == msj_radix::kBuckets && kDigitBits == msj_radix::kDigitBits, "the radix pass takes dictionary_order_math.h's digits");

constexpr uint32_t kGroupWaves = kScan / 64;  // (kScan: also the lanes of the one-workgroup kernels)
static_assert(kGroupEntries == kScan, "a lane per position");

struct State {  // cleared by a memset per call
    unsigned long long n_values, n_tied, n_equal;
    uint64_t tied;        // the tied entries at the start of the round in flight
    uint64_t rounds_run;  // rounds that found an entry tied
    uint32_t mask, spare;  // the digits that differ among the round's keys
    uint32_t tot[kBuckets];  // do_scan: the entries of every bucket of the pass in flight
};
struct Work {
    State *st;
    uint32_t *tcnt;                    // per tile of positions: entries with a value (init), tied entries (a round)
    uint64_t *or_word, *and_word, *or_rn, *and_rn;  // per tile of positions: over its tied entries' keys
    uint64_t *word[2], *rn[2];         // the tied entries' keys; a pass reads one pair and writes the other
    uint32_t *ent[2];                  // their entry numbers, moved with the keys
    uint32_t *pos;                     // their places in sorted[], ascending: not moved
    uint32_t *hv;                      // per tied entry behind the sort: its place + 1 where a group starts, else 0
    uint32_t *cnt;                     // [bucket * tiles + tile]
    uint32_t *tmax;                    // per tile of tied entries: the largest hv
};
struct Call {
    const uint64_t *offsets;
    const uint8_t *bytes;
    uint64_t bytes_capacity, n_entries;
    const uint64_t *d_n_entries;
    uint64_t capacity, depth;
    uint32_t rounds, flags;
    uint32_t *sorted, *rank;
};

static inline Work layout(msj_carver &c, uint64_t capacity) {
    const uint64_t n = most_entries(capacity), tiles = tiles_of(n);
    Work w;
    w.st = c.take<State>(1);
    w.tcnt = c.take<uint32_t>(tiles + 1);
    w.or_word = c.take<uint64_t>(tiles), w.and_word = c.take<uint64_t>(tiles);
    w.or_rn = c.take<uint64_t>(tiles), w.and_rn = c.take<uint64_t>(tiles);
    for (int b = 0; b < 2; b++) w.word[b] = c.take<uint64_t>(n), w.rn[b] = c.take<uint64_t>(n), w.ent[b] = c.take<uint32_t>(n);
    w.pos = c.take<uint32_t>(n);
    w.hv = c.take<uint32_t>(n);
    w.cnt = c.take<uint32_t>(kBuckets * tiles);
    w.tmax = c.take<uint32_t>(tiles + 1);
    return w;
}

// what every kernel reads of the call.  stop: nothing but the result is written
struct Head {
    uint64_t V;
    bool stop;
};
__device__ __forceinline__ Head load_head(const Call &call) {
    Head h;
    h.V = call.d_n_entries ? *call.d_n_entries : call.n_entries;
    h.stop = entries_over(h.V, call.capacity);
    return h;
}

__device__ __forceinline__ void write_result(const Call &call, const Head &h, msj_dictionary_order_result *__restrict__ result, uint64_t n_values,
                                             uint64_t n_tied, uint64_t n_equal, uint64_t rounds_run) {
    msj_dictionary_order_result r;
    r.flags = call.flags, r.n_entries = h.V;
    const bool blank = h.stop || h.V == 0;
    r.code = h.stop ? MSJ_CAPACITY : blank ? 0 : order_code(n_tied);
    r.n_values = blank ? 0 : n_values;
    r.n_tied = blank ? 0 : n_tied;
    r.n_equal = blank ? 0 : n_equal;
    r.depth = blank ? 0 : call.depth + kWordBytes * rounds_run;
    *result = r;
}

// ---- the one-workgroup path ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScan) void do_group(const Call call, msj_dictionary_order_result *__restrict__ result) {
    __shared__ uint32_t s_sorted[kScan], s_rank[kScan], s_ent[kScan], s_pos[kScan], s_ord[kScan];
    __shared__ uint64_t s_word[kScan], s_rn[kScan];
    __shared__ uint32_t s_w[kGroupWaves], s_a[kGroupWaves], s_b[kGroupWaves], s_c[kGroupWaves];
    const Head h = load_head(call);
    if (h.stop || h.V == 0 || h.V > kScan) {  // (V <= capacity <= 1 024: the last never)
        if (threadIdx.x == 0) write_result(call, Head{h.V, h.stop || h.V > kScan}, result, 0, 0, 0, 0);
        return;
    }
    const uint64_t V = h.V;
    const uint32_t p = threadIdx.x;
    const MemoryBytes src{call.bytes};
    if (call.flags & kContinue) {
        if (p < V) s_sorted[p] = call.sorted[p], s_rank[p] = call.rank[p];
    } else {
        const bool has = p < V && value_of(call.offsets, call.bytes_capacity, p).has;
        uint32_t n_values;
        const uint32_t before = block_flag_rank<kGroupWaves>(has, s_w, n_values);
        if (p < V) {
            s_sorted[has ? before : n_values + (p - before)] = p;
            s_rank[p] = has ? 0u : kNoRank;
        }
    }
    __syncthreads();
    uint32_t rounds_run = 0;
    for (uint32_t t = 0; t < call.rounds; t++) {
        const uint64_t depth = call.depth + (uint64_t)kWordBytes * t;
        Entry x;
        const bool tied = p < V && tied_at(s_sorted, s_rank, call.offsets, call.bytes_capacity, V, p, depth, x);
        uint32_t n;
        const uint32_t i = block_flag_rank<kGroupWaves>(tied, s_w, n);
        if (n == 0) break;
        rounds_run = t + 1;
        if (tied) {
            const Key k = key_of(s_rank[x.e], fetch_word(src, call.bytes_capacity, x.v.begin, x.v.len, depth));
            s_word[i] = k.word, s_rn[i] = k.rn, s_ent[i] = x.e, s_pos[i] = p;
        }
        __syncthreads();
        // place i of the tied entries: the keys in front of its own, equal keys in their order
        if (p < n) {
            Key mine;
            mine.word = s_word[p], mine.rn = s_rn[p];
            uint32_t to = 0;
            for (uint32_t j = 0; j < n; j++) {
                Key other;
                other.word = s_word[j], other.rn = s_rn[j];
                to += key_less(other, mine) || (j < p && key_equal(other, mine));
            }
            s_ord[to] = p;
        }
        __syncthreads();
        uint32_t hv = 0, e = 0;
        if (p < n) {
            const uint32_t at = s_ord[p];
            Key mine;
            mine.word = s_word[at], mine.rn = s_rn[at];
            bool head = p == 0;
            if (!head) {
                const uint32_t front = s_ord[p - 1];
                Key other;
                other.word = s_word[front], other.rn = s_rn[front];
                head = !key_equal(other, mine);
            }
            e = s_ent[at];
            hv = head ? s_pos[p] + 1 : 0u;
        }
        uint32_t all;
        const uint32_t m = block_scan_max<kGroupWaves>(hv, s_w, all);
        if (p < n) {
            s_sorted[s_pos[p]] = e;  // (every read of sorted[] and rank[] of this round lies behind a barrier)
            s_rank[e] = m ? m - 1 : 0u;
        }
        __syncthreads();
    }
    const uint64_t depth = call.depth + (uint64_t)kWordBytes * rounds_run;
    Entry x;
    x.v.has = false;
    const bool tied = p < V && tied_at(s_sorted, s_rank, call.offsets, call.bytes_capacity, V, p, depth, x);
    const bool has = p < V && x.v.has;
    const bool repeat = is_repeat(has, tied, has ? s_rank[x.e] : 0u, p);
    uint32_t n_values, n_tied, n_equal;
    (void)block_flag_rank<kGroupWaves>(has, s_a, n_values);
    (void)block_flag_rank<kGroupWaves>(tied, s_b, n_tied);
    (void)block_flag_rank<kGroupWaves>(repeat, s_c, n_equal);
    if (p < V) call.sorted[p] = s_sorted[p], call.rank[p] = s_rank[p];
    if (p == 0) write_result(call, h, result, n_values, n_tied, n_equal, rounds_run);
}

// ---- the grid path: the order by depth 0 --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void do_init_count(const Call call, const Work w) {
    __shared__ uint32_t s_w[kWaves];
    const Head h = load_head(call);
    if (h.stop) return;
    const uint64_t tiles = tiles_of(h.V);
    for (uint64_t v = blockIdx.x; v < tiles; v += gridDim.x) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t r = 0; r < kRounds; r++) {
            const uint64_t c = v * kTile + r * kRows + threadIdx.x;
            uint32_t n;
            (void)block_flag_rank<kWaves>(c < h.V && value_of(call.offsets, call.bytes_capacity, c).has, s_w, n);
            sum += n;
        }
        if (threadIdx.x == 0) w.tcnt[v] = sum;
    }
}
__global__ __launch_bounds__(kScan) void do_init_scan(const Call call, const Work w) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(call);
    if (h.stop) return;
    const uint64_t tiles = tiles_of(h.V);
    const uint64_t total = scan_in_place(w.tcnt, tiles, s_w);
    if (threadIdx.x == 0) w.tcnt[tiles] = (uint32_t)total;  // (room: tiles + 1 words)
}
__global__ __launch_bounds__(kThreads) void do_init_write(const Call call, const Work w) {
    __shared__ uint32_t s_w[kWaves];
    const Head h = load_head(call);
    if (h.stop) return;
    const uint64_t tiles = tiles_of(h.V);
    const uint64_t n_values = w.tcnt[tiles];
    for (uint64_t v = blockIdx.x; v < tiles; v += gridDim.x) {
        uint64_t run = w.tcnt[v];
        for (uint32_t r = 0; r < kRounds; r++) {
            const uint64_t c = v * kTile + r * kRows + threadIdx.x;
            const bool has = c < h.V && value_of(call.offsets, call.bytes_capacity, c).has;
            uint32_t n;
            const uint64_t before = run + block_flag_rank<kWaves>(has, s_w, n);
            run += n;
            if (c >= h.V) continue;
            const uint64_t at = has ? before : n_values + (c - before);
            if (at < h.V) call.sorted[at] = (uint32_t)c;  // (always)
            call.rank[c] = has ? 0u : kNoRank;
        }
    }
}

// ---- a round ------------------------------------------------------------------------------------------------------------------
// does round t run: the round in front left entries tied (round 0: always looks)
__device__ __forceinline__ bool round_idle(const Head &h, const Work &w, uint32_t t) { return h.stop || (t > 0 && w.st->rounds_run < t); }

__global__ __launch_bounds__(kThreads) void do_tied_count(const Call call, const Work w, uint32_t t) {
    __shared__ uint32_t s_w[kWaves];
    const Head h = load_head(call);
    if (round_idle(h, w, t)) return;
    const uint64_t depth = call.depth + (uint64_t)kWordBytes * t;
    const uint64_t tiles = tiles_of(h.V);
    for (uint64_t v = blockIdx.x; v < tiles; v += gridDim.x) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t r = 0; r < kRounds; r++) {
            const uint64_t p = v * kTile + r * kRows + threadIdx.x;
            Entry x;
            uint32_t n;
            (void)block_flag_rank<kWaves>(p < h.V && tied_at(call.sorted, call.rank, call.offsets, call.bytes_capacity, h.V, p, depth, x), s_w, n);
            sum += n;
        }
        if (threadIdx.x == 0) w.tcnt[v] = sum;
    }
}
__global__ __launch_bounds__(kScan) void do_tied_scan(const Call call, const Work w, uint32_t t) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(call);
    if (h.stop) return;
    if (t > 0 && w.st->rounds_run < t) {  // (uniform)
        if (threadIdx.x == 0) w.st->tied = 0;
        return;
    }
    const uint64_t total = scan_in_place(w.tcnt, tiles_of(h.V), s_w);
    if (threadIdx.x != 0) return;
    w.st->tied = total;
    if (total) w.st->rounds_run = t + 1;
}

// the round's tied entries, or 0: nothing to do
__device__ __forceinline__ uint64_t round_tied(const Head &h, const Work &w) { return h.stop ? 0 : w.st->tied; }

__global__ __launch_bounds__(kThreads) void do_compact(const Call call, const Work w, uint32_t t) {
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint64_t s_k[4][kWaves];
    const Head h = load_head(call);
    const uint64_t n = round_tied(h, w);
    if (n == 0) return;
    const uint64_t depth = call.depth + (uint64_t)kWordBytes * t;
    const uint64_t tiles = tiles_of(h.V);
    const MemoryBytes src{call.bytes};
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t v = blockIdx.x; v < tiles; v += gridDim.x) {
        uint64_t run = w.tcnt[v];
        uint64_t any_word = 0, all_word = ~0ull, any_rn = 0, all_rn = ~0ull;
        for (uint32_t r = 0; r < kRounds; r++) {
            const uint64_t p = v * kTile + r * kRows + threadIdx.x;
            Entry x;
            const bool tied = p < h.V && tied_at(call.sorted, call.rank, call.offsets, call.bytes_capacity, h.V, p, depth, x);
            uint32_t total;
            const uint64_t i = run + block_flag_rank<kWaves>(tied, s_w, total);
            run += total;
            if (!tied || i >= n) continue;  // (i < n always: the counts are the same test's)
            const Key k = key_of(call.rank[x.e], fetch_word(src, call.bytes_capacity, x.v.begin, x.v.len, depth));
            w.word[0][i] = k.word, w.rn[0][i] = k.rn, w.ent[0][i] = x.e, w.pos[i] = (uint32_t)p;
            any_word |= k.word, all_word &= k.word, any_rn |= k.rn, all_rn &= k.rn;
        }
        const auto or_op = [](unsigned long long a, unsigned long long b) { return a | b; };
        const auto and_op = [](unsigned long long a, unsigned long long b) { return a & b; };
        any_word = wave_reduce((unsigned long long)any_word, or_op), any_rn = wave_reduce((unsigned long long)any_rn, or_op);
        all_word = wave_reduce((unsigned long long)all_word, and_op), all_rn = wave_reduce((unsigned long long)all_rn, and_op);
        __syncthreads();
        if (lane == 0) s_k[0][wave] = any_word, s_k[1][wave] = all_word, s_k[2][wave] = any_rn, s_k[3][wave] = all_rn;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (uint32_t y = 1; y < (uint32_t)kWaves; y++)
                any_word |= s_k[0][y], all_word &= s_k[1][y], any_rn |= s_k[2][y], all_rn &= s_k[3][y];
            w.or_word[v] = any_word, w.and_word[v] = all_word, w.or_rn[v] = any_rn, w.and_rn[v] = all_rn;
        }
    }
}

__global__ __launch_bounds__(kScan) void do_plan(const Call call, const Work w) {
    __shared__ uint64_t s_k[4][kGroupWaves];
    const Head h = load_head(call);
    if (round_tied(h, w) == 0) return;
    const uint64_t tiles = tiles_of(h.V);
    uint64_t any_word = 0, all_word = ~0ull, any_rn = 0, all_rn = ~0ull;
    for (uint64_t v = threadIdx.x; v < tiles; v += kScan)
        any_word |= w.or_word[v], all_word &= w.and_word[v], any_rn |= w.or_rn[v], all_rn &= w.and_rn[v];
    const auto or_op = [](unsigned long long a, unsigned long long b) { return a | b; };
    const auto and_op = [](unsigned long long a, unsigned long long b) { return a & b; };
    any_word = wave_reduce((unsigned long long)any_word, or_op), any_rn = wave_reduce((unsigned long long)any_rn, or_op);
    all_word = wave_reduce((unsigned long long)all_word, and_op), all_rn = wave_reduce((unsigned long long)all_rn, and_op);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_k[0][wave] = any_word, s_k[1][wave] = all_word, s_k[2][wave] = any_rn, s_k[3][wave] = all_rn;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (uint32_t y = 1; y < kGroupWaves; y++) any_word |= s_k[0][y], all_word &= s_k[1][y], any_rn |= s_k[2][y], all_rn &= s_k[3][y];
    Key any, all;
    any.word = any_word, any.rn = any_rn, all.word = all_word, all.rn = all_rn;
    w.st->mask = varying_digits(any, all, key_digits(call.capacity));
}

// ---- the tied entries in the order of their keys ------------------------------------------------------------------------------
// a pass, and as radix_block.h's policy a tied entry of its scatter: its key and its entry number
struct Pass {
    struct Record {
        Key k;
        uint32_t ent;
    };
    uint64_t n, tiles;
    uint32_t d;
    const uint64_t *src_word, *src_rn;
    const uint32_t *src_ent;
    uint64_t *dst_word, *dst_rn;
    uint32_t *dst_ent;
    bool skip;
    __device__ __forceinline__ bool load_key(uint64_t j, Key &k) const {
        const bool active = j < n;
        k.word = active ? src_word[j] : 0, k.rn = active ? src_rn[j] : 0;  // (j < n <= V <= capacity)
        return active;
    }
    __device__ __forceinline__ bool load(uint64_t j, Record &x) const {
        const bool active = load_key(j, x.k);
        x.ent = active ? src_ent[j] : 0u;
        return active;
    }
    __device__ __forceinline__ uint32_t digit(const Record &x) const { return digit_of(x.k, d); }
    __device__ __forceinline__ uint64_t bound() const { return n; }
    __device__ __forceinline__ void store(uint32_t at, const Record &x) const { dst_word[at] = x.k.word, dst_rn[at] = x.k.rn, dst_ent[at] = x.ent; }
};
__device__ __forceinline__ Pass load_pass(const Work &w, const Head &h, uint32_t d) {
    Pass s;
    s.n = round_tied(h, w), s.d = d;
    const uint32_t mask = w.st->mask;
    s.skip = s.n == 0 || !((mask >> d) & 1u);
    s.tiles = tiles_of(s.n);
    const uint32_t from = passes_before(mask, d) & 1u;
    s.src_word = w.word[from], s.src_rn = w.rn[from], s.src_ent = w.ent[from];
    s.dst_word = w.word[from ^ 1u], s.dst_rn = w.rn[from ^ 1u], s.dst_ent = w.ent[from ^ 1u];
    return s;
}

__global__ __launch_bounds__(kThreads) void do_count(const Call call, const Work w, uint32_t d) {
    __shared__ uint32_t s_h[kBuckets];
    const Head h = load_head(call);
    const Pass s = load_pass(w, h, d);
    if (s.skip) return;
    const auto digit_at = [&](uint64_t j, uint32_t &digit) {
        Key k;
        const bool active = s.load_key(j, k);
        digit = digit_of(k, d);
        return active;
    };
    for (uint64_t v = blockIdx.x; v < s.tiles; v += gridDim.x) (void)msj_radix::count_tile(s_h, w.cnt, s.tiles, v, digit_at);
}
__global__ __launch_bounds__(kScan) void do_scan(const Call call, const Work w, uint32_t d) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(call);
    const Pass s = load_pass(w, h, d);
    if (s.skip) return;
    const uint64_t total = msj_radix::scan_bucket(w.cnt, s.tiles, s_w);
    if (threadIdx.x == 0) w.st->tot[blockIdx.x] = (uint32_t)total;
}
__global__ __launch_bounds__(kThreads) void do_scatter(const Call call, const Work w, uint32_t d) {
    __shared__ uint32_t s_run[kBuckets], s_wcnt[kWaves][kBuckets], s_w[kWaves];
    const Head h = load_head(call);
    const Pass s = load_pass(w, h, d);
    if (s.skip) return;
    const uint32_t base = msj_radix::bucket_base(w.st->tot, s_w);  // the entries in the buckets in front
    for (uint64_t v = blockIdx.x; v < s.tiles; v += gridDim.x) msj_radix::scatter_tile(s_run, s_wcnt, base, w.cnt, s.tiles, v, s);
}

// ---- back to their places; the new groups -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void do_heads(const Call call, const Work w) {
    __shared__ uint32_t s_w[kWaves];
    const Head h = load_head(call);
    const uint64_t n = round_tied(h, w);
    if (n == 0) return;
    const uint32_t f = passes_before(w.st->mask, kMaxDigits) & 1u;  // the buffer the last pass wrote
    const uint64_t tiles = tiles_of(n);
    for (uint64_t v = blockIdx.x; v < tiles; v += gridDim.x) {
        uint32_t most = 0;
        for (uint32_t r = 0; r < kRounds; r++) {
            const uint64_t i = v * kTile + r * kRows + threadIdx.x;
            uint32_t hv = 0;
            if (i < n) {
                Key mine, front;
                mine.word = w.word[f][i], mine.rn = w.rn[f][i];
                bool head = i == 0;
                if (!head) {
                    front.word = w.word[f][i - 1], front.rn = w.rn[f][i - 1];
                    head = !key_equal(front, mine);
                }
                const uint32_t p = w.pos[i];
                if (p < h.V) call.sorted[p] = w.ent[f][i];  // (always)
                hv = head ? p + 1 : 0u;
                w.hv[i] = hv;
            }
            uint32_t all;
            (void)block_scan_max<kWaves>(hv, s_w, all);
            most = max(most, all);
        }
        if (threadIdx.x == 0) w.tmax[v] = most;
    }
}
__global__ __launch_bounds__(kScan) void do_heads_scan(const Call call, const Work w) {
    __shared__ uint32_t s_w[kGroupWaves];
    const Head h = load_head(call);
    const uint64_t n = round_tied(h, w);
    if (n == 0) return;
    scan_max_in_place(w.tmax, tiles_of(n), s_w);
}
__global__ __launch_bounds__(kThreads) void do_rank(const Call call, const Work w) {
    __shared__ uint32_t s_w[kWaves];
    const Head h = load_head(call);
    const uint64_t n = round_tied(h, w);
    if (n == 0) return;
    const uint32_t f = passes_before(w.st->mask, kMaxDigits) & 1u;
    const uint64_t tiles = tiles_of(n);
    for (uint64_t v = blockIdx.x; v < tiles; v += gridDim.x) {
        uint32_t run = w.tmax[v];
        for (uint32_t r = 0; r < kRounds; r++) {
            const uint64_t i = v * kTile + r * kRows + threadIdx.x;
            uint32_t all;
            const uint32_t m = max(run, block_scan_max<kWaves>(i < n ? w.hv[i] : 0u, s_w, all));
            run = max(run, all);
            if (i >= n) continue;
            const uint32_t e = w.ent[f][i];
            if (e < h.V) call.rank[e] = m ? m - 1 : 0u;  // (always; m > 0: entry 0 is a head)
        }
    }
}

// ---- the result ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void do_finish_count(const Call call, const Work w) {
    __shared__ uint32_t s_a[kWaves], s_b[kWaves], s_c[kWaves];
    const Head h = load_head(call);
    if (h.stop) return;
    const uint64_t depth = call.depth + (uint64_t)kWordBytes * w.st->rounds_run;
    const uint64_t tiles = tiles_of(h.V);
    uint32_t n_values = 0, n_tied = 0, n_equal = 0;
    for (uint64_t v = blockIdx.x; v < tiles; v += gridDim.x) {
#pragma unroll
        for (uint32_t r = 0; r < kRounds; r++) {
            const uint64_t p = v * kTile + r * kRows + threadIdx.x;
            if (p >= h.V) continue;
            Entry x;
            const bool tied = tied_at(call.sorted, call.rank, call.offsets, call.bytes_capacity, h.V, p, depth, x);
            n_values += x.v.has, n_tied += tied;
            n_equal += is_repeat(x.v.has, tied, x.v.has ? call.rank[x.e] : 0u, p);
        }
    }
    (void)block_counter_add(n_values, s_a, reinterpret_cast<uint64_t *>(&w.st->n_values));
    (void)block_counter_add(n_tied, s_b, reinterpret_cast<uint64_t *>(&w.st->n_tied));
    (void)block_counter_add(n_equal, s_c, reinterpret_cast<uint64_t *>(&w.st->n_equal));
}
__global__ void do_result(const Call call, const Work w, msj_dictionary_order_result *__restrict__ result) {
    const Head h = load_head(call);
    write_result(call, h, result, w.st->n_values, w.st->n_tied, w.st->n_equal, w.st->rounds_run);
}

// ---- msj_rank_rows_device -----------------------------------------------------------------------------------------------------
struct RankCall {
    const int32_t *codes;
    uint64_t rows;
    const uint64_t *d_n_rows;
    const uint32_t *rank;
    uint64_t rank_capacity;
    const msj_dictionary_order_result *order;
    msj_field *fields;
    uint64_t capacity;
};
// (the two results were cleared by a memset in front)
__global__ __launch_bounds__(kThreads) void rr_rows(const RankCall call, msj_rank_rows_result *__restrict__ result,
                                                    msj_select_documents_result *__restrict__ select) {
    __shared__ uint32_t s_a[kWaves], s_b[kWaves], s_c[kWaves];
    const int32_t order_code = call.order->code;
    const uint64_t V = call.order->n_entries;
    const uint64_t R = call.d_n_rows ? *call.d_n_rows : call.rows;
    const bool over = order_code == 0 && rank_rows_over(R, call.rows, call.capacity, V, call.rank_capacity);
    const int32_t code = order_code ? order_code : over ? MSJ_CAPACITY : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        result->code = code, select->code = code;
        if (code == 0 || over) result->n_rows = R;
        if (code == 0) select->n_documents = R, select->n_paths = 1;
    }
    if (code != 0) return;
    uint32_t n_ranked = 0, n_null = 0, n_unknown = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < R; k += (uint64_t)gridDim.x * kThreads) {
        RowRecord r;
        const uint32_t kind = row_record(call.codes[k], V, call.rank, r);  // (k < R <= rows; a rank at c < V <= rank_capacity)
        n_ranked += kind == kRanked, n_null += kind == kNull, n_unknown += kind == kUnknown;
        msj_field f;
        f.bits = r.bits, f.token = r.token, f.type = r.type, f.flags = r.flags, f.code = r.code;
        call.fields[k] = f;  // (k < R <= capacity)
    }
    const uint32_t ranked = block_counter_add(n_ranked, s_a, &result->n_ranked);
    if (threadIdx.x == 0 && ranked) atomicAdd(reinterpret_cast<unsigned long long *>(&select->n_found), (unsigned long long)ranked);
    (void)block_counter_add(n_null, s_b, &result->n_null);
    (void)block_counter_add(n_unknown, s_c, &result->n_unknown);
}

}  // namespace msj_dord

extern "C" uint64_t msj_dictionary_order_workspace_bytes(uint64_t capacity) { return msj_measure(msj_dord::layout, capacity) + 64; }

extern "C" int msj_launch_dictionary_order(const uint64_t *d_dict_offsets, const uint8_t *d_dict_bytes, uint64_t dict_bytes_capacity,
                                           uint64_t n_entries, const uint64_t *d_n_entries, uint64_t capacity, uint64_t depth, uint32_t max_rounds,
                                           uint32_t flags, uint32_t mode, uint32_t *d_sorted, uint32_t *d_rank,
                                           msj_dictionary_order_result *d_result, void *d_ws, void *stream) {
    using namespace msj_dord;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool group = use_group_path(capacity, mode);
    const Call call{d_dict_offsets, d_dict_bytes, dict_bytes_capacity, n_entries, d_n_entries, capacity, depth, rounds_of(max_rounds, group), flags,
                    d_sorted,       d_rank};
    if (group) {
        hipLaunchKernelGGL(do_group, dim3(1), dim3(kScan), 0, s, call, d_result);
        return (int)hipGetLastError();
    }
    const Work w = msj_place(layout, d_ws, capacity);
    const hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(State), s);
    if (cleared != hipSuccess) return (int)cleared;
    const uint64_t tiles = tiles_of(most_entries(capacity));
    const dim3 block(kThreads), one(1), scan(kScan), grid((uint32_t)(tiles > kTileBlocks ? kTileBlocks : tiles ? tiles : 1));
    if (capacity && !(flags & kContinue)) {
        hipLaunchKernelGGL(do_init_count, grid, block, 0, s, call, w);
        hipLaunchKernelGGL(do_init_scan, one, scan, 0, s, call, w);
        hipLaunchKernelGGL(do_init_write, grid, block, 0, s, call, w);
    }
    const uint32_t digits = key_digits(capacity);
    for (uint32_t t = 0; capacity && t < call.rounds; t++) {
        hipLaunchKernelGGL(do_tied_count, grid, block, 0, s, call, w, t);
        hipLaunchKernelGGL(do_tied_scan, one, scan, 0, s, call, w, t);
        hipLaunchKernelGGL(do_compact, grid, block, 0, s, call, w, t);
        hipLaunchKernelGGL(do_plan, one, scan, 0, s, call, w);
        for (uint32_t d = 0; d < digits; d++) {
            hipLaunchKernelGGL(do_count, grid, block, 0, s, call, w, d);
            hipLaunchKernelGGL(do_scan, dim3(kBuckets), scan, 0, s, call, w, d);
            hipLaunchKernelGGL(do_scatter, grid, block, 0, s, call, w, d);
        }
        hipLaunchKernelGGL(do_heads, grid, block, 0, s, call, w);
        hipLaunchKernelGGL(do_heads_scan, one, scan, 0, s, call, w);
        hipLaunchKernelGGL(do_rank, grid, block, 0, s, call, w);
    }
    if (capacity) hipLaunchKernelGGL(do_finish_count, grid, block, 0, s, call, w);
    hipLaunchKernelGGL(do_result, one, one, 0, s, call, w, d_result);
    return (int)hipGetLastError();
}

extern "C" int msj_launch_rank_rows(const int32_t *d_codes, uint64_t rows, const uint64_t *d_n_rows, const uint32_t *d_rank, uint64_t rank_capacity,
                                    const msj_dictionary_order_result *d_order_result, msj_field *d_fields, uint64_t capacity,
                                    msj_rank_rows_result *d_result, msj_select_documents_result *d_select, void *stream) {
    using namespace msj_dord;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t cleared = hipMemsetAsync(d_result, 0, sizeof *d_result, s);
    if (cleared == hipSuccess) cleared = hipMemsetAsync(d_select, 0, sizeof *d_select, s);
    if (cleared != hipSuccess) return (int)cleared;
    const RankCall call{d_codes, rows, d_n_rows, d_rank, rank_capacity, d_order_result, d_fields, capacity};
    const uint64_t most = most_rows(rows < capacity ? rows : capacity), blocks = (most + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(rr_rows, dim3((uint32_t)(blocks > 4096 ? 4096 : blocks ? blocks : 1)), dim3(kThreads), 0, s, call, d_result, d_select);
    return (int)hipGetLastError();
}
