// A selected value's JSON text as a column -- msj_raw_column_device (include/msj_stage1.h): from any msj_field records and
// the window's token arrays, offsets[R + 1], the values' text back to back and a validity byte per row.  Verbatim: the
// window's bytes [idx[token], te(last)).  Compact (MSJ_RAW_COMPACT): the texts of the tokens token .. last back to back.
// The arithmetic -- a token's text, the row test, a row's length, the two searches -- is raw_column_math.h, host + device
// and checked on the CPU by tests/test_raw_column_math.py.  R = d_rows_select->n_documents is read on the device by every
// kernel: the host never learns it, and sizes the launches by the capacity.
//
// A block owns kRows consecutive rows -- block v the rows [v * kRows, + kRows), the grid loops over the blocks R needs.
// Launches, all on the caller's stream, behind a 64-byte memset of the call's counters:
//   rc_tokens   compact only: tl(i) of kTokBlock tokens per block, four per lane; their exclusive sum inside the block goes
//               to the workspace as 64-bit words, the block's total beside it
//   rc_tscan    compact only: one workgroup, the exclusive sum over the blocks' totals.  P(i) = base[i / kTokBlock] + loc[i]
//               is then two loads; 64 bits in both, because on arrays from anywhere (a d_idx that zigzags) a single block's
//               texts can add up to more than 2^32 bytes
//   rc_lengths  a lane per row: the 16-byte record as one load, the row test, d_valid, the length -- a closed form (verbatim)
//               or P(last + 1) - P(token) (compact).  A row LONGER THAN kLongRow = 16 384 bytes is put on the list of long
//               rows (kLongCap = 1 024 entries) and marked as listed beside its length; a long row that finds the list full
//               stays unmarked.  Lengths and block sums go to the workspace, the counts by wave and block
//   rc_scan     one workgroup: the exclusive sum over the blocks' sums, offsets[0], and the result
//   rc_copy     the exclusive sum over the block's lengths gives its rows' offsets (d_offsets leaves here) and the block's
//               contiguous range of output bytes.  Offsets and sources are staged in LDS.  The range is cut at the block's
//               listed rows, and over each stretch between them the lanes take consecutive 16-byte pieces of the OUTPUT,
//               aligned to d_bytes' address; each finds its first byte's row by binary search in LDS (row_of_byte).  A
//               piece that lies in one row is one 16-byte store: verbatim from one 16-byte load of the window, compact from
//               bytes gathered token by token (one search in P for the first byte, then a walk).  A piece that spans rows
//               is gathered into registers row by row -- a row entered at its first byte needs no search -- and leaves as
//               one store as well; only the two ends of a stretch go byte by byte.  An unmarked long row is carried by its
//               block's loop: slower, the same bytes
//   rc_long     the whole grid over the listed rows: a row is cut into pieces of kPiece = 16 KiB of aligned output, block b
//               takes every gridDim-th piece (rotated by the row's place in the list), its lanes 16 bytes each as above.
//               The root of a window that holds one large document is one such row
// Safety: a record is dereferenced only when its token (and a container's closing token) is below n; a token's text lies in
// [0, len) by construction (text_end clips to lim, lim to len); every store to d_bytes is below min(total, bytes_capacity);
// rows are below R <= capacity.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "bytes_block.h"
#include "launch.h"
#include "raw_column_math.h"

namespace msj_rcol {

using namespace msj::rcol;
using namespace msj::wave;
using namespace msj_bytes;
using msj_tape::block_scan, msj_tape::kThreads, msj_tape::kWaves;
using msj_tdocs::load_field;

constexpr uint32_t kTokPer = 4;           // tokens per lane of rc_tokens
constexpr uint32_t kTokBlock = kThreads * kTokPer;  // tokens per block of rc_tokens: 1 024
constexpr uint32_t kTokShift = 10;
constexpr uint32_t kTokGrid = 2048;       // most blocks of rc_tokens
constexpr uint64_t kLongRow = 16384;      // a row of more bytes than this is copied by the whole grid
constexpr uint32_t kLongCap = 1024;       // entries of the list of long rows
constexpr uint32_t kPiece = 16384;        // bytes of a long row one block copies at a time: 4 rounds of 256 lanes x 16
constexpr uint32_t kLongGrid = 2048;      // blocks of rc_long
constexpr uint64_t kListed = 1ull << 63;  // beside a row's length (< 2^63): the row is on the list

static_assert(sizeof(msj_raw_column_result) == 48 && sizeof(msj_field) == 16, "ABI");
static_assert(kTokBlock == 1u << kTokShift && kPiece % (16 * kThreads) == 0, "geometry");

struct State {  // cleared by a memset per call
    unsigned long long n_values, n_containers, n_other;
    uint32_t n_long, pad;  // long rows met (those past kLongCap are not on the list)
    uint64_t reserved[4];
};
struct Work {
    State *st;
    uint64_t *bsum;   // per block of rows: the sum of its rows' lengths, then (rc_scan) the bytes in front of the block
    uint64_t *lens;   // per row: its length in the output | kListed
    uint32_t *list;   // the long rows
    uint64_t *tbase;  // compact, per block of tokens: the sum of its texts, then (rc_tscan) the text bytes in front of it
    uint64_t *tloc;   // compact, per token 0 .. n: the text bytes in front of it inside its block
};
// P of raw_column_math.h
struct PSum {
    const uint64_t *base, *loc;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return base[i >> kTokShift] + loc[i]; }
};

__host__ __device__ inline uint64_t token_blocks(uint64_t n) { return n / kTokBlock + 1; }  // tokens 0 .. n: P has n + 1 entries
// (the two compact arrays have room in the compact form only: no kernel of the verbatim form reads their pointers)
static inline Work layout(msj_carver &c, uint64_t n, uint64_t capacity, bool compact) {
    const uint64_t rows = most_rows(capacity);
    Work w;
    w.st = c.take<State>(1);
    w.bsum = c.take<uint64_t>(rows / kRows + 1);
    w.lens = c.take<uint64_t>(rows);
    w.list = c.take<uint32_t>(kLongCap);
    w.tbase = c.take<uint64_t>(compact ? token_blocks(n) : 0);
    w.tloc = c.take<uint64_t>(compact ? n + 1 : 0);
    return w;
}

__global__ __launch_bounds__(kThreads) void rc_tokens(const Tokens t, const msj_select_documents_result *__restrict__ sel, uint64_t capacity,
                                                      const Work w) {
    __shared__ uint64_t s_w[kWaves];
    if (load_head(sel, capacity).stop) return;
    const uint64_t nb = token_blocks(t.n);
    for (uint64_t v = blockIdx.x; v < nb; v += gridDim.x) {
        const uint64_t mine = v * kTokBlock + kTokPer * threadIdx.x;
        uint64_t l[kTokPer], sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < kTokPer; k++) l[k] = mine + k < t.n ? text_len(t, mine + k) : 0, sum += l[k];
        uint64_t total;
        uint64_t p = block_scan(sum, s_w, total);
#pragma unroll
        for (uint32_t k = 0; k < kTokPer; k++) {
            if (mine + k <= t.n) w.tloc[mine + k] = p;
            p += l[k];
        }
        if (threadIdx.x == 0) w.tbase[v] = total;
    }
}

__global__ __launch_bounds__(1024) void rc_tscan(uint64_t n, const msj_select_documents_result *__restrict__ sel, uint64_t capacity, const Work w) {
    __shared__ uint64_t s_w[16];
    if (load_head(sel, capacity).stop) return;
    (void)scan_in_place(w.tbase, token_blocks(n), s_w);
}

template <bool kIsCompact>
__global__ __launch_bounds__(kThreads) void rc_lengths(const Tokens t, const msj_field *__restrict__ rows,
                                                       const msj_select_documents_result *__restrict__ sel, uint64_t capacity, const Work w,
                                                       uint8_t *__restrict__ valid) {
    __shared__ uint64_t s_sum[kWaves];
    __shared__ uint32_t s_cnt[kWaves];
    const Head h = load_head(sel, capacity);
    const PSum P{w.tbase, w.tloc};
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t k = v * kRows + threadIdx.x;
        Row y = row_of(msj_field{0, 0, 0, 0, 1}, t.n);  // (a row past R: a record with a code)
        uint64_t ul = 0;
        if (k < h.R) {
            y = row_of(load_field(rows, k), t.n);
            ul = kIsCompact ? compact_len(P, y) : verbatim_len(t, y);
            bool listed = false;
            if (ul > kLongRow) {
                const uint32_t slot = atomicAdd(&w.st->n_long, 1u);
                if (slot < kLongCap) w.list[slot] = (uint32_t)k, listed = true;  // (k < R < 2^31)
            }
            valid[k] = y.valid;
            w.lens[k] = ul | (listed ? kListed : 0);
        }
        block_sums_out(lane, wave, ul, y.valid, y.container, y.other, s_sum, s_cnt, &w.bsum[v], &w.st->n_values, &w.st->n_containers, &w.st->n_other);
    }
}

__global__ __launch_bounds__(1024) void rc_scan(const msj_select_documents_result *__restrict__ sel, uint64_t capacity, const Work w,
                                                uint64_t *__restrict__ offsets, bool have_bytes, uint64_t bytes_capacity, uint32_t flags,
                                                msj_raw_column_result *__restrict__ result) {
    __shared__ uint64_t s_w[16];
    const Head h = load_head(sel, capacity);
    const uint64_t run = scan_in_place(w.bsum, h.blocks, s_w);
    if (threadIdx.x != 0) return;
    msj_raw_column_result r;
    r.code = h.skip ? h.code : h.over ? MSJ_CAPACITY : bytes_code(run, have_bytes, bytes_capacity);
    r.flags = flags;
    r.n_rows = h.skip ? 0 : h.R;
    r.n_values = h.stop ? 0 : w.st->n_values;
    r.n_containers = h.stop ? 0 : w.st->n_containers;
    r.total_bytes = run;
    r.n_other = h.stop ? 0 : w.st->n_other;
    *result = r;
    if (!h.stop && offsets) offsets[0] = 0;  // (NULL only with capacity 0: R is 0 then)
}

// ---- the copy ---------------------------------------------------------------------------------------------------------------
// One row as the copy sees it: its first output byte, its source (idx[token], or P(token) in the compact form) and its tokens
struct RowSrc {
    uint64_t off, src;
    uint32_t token, last;
};

// Output bytes [p0, p1) of ONE row, p1 - p0 <= 16; 16 of them start at a 16-byte aligned address and leave as one store
template <bool kIsCompact>
__device__ __forceinline__ void copy_run(const Tokens &t, const PSum &P, uint8_t *__restrict__ bytes, uint64_t p0, uint64_t p1, const RowSrc &r) {
    const bool whole = p1 - p0 == 16;
    if (!kIsCompact) {
        const uint8_t *s = t.buf + verbatim_source(r.src, p0 - r.off);
        if (whole) {
            uint4 v;
            __builtin_memcpy(&v, s, 16);  // (any alignment; inside the row, so inside the window)
            *reinterpret_cast<uint4 *>(bytes + p0) = v;
        } else {
            for (uint64_t j = 0; j < p1 - p0; j++) bytes[p0 + j] = s[j];
        }
        return;
    }
    // compact: the first byte's token by search, the following ones by walking on
    uint64_t q = r.src + (p0 - r.off), i = token_of_byte(P, r.token, r.last, q);
    uint64_t pi = P(i), pn = P(i + 1);  // (i + 1 <= last + 1 <= n)
    const uint8_t *s = t.buf + ((uint64_t)t.idx[i] + (q - pi));
    if (whole) {
        uint32_t word[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t j = 0; j < 16; j++, q++) {
            while (q >= pn) i++, pn = P(i + 1), s = t.buf + t.idx[i];  // (q < P(last + 1): ends at or in front of last)
            word[j / 4] |= (uint32_t)*s++ << (8 * (j % 4));
        }
        *reinterpret_cast<uint4 *>(bytes + p0) = make_uint4(word[0], word[1], word[2], word[3]);
    } else {
        for (uint64_t p = p0; p < p1; p++, q++) {
            while (q >= pn) i++, pn = P(i + 1), s = t.buf + t.idx[i];
            bytes[p] = *s++;
        }
    }
}

// The output bytes [lo, hi) of a block, none of them a listed row's: lanes take 16-byte pieces at aligned addresses
template <bool kIsCompact>
__device__ __forceinline__ void copy_range(const Tokens &t, const PSum &P, uint8_t *__restrict__ bytes, uint64_t lo, uint64_t hi,
                                           const uint64_t *s_off, const uint64_t *s_src, const uint32_t *s_tok, const uint32_t *s_last) {
    if (lo >= hi) return;
    const uint64_t mis = reinterpret_cast<uintptr_t>(bytes) & 15;  // (output byte p sits at an aligned address when p + mis does)
    for (uint64_t a = ((lo + mis) & ~15ull) + 16ull * threadIdx.x; a < hi + mis; a += 16ull * kThreads) {
        const uint64_t p0 = (a > lo + mis ? a : lo + mis) - mis, p1 = (a + 16 < hi + mis ? a + 16 : hi + mis) - mis;
        uint32_t row = row_of_byte(s_off, kRows, p0);
        const bool whole = p1 - p0 == 16;
        if ((whole && p1 <= s_off[row + 1]) || !whole) {  // one row, or an end of the stretch: at most two per call
            for (uint64_t p = p0; p < p1;) {
                while (p >= s_off[row + 1]) row++;  // (p < hi <= s_off[kRows]: row stays below kRows)
                const uint64_t e = p1 < s_off[row + 1] ? p1 : s_off[row + 1];
                copy_run<kIsCompact>(t, P, bytes, p, e, RowSrc{s_off[row], s_src[row], s_tok[row], s_last[row]});
                p = e;
            }
            continue;
        }
        // a whole piece over several rows: its bytes gathered row by row into registers, one store.  The first row is
        // entered where the piece begins (compact: a search); every later one at its first byte, which needs none
        uint64_t next = s_off[row + 1], q = s_src[row] + (p0 - s_off[row]), i = 0, pn = 0;
        const uint8_t *s = t.buf + q;
        if (kIsCompact) {
            i = token_of_byte(P, s_tok[row], s_last[row], q);
            pn = P(i + 1);
            s = t.buf + ((uint64_t)t.idx[i] + (q - P(i)));
        }
        uint32_t word[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) {
            if (p0 + j >= next) {
                do row++; while (p0 + j >= s_off[row + 1]);  // (rows without a byte own nothing; row stays below kRows)
                next = s_off[row + 1], q = s_src[row], s = t.buf + q;
                if (kIsCompact) i = s_tok[row], pn = P(i + 1), s = t.buf + t.idx[i];
            }
            if (kIsCompact)
                while (q >= pn) i++, pn = P(i + 1), s = t.buf + t.idx[i];  // (q < P(last + 1): ends at or in front of last)
            word[j / 4] |= (uint32_t)*s++ << (8 * (j % 4));
            q++;
        }
        *reinterpret_cast<uint4 *>(bytes + p0) = make_uint4(word[0], word[1], word[2], word[3]);
    }
}

template <bool kIsCompact>
__global__ __launch_bounds__(kThreads) void rc_copy(const Tokens t, const msj_field *__restrict__ rows,
                                                    const msj_select_documents_result *__restrict__ sel, uint64_t capacity, const Work w,
                                                    uint64_t *__restrict__ offsets, uint8_t *__restrict__ bytes, uint64_t bytes_capacity) {
    __shared__ uint64_t s_off[kRows + 1];
    __shared__ uint64_t s_src[kRows];
    __shared__ uint32_t s_tok[kRows], s_last[kRows];
    __shared__ uint64_t s_w[kWaves];
    __shared__ uint64_t s_listed[kWaves];
    const Head h = load_head(sel, capacity);
    const PSum P{w.tbase, w.tloc};
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t k = v * kRows + threadIdx.x;
        Row y = row_of(msj_field{0, 0, 0, 0, 1}, t.n);
        uint64_t ul = 0;
        bool listed = false;
        if (k < h.R) {
            const uint64_t word = w.lens[k];
            y = row_of(load_field(rows, k), t.n), ul = word & ~kListed, listed = (word & kListed) != 0;
        }
        uint64_t total;
        const uint64_t base = w.bsum[v], off = base + block_scan(ul, s_w, total);
        if (k < h.R) offsets[k + 1] = off + ul;  // (k + 1 <= R <= capacity)
        if (!bytes || total == 0) continue;      // (the whole block: the layout-only form, or rows without a byte)
        __syncthreads();                         // (the last round's mapping has been read)
        s_off[threadIdx.x] = off, s_tok[threadIdx.x] = y.token, s_last[threadIdx.x] = y.last;
        s_src[threadIdx.x] = !y.valid ? 0 : kIsCompact ? P(y.token) : (uint64_t)t.idx[y.token];
        const uint64_t mask = __ballot(listed);
        if ((threadIdx.x & 63) == 0) s_listed[threadIdx.x >> 6] = mask;
        if (threadIdx.x == 0) s_off[kRows] = base + total;
        __syncthreads();
        const uint64_t end = base + total < bytes_capacity ? base + total : bytes_capacity;
        uint64_t lo = base;
        for (uint32_t x = 0; x < (uint32_t)kWaves; x++) {
            for (uint64_t m = s_listed[x]; m; m &= m - 1) {  // (the same in every lane of the block)
                const uint32_t r = 64 * x + (uint32_t)__ffsll((unsigned long long)m) - 1;
                copy_range<kIsCompact>(t, P, bytes, lo, s_off[r] < end ? s_off[r] : end, s_off, s_src, s_tok, s_last);
                lo = s_off[r + 1];
            }
        }
        copy_range<kIsCompact>(t, P, bytes, lo, end, s_off, s_src, s_tok, s_last);
    }
}

template <bool kIsCompact>
__global__ __launch_bounds__(kThreads) void rc_long(const Tokens t, const msj_field *__restrict__ rows,
                                                    const msj_select_documents_result *__restrict__ sel, uint64_t capacity, const Work w,
                                                    const uint64_t *__restrict__ offsets, uint8_t *__restrict__ bytes, uint64_t bytes_capacity) {
    const Head h = load_head(sel, capacity);
    if (h.stop) return;
    const PSum P{w.tbase, w.tloc};
    const uint32_t met = w.st->n_long, nl = met < kLongCap ? met : kLongCap;
    const uint64_t mis = reinterpret_cast<uintptr_t>(bytes) & 15;
    for (uint32_t j = 0; j < nl; j++) {
        const uint64_t k = w.list[j];
        if (k >= h.R) continue;  // (never: rc_lengths wrote it)
        const uint64_t off = offsets[k], all = offsets[k + 1], hi = all < bytes_capacity ? all : bytes_capacity;
        if (off >= hi) continue;
        const Row y = row_of(load_field(rows, k), t.n);
        if (!y.valid) continue;  // (never: the row has bytes)
        const RowSrc r{off, kIsCompact ? P(y.token) : (uint64_t)t.idx[y.token], y.token, y.last};
        const uint64_t a0 = (off + mis) & ~15ull, pieces = (hi + mis - a0 + kPiece - 1) / kPiece;
        for (uint64_t c = (blockIdx.x + gridDim.x - j % gridDim.x) % gridDim.x; c < pieces; c += gridDim.x) {
            const uint64_t stop = a0 + (c + 1) * kPiece < hi + mis ? a0 + (c + 1) * kPiece : hi + mis;
            for (uint64_t a = a0 + c * kPiece + 16ull * threadIdx.x; a < stop; a += 16ull * kThreads) {
                const uint64_t p0 = (a > off + mis ? a : off + mis) - mis, p1 = (a + 16 < hi + mis ? a + 16 : hi + mis) - mis;
                copy_run<kIsCompact>(t, P, bytes, p0, p1, r);
            }
        }
    }
}

}  // namespace msj_rcol

extern "C" uint64_t msj_raw_column_workspace_bytes(uint64_t n, uint64_t capacity, uint32_t flags) {
    return msj_measure(msj_rcol::layout, n, capacity, (flags & MSJ_RAW_COMPACT) != 0) + 64;
}

extern "C" int msj_launch_raw_column(const msj_token_view &tv, const msj_field *d_rows, const msj_select_documents_result *d_rows_select,
                                     uint64_t *d_offsets, uint8_t *d_valid, uint64_t capacity, uint8_t *d_bytes, uint64_t bytes_capacity,
                                     uint32_t flags, msj_raw_column_result *d_result, void *d_ws, void *stream) {
    using namespace msj_rcol;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool compact = (flags & MSJ_RAW_COMPACT) != 0;
    const Tokens t{tv.d_buf, tv.len, tv.d_idx, tv.n, tv.d_type, tv.d_end, tv.d_flags};
    const Work w = msj_place(layout, d_ws, tv.n, capacity, compact);
    const hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(State), s);
    if (cleared != hipSuccess) return (int)cleared;
    const uint64_t nb = (most_rows(capacity) + kRows - 1) / kRows;
    const dim3 grid((uint32_t)(nb > kGridBlocks ? kGridBlocks : nb));
    if (nb && compact) {
        const uint64_t tb = token_blocks(tv.n);
        hipLaunchKernelGGL(rc_tokens, dim3((uint32_t)(tb > kTokGrid ? kTokGrid : tb)), dim3(kThreads), 0, s, t, d_rows_select, capacity, w);
        hipLaunchKernelGGL(rc_tscan, dim3(1), dim3(1024), 0, s, tv.n, d_rows_select, capacity, w);
    }
    if (nb) {
        if (compact) hipLaunchKernelGGL(rc_lengths<true>, grid, dim3(kThreads), 0, s, t, d_rows, d_rows_select, capacity, w, d_valid);
        else hipLaunchKernelGGL(rc_lengths<false>, grid, dim3(kThreads), 0, s, t, d_rows, d_rows_select, capacity, w, d_valid);
    }
    hipLaunchKernelGGL(rc_scan, dim3(1), dim3(1024), 0, s, d_rows_select, capacity, w, d_offsets, d_bytes != nullptr, bytes_capacity, flags,
                       d_result);
    if (nb) {
        if (compact) hipLaunchKernelGGL(rc_copy<true>, grid, dim3(kThreads), 0, s, t, d_rows, d_rows_select, capacity, w, d_offsets, d_bytes, bytes_capacity);
        else hipLaunchKernelGGL(rc_copy<false>, grid, dim3(kThreads), 0, s, t, d_rows, d_rows_select, capacity, w, d_offsets, d_bytes, bytes_capacity);
    }
    if (nb && d_bytes) {
        if (compact) hipLaunchKernelGGL(rc_long<true>, dim3(kLongGrid), dim3(kThreads), 0, s, t, d_rows, d_rows_select, capacity, w, d_offsets, d_bytes, bytes_capacity);
        else hipLaunchKernelGGL(rc_long<false>, dim3(kLongGrid), dim3(kThreads), 0, s, t, d_rows, d_rows_select, capacity, w, d_offsets, d_bytes, bytes_capacity);
    }
    return (int)hipGetLastError();
}
