// Substring patterns over a byte column -- msj_match_strings_device (include/msj_stage1.h): for every row of a
// (d_offsets, d_valid, d_bytes) column and each of up to 16 patterns of 1 to 4 literal pieces, the first place where the
// pattern matches, as a record per (pattern, row).  The arithmetic -- the fold, the tiles and the masked word that stages
// them, the four bytes at any phase, the piece test, the row of a byte, the accept rule, the cursor, the record -- is
// match_strings_math.h, host + device and checked on the CPU by tests/test_match_strings_math.py.  R is read on the device by
// every kernel: the host sizes the launches by `rows`, `capacity` and `bytes_len`.
//
// The search is organised by BYTE, not by row: a row of 3 bytes and a row of 300 MiB cost what their bytes cost.  All
// launches on the caller's stream behind a memset of the call's state and of the two results; the steps are separated by
// kernel boundaries only, no lane ever waits for another lane or workgroup:
//   ms_check    per row: offsets[k] <= offsets[k + 1] <= bytes_len, else the call's verdict is MSJ_ERR_BAD_ARGUMENT and every
//               later kernel returns at once; the words of the row, one per pattern: "no place yet"
//   per level j < max_pieces of the chain:
//   ms_bytes    a block takes a run of consecutive tiles of kTile = 8 192 start positions, cut by ADDRESS.  Per tile: the
//               aligned 16-byte words of the tile and kHalo = 256 bytes behind it into LDS (the array's first and last word
//               masked against [0, bytes_len)); the offsets of the rows that overlap the tile into LDS, in steps of 256, where
//               the step's count of offsets at or in front of the tile's last byte also finds the row index the next tile
//               starts from (more than kStage = 1 024 of them: the searches of this tile run on memory).  A lane takes
//               kRun = 32 consecutive start positions: its 32 bytes and the word behind them as two 16-byte LDS reads and
//               one of 4, the four bytes at each position from two neighbouring words, against every pattern's piece j; on a
//               hit the rest of the piece from LDS, the row by upper bound minus one in the staged offsets, the accept rule
//               (the row's end, the cursor, the anchors), and ONE 64-bit atomicMin on the (pattern, row) word, only when a
//               plain read shows a larger value there
//   ms_step     (not behind the last level) per (pattern, row) of a pattern with a further piece: cursor = place + length, or
//               "failed"; behind level 0 the place goes into the row's record; the word back to "no place yet"
//   ms_finish   per row: the records of every pattern; n_values, n_matched and n_found by wave and block, one atomic per block
// A single-piece pattern has no cursor and one pass over the bytes.
// Safety: an offset is read only at k <= R <= rows; a byte only through load_word16, inside [0, bytes_len); valid[] only below
// R; the (pattern, row) words and records only below R <= min(rows, capacity).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "launch.h"
#include "match_strings_math.h"
#include "wave_ops.h"

namespace msj_mstr {

using namespace msj::mstr;
using msj::wave::block_counter_add;

static_assert(sizeof(msj_match_strings_result) == 48 && sizeof(msj_field) == 16 && sizeof(msj_select_documents_result) == 48 &&
                  sizeof(msj_pattern) == 32,
              "ABI");
static_assert(MSJ_MATCH_AT_START == kAtStart && MSJ_MATCH_AT_END == kAtEnd && MSJ_MATCH_NOCASE_ASCII == kNocase, "ABI");
static_assert(MSJ_MATCH_MAX_PATTERNS == kMaxPatterns && MSJ_MATCH_MAX_PIECES == kMaxPieces && MSJ_MATCH_MAX_PIECE_BYTES == kMaxPieceBytes, "ABI");
constexpr uint32_t kWaves = kThreads / 64;

struct State {  // cleared by a memset per call
    uint32_t bad, spare[3];  // the offsets do not ascend, or end behind bytes_len
};
struct Work {
    State *st;
    uint64_t *hit;  // [pattern * stride + row]: the smallest accepted place of the level in flight, or kNone
    uint64_t *cur;  // ... the cursor of the level in flight (levels behind the first), or kNone
    uint64_t stride;
};
struct Call {
    const uint64_t *offsets;
    const uint8_t *valid;
    uint64_t rows;
    const uint64_t *d_n_rows;
    const uint8_t *bytes;
    uint64_t bytes_len;
    msj_field *fields;
    uint64_t capacity;
    const Patterns *pats;
    uint32_t n_patterns, max_pieces;
};

static inline Work layout(msj_carver &c, uint64_t rows, uint32_t n_patterns) {
    Work w;
    w.stride = most_rows(rows, rows);
    w.st = c.take<State>(1);
    w.hit = c.take<uint64_t>(w.stride * n_patterns);
    w.cur = c.take<uint64_t>(w.stride * n_patterns);
    return w;
}

// what every kernel reads of the call.  stop: nothing but the results is written
struct Head {
    uint64_t R;
    bool stop;
};
__device__ __forceinline__ Head load_head(const Call &call) {
    Head h;
    h.R = call.d_n_rows ? *call.d_n_rows : call.rows;
    h.stop = rows_over(h.R, call.rows, call.capacity);
    return h;
}

__global__ __launch_bounds__(kThreads) void ms_check(const Call call, const Work w) {
    const Head h = load_head(call);
    if (h.stop) return;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < h.R; k += (uint64_t)gridDim.x * kThreads) {
        if (!offsets_ok(call.offsets[k], call.offsets[k + 1], call.bytes_len)) atomicOr(&w.st->bad, 1u);  // (k + 1 <= R <= rows)
        for (uint32_t p = 0; p < call.n_patterns; p++) w.hit[p * w.stride + k] = kNone;
    }
}

// the bytes of a place inside the staged tile
struct LdsText {
    const uint8_t *p;
    __device__ __forceinline__ uint32_t byte(uint32_t j) const { return p[j]; }
};
// a piece of the level in flight, as the lanes' loop reads it
constexpr uint32_t kMetaNocase = 1u << 8, kMetaFirst = 1u << 9, kMetaLast = 1u << 10;

__global__ __launch_bounds__(kThreads) void ms_bytes(const Call call, const Work w, uint32_t level) {
    __shared__ __attribute__((aligned(16))) uint32_t s_data[kTileWords * 4];
    __shared__ uint64_t s_off[kStage];
    __shared__ uint32_t s_first[kMaxPatterns], s_mask[kMaxPatterns], s_meta[kMaxPatterns], s_n, s_fold;
    __shared__ uint64_t s_i;
    const Head h = load_head(call);
    if (h.stop || h.R == 0 || w.st->bad) return;
    const uint64_t R = h.R;
    const uint32_t tid = threadIdx.x;
    const Patterns *__restrict__ pats = call.pats;
    if (tid == 0) {
        uint32_t n = 0, fold = 0;
        for (uint32_t p = 0; p < call.n_patterns; p++) {
            const Pattern &pat = pats->pat[p];
            if (!has_level(pat, level)) continue;
            const bool nocase = (pat.flags & kNocase) != 0;
            s_first[n] = pat.piece[level].first, s_mask[n] = pat.piece[level].mask;
            s_meta[n] = p | (nocase ? kMetaNocase : 0u) | (level == 0 ? kMetaFirst : 0u) | (is_last_level(pat, level) ? kMetaLast : 0u);
            fold |= nocase, n++;
        }
        s_n = n, s_fold = fold;
    }
    const uint32_t phase = phase_of(call.bytes);
    uint64_t first, last;
    block_tiles(tiles_of(phase, call.bytes_len), gridDim.x, blockIdx.x, first, last);
    const MemoryOffsets mem{call.offsets};
    uint64_t i_hi = 0;
    for (uint64_t t = first; t < last; t++) {
        const Tile tl = tile_of(phase, call.bytes_len, t);
        __syncthreads();  // (the tile in front has been searched; s_n, s_fold)
        // the first row index a search of this tile can give: upper_bound of the byte in front of the tile
        if (t == first) {
            if (tid == 0) s_i = tl.b0 ? upper_bound(mem, 0, R + 1, tl.b0 - 1) : 0;
            __syncthreads();
            i_hi = s_i;
        }
        const uint64_t i_start = i_hi;
        if (i_start > R) break;  // every row ends in front of this tile (uniform)
        for (uint32_t wd = tid; wd < kTileWords; wd += kThreads) {
            const Word16 x = load_word16(call.bytes, phase, call.bytes_len, tl.a0 + (uint64_t)wd * kWord);
            *reinterpret_cast<uint4 *>(s_data + 4 * wd) = make_uint4(x.w[0], x.w[1], x.w[2], x.w[3]);
        }
        // the offsets from the one in front of i_start on, until one lies behind the tile's last start position
        const uint64_t s0 = stage_first(i_start), last_b = tl.b1 - 1;
        bool staged = false;
        for (uint32_t c = 0; c < kStage / kStageChunk; c++) {
            const uint64_t idx = s0 + c * kStageChunk + tid;
            const uint64_t v = idx <= R ? call.offsets[idx] : kNone;  // (idx <= R <= rows)
            s_off[c * kStageChunk + tid] = v;
            const uint32_t cnt = (uint32_t)__syncthreads_count(v <= last_b);
            if (cnt < kStageChunk) {
                i_hi = s0 + c * kStageChunk + cnt, staged = true;
                break;
            }
        }
        if (!staged) {
            if (tid == 0) s_i = upper_bound(mem, s0 + kStage, R + 1, last_b);
            __syncthreads();
            i_hi = s_i;
        }
        const StagedOffsets lds{s_off, s0};
        const uint32_t n_act = s_n;
        const bool any_fold = s_fold != 0;
        // this lane's kRun bytes and the four behind them
        uint32_t dw[kRun / 4 + 1];
        {
            const uint32_t *d = s_data + tid * (kRun / 4);
#pragma unroll
            for (uint32_t q = 0; q < kRun / 16; q++) {
                const uint4 x = *reinterpret_cast<const uint4 *>(d + 4 * q);
                dw[4 * q] = x.x, dw[4 * q + 1] = x.y, dw[4 * q + 2] = x.z, dw[4 * q + 3] = x.w;
            }
            dw[kRun / 4] = d[kRun / 4];
        }
        const uint64_t a_run = tl.a0 + (uint64_t)tid * kRun, a_lo = tl.b0 + phase, a_hi = tl.b1 + phase;
        if (a_run + kRun <= a_lo || a_run >= a_hi) continue;  // (the barriers stand at the loop's head)
#pragma unroll
        for (uint32_t k = 0; k < kRun; k++) {
            const uint64_t a = a_run + k;
            if (a < a_lo || a >= a_hi) continue;
            const uint32_t word = fetch4(dw[k >> 2], dw[(k >> 2) + 1], k & 3);
            const uint32_t folded = any_fold ? fold4(word) : word;
            for (uint32_t q = 0; q < n_act; q++) {
                const uint32_t meta = s_meta[q];
                const bool nocase = (meta & kMetaNocase) != 0;
                if (!first_word_hits(s_first[q], s_mask[q], nocase, word, folded)) continue;
                const uint32_t p = meta & 0xFFu;
                const Pattern &pat = pats->pat[p];
                const Piece &pc = pat.piece[level];
                const LdsText text{reinterpret_cast<const uint8_t *>(s_data) + (a - tl.a0)};
                if (!rest_hits(pc, nocase, pats->bytes, text)) continue;
                const uint64_t b = a - phase;
                const uint64_t i = staged ? upper_bound(lds, i_start, i_hi, b) : upper_bound(mem, i_start, i_hi, b);
                if (!index_has_row(i, R)) continue;
                const uint64_t row = i - 1;
                const uint64_t begin = staged ? lds.at(row) : mem.at(row), end = staged ? lds.at(i) : mem.at(i);
                if (call.valid[row] == 0) continue;  // (row < R)
                const uint64_t at = p * w.stride + row;
                const uint64_t from = (meta & kMetaFirst) ? begin : w.cur[at];
                if (!accept(b, pc.len, begin, end, from, pat.flags, (meta & kMetaFirst) != 0, (meta & kMetaLast) != 0)) continue;
                unsigned long long *word_at = reinterpret_cast<unsigned long long *>(w.hit + at);
                if (*word_at > b) atomicMin(word_at, (unsigned long long)b);
            }
        }
    }
}

// behind level `level`, per (pattern p = blockIdx.y, row) of a pattern with a further piece
__global__ __launch_bounds__(kThreads) void ms_step(const Call call, const Work w, uint32_t level) {
    const Head h = load_head(call);
    if (h.stop || w.st->bad) return;
    const uint32_t p = blockIdx.y;
    const Pattern &pat = call.pats->pat[p];
    if (!has_level(pat, level + 1)) return;
    const uint32_t len = pat.piece[level].len;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < h.R; k += (uint64_t)gridDim.x * kThreads) {
        const uint64_t at = p * w.stride + k;
        const uint64_t hit = w.hit[at];
        if (level == 0 && hit != kNone) call.fields[p * call.capacity + k].bits = hit - call.offsets[k];  // (k < R <= capacity)
        w.cur[at] = next_cursor(hit, len);
        w.hit[at] = kNone;
    }
}

// (the two results were cleared by a memset in front)
__global__ __launch_bounds__(kThreads) void ms_finish(const Call call, const Work w, msj_match_strings_result *__restrict__ result,
                                                      msj_select_documents_result *__restrict__ select) {
    __shared__ uint32_t s_a[kWaves], s_b[kWaves];
    const Head h = load_head(call);
    const int32_t code = h.stop ? MSJ_CAPACITY : (h.R && w.st->bad) ? MSJ_ERR_BAD_ARGUMENT : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        result->code = code, select->code = code;
        if (code == 0 || h.stop) result->n_rows = h.R;
        if (code == 0) result->max_pieces = call.max_pieces, select->n_documents = h.R, select->n_paths = call.n_patterns;
    }
    if (code != 0) return;
    uint32_t n_values = 0, n_matched = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < h.R; k += (uint64_t)gridDim.x * kThreads) {
        const bool has = call.valid[k] != 0;
        const uint64_t begin = call.offsets[k];
        n_values += has;
        for (uint32_t p = 0; p < call.n_patterns; p++) {
            const uint64_t hit = w.hit[p * w.stride + k];
            const bool matched = has && hit != kNone;
            msj_field *out = call.fields + (p * call.capacity + k);  // (k < R <= capacity)
            // a pattern of several pieces: ms_step has left the first piece's place in the record
            const uint64_t place = !matched ? 0 : call.pats->pat[p].n_pieces > 1 ? begin + out->bits : hit;
            const RowRecord r = row_record(matched, place, begin);
            msj_field f;
            f.bits = r.bits, f.token = r.token, f.type = r.type, f.flags = r.flags, f.code = r.code;
            *out = f;
            n_matched += matched;
        }
    }
    (void)block_counter_add(n_values, s_a, &result->n_values);
    const uint32_t matched = block_counter_add(n_matched, s_b, &result->n_matched);
    if (threadIdx.x == 0 && matched) atomicAdd(reinterpret_cast<unsigned long long *>(&select->n_found), (unsigned long long)matched);
}

}  // namespace msj_mstr

extern "C" uint64_t msj_match_strings_workspace_bytes(uint64_t rows, uint32_t n_patterns) {
    return msj_measure(msj_mstr::layout, rows, n_patterns) + 64;
}

extern "C" int msj_launch_match_strings(const void *d_patterns, uint32_t n_patterns, uint32_t max_pieces, const uint64_t *d_offsets,
                                        const uint8_t *d_valid, uint64_t rows, const uint64_t *d_n_rows, const uint8_t *d_bytes, uint64_t bytes_len,
                                        msj_field *d_fields, uint64_t capacity, msj_match_strings_result *d_result,
                                        msj_select_documents_result *d_select, void *d_ws, void *stream) {
    using namespace msj_mstr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Work w = msj_place(layout, d_ws, rows, n_patterns);
    hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(State), s);
    if (cleared == hipSuccess) cleared = hipMemsetAsync(d_result, 0, sizeof *d_result, s);
    if (cleared == hipSuccess) cleared = hipMemsetAsync(d_select, 0, sizeof *d_select, s);
    if (cleared != hipSuccess) return (int)cleared;
    const Call call{d_offsets, d_valid, rows, d_n_rows, d_bytes, bytes_len, d_fields, capacity, static_cast<const Patterns *>(d_patterns),
                    n_patterns, max_pieces};
    const uint64_t most = most_rows(rows, capacity), row_blocks = (most + kThreads - 1) / kThreads;
    const uint32_t over_rows = (uint32_t)(row_blocks > kRowBlocks ? kRowBlocks : row_blocks ? row_blocks : 1);
    const uint64_t tiles = tiles_of(phase_of(d_bytes), bytes_len);
    const dim3 block(kThreads), byte_grid((uint32_t)(tiles > kByteBlocks ? kByteBlocks : tiles ? tiles : 1));
    hipLaunchKernelGGL(ms_check, dim3(over_rows), block, 0, s, call, w);
    for (uint32_t level = 0; most && tiles && level < max_pieces; level++) {
        hipLaunchKernelGGL(ms_bytes, byte_grid, block, 0, s, call, w, level);
        if (level + 1 < max_pieces) hipLaunchKernelGGL(ms_step, dim3(over_rows, n_patterns), block, 0, s, call, w, level);
    }
    hipLaunchKernelGGL(ms_finish, dim3(over_rows), block, 0, s, call, w, d_result, d_select);
    return (int)hipGetLastError();
}
