// Test-only harness: compiles mojo_simdjson_amd/csrc/match_strings_math.h for the host (g++), so that the arithmetic of
// msj_patterns_create and msj_match_strings_device -- the same fold, tiles, masked word, four-byte fetch, piece test, row
// look-up, accept rule and cursor the kernels run (csrc/match_strings_kernel.hip) -- is checked on a CPU-only box against the
// definition written in Python (tests/test_match_strings_math.py), and so that the GPU tests have an expected value.  The
// whole call serially, in the kernels' steps: the check pass over the rows; per piece level the pass over the bytes, block
// by block and tile by tile -- the tile and its halo staged word by word, the offsets of the tile's rows staged in steps or,
// past `stage` of them, searched in memory, a lane's run of start positions read from the staged words -- and the step over
// (pattern, row); the records and the counts.  NOT part of the product.
#include <string.h>

#include <vector>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/match_strings_math.h"

using namespace msj::mstr;

namespace {
bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
struct StagedText {
    const uint8_t *p;
    uint32_t byte(uint32_t j) const { return p[j]; }
};
// desc: per pattern n_pieces, flags, piece_len[4]; all_bytes: every pattern's pieces back to back
std::vector<msj_pattern> specs_of(const uint32_t *desc, const uint8_t *all_bytes, uint32_t n) {
    std::vector<msj_pattern> specs(n);
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; i++) {
        msj_pattern &s = specs[i];
        s.bytes = all_bytes + at, s.n_pieces = desc[6 * i], s.flags = desc[6 * i + 1];
        for (uint32_t j = 0; j < 4; j++) s.piece_len[j] = desc[6 * i + 2 + j], at += j < s.n_pieces ? s.piece_len[j] : 0;
    }
    return specs;
}
}  // namespace

extern "C" {

// the pieces on their own
uint32_t msm_fold1(uint32_t c) { return fold1(c); }
uint32_t msm_fold4(uint32_t w) { return fold4(w); }
uint32_t msm_fetch4(uint32_t lo, uint32_t hi, uint32_t shift) { return fetch4(lo, hi, shift); }
uint32_t msm_phase(const uint8_t *bytes) { return phase_of(bytes); }
void msm_load_word16(const uint8_t *bytes, uint64_t bytes_len, uint64_t a, uint32_t *out) {
    const Word16 x = load_word16(bytes, phase_of(bytes), bytes_len, a);
    memcpy(out, x.w, 16);
}
uint64_t msm_upper_bound(const uint64_t *offsets, uint64_t lo, uint64_t hi, uint64_t b) { return upper_bound(MemoryOffsets{offsets}, lo, hi, b); }
void msm_constants(uint32_t *out) {
    out[0] = kThreads, out[1] = kRun, out[2] = kTile, out[3] = kHalo, out[4] = kStageChunk, out[5] = kStage, out[6] = kByteBlocks, out[7] = kRowBlocks;
}
// msj_patterns_create's host part alone: -> 0 / -1; max_pieces, if given, receives the compiled value
int32_t msm_compile(const uint32_t *desc, const uint8_t *all_bytes, uint32_t n, uint32_t flags, uint32_t *max_pieces) {
    if (n > 64) return -1;
    std::vector<Patterns> pats(1);
    const std::vector<msj_pattern> specs = specs_of(desc, all_bytes, n);
    const int rc = compile_patterns(n ? specs.data() : nullptr, n, flags, pats[0]);
    if (rc == 0 && max_pieces) *max_pieces = pats[0].max_pieces;
    return rc;
}

// The whole call, serially; ctx_ok: whether the context is given; blocks / stage: the blocks of the pass over the bytes and
// the most offsets a tile stages (0: the kernels' kByteBlocks and kStage).  -> 0, or what the entry points refuse on the host,
// in the header's order, with nothing written
int32_t msm_match_strings(int32_t ctx_ok, const uint32_t *desc, const uint8_t *all_bytes, uint32_t n_patterns, const uint64_t *offsets,
                          const uint8_t *valid, uint64_t rows, const uint64_t *d_n_rows, const uint8_t *bytes, uint64_t bytes_len, msj_field *fields,
                          uint64_t capacity, msj_match_strings_result *res, msj_select_documents_result *sel, uint32_t blocks, uint32_t stage) {
    std::vector<Patterns> compiled(1);
    Patterns &pats = compiled[0];
    {
        const std::vector<msj_pattern> specs = specs_of(desc, all_bytes, n_patterns <= kMaxPatterns ? n_patterns : 0);
        if (n_patterns > kMaxPatterns || compile_patterns(n_patterns ? specs.data() : nullptr, n_patterns, 0, pats) != 0) return MSJ_ERR_BAD_ARGUMENT;
    }
    if (!ctx_ok || !res || !sel) return MSJ_ERR_BAD_ARGUMENT;
    if ((rows > 0 && (!offsets || !valid)) || (capacity > 0 && !fields)) return MSJ_ERR_BAD_ARGUMENT;
    if (bytes_len > 0 && !bytes) return MSJ_ERR_BAD_ARGUMENT;
    if (rows >= (1ull << 40) || capacity >= (1ull << 40) || bytes_len >= kMaxBytes) return MSJ_CAPACITY;
    if ((const void *)res == (const void *)sel) return MSJ_ERR_BAD_ARGUMENT;
    if (!aligned_to(fields, 16) || !aligned_to(offsets, 8) || !aligned_to(d_n_rows, 8) || !aligned_to(res, 8) || !aligned_to(sel, 8))
        return MSJ_ERR_BAD_ARGUMENT;
    if (blocks == 0) blocks = kByteBlocks;
    if (stage == 0) stage = kStage;

    const uint64_t R = d_n_rows ? *d_n_rows : rows;
    memset(res, 0, sizeof *res);
    memset(sel, 0, sizeof *sel);
    if (rows_over(R, rows, capacity)) {
        res->code = sel->code = MSJ_CAPACITY, res->n_rows = R;
        return 0;
    }
    // ms_check
    const uint64_t stride = most_rows(rows, rows);
    std::vector<uint64_t> hit(stride * n_patterns, 0x5A5A5A5A5A5A5A5Aull), cur(stride * n_patterns, 0x5A5A5A5A5A5A5A5Aull);
    bool bad = false;
    for (uint64_t k = 0; k < R; k++) {
        bad |= !offsets_ok(offsets[k], offsets[k + 1], bytes_len);
        for (uint32_t p = 0; p < n_patterns; p++) hit[p * stride + k] = kNone;
    }
    if (bad) {
        res->code = sel->code = MSJ_ERR_BAD_ARGUMENT;
        return 0;
    }
    const uint32_t phase = phase_of(bytes);
    const uint64_t tiles = tiles_of(phase, bytes_len);
    const uint64_t grid = tiles > blocks ? blocks : tiles ? tiles : 1;
    const MemoryOffsets mem{offsets};
    std::vector<uint32_t> data(kTileWords * 4);
    std::vector<uint64_t> s_off(stage);
    for (uint32_t level = 0; R && tiles && level < pats.max_pieces; level++) {
        // ms_bytes
        for (uint64_t block = 0; block < grid; block++) {
            uint64_t first, last, i_hi = 0;
            block_tiles(tiles, grid, block, first, last);
            for (uint64_t t = first; t < last; t++) {
                const Tile tl = tile_of(phase, bytes_len, t);
                if (t == first) i_hi = tl.b0 ? upper_bound(mem, 0, R + 1, tl.b0 - 1) : 0;
                const uint64_t i_start = i_hi;
                if (i_start > R) break;
                for (uint32_t wd = 0; wd < kTileWords; wd++) {
                    const Word16 x = load_word16(bytes, phase, bytes_len, tl.a0 + (uint64_t)wd * kWord);
                    memcpy(&data[4 * wd], x.w, 16);
                }
                const uint64_t s0 = stage_first(i_start), last_b = tl.b1 - 1;
                bool staged = false;
                for (uint32_t c = 0; c < stage / kStageChunk && !staged; c++) {
                    uint32_t cnt = 0;
                    for (uint32_t lane = 0; lane < kStageChunk; lane++) {
                        const uint64_t idx = s0 + c * kStageChunk + lane;
                        const uint64_t v = idx <= R ? offsets[idx] : kNone;
                        s_off[c * kStageChunk + lane] = v;
                        cnt += v <= last_b;
                    }
                    if (cnt < kStageChunk) i_hi = s0 + c * kStageChunk + cnt, staged = true;
                }
                if (!staged) i_hi = upper_bound(mem, s0 + (stage / kStageChunk) * kStageChunk, R + 1, last_b);
                const StagedOffsets lds{s_off.data(), s0};
                for (uint32_t lane = 0; lane < kThreads; lane++) {
                    const uint32_t *dw = &data[lane * (kRun / 4)];
                    const uint64_t a_run = tl.a0 + (uint64_t)lane * kRun, a_lo = tl.b0 + phase, a_hi = tl.b1 + phase;
                    for (uint32_t k = 0; k < kRun; k++) {
                        const uint64_t a = a_run + k;
                        if (a < a_lo || a >= a_hi) continue;
                        const uint32_t word = fetch4(dw[k >> 2], dw[(k >> 2) + 1], k & 3), folded = fold4(word);
                        for (uint32_t p = 0; p < n_patterns; p++) {
                            const Pattern &pat = pats.pat[p];
                            if (!has_level(pat, level)) continue;
                            const Piece &pc = pat.piece[level];
                            const bool nocase = (pat.flags & kNocase) != 0;
                            if (!first_word_hits(pc.first, pc.mask, nocase, word, folded)) continue;
                            const StagedText text{reinterpret_cast<const uint8_t *>(data.data()) + (a - tl.a0)};
                            if (!rest_hits(pc, nocase, pats.bytes, text)) continue;
                            const uint64_t b = a - phase;
                            const uint64_t i = staged ? upper_bound(lds, i_start, i_hi, b) : upper_bound(mem, i_start, i_hi, b);
                            if (!index_has_row(i, R)) continue;
                            const uint64_t row = i - 1;
                            const uint64_t begin = staged ? lds.at(row) : mem.at(row), end = staged ? lds.at(i) : mem.at(i);
                            if (valid[row] == 0) continue;
                            const uint64_t at = p * stride + row;
                            const uint64_t from = level == 0 ? begin : cur[at];
                            if (!accept(b, pc.len, begin, end, from, pat.flags, level == 0, is_last_level(pat, level))) continue;
                            if (hit[at] > b) hit[at] = b;
                        }
                    }
                }
            }
        }
        // ms_step
        if (level + 1 >= pats.max_pieces) break;
        for (uint32_t p = 0; p < n_patterns; p++) {
            const Pattern &pat = pats.pat[p];
            if (!has_level(pat, level + 1)) continue;
            for (uint64_t k = 0; k < R; k++) {
                const uint64_t at = p * stride + k;
                if (level == 0 && hit[at] != kNone) fields[p * capacity + k].bits = hit[at] - offsets[k];
                cur[at] = next_cursor(hit[at], pat.piece[level].len);
                hit[at] = kNone;
            }
        }
    }
    // ms_finish
    res->n_rows = R, res->max_pieces = pats.max_pieces;
    sel->n_documents = R, sel->n_paths = n_patterns;
    for (uint64_t k = 0; k < R; k++) {
        const bool has = valid[k] != 0;
        res->n_values += has;
        for (uint32_t p = 0; p < n_patterns; p++) {
            const uint64_t h = hit[p * stride + k];
            const bool matched = has && h != kNone;
            msj_field *out = fields + (p * capacity + k);
            const uint64_t place = !matched ? 0 : pats.pat[p].n_pieces > 1 ? offsets[k] + out->bits : h;
            const RowRecord r = row_record(matched, place, offsets[k]);
            msj_field f;
            memset(&f, 0, sizeof f);
            f.bits = r.bits, f.token = r.token, f.type = r.type, f.flags = r.flags, f.code = r.code;
            *out = f;
            res->n_matched += matched;
        }
    }
    sel->n_found = res->n_matched;
    return 0;
}

}  // extern "C"
