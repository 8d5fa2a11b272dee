// Fields by path for every complete document of a window -- msj_select_documents_device (include/msj_stage1.h): upstream
// simdjson's at_key / at_pointer, restricted to object keys, for up to 16 paths and every document in one call.  The
// arithmetic -- the compiled paths, the member test, the key compare, the state words and the record -- is select_math.h,
// host + device and checked on the CPU by tests/test_select_math.py.  D = d_docs->n_complete and T = d_docs->tokens_complete
// are read on the device by every kernel: the host never learns them.
//
// No walk: top-down, one pass over the window per path LEVEL, for all paths and all documents at once.  The state is one
// uint32 per (path, document): the object the path has reached (a window token), or a code above 0x7FFFFFFF.  A document
// starts at depth 0, so at level l the keys that can match sit at depth l + 1.  Launches, all on the caller's stream:
//   sel_init    per (p, k): state 0 = f_k, or the verdict's code, or 17 when f_k is no object and the path is not "";
//               the next level's word "not found"; one lane writes the result's fixed part (MSJ_CAPACITY when D >
//               capacity, and every later kernel returns at once)
//   sel_level   the hot path, once per level l < the longest path's segment count: a block of 1 024 tokens, 4 per lane; the
//               type word as one 4-byte load, the depths as one 16-byte load, one token of halo behind the block for the
//               ':'.  A block without a candidate (a string at depth l + 1 with ':' behind it) ends there.  The tokens'
//               documents as td_emit finds them (docs_block.h).  Only a candidate gathers d_idx / d_end / d_flags, and
//               per path whose segment can have its raw length the state word, the object's partner and the key's bytes
//               (the level's segments are staged into LDS once per block).  A match issues one atomicMin of its index on
//               the next level's word: "first match wins" is the minimum, a document without the key issues no atomic
//   sel_step    per (p, k), behind each level: the minimum into the next level's state -- v = i + 2, checked for '{' and a
//               partner inside the document unless it is the path's last level -- and the word of the level after it "not
//               found" (the two word arrays alternate)
//   sel_finish  per (p, k), coalesced along k: the record; n_found / n_no_bits by wave and block, one atomic per block
// Every index from d_match, d_end or d_doc_first is checked before it is used; a state word that is a token is below T.
// The steps select_elements_kernel.hip takes in the same way are select_block.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "launch.h"
#include "select_block.h"

namespace msj_sel {

using namespace msj_selblock;

static_assert(sizeof(Paths) % 8 == 0, "the blob is copied as it is");

// the two state words of (p, k): level l's in word[l & 1]
struct Words {
    uint32_t *word[2];
    uint64_t stride;  // documents per path
};

__global__ __launch_bounds__(kThreads) void sel_init(const Paths *__restrict__ paths, const uint8_t *__restrict__ type,
                                                     const uint32_t *__restrict__ match, uint64_t n, const uint32_t *__restrict__ first,
                                                     const msj_documents_result *__restrict__ docs, uint64_t capacity,
                                                     const msj_document_verdict *__restrict__ verdicts, const Words ws,
                                                     msj_select_documents_result *__restrict__ result) {
    const Window win = load_window(docs, first, n, capacity);
    const uint32_t p = blockIdx.y;
    if (blockIdx.x == 0 && p == 0 && threadIdx.x == 0) {
        msj_select_documents_result r;
        r.code = win.over ? MSJ_CAPACITY : 0;
        r.flags = 0;
        r.n_documents = win.D;
        r.n_paths = paths->n_paths;
        r.n_found = r.n_no_bits = r.reserved = 0;
        *result = r;
    }
    if (win.over) return;
    const uint32_t levels = paths->levels[p];
    const uint64_t lanes = (uint64_t)gridDim.x * kThreads;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < win.D; k += lanes) {
        uint64_t f, e;
        const bool ok = document_bounds(first, win, k, f, e);
        const int32_t code = verdicts ? verdicts[k].code : 0;
        uint32_t t = 0, m = kNoPartner;
        if (ok && code == 0 && levels > 0) t = type[f], m = match[f];
        ws.word[0][p * ws.stride + k] = first_state(code, ok, levels, t, m, f, e);
        ws.word[1][p * ws.stride + k] = kNotFound;
    }
}

__global__ __launch_bounds__(kThreads) void sel_level(const Paths *__restrict__ paths, uint32_t level, const uint8_t *__restrict__ buf,
                                                      uint64_t len, const uint32_t *__restrict__ idx, uint64_t n,
                                                      const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                      const uint32_t *__restrict__ match, const uint32_t *__restrict__ end,
                                                      const uint8_t *__restrict__ flags, const uint32_t *__restrict__ first,
                                                      const msj_documents_result *__restrict__ docs, uint64_t capacity, const Words ws) {
    __shared__ Segments s_seg;
    __shared__ uint32_t s_type[kThreads + 1];
    __shared__ uint32_t s_flag[kThreads], s_k[2], s_w32[kWaves];
    const Window win = load_window(docs, first, n, capacity);
    const uint64_t base = (uint64_t)blockIdx.x * kBlock, mine = base + (uint64_t)threadIdx.x * kPer;
    if (win.over || win.D == 0 || base >= win.T) return;
    // tokens at or past T read as nothing: they belong to the cut document.  A candidate: a string at depth level + 1 with
    // ':' behind it
    const TokenQuad t = load_block(paths, level, type, depth, base, win.T, s_type, s_seg);
    uint32_t cand;
    if (!key_candidates(t, base, win.T, s_type, cand,
                        [&](uint64_t i, uint32_t ty, uint32_t t_next, int32_t d) { return i >= win.f0 && is_key_at(ty, t_next, d, level); }))
        return;
    stage_segments(paths, level, s_seg);
    const BlockDocs bd = block_docs(first, win, base, s_flag, s_k, s_w32);  // (its barriers publish the segments)
    const ByteReader r{buf, len};
    const uint32_t n_paths = paths->n_paths;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        if (!((cand >> k) & 1u)) continue;
        const uint64_t i = mine + k;
        const uint64_t doc = (uint64_t)bd.k0 + bd.rank[k];  // 1 + the document's number
        if (doc == 0 || doc > win.D) continue;               // (<= capacity)
        match_key(r, idx, match, end, flags, i, doc - 1, n_paths, level, s_seg, ws, [&](uint32_t lo, uint32_t m) { return is_member_of(i, lo, m); });
    }
}

__global__ __launch_bounds__(kThreads) void sel_step(const Paths *__restrict__ paths, uint32_t level, const uint8_t *__restrict__ type,
                                                     const uint32_t *__restrict__ match, uint64_t n, const uint32_t *__restrict__ first,
                                                     const msj_documents_result *__restrict__ docs, uint64_t capacity, const Words ws) {
    const Window win = load_window(docs, first, n, capacity);
    if (win.over) return;
    step_rows(paths, level, type, match, ws, win.D, [&](uint64_t k) {
        uint64_t f, e;
        (void)document_bounds(first, win, k, f, e);  // (judged by sel_init: a document out of bounds has a code)
        return e;
    });
}

__global__ __launch_bounds__(kThreads) void sel_finish(const Paths *__restrict__ paths, const uint32_t *__restrict__ idx, uint64_t n,
                                                       const uint8_t *__restrict__ type, const uint32_t *__restrict__ match,
                                                       const uint32_t *__restrict__ end, const uint8_t *__restrict__ flags,
                                                       const uint32_t *__restrict__ first, const msj_documents_result *__restrict__ docs,
                                                       const msj_number *__restrict__ numbers, uint64_t numbers_capacity,
                                                       const msj_numbers_result *__restrict__ nr, const Words ws,
                                                       msj_field *__restrict__ fields, uint64_t capacity,
                                                       msj_select_documents_result *__restrict__ result) {
    const Window win = load_window(docs, first, n, capacity);
    if (win.over || win.D == 0) return;
    const uint32_t *word = ws.word[paths->levels[blockIdx.y] & 1] + blockIdx.y * ws.stride;
    finish_rows(idx, type, match, end, flags, number_records(numbers, numbers_capacity, nr), win.D, fields, capacity, result,
                [&](uint64_t k) { return word[k]; });
}

static inline Words words_layout(msj_carver &c, uint64_t n, uint64_t capacity, uint32_t n_paths) {
    Words ws;
    ws.stride = most_documents(n, capacity);
    for (int b = 0; b < 2; b++) ws.word[b] = c.take<uint32_t>((uint64_t)n_paths * ws.stride, 4);
    return ws;
}

}  // namespace msj_sel

extern "C" uint64_t msj_select_documents_workspace_bytes(uint64_t n, uint64_t len, uint64_t capacity, uint32_t n_paths) {
    (void)len;
    return msj_measure(msj_sel::words_layout, n, capacity, n_paths) + 64;
}

extern "C" int msj_launch_select_documents(const void *d_paths, uint32_t n_paths, uint32_t max_levels, const msj_token_view &t,
                                           const msj_split_view &sp, const msj_number_view &nv, const msj_document_verdict *d_verdicts,
                                           msj_field *d_fields, uint64_t capacity, msj_select_documents_result *d_result, void *d_ws,
                                           void *stream) {
    using namespace msj_sel;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Paths *paths = static_cast<const Paths *>(d_paths);
    const Words ws = msj_place(words_layout, d_ws, t.n, capacity, n_paths);
    const dim3 doc_grid(row_grid_blocks(ws.stride), n_paths);
    hipLaunchKernelGGL(sel_init, doc_grid, dim3(kThreads), 0, s, paths, t.d_type, t.d_match, t.n, sp.d_doc_first, sp.d_docs, capacity, d_verdicts, ws,
                       d_result);
    if (t.n == 0) return (int)hipGetLastError();  // no document: the zero result is all there is
    const uint32_t nb = (uint32_t)((t.n + kBlock - 1) / kBlock);
    for (uint32_t l = 0; l < max_levels; l++) {
        hipLaunchKernelGGL(sel_level, dim3(nb), dim3(kThreads), 0, s, paths, l, t.d_buf, t.len, t.d_idx, t.n, t.d_type, t.d_depth, t.d_match, t.d_end,
                           t.d_flags, sp.d_doc_first, sp.d_docs, capacity, ws);
        hipLaunchKernelGGL(sel_step, doc_grid, dim3(kThreads), 0, s, paths, l, t.d_type, t.d_match, t.n, sp.d_doc_first, sp.d_docs, capacity, ws);
    }
    hipLaunchKernelGGL(sel_finish, doc_grid, dim3(kThreads), 0, s, paths, t.d_idx, t.n, t.d_type, t.d_match, t.d_end, t.d_flags, sp.d_doc_first,
                       sp.d_docs, nv.d_numbers, nv.numbers_capacity, nv.d_numbers_result, ws, d_fields, capacity, d_result);
    return (int)hipGetLastError();
}
