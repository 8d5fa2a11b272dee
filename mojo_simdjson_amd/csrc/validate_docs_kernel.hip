// Stage 2's verdict for every complete document of a window -- msj_validate_documents_device (include/msj_stage1.h): what
// msj_validate_device (validate_kernel.hip) gives for each document's token sub-arrays, in one pass over the window
// instead of one call per document.  The rule is the unchanged token_rule of validate_math.h behind the accessor of
// validate_docs_math.h (each token sees its own document's [f, e)); both are host + device and checked on the CPU by
// tests/test_validate_documents_math.py.  D = d_docs->n_complete and T = d_docs->tokens_complete are read on the device by
// every kernel: the host never learns them.
//
// Launches, all on the caller's stream, no host round trip:
//   vd_init     every document's packed error word set to kNoError, in place: d_verdicts[k] = {0, 0, UINT64_MAX} is also the
//               verdict of a valid document, which nobody has to touch again.  One lane clears the lists and writes the
//               result's fixed part (D, the numbers flag; MSJ_CAPACITY when D > capacity, and every later kernel returns)
//   vd_tokens   the hot path, the shape of val_tokens: type bytes and partners of the block's 1 024 tokens and the 4 in
//               front into LDS.  The block's documents: two binary searches in d_doc_first per block, the starts that fall
//               into the block scattered into LDS, then a running maximum (the last start at or in front of a token = f)
//               and a running minimum from the other end (the first start behind it = e) over the block; the starts to
//               the left and right of the block come from the same two searches.  Linear for a block inside one document
//               and for a block of 1 024 one-token documents alike; d_depth is read by opening brackets only, as before.
//               A token that starts a document (and token T) is judged twice: as a token of its own document and as the
//               end of the stream of the one in front.  A token in error issues one atomicMin on its document's word (the
//               document's number by a binary search: on error only); a valid stream issues none
//   vd_strings  long and huge escaped bodies, as val_strings; an error finds its document by binary search
//   vd_count    direct commas of up to MSJ_VALIDATE_BIG_CONTAINERS wide containers, as val_count
//   vd_records  the ERR records of the number call, each competing in its document (returns at once when the number call
//               found no error or the records are not all there); its first block settles the counts of vd_count
//   vd_finish   grid-stride over the documents: a word that is not kNoError is unpacked into its verdict; n_invalid,
//               first_invalid and n_escaped by wave reductions and one atomic per block and field
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "launch.h"
#include "validate_block.h"
#include "validate_docs_math.h"

namespace msj_vdocs {

using namespace msj_val;

constexpr int kGridBlocks = 1024;  // most blocks of the grid-stride kernels over the documents

static_assert(sizeof(msj_document_verdict) == 16 && sizeof(msj_validate_documents_result) == 48, "ABI");

struct Window {
    uint64_t D, T;  // complete documents, the tokens they cover
    bool over;      // more documents than verdicts: nothing is judged
};
__device__ __forceinline__ Window window_of(const msj_documents_result *__restrict__ docs, uint64_t n, uint64_t capacity) {
    Window w;
    w.T = docs->tokens_complete < n ? docs->tokens_complete : n;
    w.D = docs->n_complete < w.T ? docs->n_complete : w.T;  // (a document has a token)
    w.over = w.D > capacity;
    if (w.over) w.D = 0;
    return w;
}

// the ERR records compete when the number call found errors and stored every record
__device__ __forceinline__ bool records_usable(const msj_numbers_result *__restrict__ nr, const msj_number *__restrict__ numbers,
                                               uint64_t numbers_capacity) {
    return nr && nr->n_errors > 0 && numbers && nr->n_numbers <= numbers_capacity;
}

__device__ __forceinline__ unsigned long long *word_of(msj_document_verdict *__restrict__ verdicts, uint64_t k) {
    return reinterpret_cast<unsigned long long *>(&verdicts[k].error_token);
}
// the packed error `e` goes to the document that holds token `tok` (its first token will do)
__device__ __forceinline__ void report(msj_document_verdict *__restrict__ verdicts, const uint32_t *__restrict__ first, uint64_t D,
                                       uint64_t tok, uint64_t e) {
    const uint64_t k = docs_starting_up_to(first, D, tok);
    if (k) atomicMin(word_of(verdicts, k - 1), (unsigned long long)e);  // (k - 1 < D <= capacity)
}

__global__ __launch_bounds__(kThreads) void vd_init(const msj_documents_result *__restrict__ docs, uint64_t n, uint64_t capacity,
                                                    const msj_numbers_result *__restrict__ nr, const msj_number *__restrict__ numbers,
                                                    uint64_t numbers_capacity, State *__restrict__ st,
                                                    msj_document_verdict *__restrict__ verdicts,
                                                    msj_validate_documents_result *__restrict__ result) {
    const Window w = window_of(docs, n, capacity);
    const uint64_t lanes = (uint64_t)gridDim.x * kThreads, lane = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    for (uint64_t k = lane; k < w.D; k += lanes) {
        msj_document_verdict v;
        v.code = 0;
        v.reserved = 0;
        v.error_token = kNoError;
        verdicts[k] = v;
    }
    if (lane != 0) return;
    st->err = kNoError;
    st->reserved64 = 0;
    st->big_count = st->long_count = st->huge_count = st->reserved = 0;
    for (uint32_t k = 0; k < kBig; k++) st->big_open[k] = st->big_close[k] = st->big_commas[k] = 0;
    msj_validate_documents_result r;
    r.code = w.over ? MSJ_CAPACITY : 0;
    r.flags = 0;
    if (w.D > 0 && (!nr || (nr->n_errors > 0 && !records_usable(nr, numbers, numbers_capacity)))) r.flags = MSJ_VALIDATE_NUMBERS_UNCHECKED;
    r.n_documents = w.over ? docs->n_complete : w.D;
    r.n_invalid = 0;
    r.first_invalid = ~0ull;
    r.n_escaped = 0;
    r.reserved = 0;
    *result = r;
}

__global__ __launch_bounds__(kThreads) void vd_tokens(const uint8_t *__restrict__ buf, uint64_t len, const uint32_t *__restrict__ idx,
                                                      uint64_t n64, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                      const uint32_t *__restrict__ match, const uint32_t *__restrict__ end,
                                                      const uint8_t *__restrict__ flags, const uint32_t *__restrict__ first,
                                                      const msj_documents_result *__restrict__ docs, uint64_t capacity, uint32_t max_depth,
                                                      State *__restrict__ st, msj_document_verdict *__restrict__ verdicts,
                                                      uint32_t *__restrict__ long_list, uint32_t long_cap, uint32_t *__restrict__ huge_list,
                                                      uint32_t huge_cap, uint32_t *__restrict__ block_esc) {
    __shared__ uint32_t s_type[(kBlock + kHalo + 4) / 4];
    __shared__ uint32_t s_match[kBlock + kHalo];
    __shared__ uint32_t s_start[kBlock];  // start + 1 where a document starts at the token, else 0
    __shared__ uint32_t s_k[2], w_f[kThreads / 64], w_e[kThreads / 64], w_esc[kThreads / 64];
    const Window w = window_of(docs, n64, capacity);
    const int64_t T = (int64_t)w.T, base = (int64_t)blockIdx.x * kBlock;
    if (w.D == 0 || base > T) {  // (the whole block: nothing of it is judged)
        if (threadIdx.x == 0) block_esc[blockIdx.x] = 0;
        return;
    }
    const int64_t mine = base + (int64_t)threadIdx.x * kPer;
    // tokens at or past T read as nothing: they belong to the cut document
    s_type[threadIdx.x + 1] = load_type_word(type, mine, T);
    {
        const uint4 m = load_match_quad(match, mine, T);
        uint32_t *d = s_match + kHalo + threadIdx.x * kPer;
        d[0] = m.x, d[1] = m.y, d[2] = m.z, d[3] = m.w;
        uint32_t *z = s_start + threadIdx.x * kPer;
        z[0] = z[1] = z[2] = z[3] = 0;
    }
    if (threadIdx.x == 0) {
        s_type[0] = load_type_word(type, base - kHalo, T);
        const uint4 m = load_match_quad(match, base - kHalo, T);
        s_match[0] = m.x, s_match[1] = m.y, s_match[2] = m.z, s_match[3] = m.w;
        s_k[0] = base > 0 ? (uint32_t)docs_starting_up_to(first, w.D, (uint64_t)base - 1) : 0u;  // documents that start in front of the block
    }
    if (threadIdx.x == 64) {
        s_type[kThreads + 1] = load_type_word(type, base + kBlock, T);
        s_k[1] = (uint32_t)docs_starting_up_to(first, w.D, (uint64_t)base + kBlock - 1);  // ... and up to its last token
    }
    __syncthreads();
    const uint32_t k0 = s_k[0], k1 = s_k[1];
    for (uint32_t k = k0 + threadIdx.x; k < k1; k += kThreads) {  // at most kBlock starts: 4 per lane
        const uint64_t s = first[k], o = s - (uint64_t)base;
        if (o < kBlock && s < (uint64_t)T) s_start[o] = (uint32_t)s + 1u;  // (no value from d_doc_first is used unchecked)
    }
    // the start (+ 1) of the document that holds token base - 1, and the first start behind the block
    uint32_t f_run = 0, e_run = (uint32_t)T;
    if (k0 > 0) {
        const uint32_t s = first[k0 - 1];
        if ((int64_t)s < base) f_run = s + 1u;
    }
    if (k1 < w.D) {
        const uint32_t s = first[k1];
        if ((int64_t)s < T && (int64_t)s >= base + (int64_t)kBlock) e_run = s;
    }
    __syncthreads();
    uint32_t start[kPer];
    {
        const uint32_t *z = s_start + threadIdx.x * kPer;
        uint32_t last = 0, head = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            start[k] = z[k];
            if (start[k]) last = start[k];
            if (start[k] && head == 0xFFFFFFFFu) head = start[k] - 1u;
        }
        const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const uint32_t inc_f = wave_scan_max(last), inc_e = wave_rscan_min(head);
        if (lane == 63) w_f[wave] = inc_f;
        if (lane == 0) w_e[wave] = inc_e;
        const uint32_t left = (uint32_t)__shfl_up((int)inc_f, 1), right = (uint32_t)__shfl_down((int)inc_e, 1);
        __syncthreads();
        for (uint32_t v = 0; v < wave; v++) f_run = max(f_run, w_f[v]);
        for (uint32_t v = wave + 1; v < kThreads / 64; v++) e_run = min(e_run, w_e[v]);
        if (lane > 0) f_run = max(f_run, left);
        if (lane < 63) e_run = min(e_run, right);
    }
    uint32_t e_of[kPer];  // the first start behind each of this lane's tokens
#pragma unroll
    for (int k = kPer - 1; k >= 0; k--) {
        e_of[k] = e_run;
        if (start[k]) e_run = start[k] - 1u;
    }

    const BlockTokens a{reinterpret_cast<const uint8_t *>(s_type), s_match, base, T, type, match, depth};
    const ByteReader r{buf, len};
    uint32_t escaped = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int64_t i = mine + k;
        if (i > T) break;
        // as the end of the stream of the document in front: only the structure can be wrong there
        if ((start[k] || i == T) && f_run) {
            uint32_t role;
            const uint32_t code = doc_token_rule(a, (int64_t)f_run - 1, i, i, max_depth, role);
            if (code) report(verdicts, first, w.D, f_run - 1u, pack_error((uint64_t)i, 0, code));
        }
        if (start[k]) f_run = start[k];
        if (i == T || !f_run) continue;  // (a token in front of the first document belongs to none)
        const int64_t f = (int64_t)f_run - 1, e = e_of[k];
        uint32_t role;
        const uint32_t code = doc_token_rule(a, f, e, i, max_depth, role);
        unsigned long long err = kNoError;
        if (code) {
            err = pack_error((uint64_t)i, 0, code);
        } else if (role == kRoleScalar) {
            const uint32_t t = a.type(i);
            if (t == '"') {
                if (flags[i] & MSJ_SPAN_ESCAPED) {
                    escaped++;
                    const uint64_t b = (uint64_t)idx[i] + 1, q = end[i];
                    if (q > len || q < b) {
                        err = pack_error((uint64_t)i, 1, kString);  // not what the span call writes: never read
                    } else if (q - b <= kLaneBody) {
                        if (string_bad_serial(r, b, q)) err = pack_error((uint64_t)i, 1, kString);
                    } else if (q - b <= kWaveBody) {
                        const uint32_t s = atomicAdd(&st->long_count, 1u);
                        if (s < long_cap) long_list[s] = (uint32_t)i;
                    } else {
                        const uint32_t s = atomicAdd(&st->huge_count, 1u);
                        if (s < huge_cap) huge_list[s] = (uint32_t)i;
                    }
                }
            } else if (t == 't' || t == 'f' || t == 'n') {
                const uint32_t c = atom_code(r, idx[i], t);
                if (c) err = pack_error((uint64_t)i, 1, c);
            }
        }
        if (err != kNoError) report(verdicts, first, w.D, (uint64_t)f, err);
        // a container wide enough for more than kMaxElements elements: its commas are counted behind this pass
        if (is_close(a.type(i))) {
            const uint32_t m = a.match(i);
            if (m != kNoPartner && (int64_t)m >= f && (int64_t)m < i && (uint64_t)(i - (int64_t)m - 1) >= kBigSpan) {
                const uint32_t s = atomicAdd(&st->big_count, 1u);
                if (s < kBig) st->big_open[s] = m, st->big_close[s] = (uint32_t)i;
            }
        }
    }
    escaped = wave_sum(escaped);
    if ((threadIdx.x & 63) == 0) w_esc[threadIdx.x >> 6] = escaped;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (int v = 0; v < kThreads / 64; v++) c += w_esc[v];
        block_esc[blockIdx.x] = c;  // a plain store per block: an atomic per block on one word serialises the whole grid
    }
}

__global__ __launch_bounds__(kThreads) void vd_strings(const uint8_t *__restrict__ buf, uint64_t len, const uint32_t *__restrict__ idx,
                                                       uint64_t n, const uint32_t *__restrict__ end, const uint32_t *__restrict__ first,
                                                       const msj_documents_result *__restrict__ docs, uint64_t capacity,
                                                       const State *__restrict__ st, msj_document_verdict *__restrict__ verdicts,
                                                       const uint32_t *__restrict__ long_list, uint32_t long_cap,
                                                       const uint32_t *__restrict__ huge_list, uint32_t huge_cap) {
    const uint32_t n_long = min(st->long_count, long_cap), n_huge = min(st->huge_count, huge_cap);
    if (n_long == 0 && n_huge == 0) return;
    const Window w = window_of(docs, n, capacity);
    const ByteReader r{buf, len};
    const uint32_t waves = gridDim.x * (kThreads / 64), wave = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const bool lane0 = (threadIdx.x & 63) == 0;
    for (uint32_t j = wave; j < n_long; j += waves) {
        const uint32_t tok = long_list[j];
        const uint64_t b = (uint64_t)idx[tok] + 1, e = end[tok];
        if (wave_body_bad(r, b, e, b, e) && lane0) report(verdicts, first, w.D, tok, pack_error(tok, 1, kString));
    }
    // a huge body: one contiguous piece per wave (at least kChunk bytes), so that the run in front of a piece is looked
    // at once per wave and the whole stays linear in the body
    for (uint32_t j = 0; j < n_huge; j++) {
        const uint32_t tok = huge_list[j];
        const uint64_t b = (uint64_t)idx[tok] + 1, e = end[tok];
        uint64_t piece = ((e - b + waves - 1) / waves + 63) & ~63ull;
        piece = piece < kChunk ? kChunk : piece;
        const uint64_t lo = b + (uint64_t)wave * piece;
        if (lo < e && wave_body_bad(r, b, e, lo, lo + piece < e ? lo + piece : e) && lane0)
            report(verdicts, first, w.D, tok, pack_error(tok, 1, kString));
    }
}

__global__ __launch_bounds__(kThreads) void vd_count(const uint8_t *__restrict__ type, const int32_t *__restrict__ depth, uint64_t n,
                                                     const msj_documents_result *__restrict__ docs, State *__restrict__ st) {
    if (st->big_count == 0) return;
    count_listed_commas(type, depth, docs->tokens_complete < n ? docs->tokens_complete : n, st);
}

__global__ __launch_bounds__(kThreads) void vd_records(const uint32_t *__restrict__ first, const msj_documents_result *__restrict__ docs,
                                                       uint64_t n, uint64_t capacity, const msj_numbers_result *__restrict__ nr,
                                                       const msj_number *__restrict__ numbers, uint64_t numbers_capacity,
                                                       const State *__restrict__ st, msj_document_verdict *__restrict__ verdicts,
                                                       msj_validate_documents_result *__restrict__ result) {
    const uint32_t cnt = st->big_count;
    const bool usable = records_usable(nr, numbers, numbers_capacity);
    if (cnt == 0 && !usable) return;
    const Window w = window_of(docs, n, capacity);
    if (w.D == 0) return;
    if (blockIdx.x == 0) {
        if (cnt > kBig) {
            // all or nothing: which 64 made it into the list depends on the order of the blocks
            if (threadIdx.x == 0) atomicOr(&result->flags, MSJ_VALIDATE_COUNTS_CLIPPED);
        } else if (threadIdx.x < cnt && 1ull + st->big_commas[threadIdx.x] > kMaxElements) {
            const uint32_t close = st->big_close[threadIdx.x];
            report(verdicts, first, w.D, close, pack_error(close, 1, kCapacity));
        }
    }
    if (!usable) return;
    const uint64_t lanes = (uint64_t)gridDim.x * kThreads, lane = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t records = nr->n_numbers;
    for (uint64_t j = lane; j < records; j += lanes) {
        const msj_number rec = numbers[j];
        if (rec.kind >= MSJ_NUMBER_ERR_SYNTAX && rec.token < w.T) report(verdicts, first, w.D, rec.token, pack_error(rec.token, 1, kNumber));
    }
}

__global__ __launch_bounds__(kThreads) void vd_finish(const msj_documents_result *__restrict__ docs, uint64_t n, uint64_t capacity,
                                                      const uint32_t *__restrict__ block_esc, uint32_t nb,
                                                      msj_document_verdict *__restrict__ verdicts,
                                                      msj_validate_documents_result *__restrict__ result) {
    __shared__ unsigned long long w_bad[kThreads / 64], w_first[kThreads / 64], w_esc[kThreads / 64];
    const Window w = window_of(docs, n, capacity);
    if (w.D == 0) return;
    const uint64_t lanes = (uint64_t)gridDim.x * kThreads, lane = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    unsigned long long bad = 0, lowest = ~0ull, esc = 0;
    for (uint64_t k = lane; k < w.D; k += lanes) {
        const uint64_t e = *word_of(verdicts, k);
        if (e == kNoError) continue;
        msj_document_verdict v;
        v.code = (int32_t)packed_code(e);
        v.reserved = 0;
        v.error_token = packed_token(e);
        verdicts[k] = v;
        bad++;
        lowest = k < lowest ? k : lowest;
    }
    for (uint64_t b = lane; b < nb; b += lanes) esc += block_esc[b];
    bad = wave_sum64(bad);
    lowest = wave_min(lowest);
    esc = wave_sum64(esc);
    if ((threadIdx.x & 63) == 0) w_bad[threadIdx.x >> 6] = bad, w_first[threadIdx.x >> 6] = lowest, w_esc[threadIdx.x >> 6] = esc;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int v = 1; v < kThreads / 64; v++) {
        bad += w_bad[v];
        esc += w_esc[v];
        lowest = w_first[v] < lowest ? w_first[v] : lowest;
    }
    if (bad) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&result->n_invalid), bad);
        atomicMin(reinterpret_cast<unsigned long long *>(&result->first_invalid), lowest);
    }
    if (esc) atomicAdd(reinterpret_cast<unsigned long long *>(&result->n_escaped), esc);
}

}  // namespace msj_vdocs

// (capacity: the documents' error words live in d_verdicts, so nothing here grows with it)
extern "C" uint64_t msj_validate_documents_workspace_bytes(uint64_t n, uint64_t len, uint64_t capacity) {
    (void)capacity;
    return msj_measure(msj_val::layout, n, len) + 64;
}

extern "C" int msj_launch_validate_documents(const msj_token_view &t, const msj_split_view &sp, const msj_number_view &nv, uint32_t max_depth,
                                             msj_document_verdict *d_verdicts, uint64_t capacity, msj_validate_documents_result *d_result,
                                             void *d_ws, void *stream) {
    using namespace msj_vdocs;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const msj_val::Work w = msj_place(msj_val::layout, d_ws, t.n, t.len);  // (token T <= n, the last document's end of stream, is judged too)
    // the grid-stride kernels over the documents: there are at most min(n, capacity) of them
    const uint64_t most = t.n < capacity ? t.n : capacity;
    const uint32_t gb = (uint32_t)((most + (uint64_t)kThreads * 4 - 1) / ((uint64_t)kThreads * 4));
    const uint32_t doc_blocks = gb < 1 ? 1u : (gb > (uint32_t)kGridBlocks ? (uint32_t)kGridBlocks : gb);
    hipLaunchKernelGGL(vd_init, dim3(doc_blocks), dim3(kThreads), 0, s, sp.d_docs, t.n, capacity, nv.d_numbers_result, nv.d_numbers,
                       nv.numbers_capacity, w.st, d_verdicts, d_result);
    if (t.n == 0) return (int)hipGetLastError();  // no document: the zero result is all there is
    hipLaunchKernelGGL(vd_tokens, dim3(w.nb), dim3(kThreads), 0, s, t.d_buf, t.len, t.d_idx, t.n, t.d_type, t.d_depth, t.d_match, t.d_end, t.d_flags,
                       sp.d_doc_first, sp.d_docs, capacity, max_depth, w.st, d_verdicts, w.long_list, w.long_cap, w.huge_list, w.huge_cap, w.block_esc);
    hipLaunchKernelGGL(vd_strings, dim3(kListBlocks), dim3(kThreads), 0, s, t.d_buf, t.len, t.d_idx, t.n, t.d_end, sp.d_doc_first, sp.d_docs,
                       capacity, w.st, d_verdicts, w.long_list, w.long_cap, w.huge_list, w.huge_cap);
    hipLaunchKernelGGL(vd_count, dim3(kListBlocks * 4), dim3(kThreads), 0, s, t.d_type, t.d_depth, t.n, sp.d_docs, w.st);
    hipLaunchKernelGGL(vd_records, dim3(kListBlocks), dim3(kThreads), 0, s, sp.d_doc_first, sp.d_docs, t.n, capacity, nv.d_numbers_result,
                       nv.d_numbers, nv.numbers_capacity, w.st, d_verdicts, d_result);
    hipLaunchKernelGGL(vd_finish, dim3(doc_blocks), dim3(kThreads), 0, s, sp.d_docs, t.n, capacity, w.block_esc, w.nb, d_verdicts, d_result);
    return (int)hipGetLastError();
}
