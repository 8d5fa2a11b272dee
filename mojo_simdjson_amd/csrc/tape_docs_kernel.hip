// A tape and a string buffer for every complete document of a window -- msj_tape_documents_device (include/msj_stage1.h):
// what msj_tape_device (tape_kernel.hip) gives for each document's token sub-arrays, in one pass over the window instead of
// one call per document.  The per-token arithmetic is the unchanged tape_math.h; where a word, a record and a root word lie
// in the window's arrays, and what is local to a document, is tape_docs_math.h.  Both are host + device and checked on the
// CPU by tests/test_tape_documents_math.py.  D = d_docs->n_complete and T = d_docs->tokens_complete are read on the device
// by every kernel: the host never learns them.
//
// The layout is a closed form of the window's prefix sums (W words, S string bytes, N number tokens; tape_docs_math.h), so
// the launches are msj_tape_device's, each over the whole window (a block is kBlock tokens; tape_block.h holds what is
// shared):
//   (memset)     the call's state, the blocks' byte sums, the element counts
//   td_sums      tape_sums over the tokens [f_0, T) (number tokens from token 0: the records are the window's).  New: the
//                block's document starts (block_docs, docs_block.h) and, for each of them, the string bytes of the block's tokens in
//                front of it: doc_sbase[k], 8 bytes per document
//   td_long_len  tape_long_len; a long body adds its length to its block's byte sum and to doc_sbase[k] of the documents
//                that start behind it in the same block (fewer than kBlock, and the body has more than kLaneBody bytes:
//                linear in len).  Behind the scan S(f_k) = doc_sbase[k] + the prefix of f_k's block, for every lane
//   td_scan      tape_scan's sums over the blocks; the result but for n_built
//   td_pos       tape_pos (pos_block) with the tokens outside [f_0, T) masked: pos[i] - 1 = W(i).  Every comma credits its
//                container unchanged: a comma at depth >= 1 finds its bracket at or behind its document's first token, whose
//                depth is 0
//   tape_min64 (twice), td_span: unchanged
//   td_emit      the words, through LDS.  A block's tokens with their document: two binary searches in d_doc_first per
//                block, the starts inside it scattered into LDS as flags, a prefix count = the document's number in the
//                block (linear for a block inside one document and for a block of kBlock one-token documents); f_k, W(f_k),
//                S(f_k) and the verdict's code of the block's documents in LDS tables.  The lane that holds f_k stages the
//                two root words in front of its token (the end of document k - 1, the start of k) and writes record k.  A
//                block writes W(next) - W(base) + 2 * (its starts) <= 4 * kBlock contiguous words
//   td_long_out  the blocks' counts of built documents into n_built, then tape_long_out
// A document with a verdict code keeps its slot; its words are stored as 0 and its short strings are not written.  Every
// index from d_match, d_end or d_doc_first is checked before it is used and every store is checked against its capacity;
// no store address depends on doc_sbase or on a table entry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "docs_block.h"
#include "launch.h"
#include "tape_block.h"
#include "tape_docs_math.h"

namespace msj_tdocs {

using namespace msj_tape;
using namespace msj::tdocs;

constexpr uint32_t kStage = 4 * kBlock;  // words a block stages at most: kBlock one-token number documents, 2 + 2 root words each

static_assert(sizeof(msj_document_tape) == 32 && sizeof(msj_tape_documents_result) == 64, "ABI");

__global__ __launch_bounds__(kThreads) void td_sums(const uint8_t *__restrict__ buf, uint64_t len, const uint32_t *__restrict__ idx, uint64_t n,
                                                    const uint8_t *__restrict__ type, const uint32_t *__restrict__ end,
                                                    const uint8_t *__restrict__ flags, const uint32_t *__restrict__ first,
                                                    const msj_documents_result *__restrict__ docs, uint64_t capacity, const Work w) {
    __shared__ uint32_t s_a[3][kWaves];
    __shared__ uint64_t s_b[kWaves];
    __shared__ uint32_t s_flag[kThreads], s_k[2], s_w32[kWaves];
    __shared__ uint64_t s_w64[kWaves];
    const Window win = load_window(docs, first, n, capacity);
    const uint64_t base = (uint64_t)blockIdx.x * kBlock, mine = base + (uint64_t)threadIdx.x * kPer;
    if (win.D == 0 || base >= win.T) {  // (the whole block)
        if (threadIdx.x == 0) w.b_words[blockIdx.x] = w.b_nums[blockIdx.x] = w.b_nstr[blockIdx.x] = 0;
        return;
    }
    uint32_t words = 0, nums = 0, nstr = 0;
    uint64_t sbytes = 0, before[kPer] = {0, 0, 0, 0};
    if (mine < win.T) {
        const uint32_t tw = load_byte_quad(type, mine, n), fw = load_byte_quad(flags, mine, n);
        const ByteReader r{buf, len};
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            const uint64_t i = mine + k;
            before[k] = sbytes;
            if (i >= win.T) continue;
            const uint32_t t = (tw >> (8 * k)) & 0xFFu, fl = (fw >> (8 * k)) & 0xFFu;
            nums += is_number(fl);
            if (i < win.f0) continue;
            words += words_per_token(t, fl);
            if (is_string(t) && !is_number(fl)) {
                nstr++;
                sbytes += 4;
                const Body y = body_of(idx, end, fl, i, len);
                if (y.is_long) {
                    const uint32_t s = atomicAdd(&w.st->long_count, 1u);
                    if (s < w.long_cap) w.long_list[s] = (uint32_t)i;
                } else if (y.ok) {
                    sbytes += y.escaped ? unescape_serial(r, NoWrite{}, y.b, y.q) : y.q - y.b;
                }
            }
        }
    }
    if (!win.over) {  // S(f_k) within the block, short bodies (the long ones add theirs in td_long_len)
        const BlockDocs bd = block_docs(first, win, base, s_flag, s_k, s_w32);
        uint64_t total;
        const uint64_t excl = block_scan(sbytes, s_w64, total);
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            const uint64_t kdoc = (uint64_t)bd.k0 + bd.rank[k] - 1;
            if (((bd.starts >> k) & 1u) && kdoc < win.D) w.doc_sbase[kdoc] = excl + before[k];
        }
    }
    words = wave_sum(words), nums = wave_sum(nums), nstr = wave_sum(nstr), sbytes = wave_sum64(sbytes);
    if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        s_a[0][wv] = words, s_a[1][wv] = nums, s_a[2][wv] = nstr, s_b[wv] = sbytes;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int wv = 1; wv < kWaves; wv++) words += s_a[0][wv], nums += s_a[1][wv], nstr += s_a[2][wv], sbytes += s_b[wv];
        w.b_words[blockIdx.x] = words, w.b_nums[blockIdx.x] = nums, w.b_nstr[blockIdx.x] = nstr;
        atomicAdd(reinterpret_cast<unsigned long long *>(w.b_sbytes + blockIdx.x), (unsigned long long)sbytes);
    }
}

__global__ __launch_bounds__(kThreads) void td_long_len(const uint8_t *__restrict__ buf, uint64_t len, const uint32_t *__restrict__ idx,
                                                        uint64_t n, const uint32_t *__restrict__ end, const uint8_t *__restrict__ flags,
                                                        const uint32_t *__restrict__ first, const msj_documents_result *__restrict__ docs,
                                                        uint64_t capacity, const Work w) {
    const uint32_t cnt = min(w.st->long_count, w.long_cap);
    if (cnt == 0) return;
    const Window win = load_window(docs, first, n, capacity);
    const ByteReader r{buf, len};
    const uint32_t waves = gridDim.x * kWaves, wave = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (uint32_t j = wave; j < cnt; j += waves) {
        const uint32_t tok = w.long_list[j];
        const Body y = body_of(idx, end, flags[tok], tok, len);
        const uint64_t ulen = y.escaped ? wave_unescape(r, BufWriter{nullptr, 0, 0}, y.b, y.q, true) : y.q - y.b;
        if (lane == 0) {
            w.long_ulen[(y.b - 1) >> 10] = (uint32_t)ulen;
            atomicAdd(reinterpret_cast<unsigned long long *>(w.b_sbytes + tok / kBlock), (unsigned long long)ulen);
        }
        if (win.over) continue;
        // the documents that start behind the body in its block: their bases were stored by td_sums
        const uint64_t block_end = umin64(((uint64_t)tok / kBlock + 1) * kBlock, win.T);
        const uint64_t k_lo = docs_starting_up_to(first, win.D, tok), k_hi = docs_starting_up_to(first, win.D, block_end - 1);
        for (uint64_t k = k_lo + lane; k < k_hi; k += 64) {
            const uint64_t s = first[k];
            if (s > tok && s < block_end) atomicAdd(reinterpret_cast<unsigned long long *>(w.doc_sbase + k), (unsigned long long)ulen);
        }
    }
}

__global__ __launch_bounds__(1024) void td_scan(const Work w, uint64_t n, const uint32_t *__restrict__ first,
                                                const msj_documents_result *__restrict__ docs, uint64_t capacity, uint64_t tape_capacity,
                                                const uint8_t *string_buf, uint64_t string_capacity, uint64_t numbers_capacity,
                                                msj_tape_documents_result *__restrict__ result) {
    __shared__ uint64_t s_w[4][16];
    uint64_t run[4] = {0, 0, 0, 0};
    scan_blocks(w, s_w, run);
    if (threadIdx.x != 0) return;
    const Window win = load_window(docs, first, n, capacity);
    State *st = w.st;
    st->words = run[0], st->nums = run[1], st->nstr = run[2], st->sbytes = run[3];
    st->skip = (win.over || win.D == 0) ? 1u : 0u;
    msj_tape_documents_result res;
    res.flags = 0;
    res.n_documents = win.D;
    res.n_built = 0;  // (td_long_out adds the blocks' counts)
    res.tape_words = window_words(run[0], win.D);
    res.string_bytes = run[3];
    res.n_strings = run[2];
    res.n_numbers = run[1];
    res.reserved = 0;
    const bool fits = !win.over && res.tape_words <= tape_capacity && (!string_buf || res.string_bytes <= string_capacity) &&
                      run[1] <= numbers_capacity;
    res.code = fits ? MSJ_SUCCESS : MSJ_CAPACITY;
    *result = res;
}

__global__ __launch_bounds__(kThreads) void td_pos(uint64_t n, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                   const uint32_t *__restrict__ match, const uint8_t *__restrict__ flags,
                                                   const uint32_t *__restrict__ first, const msj_documents_result *__restrict__ docs,
                                                   uint64_t capacity, const Work w) {
    if (w.st->skip) return;
    const Window win = load_window(docs, first, n, capacity);
    pos_block(n, win.f0, win.T, type, depth, match, flags, w);
}

__global__ __launch_bounds__(kThreads) void td_min64(const int32_t *__restrict__ in, uint32_t n_in, int32_t *__restrict__ out,
                                                     const State *__restrict__ st) {
    if (st->skip) return;
    min64_body(in, n_in, out);
}

__global__ __launch_bounds__(kThreads) void td_span(uint64_t n, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                    const Work w) {
    if (w.st->skip) return;
    span_body(n, type, depth, w);
}

// What td_emit's emission loop and copy-out need of the call's arguments.  Thread 0 leaves them in LDS and every lane reads
// them back behind the table pass: from there on they live in vector registers, of which this kernel has plenty (its LDS
// sets the occupancy), instead of in scalar ones held across the table pass and the two scans
struct EmitLate {
    const uint32_t *match, *cnt;
    const msj_number *numbers;
    uint64_t numbers_capacity;
    uint64_t *tape;
    uint64_t tape_capacity;
    uint8_t *string_buf;
    uint64_t string_capacity;
    msj_document_tape *doc_tapes;
    uint64_t *long_soff;
};

__global__ __launch_bounds__(kThreads) void td_emit(const uint8_t *__restrict__ buf, uint64_t len, const uint32_t *__restrict__ idx, uint64_t n,
                                                    const uint8_t *__restrict__ type, const uint32_t *__restrict__ match_,
                                                    const uint32_t *__restrict__ end, const uint8_t *__restrict__ flags,
                                                    const uint32_t *__restrict__ first, const msj_documents_result *__restrict__ docs,
                                                    uint64_t capacity, const msj_document_verdict *__restrict__ verdicts,
                                                    const msj_number *__restrict__ numbers_, uint64_t numbers_capacity_,
                                                    uint64_t *__restrict__ tape_, uint64_t tape_capacity_, uint8_t *__restrict__ string_buf_,
                                                    uint64_t string_capacity_, msj_document_tape *__restrict__ doc_tapes_, const Work w) {
    __shared__ uint64_t s_words[kStage];
    // per document of the block, entry j = document k0 - 1 + j (0: the one that began in front; nd + 1: the first behind)
    __shared__ uint64_t s_sf[kBlock + 2];                  // S(f)
    __shared__ uint32_t s_f[kBlock + 2], s_wf[kBlock + 2];  // f, W(f)
    __shared__ int32_t s_code[kBlock + 2];
    __shared__ uint32_t s_flag[kThreads], s_k[2], s_w32[kWaves];
    __shared__ uint64_t s_w64[kWaves];
    __shared__ EmitLate s_late;
    if (w.st->skip) return;
    const Window win = load_window(docs, first, n, capacity);
    const uint64_t base = (uint64_t)blockIdx.x * kBlock, mine = base + (uint64_t)threadIdx.x * kPer;
    if (base >= win.T) {
        if (threadIdx.x == 0) w.b_built[blockIdx.x] = 0;
        return;
    }
    if (threadIdx.x == 0)
        s_late = EmitLate{match_, w.cnt, numbers_, numbers_capacity_, tape_, tape_capacity_, string_buf_, string_capacity_, doc_tapes_, w.long_soff};
    const BlockDocs bd = block_docs(first, win, base, s_flag, s_k, s_w32);
    const uint64_t w_total = w.st->words, s_total = w.st->sbytes;
    const uint64_t w_base = w.b_words[blockIdx.x], w_next = blockIdx.x + 1 < w.nb ? w.b_words[blockIdx.x + 1] : w_total;
    for (uint32_t j = threadIdx.x; j <= bd.nd + 1; j += kThreads) {
        const int64_t k = (int64_t)bd.k0 - 1 + j;
        uint32_t f = (uint32_t)win.T, wf = (uint32_t)w_total;  // (behind the last document: the window's end)
        uint64_t sf = s_total;
        int32_t code = 0;
        if (k < 0) {
            f = 0, wf = 0, sf = 0;
        } else if ((uint64_t)k < win.D) {
            const uint32_t s = first[k];
            if (s < win.T) f = s, wf = w.pos[s] - 1, sf = w.doc_sbase[k] + w.b_sbytes[s / kBlock];
            if (verdicts) code = verdicts[k].code;
        }
        s_f[j] = f, s_wf[j] = wf, s_sf[j] = sf, s_code[j] = code;
    }
    const ByteReader r{buf, len};
    uint32_t tw = 0, fw = 0, pk[kPer] = {0, 0, 0, 0};
    {
        tw = load_byte_quad(type, mine, win.T), fw = load_byte_quad(flags, mine, win.T);  // (nothing at or past T)
        if (mine + 4 <= n) {
            const uint4 q = *reinterpret_cast<const uint4 *>(w.pos + mine);
            pk[0] = q.x, pk[1] = q.y, pk[2] = q.z, pk[3] = q.w;
        } else {
            for (int k = 0; k < kPer && mine + k < n; k++) pk[k] = w.pos[mine + k];
        }
    }
    // this lane's numbers and string bytes, then their ranks / offsets in the window
    uint32_t nums = 0;
    uint64_t sb[kPer] = {0, 0, 0, 0}, sbytes = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint64_t i = mine + k;
        if (i >= win.T) break;
        const uint32_t t = (tw >> (8 * k)) & 0xFFu, fl = (fw >> (8 * k)) & 0xFFu;
        nums += is_number(fl);
        if (i >= win.f0 && is_string(t) && !is_number(fl)) {
            const Body y = body_of(idx, end, fl, i, len);
            uint64_t ulen = 0;
            if (y.is_long)
                ulen = w.long_ulen[(y.b - 1) >> 10];
            else if (y.ok)
                ulen = y.escaped ? unescape_serial(r, NoWrite{}, y.b, y.q) : y.q - y.b;
            sb[k] = 4 + ulen;
            sbytes += sb[k];
        }
    }
    uint32_t tot32;
    uint64_t tot64;
    uint64_t rank = (uint64_t)w.b_nums[blockIdx.x] + block_scan(nums, s_w32, tot32);
    uint64_t soff = w.b_sbytes[blockIdx.x] + block_scan(sbytes, s_w64, tot64);  // (has the barriers that publish the tables)
    uint32_t built = 0;
    const EmitLate late = s_late;  // (published by the scans' barriers)
    const uint32_t *match = late.match;
    const msj_number *numbers = late.numbers;
    const uint64_t numbers_capacity = late.numbers_capacity, tape_capacity = late.tape_capacity, string_capacity = late.string_capacity;
    uint64_t *tape = late.tape;
    uint8_t *string_buf = late.string_buf;
    msj_document_tape *doc_tapes = late.doc_tapes;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint64_t i = mine + k;
        if (i >= win.T) break;
        const uint32_t t = (tw >> (8 * k)) & 0xFFu, fl = (fw >> (8 * k)) & 0xFFu;
        if (i < win.f0) {  // in front of the first document: nothing but the number's rank
            rank += is_number(fl);
            continue;
        }
        const uint32_t j = bd.rank[k];  // <= nd <= kBlock
        const uint32_t slot = block_slot(pk[k] - 1, w_base, j);
        const bool stage = slot + 1 < kStage;  // (pos[] is this call's own prefix sum: always, on arrays of the split)
        const uint64_t f = s_f[j], e = s_f[j + 1], wf = s_wf[j], sf = s_sf[j];
        const bool dropped = s_code[j] != 0;
        if ((bd.starts >> k) & 1u) {
            const uint64_t kdoc = (uint64_t)bd.k0 + j - 1, we = s_wf[j + 1];
            if (stage && slot >= 2) s_words[slot - 2] = root_last_word(), s_words[slot - 1] = root_first_word(document_words(wf, we));
            if (kdoc < win.D) {  // (<= capacity)
                doc_tapes[kdoc] = document_record<msj_document_tape>(kdoc, wf, we, sf, s_sf[j + 1], s_code[j]);
                built += !dropped;
            }
        }
        if (is_number(fl)) {
            uint64_t bits = 0;
            uint32_t kind = kNumberInt64;
            if (rank < numbers_capacity) {
                const msj_number rec = numbers[rank];
                if (rec.kind == kNumberInt64 || rec.kind == kNumberDouble) bits = rec.bits, kind = rec.kind;
            }
            rank++;
            if (stage) s_words[slot] = dropped ? 0 : number_tag_word(kind), s_words[slot + 1] = dropped ? 0 : bits;
        } else if (is_open(t) || is_close(t)) {
            const uint32_t m = match[i];
            const uint64_t pm = partner_inside(m, f, e) ? local_pos((uint64_t)w.pos[m] - 1, wf) : 0;  // (e <= T <= n)
            uint64_t word = 0;
            if (!dropped) word = is_open(t) ? open_word(t, elements(m == i + 1, late.cnt[i]), pm) : close_word(t, pm);
            if (stage) s_words[slot] = word;
        } else if (is_string(t)) {
            if (stage) s_words[slot] = dropped ? 0 : string_word(local_offset(soff, sf));
            const Body y = body_of(idx, end, fl, i, len);
            if (y.is_long) {
                late.long_soff[(y.b - 1) >> 10] = soff;  // (also of a dropped document: td_long_out writes what the list holds)
            } else if (string_buf && !dropped) {
                const BufWriter wr{string_buf, soff, string_capacity};
                const uint64_t ulen = sb[k] - 4;
                for (int x = 0; x < 4; x++) wr.put(x, (uint32_t)(ulen >> (8 * x)) & 0xFFu);
                const BufWriter body{string_buf, soff + 4, string_capacity};
                if (y.ok) {
                    if (y.escaped) {
                        (void)unescape_serial(r, body, y.b, y.q);
                    } else {
                        for (uint64_t x = 0; x < ulen; x++) body.put(x, r.at(y.b + x));
                    }
                }
            }
            soff += sb[k];
        } else if (is_atom(t)) {
            if (stage) s_words[slot] = dropped ? 0 : atom_word(t);
        }
        if (i + 1 == win.T) {  // the last document's end: the one root word no block's slice holds
            const uint64_t a = window_words(w_total, win.D) - 1;
            if (a < tape_capacity) tape[a] = root_last_word();
        }
    }
    built = wave_sum(built);
    if ((threadIdx.x & 63) == 0) s_w32[threadIdx.x >> 6] = built;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int wv = 1; wv < kWaves; wv++) built += s_w32[wv];
        w.b_built[blockIdx.x] = built;
    }
    const int64_t origin = block_origin(w_base, bd.k0);
    const uint64_t nwords = umin64((w_next - w_base) + 2ull * bd.nd, kStage);
    for (uint32_t x = threadIdx.x; x < nwords; x += kThreads) {
        const int64_t a = origin + x;
        if (a >= 0 && (uint64_t)a < tape_capacity) tape[a] = s_words[x];
    }
}

__global__ __launch_bounds__(kThreads) void td_long_out(const uint8_t *__restrict__ buf, uint64_t len, const uint32_t *__restrict__ idx,
                                                        const uint32_t *__restrict__ end, const uint8_t *__restrict__ flags,
                                                        uint8_t *__restrict__ string_buf, uint64_t string_capacity,
                                                        msj_tape_documents_result *__restrict__ result, const Work w) {
    if (w.st->skip) return;
    const uint32_t lanes = gridDim.x * kThreads;
    uint64_t built = 0;
    for (uint32_t b = blockIdx.x * kThreads + threadIdx.x; b < w.nb; b += lanes) built += w.b_built[b];
    built = wave_sum64(built);
    if ((threadIdx.x & 63) == 0 && built) atomicAdd(reinterpret_cast<unsigned long long *>(&result->n_built), (unsigned long long)built);
    if (!string_buf) return;
    long_out_body(buf, len, idx, end, flags, string_buf, string_capacity, w);
}

}  // namespace msj_tdocs

extern "C" uint64_t msj_tape_documents_workspace_bytes(uint64_t n, uint64_t len, uint64_t capacity) {
    return msj_measure(msj_tape::layout, n, len, msj_tdocs::most_documents(n, capacity)) + 64;
}

extern "C" int msj_launch_tape_documents(const msj_token_view &t, const msj_split_view &sp, const msj_number_view &nv,
                                         const msj_document_verdict *d_verdicts, uint64_t *d_tape, uint64_t tape_capacity,
                                         uint8_t *d_string_buf, uint64_t string_capacity, msj_document_tape *d_doc_tapes, uint64_t capacity,
                                         msj_tape_documents_result *d_result, void *d_ws, void *stream) {
    using namespace msj_tdocs;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Work w = msj_place(layout, d_ws, t.n, t.len, most_documents(t.n, capacity));
    const uint32_t nb = w.nb, nb64 = (nb + 63) / 64, nb4096 = (nb64 + 63) / 64;
    if (hipMemsetAsync(w.st, 0, (size_t)(reinterpret_cast<uint8_t *>(w.pos) - reinterpret_cast<uint8_t *>(w.st)), s) != hipSuccess)
        return (int)hipGetLastError();
    if (t.n > 0) {
        hipLaunchKernelGGL(td_sums, dim3(nb), dim3(kThreads), 0, s, t.d_buf, t.len, t.d_idx, t.n, t.d_type, t.d_end, t.d_flags, sp.d_doc_first,
                           sp.d_docs, capacity, w);
        hipLaunchKernelGGL(td_long_len, dim3(kListBlocks), dim3(kThreads), 0, s, t.d_buf, t.len, t.d_idx, t.n, t.d_end, t.d_flags, sp.d_doc_first,
                           sp.d_docs, capacity, w);
    }
    hipLaunchKernelGGL(td_scan, dim3(1), dim3(1024), 0, s, w, t.n, sp.d_doc_first, sp.d_docs, capacity, tape_capacity, d_string_buf, string_capacity,
                       nv.numbers_capacity, d_result);
    if (t.n == 0) return (int)hipGetLastError();  // no document: the zero result is all there is
    hipLaunchKernelGGL(td_pos, dim3(nb), dim3(kThreads), 0, s, t.n, t.d_type, t.d_depth, t.d_match, t.d_flags, sp.d_doc_first, sp.d_docs, capacity,
                       w);
    hipLaunchKernelGGL(td_min64, dim3((nb64 + kWaves - 1) / kWaves), dim3(kThreads), 0, s, w.b_min, nb, w.b_min64, w.st);
    hipLaunchKernelGGL(td_min64, dim3((nb4096 + kWaves - 1) / kWaves), dim3(kThreads), 0, s, w.b_min64, nb64, w.b_min4096, w.st);
    hipLaunchKernelGGL(td_span, dim3((nb + kWaves - 1) / kWaves), dim3(kThreads), 0, s, t.n, t.d_type, t.d_depth, w);
    hipLaunchKernelGGL(td_emit, dim3(nb), dim3(kThreads), 0, s, t.d_buf, t.len, t.d_idx, t.n, t.d_type, t.d_match, t.d_end, t.d_flags, sp.d_doc_first,
                       sp.d_docs, capacity, d_verdicts, nv.d_numbers, nv.numbers_capacity, d_tape, tape_capacity, d_string_buf, string_capacity,
                       d_doc_tapes, w);
    hipLaunchKernelGGL(td_long_out, dim3(kListBlocks), dim3(kThreads), 0, s, t.d_buf, t.len, t.d_idx, t.d_end, t.d_flags, d_string_buf,
                       string_capacity, d_result, w);
    return (int)hipGetLastError();
}
