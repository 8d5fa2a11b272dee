// The document's tape and string buffer -- msj_tape_device (include/msj_stage1.h): what the reference's TapeBuilder
// (generic/stage2/tape_builder.mojo) leaves in Document.tape / Document.string_buf, without the walk.  The per-token
// arithmetic is tape_math.h, host + device, checked on the CPU by tests/test_tape_math.py.
//
// Launches, all on the caller's stream, no host round trip (a block is kBlock tokens):
//   (memset)      the call's state and the element counts
//   tape_sums     per block: words, number tokens, strings and string-buffer bytes.  idx / end are loaded at string tokens
//                 only, the escape walk runs only where MSJ_SPAN_ESCAPED is set; a body over kLaneBody bytes goes to the long
//                 list (bounded by len / kLaneBody: never full)
//   tape_long_len one wave per long body: its unescaped length, 64 bytes per step, into the long table (a body of more
//                 than kLaneBody bytes is the only one that starts in its KiB of the buffer: the table is indexed by
//                 idx >> 10) and onto its block's byte sum
//   tape_scan     one workgroup: exclusive sums over the blocks; sizes, code and the two root words
//   tape_pos      pos[] (uint32 per token, workspace) and the element counts: every comma credits its container.  Its
//                 opening bracket is the nearest token in front with a smaller depth, its closing bracket the nearest one
//                 behind: both from an 8-ary min tree over the block's depths in LDS.  A comma whose container opens in
//                 front of the block credits the closing bracket, which hands the sum to its partner with one atomic;
//                 only commas at the block's minimum depth have a container that spans the whole block: one pending
//                 count per block
//   tape_min64    (twice) minima over 64 and 4096 blocks
//   tape_span     one wave per block with a pending count: the nearest token in front of the block with a smaller depth,
//                 down the block minima; one atomic
//   tape_emit     the words, through LDS, as coalesced stores; partners' positions, number records and counts as
//                 gathers; a string of at most kLaneBody bytes is written by its lane, a longer one leaves its offset
//                 in the long table
//   tape_long_out one wave per long body: length prefix and bytes, 64 bytes per step
// Work is linear in n and len whatever the nesting and whatever a body holds.  Every index that comes from d_match or
// d_end is checked before it is used, every store is checked against its capacity.  What the window call
// (tape_docs_kernel.hip) runs unchanged lives in tape_block.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "launch.h"
#include "tape_block.h"

namespace msj_tape {

__global__ __launch_bounds__(kThreads) void tape_sums(const uint8_t *__restrict__ buf, uint64_t len, const uint32_t *__restrict__ idx,
                                                      uint64_t n, const uint8_t *__restrict__ type, const uint32_t *__restrict__ end,
                                                      const uint8_t *__restrict__ flags, const Work w) {
    __shared__ uint32_t s_a[3][kWaves];
    __shared__ uint64_t s_b[kWaves];
    const uint64_t mine = (uint64_t)blockIdx.x * kBlock + (uint64_t)threadIdx.x * kPer;
    uint32_t words = 0, nums = 0, nstr = 0;
    uint64_t sbytes = 0;
    if (mine < n) {
        const uint32_t tw = load_byte_quad(type, mine, n), fw = load_byte_quad(flags, mine, n);
        const ByteReader r{buf, len};
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            const uint64_t i = mine + k;
            if (i >= n) break;
            const uint32_t t = (tw >> (8 * k)) & 0xFFu, fl = (fw >> (8 * k)) & 0xFFu;
            words += words_per_token(t, fl);
            nums += is_number(fl);
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
    words = wave_sum(words), nums = wave_sum(nums), nstr = wave_sum(nstr), sbytes = wave_sum64(sbytes);
    if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        s_a[0][wv] = words, s_a[1][wv] = nums, s_a[2][wv] = nstr, s_b[wv] = sbytes;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int wv = 1; wv < kWaves; wv++) words += s_a[0][wv], nums += s_a[1][wv], nstr += s_a[2][wv], sbytes += s_b[wv];
        w.b_words[blockIdx.x] = words, w.b_nums[blockIdx.x] = nums, w.b_nstr[blockIdx.x] = nstr;
        // (the long bodies of the block add theirs behind this kernel: an atomic, so that the order does not matter)
        atomicAdd(reinterpret_cast<unsigned long long *>(w.b_sbytes + blockIdx.x), (unsigned long long)sbytes);
    }
}

__global__ __launch_bounds__(kThreads) void tape_long_len(const uint8_t *__restrict__ buf, uint64_t len, const uint32_t *__restrict__ idx,
                                                          uint64_t n, const uint32_t *__restrict__ end,
                                                          const uint8_t *__restrict__ flags, const Work w) {
    const ByteReader r{buf, len};
    const uint32_t waves = gridDim.x * kWaves, wave = blockIdx.x * kWaves + (threadIdx.x >> 6);
    const uint32_t cnt = min(w.st->long_count, w.long_cap);
    for (uint32_t j = wave; j < cnt; j += waves) {
        const uint32_t tok = w.long_list[j];
        const Body y = body_of(idx, end, flags[tok], tok, len);
        const uint64_t ulen = y.escaped ? wave_unescape(r, BufWriter{nullptr, 0, 0}, y.b, y.q, true) : y.q - y.b;
        if ((threadIdx.x & 63) == 0) {
            w.long_ulen[(y.b - 1) >> 10] = (uint32_t)ulen;
            atomicAdd(reinterpret_cast<unsigned long long *>(w.b_sbytes + tok / kBlock), (unsigned long long)ulen);
        }
    }
}

__global__ __launch_bounds__(1024) void tape_scan(const Work w, uint64_t n, const msj_validate_result *__restrict__ verdict,
                                                  uint64_t *__restrict__ tape, uint64_t tape_capacity, const uint8_t *string_buf,
                                                  uint64_t string_capacity, uint64_t numbers_capacity, msj_tape_result *__restrict__ result) {
    __shared__ uint64_t s_w[4][16];
    uint64_t run[4] = {0, 0, 0, 0};
    scan_blocks(w, s_w, run);
    if (threadIdx.x != 0) return;
    State *st = w.st;
    st->words = run[0], st->nums = run[1], st->nstr = run[2], st->sbytes = run[3];
    msj_tape_result res;
    res.flags = 0;
    if (verdict && verdict->code != 0) {
        st->skip = 1;
        res.code = verdict->code;
        res.tape_words = res.string_bytes = res.n_strings = 0;
        *result = res;
        return;
    }
    res.tape_words = run[0] + 2;  // E + 1, E = 1 + the tokens' words
    res.string_bytes = run[3];
    res.n_strings = run[2];
    const bool fits = res.tape_words <= tape_capacity && (!string_buf || res.string_bytes <= string_capacity) && run[1] <= numbers_capacity;
    res.code = fits ? MSJ_SUCCESS : MSJ_CAPACITY;
    *result = res;
    if (tape_capacity > 0) tape[0] = root_first_word(res.tape_words);
    if (run[0] + 1 < tape_capacity) tape[run[0] + 1] = root_last_word();
}

__global__ __launch_bounds__(kThreads) void tape_pos(uint64_t n, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                     const uint32_t *__restrict__ match, const uint8_t *__restrict__ flags, const Work w) {
    if (w.st->skip) return;
    pos_block(n, 0, n, type, depth, match, flags, w);
}

__global__ __launch_bounds__(kThreads) void tape_min64(const int32_t *__restrict__ in, uint32_t n_in, int32_t *__restrict__ out,
                                                       const State *__restrict__ st) {
    if (st->skip) return;
    min64_body(in, n_in, out);
}

__global__ __launch_bounds__(kThreads) void tape_span(uint64_t n, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                      const Work w) {
    if (w.st->skip) return;
    span_body(n, type, depth, w);
}

// ---- the words -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tape_emit(const uint8_t *__restrict__ buf, uint64_t len, const uint32_t *__restrict__ idx,
                                                      uint64_t n, const uint8_t *__restrict__ type, const uint32_t *__restrict__ match,
                                                      const uint32_t *__restrict__ end, const uint8_t *__restrict__ flags,
                                                      const msj_number *__restrict__ numbers, uint64_t numbers_capacity,
                                                      uint64_t *__restrict__ tape, uint64_t tape_capacity, uint8_t *__restrict__ string_buf,
                                                      uint64_t string_capacity, const Work w) {
    __shared__ uint64_t s_words[2 * kBlock];
    __shared__ uint64_t s_w64[kWaves];
    __shared__ uint32_t s_w32[kWaves];
    if (w.st->skip) return;
    const uint64_t base = (uint64_t)blockIdx.x * kBlock, mine = base + (uint64_t)threadIdx.x * kPer;
    const uint32_t pos0 = 1 + w.b_words[blockIdx.x];
    const uint32_t nwords = (blockIdx.x + 1 < w.nb ? w.b_words[blockIdx.x + 1] : (uint32_t)w.st->words) - (pos0 - 1);
    const ByteReader r{buf, len};
    uint32_t tw = 0, fw = 0, pk[kPer] = {0, 0, 0, 0};
    if (mine < n) {
        tw = load_byte_quad(type, mine, n), fw = load_byte_quad(flags, mine, n);
        if (mine + 4 <= n) {
            const uint4 q = *reinterpret_cast<const uint4 *>(w.pos + mine);
            pk[0] = q.x, pk[1] = q.y, pk[2] = q.z, pk[3] = q.w;
        } else {
            for (int k = 0; k < kPer && mine + k < n; k++) pk[k] = w.pos[mine + k];
        }
    }
    // this lane's numbers and string bytes, then their ranks / offsets in the call
    uint32_t nums = 0;
    uint64_t sb[kPer] = {0, 0, 0, 0}, sbytes = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint64_t i = mine + k;
        if (i >= n) break;
        const uint32_t t = (tw >> (8 * k)) & 0xFFu, fl = (fw >> (8 * k)) & 0xFFu;
        nums += is_number(fl);
        if (is_string(t) && !is_number(fl)) {
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
    uint64_t soff = w.b_sbytes[blockIdx.x] + block_scan(sbytes, s_w64, tot64);
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint64_t i = mine + k;
        if (i >= n) break;
        const uint32_t t = (tw >> (8 * k)) & 0xFFu, fl = (fw >> (8 * k)) & 0xFFu;
        const uint32_t slot = pk[k] - pos0;  // < 2 * kBlock: pos[] is this call's own prefix sum
        if (is_number(fl)) {
            uint64_t bits = 0;
            uint32_t kind = kNumberInt64;
            if (rank < numbers_capacity) {
                const msj_number rec = numbers[rank];
                if (rec.kind == kNumberInt64 || rec.kind == kNumberDouble) bits = rec.bits, kind = rec.kind;
            }
            rank++;
            s_words[slot] = number_tag_word(kind);
            s_words[slot + 1] = bits;  // deviation 2: a double is its bit pattern
        } else if (is_open(t) || is_close(t)) {
            const uint32_t m = match[i];
            const bool usable = m != kNoPartner && (uint64_t)m < n;  // no index from d_match is used unchecked
            const uint64_t pm = usable ? w.pos[m] : 0;
            if (is_open(t))
                s_words[slot] = open_word(t, elements(m == i + 1, w.cnt[i]), pm);
            else
                s_words[slot] = close_word(t, pm);
        } else if (is_string(t)) {
            s_words[slot] = string_word(soff);
            const Body y = body_of(idx, end, fl, i, len);
            if (y.is_long) {
                w.long_soff[(y.b - 1) >> 10] = soff;
            } else if (string_buf) {
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
            s_words[slot] = atom_word(t);
        }
    }
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < nwords; x += kThreads) {
        const uint64_t a = (uint64_t)pos0 + x;
        if (a < tape_capacity) tape[a] = s_words[x];
    }
}

__global__ __launch_bounds__(kThreads) void tape_long_out(const uint8_t *__restrict__ buf, uint64_t len, const uint32_t *__restrict__ idx,
                                                          const uint32_t *__restrict__ end, const uint8_t *__restrict__ flags,
                                                          uint8_t *__restrict__ string_buf, uint64_t string_capacity, const Work w) {
    if (w.st->skip || !string_buf) return;
    long_out_body(buf, len, idx, end, flags, string_buf, string_capacity, w);
}

}  // namespace msj_tape

extern "C" uint64_t msj_tape_workspace_bytes(uint64_t n, uint64_t len) {
    return msj_measure(msj_tape::layout, n, len, 0) + 64;
}

extern "C" int msj_launch_tape(const msj_token_view &t, const msj_number_view &nv, const msj_validate_result *d_verdict, uint64_t *d_tape,
                               uint64_t tape_capacity, uint8_t *d_string_buf, uint64_t string_capacity, msj_tape_result *d_result,
                               void *d_ws, void *stream) {
    using namespace msj_tape;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Work w = msj_place(layout, d_ws, t.n, t.len, 0);
    const uint32_t nb = w.nb, nb64 = (nb + 63) / 64, nb4096 = (nb64 + 63) / 64;
    if (hipMemsetAsync(w.st, 0, (size_t)(reinterpret_cast<uint8_t *>(w.pos) - reinterpret_cast<uint8_t *>(w.st)), s) != hipSuccess)
        return (int)hipGetLastError();
    hipLaunchKernelGGL(tape_sums, dim3(nb), dim3(kThreads), 0, s, t.d_buf, t.len, t.d_idx, t.n, t.d_type, t.d_end, t.d_flags, w);
    hipLaunchKernelGGL(tape_long_len, dim3(kListBlocks), dim3(kThreads), 0, s, t.d_buf, t.len, t.d_idx, t.n, t.d_end, t.d_flags, w);
    hipLaunchKernelGGL(tape_scan, dim3(1), dim3(1024), 0, s, w, t.n, d_verdict, d_tape, tape_capacity, d_string_buf, string_capacity,
                       nv.numbers_capacity, d_result);
    hipLaunchKernelGGL(tape_pos, dim3(nb), dim3(kThreads), 0, s, t.n, t.d_type, t.d_depth, t.d_match, t.d_flags, w);
    hipLaunchKernelGGL(tape_min64, dim3((nb64 + kWaves - 1) / kWaves), dim3(kThreads), 0, s, w.b_min, nb, w.b_min64, w.st);
    hipLaunchKernelGGL(tape_min64, dim3((nb4096 + kWaves - 1) / kWaves), dim3(kThreads), 0, s, w.b_min64, nb64, w.b_min4096, w.st);
    hipLaunchKernelGGL(tape_span, dim3((nb + kWaves - 1) / kWaves), dim3(kThreads), 0, s, t.n, t.d_type, t.d_depth, w);
    hipLaunchKernelGGL(tape_emit, dim3(nb), dim3(kThreads), 0, s, t.d_buf, t.len, t.d_idx, t.n, t.d_type, t.d_match, t.d_end, t.d_flags, nv.d_numbers,
                       nv.numbers_capacity, d_tape, tape_capacity, d_string_buf, string_capacity, w);
    hipLaunchKernelGGL(tape_long_out, dim3(kListBlocks), dim3(kThreads), 0, s, t.d_buf, t.len, t.d_idx, t.d_end, t.d_flags, d_string_buf,
                       string_capacity, w);
    return (int)hipGetLastError();
}
