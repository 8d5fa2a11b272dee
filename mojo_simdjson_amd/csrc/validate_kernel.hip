// Stage 2's verdict for one document -- msj_validate_device (include/msj_stage1.h): the code and the token at which the
// reference's walk_document (generic/stage2/json_iterator.mojo:40-254) with TapeBuilder's visitors would stop, without the
// walk.  The per-token rule, the atom check and the escape walk are validate_math.h, host + device, checked on the CPU by
// tests/test_validate_math.py.
//
// Launches, all on the caller's stream, no host round trip:
//   val_init    one lane: clears the call's state (error word, list counters, comma counts)
//   val_tokens  the hot path.  Per block of kBlock tokens (token n, the end of the stream, included): type bytes and
//               partners of the block and of the 4 tokens in front of it into LDS (one 4-byte / one 16-byte load per
//               lane), then one lane per 4 tokens: the rule from LDS, depth / index / end / flags loaded only by the
//               tokens that need them (opening brackets; atoms and escaped strings), the partner's neighbour and the atom
//               / string bytes as gathers.  The error is a packed (token, rank, code) word: minimum per wave, per block,
//               then one atomic per block that found one.  Escaped bodies over kLaneBody bytes go to the long list
//               (bounded by len / kLaneBody: never full), over kWaveBody to the huge list; closing brackets of containers
//               wide enough to overflow the element count to the big list (MSJ_VALIDATE_BIG_CONTAINERS entries).
//   val_strings one wave per long body, then the whole grid over every huge body, a contiguous piece per wave: 64 bytes
//               per step, the escape starts from the ballot of the step's backslashes and one carried parity bit
//               (validate_math.h: escape_start_mask), every escape judged on its own (escape_bad<true>), so the body
//               splits anywhere and the cost is linear in its length whatever it holds
//   val_count   only when the big list holds 1 .. MSJ_VALIDATE_BIG_CONTAINERS containers: their direct commas
//   val_finish  one workgroup: the blocks' counts of escaped strings summed, then one lane lets the number call's first
//               error and the counts compete and writes d_result
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "launch.h"
#include "validate_block.h"

namespace msj_val {

__global__ void val_init(State *__restrict__ st) {
    st->err = kNoError;
    st->reserved64 = 0;
    st->big_count = st->long_count = st->huge_count = st->reserved = 0;
    for (uint32_t k = 0; k < kBig; k++) st->big_open[k] = st->big_close[k] = st->big_commas[k] = 0;
}

__global__ __launch_bounds__(kThreads) void val_tokens(const uint8_t *__restrict__ buf, uint64_t len, const uint32_t *__restrict__ idx,
                                                       uint64_t n64, const uint8_t *__restrict__ type,
                                                       const int32_t *__restrict__ depth, const uint32_t *__restrict__ match,
                                                       const uint32_t *__restrict__ end, const uint8_t *__restrict__ flags,
                                                       uint32_t max_depth, State *__restrict__ st, uint32_t *__restrict__ long_list,
                                                       uint32_t long_cap, uint32_t *__restrict__ huge_list, uint32_t huge_cap,
                                                       uint32_t *__restrict__ block_esc) {
    __shared__ uint32_t s_type[(kBlock + kHalo + 4) / 4];
    __shared__ uint32_t s_match[kBlock + kHalo];
    __shared__ unsigned long long w_err[kThreads / 64];
    __shared__ uint32_t w_esc[kThreads / 64];
    const int64_t n = (int64_t)n64, base = (int64_t)blockIdx.x * kBlock;
    const int64_t mine = base + (int64_t)threadIdx.x * kPer;
    s_type[threadIdx.x + 1] = load_type_word(type, mine, n);
    {
        const uint4 m = load_match_quad(match, mine, n);
        uint32_t *d = s_match + kHalo + threadIdx.x * kPer;
        d[0] = m.x, d[1] = m.y, d[2] = m.z, d[3] = m.w;
    }
    if (threadIdx.x == 0) {
        s_type[0] = load_type_word(type, base - kHalo, n);
        const uint4 m = load_match_quad(match, base - kHalo, n);
        s_match[0] = m.x, s_match[1] = m.y, s_match[2] = m.z, s_match[3] = m.w;
    }
    if (threadIdx.x == 64) s_type[kThreads + 1] = load_type_word(type, base + kBlock, n);
    __syncthreads();

    const BlockTokens a{reinterpret_cast<const uint8_t *>(s_type), s_match, base, n, type, match, depth};
    const ByteReader r{buf, len};
    unsigned long long best = kNoError;
    uint32_t escaped = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int64_t i = mine + k;
        if (i > n) break;
        uint32_t role;
        const uint32_t code = token_rule(a, i, n, max_depth, role);
        unsigned long long e = kNoError;
        if (code) {
            e = pack_error((uint64_t)i, 0, code);
        } else if (role == kRoleScalar) {
            const uint32_t t = a.type(i);
            if (t == '"') {
                if (flags[i] & MSJ_SPAN_ESCAPED) {
                    escaped++;
                    const uint64_t b = (uint64_t)idx[i] + 1, q = end[i];
                    if (q > len || q < b) {
                        e = pack_error((uint64_t)i, 1, kString);  // not what the span call writes: never read
                    } else if (q - b <= kLaneBody) {
                        if (string_bad_serial(r, b, q)) e = pack_error((uint64_t)i, 1, kString);
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
                if (c) e = pack_error((uint64_t)i, 1, c);
            }
        }
        best = e < best ? e : best;
        // a container wide enough for more than kMaxElements elements: its commas are counted behind this pass
        if (i < n && is_close(a.type(i))) {
            const uint32_t m = a.match(i);
            if (m != kNoPartner && (int64_t)m < i && (uint64_t)(i - (int64_t)m - 1) >= kBigSpan) {
                const uint32_t s = atomicAdd(&st->big_count, 1u);
                if (s < kBig) st->big_open[s] = m, st->big_close[s] = (uint32_t)i;
            }
        }
    }
    best = wave_min(best);
    escaped = wave_sum(escaped);
    if ((threadIdx.x & 63) == 0) w_err[threadIdx.x >> 6] = best, w_esc[threadIdx.x >> 6] = escaped;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b = w_err[0];
        uint32_t c = w_esc[0];
        for (int w = 1; w < kThreads / 64; w++) {
            b = w_err[w] < b ? w_err[w] : b;
            c += w_esc[w];
        }
        if (b != kNoError) atomicMin(&st->err, b);
        block_esc[blockIdx.x] = c;  // a plain store per block: an atomic per block on one word serialises the whole grid
    }
}

// bytes [lo, hi) of the body [b, e) of string token `tok`, by one wave (validate_block.h: wave_body_bad)
__device__ __forceinline__ void wave_body(const ByteReader &r, uint64_t b, uint64_t e, uint64_t lo, uint64_t hi, uint32_t tok,
                                          State *__restrict__ st) {
    if (wave_body_bad(r, b, e, lo, hi) && (threadIdx.x & 63) == 0) atomicMin(&st->err, (unsigned long long)pack_error(tok, 1, kString));
}

__global__ __launch_bounds__(kThreads) void val_strings(const uint8_t *__restrict__ buf, uint64_t len, const uint32_t *__restrict__ idx,
                                                        const uint32_t *__restrict__ end, State *__restrict__ st,
                                                        const uint32_t *__restrict__ long_list, uint32_t long_cap,
                                                        const uint32_t *__restrict__ huge_list, uint32_t huge_cap) {
    const ByteReader r{buf, len};
    const uint32_t waves = gridDim.x * (kThreads / 64), wave = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const uint32_t n_long = min(st->long_count, long_cap), n_huge = min(st->huge_count, huge_cap);
    for (uint32_t j = wave; j < n_long; j += waves) {
        const uint32_t tok = long_list[j];
        const uint64_t b = (uint64_t)idx[tok] + 1, e = end[tok];
        wave_body(r, b, e, b, e, tok, st);
    }
    // a huge body: one contiguous piece per wave (at least kChunk bytes), so that the run in front of a piece is looked
    // at once per wave and the whole stays linear in the body
    for (uint32_t j = 0; j < n_huge; j++) {
        const uint32_t tok = huge_list[j];
        const uint64_t b = (uint64_t)idx[tok] + 1, e = end[tok];
        uint64_t piece = ((e - b + waves - 1) / waves + 63) & ~63ull;
        piece = piece < kChunk ? kChunk : piece;
        const uint64_t lo = b + (uint64_t)wave * piece;
        if (lo < e) wave_body(r, b, e, lo, lo + piece < e ? lo + piece : e, tok, st);
    }
}

// direct commas of the listed containers; nothing is read when the main pass listed none (or too many)
__global__ __launch_bounds__(kThreads) void val_count(const uint8_t *__restrict__ type, const int32_t *__restrict__ depth, uint64_t n,
                                                      State *__restrict__ st) {
    count_listed_commas(type, depth, n, st);
}

__global__ __launch_bounds__(kThreads) void val_finish(const State *__restrict__ st, const uint32_t *__restrict__ idx, uint64_t n,
                                                       uint64_t len, const msj_numbers_result *__restrict__ numbers,
                                                       const uint32_t *__restrict__ block_esc, uint32_t nb,
                                                       msj_validate_result *__restrict__ result) {
    __shared__ unsigned long long w_esc[kThreads / 64];
    unsigned long long esc = 0;
    for (uint32_t b = threadIdx.x; b < nb; b += kThreads) esc += block_esc[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) esc += __shfl_xor(esc, o);
    if ((threadIdx.x & 63) == 0) w_esc[threadIdx.x >> 6] = esc;
    __syncthreads();
    if (threadIdx.x != 0) return;
    esc = 0;
    for (int w = 0; w < kThreads / 64; w++) esc += w_esc[w];
    uint64_t best = st->err;
    uint32_t fl = numbers ? 0u : MSJ_VALIDATE_NUMBERS_UNCHECKED;
    if (numbers && numbers->first_error < n) {
        const uint64_t e = pack_error(numbers->first_error, 1, kNumber);
        best = e < best ? e : best;
    }
    const uint32_t cnt = st->big_count;
    if (cnt > kBig) {
        fl |= MSJ_VALIDATE_COUNTS_CLIPPED;  // all or nothing: which 64 made it into the list depends on the order of the blocks
    } else {
        for (uint32_t c = 0; c < cnt; c++) {
            if (1ull + st->big_commas[c] > kMaxElements) {
                const uint64_t e = pack_error(st->big_close[c], 1, kCapacity);
                best = e < best ? e : best;
            }
        }
    }
    msj_validate_result res;
    res.flags = fl;
    res.n_escaped = esc;
    if (best == kNoError) {
        res.code = 0;
        res.error_token = res.error_offset = ~0ull;
    } else {
        res.code = (int32_t)packed_code(best);
        res.error_token = packed_token(best);
        res.error_offset = res.error_token >= n ? len : idx[res.error_token];
    }
    *result = res;
}

}  // namespace msj_val

extern "C" uint64_t msj_validate_workspace_bytes(uint64_t n, uint64_t len) { return msj_measure(msj_val::layout, n, len) + 64; }

extern "C" int msj_launch_validate(const msj_token_view &t, const msj_number_view &nv, uint32_t max_depth, msj_validate_result *d_result,
                                   void *d_ws, void *stream) {
    using namespace msj_val;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Work w = msj_place(layout, d_ws, t.n, t.len);
    hipLaunchKernelGGL(val_init, dim3(1), dim3(1), 0, s, w.st);
    hipLaunchKernelGGL(val_tokens, dim3(w.nb), dim3(kThreads), 0, s, t.d_buf, t.len, t.d_idx, t.n, t.d_type, t.d_depth, t.d_match, t.d_end, t.d_flags,
                       max_depth, w.st, w.long_list, w.long_cap, w.huge_list, w.huge_cap, w.block_esc);
    hipLaunchKernelGGL(val_strings, dim3(kListBlocks), dim3(kThreads), 0, s, t.d_buf, t.len, t.d_idx, t.d_end, w.st, w.long_list, w.long_cap, w.huge_list,
                       w.huge_cap);
    hipLaunchKernelGGL(val_count, dim3(kListBlocks * 4), dim3(kThreads), 0, s, t.d_type, t.d_depth, t.n, w.st);
    hipLaunchKernelGGL(val_finish, dim3(1), dim3(kThreads), 0, s, w.st, t.d_idx, t.n, t.len, nv.d_numbers_result, w.block_esc, w.nb, d_result);
    return (int)hipGetLastError();
}
