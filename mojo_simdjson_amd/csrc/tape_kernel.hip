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
// d_end is checked before it is used, every store is checked against its capacity.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "launch.h"
#include "tape_math.h"
#include "wave_ops.h"

namespace msj_tape {

using namespace msj::tape;
using namespace msj::wave;
using msj::val::ByteReader;

constexpr int kThreads = 256;
constexpr int kPer = 4;                        // tokens per lane
constexpr uint32_t kBlock = kThreads * kPer;   // tokens per workgroup
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kLaneBody = 1024;           // bodies up to this many bytes are measured and written by their lane
constexpr int kListBlocks = 512;               // grid of the list kernels (they loop over what the list holds)
constexpr int32_t kFar = 0x7FFFFFFF;

struct State {
    uint64_t words, nums, nstr, sbytes;  // totals
    uint32_t long_count, skip;           // skip: d_verdict's code is not 0, nothing but d_result is written
    uint32_t reserved[6];
};

struct Work {  // the workspace, carved by layout()
    State *st;
    uint32_t *cnt, *pos;                 // per token: direct commas of an opening bracket; tape position
    uint32_t *b_words, *b_nums, *b_nstr; // per block, sums and then exclusive prefixes
    uint64_t *b_sbytes;
    int32_t *b_min, *b_min64, *b_min4096;
    uint32_t *b_span;                    // commas of the block whose container spans the whole block
    uint32_t *long_list, *long_ulen;
    uint64_t *long_soff;
    uint32_t long_cap, nb;
    uint64_t bytes;                      // of the whole workspace
};

__host__ __device__ inline uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__host__ __device__ inline uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

// exclusive sum over the workgroup (s_w: kWaves words of LDS, free again after the call); total receives the sum
template <class T>
__device__ __forceinline__ T block_scan(T v, T *s_w, T &total) {
    const T inc = wave_scan(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = inc;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
        const T x = s_w[w];
        if (w < (int)(threadIdx.x >> 6)) before += x;
        all += x;
    }
    total = all;
    return before + inc - v;
}

// the unescaped length of string token's body [b, q), or ~0 for a body that belongs on the long list
struct Body {
    uint64_t b, q;
    bool ok, is_long, escaped;
};
__device__ __forceinline__ Body body_of(const uint32_t *__restrict__ idx, const uint32_t *__restrict__ end, uint32_t fl, uint64_t i,
                                        uint64_t len) {
    Body y;
    y.b = (uint64_t)idx[i] + 1, y.q = end[i];
    y.ok = y.q <= len && y.q >= y.b;  // (what the span call writes for a closed string; anything else is never read)
    y.is_long = y.ok && y.q - y.b > kLaneBody;
    y.escaped = (fl & kSpanEscaped) != 0;
    return y;
}

struct BufWriter {  // byte o of a string's record (its length prefix included): checked against the capacity
    uint8_t *out;
    uint64_t base, cap;
    __device__ __forceinline__ void put(uint64_t o, uint32_t byte) const {
        const uint64_t a = base + o;
        if (out && a < cap) out[a] = (uint8_t)byte;
    }
};

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

// One long body by one wave, 64 bytes per step (tape_math.h: unescape_step is the host's form of this loop).  wr.out ==
// NULL measures.  Returns the unescaped length (in every lane).
__device__ __forceinline__ uint64_t wave_unescape(const ByteReader &r, const BufWriter &wr, uint64_t b, uint64_t e, bool measure) {
    const uint32_t lane = threadIdx.x & 63;
    StepState st = step_begin();
    for (uint64_t p0 = b; p0 < e; p0 += 64) {
        const uint64_t p = p0 + lane;
        const uint32_t c = p < e ? r.at(p) : 0u;
        const uint64_t bs = __ballot(p < e && c == '\\');
        uint64_t carry = st.carry;
        const uint64_t starts = escape_start_mask(bs, carry);
        const bool is_start = (starts >> lane) & 1u;
        LaneOut lo{0, 0};
        if (p < e) {
            lo.out = 1;
            if (is_start) lo = step_lane(r, NoWrite{}, b, e, p0, lane, 64, starts, st, 0, true);
        }
        // the bytes the step's escapes cover: every escape covers the byte behind it, a \u escape four more
        const uint64_t six = __ballot(is_start && lo.len == 6);
        uint64_t cover_lo = st.cover | (starts << 1), cover_hi = starts >> 63;
#pragma unroll
        for (int k = 1; k <= 5; k++) cover_lo |= six << k, cover_hi |= six >> (64 - k);
        if (!is_start && ((cover_lo >> lane) & 1u)) lo.out = 0;
        const uint32_t inc = wave_scan(lo.out);
        const uint64_t o = st.out + inc - lo.out;
        if (!measure && lo.out) {
            if (is_start)
                (void)step_lane(r, wr, b, e, p0, lane, 64, starts, st, o, false);
            else
                wr.put(o, c);
        }
        step_end(st, 64, starts, cover_lo, cover_hi, st.out + (uint32_t)__shfl((int)inc, 63));
    }
    return st.out;
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
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (uint32_t b0 = 0; b0 < w.nb; b0 += 1024) {
        const uint32_t b = b0 + threadIdx.x;
        uint64_t v[4] = {0, 0, 0, 0}, inc[4];
        if (b < w.nb) v[0] = w.b_words[b], v[1] = w.b_nums[b], v[2] = w.b_nstr[b], v[3] = w.b_sbytes[b];
#pragma unroll
        for (int k = 0; k < 4; k++) inc[k] = wave_scan(v[k]);
        __syncthreads();
        if (lane == 63)
            for (int k = 0; k < 4; k++) s_w[k][wv] = inc[k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint64_t before = 0, all = 0;
#pragma unroll 2
            for (uint32_t x = 0; x < 16; x++) {
                const uint64_t y = s_w[k][x];
                if (x < wv) before += y;
                all += y;
            }
            inc[k] += run[k] + before - v[k];
            run[k] += all;
        }
        if (b < w.nb) w.b_words[b] = (uint32_t)inc[0], w.b_nums[b] = (uint32_t)inc[1], w.b_nstr[b] = (uint32_t)inc[2], w.b_sbytes[b] = inc[3];
    }
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

// ---- positions and element counts -----------------------------------------------------------------------------------
// 8-ary min tree over the block's depths in LDS: level 0 = kBlock depths, then 128, 16, 2
struct Tree {
    int32_t d[kBlock + kBlock / 8 + kBlock / 64 + 8];
    __device__ __forceinline__ static int off(int lev) { return lev == 0 ? 0 : lev == 1 ? (int)kBlock : lev == 2 ? (int)(kBlock + kBlock / 8) : (int)(kBlock + kBlock / 8 + kBlock / 64); }
    __device__ __forceinline__ static int size(int lev) { return lev == 0 ? (int)kBlock : lev == 1 ? (int)kBlock / 8 : lev == 2 ? (int)kBlock / 64 : 2; }
    __device__ __forceinline__ int32_t at(int lev, int j) const { return d[off(lev) + j]; }
    __device__ __forceinline__ int32_t &at(int lev, int j) { return d[off(lev) + j]; }
};
// the nearest token in front of k (behind k) with a depth below D, or -1
__device__ __forceinline__ int nearest_left(const Tree &t, int k, int32_t D) {
    int p = k;  // searching [0, p)
    while (p & 7) {
        if (t.at(0, p - 1) < D) return p - 1;
        p--;
    }
    p >>= 3;
    int lev = 1;
    int hit = -1;
    while (lev <= 3) {
        while (p & 7) {
            if (t.at(lev, p - 1) < D) {
                hit = p - 1;
                break;
            }
            p--;
        }
        if (hit >= 0 || p == 0) break;
        p >>= 3;
        lev++;
    }
    if (hit < 0) return -1;
    while (lev > 0) {  // down: the last child below D
        lev--;
        int c = hit * 8 + 7;
        while (t.at(lev, c) >= D) c--;  // (one of the 8 is: the node's minimum)
        hit = c;
    }
    return hit;
}
__device__ __forceinline__ int nearest_right(const Tree &t, int k, int32_t D) {
    int p = k + 1;  // searching [p, kBlock)
    while (p & 7) {
        if (t.at(0, p) < D) return p;
        p++;
    }
    p >>= 3;
    int lev = 1;
    int hit = -1;
    while (lev <= 3) {
        while ((p & 7) && p < Tree::size(lev)) {
            if (t.at(lev, p) < D) {
                hit = p;
                break;
            }
            p++;
        }
        if (hit >= 0 || p >= Tree::size(lev)) break;
        p >>= 3;
        lev++;
    }
    if (hit < 0) return -1;
    while (lev > 0) {
        lev--;
        int c = hit * 8;
        while (t.at(lev, c) >= D) c++;
        hit = c;
    }
    return hit;
}

__global__ __launch_bounds__(kThreads) void tape_pos(uint64_t n, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                     const uint32_t *__restrict__ match, const uint8_t *__restrict__ flags, const Work w) {
    __shared__ Tree t;
    __shared__ uint32_t s_type[kBlock / 4];
    __shared__ uint32_t s_cnt[kBlock];
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint32_t s_span;
    if (w.st->skip) return;
    const uint64_t base = (uint64_t)blockIdx.x * kBlock, mine = base + (uint64_t)threadIdx.x * kPer;
    const int lk = threadIdx.x * kPer;
    uint32_t tw = 0, fw = 0;
    int32_t d[kPer] = {kFar, kFar, kFar, kFar};
    if (mine < n) {
        tw = load_byte_quad(type, mine, n), fw = load_byte_quad(flags, mine, n);
        if (mine + 4 <= n) {
            const int4 q = *reinterpret_cast<const int4 *>(depth + mine);
            d[0] = q.x, d[1] = q.y, d[2] = q.z, d[3] = q.w;
        } else {
            for (int k = 0; k < kPer && mine + k < n; k++) d[k] = depth[mine + k];
        }
    }
    uint32_t wsum = 0, wk[kPer];
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        wk[k] = mine + k < n ? words_per_token((tw >> (8 * k)) & 0xFFu, (fw >> (8 * k)) & 0xFFu) : 0u;
        wsum += wk[k];
        t.at(0, lk + k) = d[k];
        s_cnt[lk + k] = 0;
    }
    s_type[threadIdx.x] = tw;
    if (threadIdx.x == 0) s_span = 0;
    uint32_t total;
    uint32_t p = 1 + w.b_words[blockIdx.x] + block_scan(wsum, s_w, total);  // (has the barriers that publish d0)
    if (mine < n) {
        uint32_t pk[kPer];
#pragma unroll
        for (int k = 0; k < kPer; k++) pk[k] = p, p += wk[k];
        if (mine + 4 <= n) {
            *reinterpret_cast<uint4 *>(w.pos + mine) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        } else {
            for (int k = 0; k < kPer && mine + k < n; k++) w.pos[mine + k] = pk[k];
        }
    }
    // the tree
    if (threadIdx.x < kBlock / 8) {
        int32_t m = kFar;
        for (int k = 0; k < 8; k++) m = min(m, t.at(0, threadIdx.x * 8 + k));
        t.at(1, threadIdx.x) = m;
    }
    __syncthreads();
    if (threadIdx.x < kBlock / 64) {
        int32_t m = kFar;
        for (int k = 0; k < 8; k++) m = min(m, t.at(1, threadIdx.x * 8 + k));
        t.at(2, threadIdx.x) = m;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        int32_t m = kFar;
        if (threadIdx.x < 2)
            for (int k = 0; k < 8; k++) m = min(m, t.at(2, threadIdx.x * 8 + k));
        t.at(3, threadIdx.x) = m;
    }
    __syncthreads();
    const int32_t dmin = min(t.at(3, 0), t.at(3, 1));
    const uint8_t *types = reinterpret_cast<const uint8_t *>(s_type);
    uint32_t span = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        if (((tw >> (8 * k)) & 0xFFu) != ',' || mine + k >= n) continue;
        const int32_t D = d[k];
        if (D == dmin) {  // nothing in the block is shallower: the container spans the block
            span++;
            continue;
        }
        int j = nearest_left(t, lk + k, D);
        if (j < 0) j = nearest_right(t, lk + k, D);
        // the opening bracket (its depth is D - 1), or the closing one of a container that opened in front of the block
        if (j >= 0 && t.at(0, j) == D - 1 && (is_open(types[j]) || is_close(types[j]))) atomicAdd(&s_cnt[j], 1u);
    }
    span = wave_sum(span);
    if ((threadIdx.x & 63) == 0 && span) atomicAdd(&s_span, span);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint32_t c = s_cnt[lk + k];
        if (!c) continue;
        const uint64_t i = mine + k;
        uint64_t target = i;
        if (is_close(types[lk + k])) {
            const uint32_t m = match[i];
            if (m == kNoPartner || (uint64_t)m >= i) continue;  // no index from d_match is used unchecked
            target = m;
        }
        atomicAdd(&w.cnt[target], c);
    }
    if (threadIdx.x == 0) w.b_min[blockIdx.x] = dmin, w.b_span[blockIdx.x] = s_span;
}

__global__ __launch_bounds__(kThreads) void tape_min64(const int32_t *__restrict__ in, uint32_t n_in, int32_t *__restrict__ out,
                                                       const State *__restrict__ st) {
    if (st->skip) return;
    const uint32_t wave = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint32_t j = wave * 64 + lane;
    int32_t m = j < n_in ? in[j] : kFar;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
    if (lane == 0 && wave * 64 < n_in) out[wave] = m;
}

// the last j in [lo, hi) (hi - lo <= 64, lo a multiple of 64) with a[j] < D, by one wave; -1 if none
__device__ __forceinline__ int64_t wave_last_below(const int32_t *__restrict__ a, uint64_t lo, uint64_t hi, int32_t D) {
    const uint64_t j = lo + (threadIdx.x & 63);
    const uint64_t hit = __ballot(j < hi && a[j] < D);
    return hit ? (int64_t)(lo + 63 - __clzll((long long)hit)) : -1;
}

__global__ __launch_bounds__(kThreads) void tape_span(uint64_t n, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                      const Work w) {
    if (w.st->skip) return;
    const uint32_t blk = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (blk >= w.nb || blk == 0) return;
    const uint32_t c = w.b_span[blk];
    if (!c) return;
    const int32_t D = w.b_min[blk];
    // up: the 64 blocks of its group, the 64 groups of its group, then all groups of 4096 in front
    int64_t b = wave_last_below(w.b_min, blk & ~63u, blk, D);
    if (b < 0) {
        const uint32_t g = blk >> 6;
        int64_t g1 = wave_last_below(w.b_min64, g & ~63u, g, D);
        if (g1 < 0) {
            int64_t g2 = -1;
            for (int64_t hi = g >> 6; hi > 0 && g2 < 0; hi = (hi - 1) & ~63ll) g2 = wave_last_below(w.b_min4096, (hi - 1) & ~63ll, hi, D);
            if (g2 < 0) return;  // nothing in front is shallower: no container (not a valid document)
            g1 = wave_last_below(w.b_min64, (uint64_t)g2 * 64, umin64((uint64_t)g2 * 64 + 64, ((uint64_t)w.nb + 63) / 64), D);
            if (g1 < 0) return;
        }
        b = wave_last_below(w.b_min, (uint64_t)g1 * 64, umin64((uint64_t)g1 * 64 + 64, (uint64_t)w.nb), D);
        if (b < 0) return;
    }
    const uint64_t lo = (uint64_t)b * kBlock, hi = umin64(lo + kBlock, n);
    for (uint64_t e = hi; e > lo; e = (e - 1) & ~63ull) {
        const int64_t tkn = wave_last_below(depth, (e - 1) & ~63ull, e, D);
        if (tkn >= 0) {
            if ((threadIdx.x & 63) == 0 && depth[tkn] == D - 1 && is_open(type[tkn])) atomicAdd(&w.cnt[tkn], c);
            return;
        }
    }
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
    const ByteReader r{buf, len};
    const uint32_t waves = gridDim.x * kWaves, wave = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint32_t cnt = min(w.st->long_count, w.long_cap);
    for (uint32_t j = wave; j < cnt; j += waves) {
        const uint32_t tok = w.long_list[j];
        const Body y = body_of(idx, end, flags[tok], tok, len);
        const uint64_t slot = (y.b - 1) >> 10, soff = w.long_soff[slot];
        const uint32_t ulen = w.long_ulen[slot];
        const BufWriter pre{string_buf, soff, string_capacity}, body{string_buf, soff + 4, string_capacity};
        if (lane < 4) pre.put(lane, (ulen >> (8 * lane)) & 0xFFu);
        if (y.escaped) {
            (void)wave_unescape(r, body, y.b, y.q, false);
        } else {
            for (uint64_t x = lane; x < y.q - y.b; x += 64) body.put(x, r.at(y.b + x));
        }
    }
}

static Work layout(void *ws, uint64_t n, uint64_t len) {
    Work w;
    const uint64_t nb = (n + kBlock - 1) / kBlock, lcap = len / kLaneBody + 1;
    uint8_t *p = static_cast<uint8_t *>(ws);
    auto take = [&](uint64_t bytes) {
        uint8_t *q = p;
        p += up16(bytes);
        return q;
    };
    // (the first three are cleared by one memset per call)
    w.st = reinterpret_cast<State *>(take(sizeof(State)));
    w.b_sbytes = reinterpret_cast<uint64_t *>(take(8 * nb));
    w.cnt = reinterpret_cast<uint32_t *>(take(4 * n));
    w.pos = reinterpret_cast<uint32_t *>(take(4 * n));
    w.b_words = reinterpret_cast<uint32_t *>(take(4 * nb));
    w.b_nums = reinterpret_cast<uint32_t *>(take(4 * nb));
    w.b_nstr = reinterpret_cast<uint32_t *>(take(4 * nb));
    w.b_min = reinterpret_cast<int32_t *>(take(4 * nb));
    w.b_min64 = reinterpret_cast<int32_t *>(take(4 * ((nb + 63) / 64)));
    w.b_min4096 = reinterpret_cast<int32_t *>(take(4 * ((nb + 4095) / 4096)));
    w.b_span = reinterpret_cast<uint32_t *>(take(4 * nb));
    w.long_list = reinterpret_cast<uint32_t *>(take(4 * lcap));
    w.long_ulen = reinterpret_cast<uint32_t *>(take(4 * lcap));
    w.long_soff = reinterpret_cast<uint64_t *>(take(8 * lcap));
    w.long_cap = (uint32_t)lcap;
    w.nb = (uint32_t)nb;
    w.bytes = (uint64_t)(p - static_cast<uint8_t *>(ws));
    return w;
}

}  // namespace msj_tape

extern "C" uint64_t msj_tape_workspace_bytes(uint64_t n, uint64_t len) {
    return msj_tape::layout(nullptr, n, len).bytes + 64;
}

extern "C" int msj_launch_tape(const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n, const uint8_t *d_type,
                               const int32_t *d_depth, const uint32_t *d_match, const uint32_t *d_end, const uint8_t *d_flags,
                               const msj_number *d_numbers, uint64_t numbers_capacity, const msj_validate_result *d_verdict,
                               uint64_t *d_tape, uint64_t tape_capacity, uint8_t *d_string_buf, uint64_t string_capacity,
                               msj_tape_result *d_result, void *d_ws, void *stream) {
    using namespace msj_tape;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Work w = layout(d_ws, n, len);
    const uint32_t nb = w.nb, nb64 = (nb + 63) / 64, nb4096 = (nb64 + 63) / 64;
    if (hipMemsetAsync(w.st, 0, (size_t)(reinterpret_cast<uint8_t *>(w.pos) - reinterpret_cast<uint8_t *>(w.st)), s) != hipSuccess)
        return (int)hipGetLastError();
    hipLaunchKernelGGL(tape_sums, dim3(nb), dim3(kThreads), 0, s, d_buf, len, d_idx, n, d_type, d_end, d_flags, w);
    hipLaunchKernelGGL(tape_long_len, dim3(kListBlocks), dim3(kThreads), 0, s, d_buf, len, d_idx, n, d_end, d_flags, w);
    hipLaunchKernelGGL(tape_scan, dim3(1), dim3(1024), 0, s, w, n, d_verdict, d_tape, tape_capacity, d_string_buf, string_capacity,
                       numbers_capacity, d_result);
    hipLaunchKernelGGL(tape_pos, dim3(nb), dim3(kThreads), 0, s, n, d_type, d_depth, d_match, d_flags, w);
    hipLaunchKernelGGL(tape_min64, dim3((nb64 + kWaves - 1) / kWaves), dim3(kThreads), 0, s, w.b_min, nb, w.b_min64, w.st);
    hipLaunchKernelGGL(tape_min64, dim3((nb4096 + kWaves - 1) / kWaves), dim3(kThreads), 0, s, w.b_min64, nb64, w.b_min4096, w.st);
    hipLaunchKernelGGL(tape_span, dim3((nb + kWaves - 1) / kWaves), dim3(kThreads), 0, s, n, d_type, d_depth, w);
    hipLaunchKernelGGL(tape_emit, dim3(nb), dim3(kThreads), 0, s, d_buf, len, d_idx, n, d_type, d_match, d_end, d_flags, d_numbers,
                       numbers_capacity, d_tape, tape_capacity, d_string_buf, string_capacity, w);
    hipLaunchKernelGGL(tape_long_out, dim3(kListBlocks), dim3(kThreads), 0, s, d_buf, len, d_idx, d_end, d_flags, d_string_buf,
                       string_capacity, w);
    return (int)hipGetLastError();
}
