// tape_block.h -- the device pieces that tape_kernel.hip (one document) and tape_docs_kernel.hip (every document of a
// window) share: the geometry of the token passes, the call's state and workspace, the exclusive sum over a workgroup and
// over the blocks, a string token's body (the checked writer and the wave's walk over a long body are wave_unescape.h, which
// string_column_kernel.hip shares), the 8-ary min tree of a
// block's depths with its two searches, and the bodies of the kernels that are the same in both calls (positions and
// element counts, the block minima, the pending counts, the long bodies' bytes).  Device code but for the workspace's
// layout, which is also its size (launch.h: msj_carver); the per-token arithmetic is tape_math.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "launch.h"
#include "tape_math.h"
#include "wave_ops.h"
#include "wave_unescape.h"

namespace msj_tape {

using namespace msj::tape;
using namespace msj::wave;
using msj::val::ByteReader;

constexpr int kThreads = 256;
constexpr int kPer = 4;                        // tokens per lane
constexpr uint32_t kBlock = kThreads * kPer;   // tokens per workgroup
constexpr int kWaves = kThreads / 64;
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
    uint64_t *doc_sbase;                 // the window call: per document, the string bytes in front of its first token
    uint32_t *b_built;                   // ... and per block, the records written with code 0
    uint32_t long_cap, nb;
    uint64_t bytes;                      // of the whole workspace
};

__host__ __device__ inline uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }

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

// exclusive sums over the blocks by ONE workgroup of 1 024 lanes: b_words / b_nums / b_nstr / b_sbytes become prefixes, run[]
// receives the totals (words, number tokens, strings, string bytes) in every lane
__device__ __forceinline__ void scan_blocks(const Work &w, uint64_t (&s_w)[4][16], uint64_t (&run)[4]) {
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

// pos[] and the element counts of one block (the comment at the head of tape_kernel.hip: tape_pos).  Tokens outside [lo, hi)
// are nothing: no words, no depth, no comma (the window call: in front of the first document, and the cut one)
__device__ __forceinline__ void pos_block(uint64_t n, uint64_t lo, uint64_t hi, const uint8_t *__restrict__ type,
                                          const int32_t *__restrict__ depth, const uint32_t *__restrict__ match,
                                          const uint8_t *__restrict__ flags, const Work &w) {
    __shared__ Tree t;
    __shared__ uint32_t s_type[kBlock / 4];
    __shared__ uint32_t s_cnt[kBlock];
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint32_t s_span;
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
        if (mine < lo || mine + 4 > hi) {  // (never in the one-document call)
#pragma unroll
            for (int k = 0; k < kPer; k++)
                if (mine + k < lo || mine + k >= hi) tw &= ~(0xFFu << (8 * k)), fw &= ~(0xFFu << (8 * k)), d[k] = kFar;
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

// minima over groups of 64 entries, a wave per group
__device__ __forceinline__ void min64_body(const int32_t *__restrict__ in, uint32_t n_in, int32_t *__restrict__ out) {
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

// the pending count of a block goes to the nearest token in front of the block with a smaller depth, a wave per block
__device__ __forceinline__ void span_body(uint64_t n, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth, const Work &w) {
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

// the records of the long bodies, a wave per body: length prefix and bytes, 64 bytes per step
__device__ __forceinline__ void long_out_body(const uint8_t *__restrict__ buf, uint64_t len, const uint32_t *__restrict__ idx,
                                              const uint32_t *__restrict__ end, const uint8_t *__restrict__ flags,
                                              uint8_t *__restrict__ string_buf, uint64_t string_capacity, const Work &w) {
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

// n_docs: the window call's documents at most (0: the one-document call)
static inline Work layout(msj_carver &c, uint64_t n, uint64_t len, uint64_t n_docs) {
    Work w;
    const uint64_t nb = (n + kBlock - 1) / kBlock, lcap = len / kLaneBody + 1;
    // (the first three are cleared by one memset per call)
    w.st = c.take<State>(1);
    w.b_sbytes = c.take<uint64_t>(nb);
    w.cnt = c.take<uint32_t>(n);
    w.pos = c.take<uint32_t>(n);
    w.b_words = c.take<uint32_t>(nb);
    w.b_nums = c.take<uint32_t>(nb);
    w.b_nstr = c.take<uint32_t>(nb);
    w.b_min = c.take<int32_t>(nb);
    w.b_min64 = c.take<int32_t>((nb + 63) / 64);
    w.b_min4096 = c.take<int32_t>((nb + 4095) / 4096);
    w.b_span = c.take<uint32_t>(nb);
    w.long_list = c.take<uint32_t>(lcap);
    w.long_ulen = c.take<uint32_t>(lcap);
    w.long_soff = c.take<uint64_t>(lcap);
    w.doc_sbase = c.take<uint64_t>(n_docs);
    w.b_built = c.take<uint32_t>(n_docs ? nb : 0);
    w.long_cap = (uint32_t)lcap;
    w.nb = (uint32_t)nb;
    w.bytes = c.bytes;
    return w;
}

}  // namespace msj_tape
