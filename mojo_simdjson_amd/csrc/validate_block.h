// validate_block.h -- the device pieces that validate_kernel.hip (one document) and validate_docs_kernel.hip (every
// document of a window) share: the geometry of the token pass, the block's neighbourhood in LDS as the rule's accessor,
// the wave's walk over a long escaped body, and the calls' state and workspace.  Device code but for the workspace's layout;
// the rule itself is validate_math.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "launch.h"
#include "validate_math.h"
#include "wave_ops.h"

namespace msj_val {

using namespace msj::val;
using namespace msj::wave;

constexpr int kThreads = 256;
constexpr int kPer = 4;                        // tokens per lane
constexpr uint32_t kBlock = kThreads * kPer;   // tokens per workgroup
constexpr int kHalo = 4;                       // tokens in front of the block kept in LDS (the rule looks back 3)
constexpr uint32_t kLaneBody = 1024;           // escaped bodies up to this many bytes are walked by their lane
constexpr uint32_t kWaveBody = 1u << 20;       // ... up to this many by a wave, longer ones by the grid
constexpr uint32_t kChunk = 4096;              // bytes of a huge body a wave takes at least
constexpr int kListBlocks = 512;               // grid of the list kernels (they loop over what the lists hold)
constexpr uint32_t kBig = MSJ_VALIDATE_BIG_CONTAINERS;

// the token arrays as the rule sees them: the block's neighbourhood from LDS, anything else (the partner's neighbour,
// the document's last token) from memory; outside [0, n) a token that matches nothing
struct BlockTokens {
    const uint8_t *s_type;    // tokens base - kHalo .. base + kBlock + 3
    const uint32_t *s_match;  // tokens base - kHalo .. base + kBlock - 1
    int64_t base, n;
    const uint8_t *g_type;
    const uint32_t *g_match;
    const int32_t *g_depth;
    __device__ __forceinline__ uint32_t type(int64_t j) const {
        const int64_t o = j - base + kHalo;
        if ((uint64_t)o < (uint64_t)(kBlock + kHalo + 4)) return s_type[o];
        return (uint64_t)j < (uint64_t)n ? g_type[j] : 0u;
    }
    __device__ __forceinline__ uint32_t match(int64_t j) const {
        const int64_t o = j - base + kHalo;
        if ((uint64_t)o < (uint64_t)(kBlock + kHalo)) return s_match[o];
        return (uint64_t)j < (uint64_t)n ? g_match[j] : kNoPartner;
    }
    __device__ __forceinline__ int32_t depth(int64_t j) const { return g_depth[j]; }  // asked for tokens in [0, n) only
};

__device__ __forceinline__ uint32_t load_type_word(const uint8_t *__restrict__ type, int64_t j, int64_t n) {  // j % 4 == 0
    if (j < 0 || j >= n) return 0;  // (signed and guarded: not wave_ops.h's load_byte_quad, which compiles to other compares here)
    if (j + 4 <= n) return *reinterpret_cast<const uint32_t *>(type + j);
    uint32_t w = 0;
    for (int k = 0; k < 4 && j + k < n; k++) w |= (uint32_t)type[j + k] << (8 * k);
    return w;
}
__device__ __forceinline__ uint4 load_match_quad(const uint32_t *__restrict__ match, int64_t j, int64_t n) {  // j % 4 == 0
    if (j >= 0 && j + 4 <= n) return *reinterpret_cast<const uint4 *>(match + j);
    uint32_t v[4];
    for (int k = 0; k < 4; k++) v[k] = (j + k >= 0 && j + k < n) ? match[j + k] : kNoPartner;
    return make_uint4(v[0], v[1], v[2], v[3]);
}

// Parity of the run of backslashes that ends directly in front of s, by one wave: 8 bytes per lane and step, so a body
// that is one run of backslashes costs a wave (s - b) / 512 steps, once.  (Whole steps of backslashes hold an even
// number of them; the parity is that of the lane in which the run begins.)
__device__ __forceinline__ uint64_t wave_run_parity_before(const ByteReader &r, uint64_t b, uint64_t s) {
    const uint32_t lane = threadIdx.x & 63;
    while (s > b) {
        // this lane's bytes: [s - 512 + 8 * lane, + 8); in front of b nothing is a backslash
        uint32_t trailing = 0;  // backslashes at the end of this lane's 8 bytes
        bool all = true;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint64_t off = 512u - 8u * lane - (uint32_t)k;  // distance in front of s: 512 .. 1
            const bool is = off <= s - b && r.at(s - off) == '\\';
            // (k runs from the first byte of the group to its last: a non-backslash resets the count)
            trailing = is ? trailing + 1 : 0;
            all = all && is;
        }
        const uint64_t broken = __ballot(!all);
        if (broken) {
            const int top = 63 - __clzll((long long)broken);  // the last lane that holds a byte that is no backslash
            return (uint64_t)__shfl((int)trailing, top) & 1u;  // the lanes behind it hold 8 backslashes each
        }
        s -= 512;  // (never below b: a lane in front of b is not `all`)
    }
    return 0;
}

// bytes [lo, hi) of the string body [b, e), by one wave: 64 bytes per step, the escape starts of a step from the ballot
// of its backslashes (validate_math.h: escape_start_mask), one parity bit carried from step to step.  True (in every
// lane) if an escape that starts in [lo, hi) is in error.
__device__ __forceinline__ bool wave_body_bad(const ByteReader &r, uint64_t b, uint64_t e, uint64_t lo, uint64_t hi) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t s = scan_begin(b, lo);
    ScanState sc{s == b ? 0ull : wave_run_parity_before(r, b, s), 0};
    bool bad = false;
    for (uint64_t p0 = s; p0 < hi; p0 += 64) {
        const uint64_t p = p0 + lane;
        const uint64_t bs = __ballot(p < hi && r.at(p) == '\\');
        const uint64_t starts = escape_start_mask(bs, sc.carry);
        bad |= step_lane_bad(r, b, e, lo, p0, lane, starts, sc.prev_starts);
        sc.prev_starts = starts;
    }
    return __ballot(bad) != 0;
}

// a call's state in its workspace: the minimum packed error (the one-document call; the window call keeps a word per
// document in d_verdicts instead), the fill of the three lists, the wide containers and their direct commas
struct State {
    unsigned long long err;        // minimum packed error
    unsigned long long reserved64;
    uint32_t big_count, long_count, huge_count, reserved;
    uint32_t big_open[kBig], big_close[kBig], big_commas[kBig];
};

// direct commas of the listed containers, by the whole grid; nothing is read when the main pass listed none (or too many)
__device__ __forceinline__ void count_listed_commas(const uint8_t *__restrict__ type, const int32_t *__restrict__ depth, uint64_t n,
                                                    State *__restrict__ st) {
    const uint32_t cnt = st->big_count;
    if (cnt == 0 || cnt > kBig) return;
    const uint64_t lanes = (uint64_t)gridDim.x * kThreads, lane = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    for (uint32_t c = 0; c < cnt; c++) {
        const uint64_t open = st->big_open[c], close = st->big_close[c];
        const int32_t d = depth[open] + 1;
        uint32_t commas = 0;
        // aligned groups of 4 type bytes; the partial groups at both ends are masked by the bounds
        for (uint64_t g = (open & ~3ull) + 4 * lane; g < close; g += 4 * lanes) {
            const uint32_t w = load_type_word(type, (int64_t)g, (int64_t)n);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint64_t j = g + k;
                if (((w >> (8 * k)) & 0xFFu) == ',' && j > open && j < close && depth[j] == d) commas++;
            }
        }
        commas = wave_sum(commas);
        if ((threadIdx.x & 63) == 0 && commas) atomicAdd(&st->big_commas[c], commas);
    }
}

// the workspace of both calls (host): the state, the two lists of escaped bodies -- a body over kLaneBody (kWaveBody) bytes
// takes that many bytes, so they are never full -- and one count per block of the token pass, which judges token n too
struct Work {
    State *st;
    uint32_t *long_list, *huge_list, *block_esc;
    uint32_t long_cap, huge_cap, nb;
};
static inline Work layout(msj_carver &c, uint64_t n, uint64_t len) {
    Work w;
    w.long_cap = (uint32_t)(len / kLaneBody + 1), w.huge_cap = (uint32_t)(len / kWaveBody + 1);
    w.nb = (uint32_t)((n + 1 + kBlock - 1) / kBlock);
    w.st = c.take<State>(1, 4);
    w.long_list = c.take<uint32_t>(w.long_cap, 4);
    w.huge_list = c.take<uint32_t>(w.huge_cap, 4);
    w.block_esc = c.take<uint32_t>(w.nb, 4);
    return w;
}

}  // namespace msj_val
