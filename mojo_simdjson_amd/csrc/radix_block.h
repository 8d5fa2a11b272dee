// radix_block.h -- the one stable least-significant-digit radix pass that sort_rows_kernel.hip (sr_count / sr_scan /
// sr_scatter), join_rows_kernel.hip (jn_*) and dictionary_order_kernel.hip (do_*) share: the geometry and the three steps,
// each for ONE tile, so that the kernels stay in their files as loops over the tiles they own.  Device code but for
// tiles_of; what a record is -- its words, its digit, who is active, the bound a place is tested against -- is the policy
// the caller hands in (below), and the digits themselves are the math headers'.
//   count    a block owns tiles of kTile = 1 024 consecutive records, four rounds of 256: its count per bucket, summed in LDS
//            (a wave whose records share the bucket adds once), to cnt[bucket * tiles + tile]
//   scan     256 workgroups of 1 024 lanes, one per bucket: the bucket's counts become running sums over the tiles (kScan
//            tiles per chunk); the bucket's total is returned
//   scatter  given the records in the buckets in front (bucket_base, or the caller's own plan), a tile's records are ranked
//            round by round: those of a wave that share the bucket by eight ballots and v_mbcnt (the same bucket in the
//            lanes below), the waves in front and the rounds in front by counters in LDS.  Records of one bucket keep their
//            order: STABLE, which the join ("ascending r inside a key") and the dictionary order rely on
// Every count is an integer sum and every place a function of the counts: the same bytes from run to run.  Safety: a record
// is loaded only where the policy says it is active, and a place is tested against the policy's bound once more.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bytes_block.h"

namespace msj_radix {

using namespace msj::wave;
using msj_bytes::kRows;
using msj_tape::kThreads, msj_tape::kWaves;

constexpr uint32_t kDigitBits = 8, kBuckets = 1u << kDigitBits;  // (each math header's own, which the host twins keep)
constexpr uint32_t kRounds = 4;
constexpr uint32_t kTile = kRounds * kRows;  // records of a block's tile
constexpr uint32_t kScan = 1024;             // tiles per chunk of the scan: scan_in_place's workgroup
constexpr uint32_t kTileBlocks = 1024;       // most blocks of the kernels over tiles (they loop over what n needs)
static_assert(kRows == (uint32_t)kThreads && kWaves == 4 && kBuckets == (uint32_t)kThreads, "a lane per bucket and per record of a round");

__host__ __device__ inline uint64_t tiles_of(uint64_t n) { return (n + kTile - 1) / kTile; }

// The count of tile v.  digit_at(j, digit) -> whether record j counts, and its digit of the pass: the caller's, so that it
// may load less than the scatter does and count what else it has to.  -> the tile's count of bucket threadIdx.x
template <class DigitAt>
__device__ __forceinline__ uint32_t count_tile(uint32_t (&s_h)[kBuckets], uint32_t *__restrict__ cnt, uint64_t tiles, uint64_t v, DigitAt digit_at) {
    s_h[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        uint32_t digit = 0;
        const bool active = digit_at(v * kTile + r * kRows + threadIdx.x, digit);
        wave_hist_add(s_h, digit, active);
    }
    __syncthreads();
    const uint32_t mine = s_h[threadIdx.x];
    cnt[(uint64_t)threadIdx.x * tiles + v] = mine;
    __syncthreads();  // (read before the next tile zeroes it)
    return mine;
}

// bucket blockIdx.x's counts become their running sum over the tiles; -> its total (a sum stays below the records < 2^31)
__device__ __forceinline__ uint64_t scan_bucket(uint32_t *__restrict__ cnt, uint64_t tiles, uint64_t (&s_w)[16]) {
    return scan_in_place(cnt + (uint64_t)blockIdx.x * tiles, tiles, s_w);
}

// the records in the buckets in front of bucket threadIdx.x, from every bucket's total (one barrier)
__device__ __forceinline__ uint32_t bucket_base(const uint32_t *__restrict__ tot, uint32_t (&s_w)[kWaves]) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t mine = tot[threadIdx.x];
    uint32_t inc = wave_scan32(mine, (int)lane);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    inc = add_waves_before(inc, s_w, (int)wave);
    return inc - mine;
}

// The scatter of tile v.  base: the records in the buckets in front of bucket threadIdx.x.  The policy p:
//   P::Record              a record's words, in registers
//   p.load(j, x) -> bool   whether record j takes part; x = its words (what an idle lane holds only has to be defined)
//   p.digit(x)             its digit of the pass
//   p.bound()              the records the pass writes: a place is tested against it
//   p.store(at, x)         the record to place at
template <class P>
__device__ __forceinline__ void scatter_tile(uint32_t (&s_run)[kBuckets], uint32_t (&s_wcnt)[kWaves][kBuckets], uint32_t base,
                                             const uint32_t *__restrict__ cnt, uint64_t tiles, uint64_t v, const P &p) {
    const uint32_t wave = threadIdx.x >> 6;
    __syncthreads();  // (the last tile's counters have been read)
    s_run[threadIdx.x] = base + cnt[(uint64_t)threadIdx.x * tiles + v];  // where the tile's first record of the bucket goes
#pragma unroll
    for (uint32_t x = 0; x < (uint32_t)kWaves; x++) s_wcnt[x][threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t r = 0; r < kRounds; r++) {
        typename P::Record x;
        const bool active = p.load(v * kTile + r * kRows + threadIdx.x, x);
        const uint32_t digit = p.digit(x);
        const uint64_t peers = wave_match<kDigitBits>(digit, active);  // the wave's active lanes with my digit
        const uint32_t rank = lanes_below(peers);
        if (active && rank == 0) s_wcnt[wave][digit] = (uint32_t)__popcll((unsigned long long)peers);
        __syncthreads();
        if (active) {
            uint32_t at = s_run[digit] + rank;
            for (uint32_t y = 0; y < wave; y++) at += s_wcnt[y][digit];
            if (at < p.bound()) p.store(at, x);  // (always: the counts are the records' own)
        }
        __syncthreads();
        uint32_t round = 0;
#pragma unroll
        for (uint32_t y = 0; y < (uint32_t)kWaves; y++) round += s_wcnt[y][threadIdx.x], s_wcnt[y][threadIdx.x] = 0;
        s_run[threadIdx.x] += round;
        __syncthreads();
    }
}

}  // namespace msj_radix
