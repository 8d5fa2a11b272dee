// wave_ops.h -- reductions and scans over one wave64 and the padded four-byte load that documents_kernel.hip,
// numbers_kernel.hip, validate_kernel.hip, validate_docs_kernel.hip and tape_kernel.hip share; a workgroup's counter and
// the running sum over an array by one workgroup, which the select and column kernels share; the ballot ranks, the
// histogram add and the workgroup ranks and running maxima of the query kernels (filter_rows, cast_strings, sort_rows,
// join_rows, dictionary_order; radix_block.h).  Device code only.  (tokens_kernel.hip has its own DPP scans and
// stage1_kernel.hip its own ballot rank.)  The device code of the four older files is pinned instruction for
// instruction: see the notes on the forms below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msj::wave {

// op over the wave (xor butterfly): every lane gets the result
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, (T)__shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return wave_reduce(v, [](uint32_t a, uint32_t b) { return a + b; }); }
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) { return wave_reduce((unsigned long long)v, [](uint64_t a, uint64_t b) { return a + b; }); }
__device__ __forceinline__ uint32_t wave_max(uint32_t v) { return wave_reduce(v, [](uint32_t a, uint32_t b) { return max(a, b); }); }
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) { return wave_reduce(v, [](auto a, auto b) { return b < a ? b : a; }); }

// Inclusive sum over the wave, two forms because they compile to different instructions.  wave_scan32 shuffles the 32-bit
// value as it is (documents_kernel.hip, numbers_kernel.hip); wave_scan<T> shuffles every T as 64 bits, a 32-bit one included
// (tape_kernel.hip).  maybe_undef: a plain by-value parameter is `noundef`, which lets the compiler drop the freeze of the
// caller's value and changes the instructions of the kernels these loops were written out in.
__device__ __forceinline__ uint32_t wave_scan32(__attribute__((maybe_undef)) uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t p = (uint32_t)__shfl_up((int)v, o);
        if (lane >= o) v += p;
    }
    return v;
}
template <class T>
__device__ __forceinline__ T wave_scan(T v) {
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = (T)__shfl_up((unsigned long long)v, o);
        if (lane >= (uint32_t)o) v += u;
    }
    return v;
}

// Running maximum over the wave (lane l: the maximum of lanes 0 .. l) and running minimum from the other end (lane l: the
// minimum of lanes l .. 63): validate_docs_kernel.hip finds every token's document with them -- the last start at or in
// front of a token, the first start behind it.
__device__ __forceinline__ uint32_t wave_scan_max(uint32_t v) {
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t p = (uint32_t)__shfl_up((int)v, o);
        if (lane >= (uint32_t)o) v = max(v, p);
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_rscan_min(uint32_t v) {
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t p = (uint32_t)__shfl_down((int)v, o);
        if (lane + (uint32_t)o < 64u) v = min(v, p);
    }
    return v;
}

// the lanes below this one whose bit is set in the ballot m (v_mbcnt): a flagged lane's rank inside its wave
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// the wave's active lanes whose x agrees with this lane's in its low `Bits` bits: a ballot per bit
template <uint32_t Bits>
__device__ __forceinline__ uint64_t wave_match(uint32_t x, bool active) {
    uint64_t peers = __ballot(active);
#pragma unroll
    for (uint32_t b = 0; b < Bits; b++) {
        const bool bit = (x >> b) & 1u;
        const uint64_t set = __ballot(bit);
        peers &= bit ? set : ~set;
    }
    return peers;
}
// one more in hist[x] for every active lane; a wave whose active lanes share one x adds once
__device__ __forceinline__ void wave_hist_add(uint32_t *hist, uint32_t x, bool active) {
    const uint64_t m = __ballot(active);
    if (m == 0) return;
    const int first_lane = __ffsll((unsigned long long)m) - 1;
    const uint32_t first = (uint32_t)__shfl((int)x, first_lane);
    if (__ballot(active && x != first) == 0) {
        if ((int)(threadIdx.x & 63) == first_lane) atomicAdd(&hist[first], (uint32_t)__popcll((unsigned long long)m));
    } else if (active) {
        atomicAdd(&hist[x], 1u);
    }
}

// wave totals through LDS: lane 63 of every wave has left its inclusive sum in s_w[wave] and the workgroup has met at a
// barrier; adds what the waves in front of `wave` hold to sum
template <class A, class T, int N>
__device__ __forceinline__ A add_waves_before(__attribute__((maybe_undef)) A sum, const T (&s_w)[N], int wave) {
    for (int w = 0; w < wave; w++) sum += s_w[w];
    return sum;
}

// One counter for the workgroup, every lane calls: v summed by wave, through s_w (a word per wave no lane still reads; free
// behind the next barrier) to lane 0, which adds the sum to *counter with one atomic, none when it is 0, and returns it.
// (One barrier per call: a kernel with two counters calls twice and meets twice, once per workgroup at its end.)
template <int N>
__device__ __forceinline__ uint32_t block_counter_add(uint32_t v, uint32_t (&s_w)[N], uint64_t *counter) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x != 0) return 0;
    for (int w = 1; w < N; w++) v += s_w[w];
    if (v) atomicAdd(reinterpret_cast<unsigned long long *>(counter), (unsigned long long)v);
    return v;
}

// a[0 .. count) becomes its exclusive running sum, by ONE workgroup of 1 024 lanes in chunks of 1 024; -> the total
template <class T>
__device__ __forceinline__ uint64_t scan_in_place(T *__restrict__ a, uint64_t count, uint64_t (&s_w)[16]) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t run = 0;
    for (uint64_t v0 = 0; v0 < count; v0 += 1024) {
        const uint64_t v = v0 + threadIdx.x;
        const uint64_t x = v < count ? a[v] : 0, inc = wave_scan(x);
        __syncthreads();
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        uint64_t before = 0, all = 0;
#pragma unroll 4
        for (uint32_t j = 0; j < 16; j++) {
            const uint64_t t = s_w[j];
            if (j < wave) before += t;
            all += t;
        }
        if (v < count) a[v] = (T)(run + before + inc - x);
        run += all;
    }
    return run;
}

// the flagged lanes in front of this one in the workgroup of W waves, and all of them (s_w: W words no lane still reads)
template <uint32_t W>
__device__ __forceinline__ uint32_t block_flag_rank(bool flag, uint32_t *s_w, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t m = __ballot(flag);
    __syncthreads();  // (the last round's totals have been read)
    if (lane == 0) s_w[wave] = (uint32_t)__popcll((unsigned long long)m);
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t x = 0; x < W; x++) {
        const uint32_t t = s_w[x];
        if (x < wave) before += t;
        all += t;
    }
    total = all;
    return before + lanes_below(m);
}
// the maximum of x over this lane and the lanes in front in the workgroup of W waves, and over all of them
template <uint32_t W>
__device__ __forceinline__ uint32_t block_scan_max(uint32_t x, uint32_t *s_w, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t inc = wave_scan_max(x);
    __syncthreads();
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t y = 0; y < W; y++) {
        const uint32_t t = s_w[y];
        if (y < wave) before = max(before, t);
        all = max(all, t);
    }
    total = all;
    return max(before, inc);
}
// a[0 .. count) becomes the maximum of the entries in front of each (0 at the first), by ONE workgroup of 1 024 lanes in
// chunks of 1 024 (s_w: 16 words)
__device__ __forceinline__ void scan_max_in_place(uint32_t *__restrict__ a, uint64_t count, uint32_t *s_w) {
    uint32_t run = 0;
    for (uint64_t v0 = 0; v0 < count; v0 += 1024) {
        const uint64_t v = v0 + threadIdx.x;
        const uint32_t x = v < count ? a[v] : 0u;
        uint32_t total;
        const uint32_t inc = block_scan_max<16>(x, s_w, total);
        // what stands in front: the inclusive maximum of the lane in front, or at a wave's first lane that of the waves in front
        uint32_t prev = (uint32_t)__shfl_up((int)inc, 1);
        if ((threadIdx.x & 63) == 0) {
            prev = 0;
            for (uint32_t y = 0; y < (threadIdx.x >> 6); y++) prev = max(prev, s_w[y]);
        }
        if (v < count) a[v] = max(run, prev);
        run = max(run, total);
        __syncthreads();  // (s_w read before the next chunk writes it)
    }
}

// bytes a[j .. j + 4) as one word, j a multiple of 4; bytes from n on read as 0
__device__ __forceinline__ uint32_t load_byte_quad(const uint8_t *__restrict__ a, uint64_t j, uint64_t n) {
    if (j + 4 <= n) return *reinterpret_cast<const uint32_t *>(a + j);
    uint32_t w = 0;
    for (int k = 0; k < 4 && j + k < n; k++) w |= (uint32_t)a[j + k] << (8 * k);
    return w;
}

}  // namespace msj::wave
