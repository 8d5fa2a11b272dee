// Number values for stage 2 -- msj_number_values_device (include/msj_stage1.h): the reference's Int(span) /
// Float64(span) (number_parsing.mojo:60-78, feeding TapeWriter.append_s64 / append_double) for every number token of a
// segment at once.  The per-number arithmetic (scan, Clinger, Eisel-Lemire, the exact big-integer path) is
// number_math.h, host + device, checked on the CPU by tests/test_number_math.py.
//
// Launches, all on the caller's stream, no host round trip:
//   num_count     per block of kBlock tokens: how many carry MSJ_SPAN_NUMBER (flags read 8 bytes at a time)
//   num_scan      one workgroup: exclusive scan of the block counts = the rank of each block's first number; writes
//                 the call's result (n_numbers; errors and first_error start empty) and clears the list counters
//   num_convert   per block: the block's numbers compacted into LDS in token order, then one lane per number, 64 numbers
//                 per wave: scan + Clinger + Eisel-Lemire, one 16-byte record.  Numbers those cannot decide go to the
//                 fallback list (bounded; an append past its end sets the overflow marker instead), numbers flagged
//                 MSJ_SPAN_LONG (over 1024 characters) to the long list (bounded by len / 1025: never full)
//   num_long      one wave per long number: the runs of digits found 64 bytes per step (ballots), then the same
//                 arithmetic, exact path included
//   num_fallback  one lane per entry of the fallback list: the exact path; nothing when the list overflowed
//   num_sweep     only when the list overflowed: num_convert again, resolving every number the fast paths cannot
//                 decide in place (a document whose numbers all need the exact path still finishes, correctly)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "launch.h"
#include "number_math.h"
#include "wave_ops.h"

namespace msj_nums {

using namespace msj::num;
using namespace msj::wave;

constexpr int kThreads = 256;
constexpr int kPer = 16;                      // flags per thread
constexpr uint32_t kBlock = kThreads * kPer;  // tokens per workgroup
static_assert(kBlock <= 65536, "num_convert keeps block-relative token numbers as uint16");
constexpr int kScanThreads = 1024;
constexpr int kListBlocks = 512;              // grid of the list kernels (they loop over what the lists hold)
constexpr int kWin = 64;                      // bytes of a number's window staged in LDS (from its 16-byte line on)
constexpr int kWinStride = kWin + 4;          // per lane; 17 dwords: lanes spread over the banks

struct Counters {
    uint32_t fb_count, fb_overflow, long_count, reserved;
};

static_assert(sizeof(msj_number) == 16, "one 16-byte store per record");

// 32 flags of this thread, bit k: token base + k is a number
__device__ __forceinline__ uint32_t number_mask(const uint8_t *__restrict__ flags, uint64_t n, uint64_t base) {
    if (base >= n) return 0;
    uint32_t m = 0;
    if (base + kPer <= n) {
        const uint2 *p = reinterpret_cast<const uint2 *>(flags + base);
#pragma unroll
        for (int j = 0; j < kPer / 8; j++) {
            const uint2 v = p[j];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                m |= ((v.x >> (8 * k + 2)) & 1u) << (8 * j + k);
                m |= ((v.y >> (8 * k + 2)) & 1u) << (8 * j + 4 + k);
            }
        }
    } else {
        for (int k = 0; k < kPer && base + k < n; k++) m |= ((flags[base + k] & MSJ_SPAN_NUMBER) ? 1u : 0u) << k;
    }
    return m;
}

// The lane path's reader: the kWin bytes from the number's 16-byte line on, loaded with four independent 16-byte loads
// into this lane's slot of LDS, so that the scan's byte-by-byte reads (each depends on the one before) wait for LDS
// instead of for memory; bytes beyond the window are read from memory.  Same answers as SerialRuns.
struct WindowRuns {
    const uint8_t *buf;
    uint64_t len;
    uint64_t a;          // first byte of the window (16-byte aligned)
    const uint8_t *win;  // this lane's LDS slot
    __device__ __forceinline__ void load(uint8_t *slot, uint64_t start) {
        a = start & ~15ull;
        win = slot;
        uint4 q[kWin / 16];
#pragma unroll
        for (int c = 0; c < kWin / 16; c++) {
            const uint64_t b = a + 16u * c;
            if (b + 16 <= len) {
                q[c] = *reinterpret_cast<const uint4 *>(buf + b);
            } else {
                uint32_t v[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    v[k] = 0;
#pragma unroll
                    for (int i = 0; i < 4; i++) v[k] |= (b + 4 * k + i < len ? (uint32_t)buf[b + 4 * k + i] : 0x20u) << (8 * i);
                }
                q[c] = make_uint4(v[0], v[1], v[2], v[3]);
            }
        }
        uint32_t *d = reinterpret_cast<uint32_t *>(slot);
#pragma unroll
        for (int c = 0; c < kWin / 16; c++) {
            d[4 * c] = q[c].x, d[4 * c + 1] = q[c].y, d[4 * c + 2] = q[c].z, d[4 * c + 3] = q[c].w;
        }
    }
    __device__ __forceinline__ uint32_t at(uint64_t p) const {
        const uint64_t o = p - a;
        if (o < (uint64_t)kWin) return win[o];
        return p < len ? buf[p] : 0x20u;
    }
    __device__ __forceinline__ uint64_t run_end(uint64_t p) const {
        while (is_digit(at(p))) p++;
        return p;
    }
    __device__ __forceinline__ uint64_t first_nonzero(uint64_t b, uint64_t e) const {
        while (b < e && at(b) == '0') b++;
        return b;
    }
    __device__ __forceinline__ bool any_nonzero(uint64_t b, uint64_t e) const { return first_nonzero(b, e) < e; }
};

__global__ __launch_bounds__(kThreads) void num_count(const uint8_t *__restrict__ flags, uint64_t n, uint32_t *__restrict__ block_cnt) {
    __shared__ uint32_t w_cnt[kThreads / 64];
    const uint64_t base = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) * kPer;
    const uint32_t c = wave_sum(__popc(number_mask(flags, n, base)));
    if ((threadIdx.x & 63) == 0) w_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = w_cnt[0] + w_cnt[1] + w_cnt[2] + w_cnt[3];
}

__global__ __launch_bounds__(kScanThreads) void num_scan(const uint32_t *__restrict__ block_cnt, uint32_t nb, uint32_t *__restrict__ block_off,
                                                         msj_numbers_result *__restrict__ result, Counters *__restrict__ counters) {
    __shared__ uint32_t s_cnt[kScanThreads / 64];
    const uint32_t per = (nb + kScanThreads - 1u) / kScanThreads;
    const uint32_t b0 = threadIdx.x * per, b1 = min(nb, b0 + per);
    uint32_t c = 0;
    for (uint32_t b = b0; b < b1; b++) c += block_cnt[b];
    const int lane = threadIdx.x & 63;
    uint32_t inc = c;
    inc = wave_scan32(inc, lane);
    const int wave = threadIdx.x >> 6;
    if (lane == 63) s_cnt[wave] = inc;
    __syncthreads();
    uint32_t run = inc - c;
    run = add_waves_before(run, s_cnt, wave);
    for (uint32_t b = b0; b < b1; b++) {
        block_off[b] = run;
        run += block_cnt[b];
    }
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (int w = 0; w < kScanThreads / 64; w++) total += s_cnt[w];
        msj_numbers_result r;
        r.n_numbers = total;
        r.n_errors = 0;
        r.first_error = ~0ull;
        r.n_slow = 0;
        *result = r;
        *counters = Counters{0, 0, 0, 0};
    }
}

__device__ __forceinline__ void emit(msj_number *__restrict__ out, uint64_t capacity, uint32_t slot, uint32_t token, const Result &res,
                                     msj_numbers_result *__restrict__ result) {
    if (slot < capacity) {
        ulonglong2 v;
        v.x = res.bits;
        v.y = (uint64_t)token | ((uint64_t)res.kind << 32);
        *reinterpret_cast<ulonglong2 *>(out + slot) = v;
    }
    if (res.kind == kErrSyntax || res.kind == kErrRange) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&result->n_errors), 1ull);
        atomicMin(reinterpret_cast<unsigned long long *>(&result->first_error), (unsigned long long)token);
    }
    if (res.path == 2) atomicAdd(reinterpret_cast<unsigned long long *>(&result->n_slow), 1ull);
}

// kSweep = false: num_convert; true: num_sweep (acts only when the fallback list overflowed, and only on the numbers the
// fast paths cannot decide)
template <bool kSweep>
__global__ __launch_bounds__(kThreads) void num_convert(const uint8_t *__restrict__ buf, uint64_t len, const uint32_t *__restrict__ idx,
                                                        uint64_t n, const uint8_t *__restrict__ flags,
                                                        const uint32_t *__restrict__ block_off, msj_number *__restrict__ out,
                                                        uint64_t capacity, msj_numbers_result *__restrict__ result,
                                                        Counters *__restrict__ counters, uint2 *__restrict__ fb_list, uint32_t fb_cap,
                                                        uint2 *__restrict__ long_list, uint32_t long_cap) {
    __shared__ uint16_t s_tok[kBlock];  // the block's number tokens, relative to its first token
    __shared__ uint32_t w_cnt[kThreads / 64];
    __shared__ uint32_t s_win[kThreads * kWinStride / 4];
    if (kSweep && *reinterpret_cast<volatile uint32_t *>(&counters->fb_overflow) == 0) return;
    const uint64_t base = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) * kPer;
    uint32_t m = number_mask(flags, n, base);
    const uint32_t c = __popc(m);
    const int lane = threadIdx.x & 63;
    uint32_t inc = c;
    inc = wave_scan32(inc, lane);
    const int wave = threadIdx.x >> 6;
    if (lane == 63) w_cnt[wave] = inc;
    __syncthreads();
    uint32_t pos = inc - c, total = 0;
    for (int w = 0; w < kThreads / 64; w++) {
        pos += w < wave ? w_cnt[w] : 0u;
        total += w_cnt[w];
    }
    while (m) {
        const uint32_t k = __ffs(m) - 1u;
        m &= m - 1u;
        s_tok[pos++] = (uint16_t)(threadIdx.x * kPer + k);
    }
    __syncthreads();
    const uint32_t first = block_off[blockIdx.x], tok0 = blockIdx.x * kBlock;
    const SerialRuns r{buf, len};
    WindowRuns wr{buf, len, 0, nullptr};
    uint8_t *my_win = reinterpret_cast<uint8_t *>(s_win) + threadIdx.x * kWinStride;
    for (uint32_t j = threadIdx.x; j < total; j += kThreads) {
        const uint32_t token = tok0 + s_tok[j], slot = first + j;
        const uint32_t f = flags[token];
        if (f & MSJ_SPAN_LONG) {
            if (!kSweep) {
                const uint32_t k = atomicAdd(&counters->long_count, 1u);
                if (k < long_cap) long_list[k] = make_uint2(token, slot);
            }
            continue;
        }
        const uint32_t start = idx[token];
        wr.load(my_win, start);
        const Scan sc = scan_number(wr, start);
        Result res = convert_fast(wr, sc);
        if (res.kind == kPending) {
            if (kSweep) {
                emit(out, capacity, slot, token, convert_exact(r, sc, res), result);
            } else {
                const uint32_t k = atomicAdd(&counters->fb_count, 1u);
                if (k < fb_cap) {
                    fb_list[k] = make_uint2(token, slot);
                } else {
                    atomicOr(&counters->fb_overflow, 1u);
                }
            }
            continue;
        }
        if (!kSweep) emit(out, capacity, slot, token, res, result);
    }
}

__global__ __launch_bounds__(kThreads) void num_fallback(const uint8_t *__restrict__ buf, uint64_t len, const uint32_t *__restrict__ idx,
                                                         msj_number *__restrict__ out, uint64_t capacity,
                                                         msj_numbers_result *__restrict__ result, const Counters *__restrict__ counters,
                                                         const uint2 *__restrict__ fb_list, uint32_t fb_cap) {
    if (counters->fb_overflow) return;  // num_sweep resolves all of them
    const uint32_t cnt = min(counters->fb_count, fb_cap);
    const SerialRuns r{buf, len};
    for (uint32_t j = blockIdx.x * kThreads + threadIdx.x; j < cnt; j += gridDim.x * kThreads) {
        const uint2 e = fb_list[j];
        const Scan sc = scan_number(r, idx[e.x]);
        const Result f = convert_fast(r, sc);
        emit(out, capacity, e.y, e.x, f.kind == kPending ? convert_exact(r, sc, f) : f, result);
    }
}

// The runs of digits of one number, answered by a whole wave 64 bytes per step.  Every lane calls with the same
// arguments and gets the same answer, so the arithmetic above stays wave-uniform.
struct WaveRuns {
    const uint8_t *buf;
    uint64_t len;
    __device__ __forceinline__ uint32_t at(uint64_t p) const { return p < len ? buf[p] : 0x20u; }
    __device__ __forceinline__ uint64_t run_end(uint64_t p) const {
        const uint32_t lane = threadIdx.x & 63;
        for (;;) {
            const uint64_t nd = __ballot(!is_digit(at(p + lane)));
            if (nd) return p + (uint64_t)(__ffsll((unsigned long long)nd) - 1);
            p += 64;
        }
    }
    __device__ __forceinline__ uint64_t first_nonzero(uint64_t b, uint64_t e) const {
        const uint32_t lane = threadIdx.x & 63;
        for (; b < e; b += 64) {
            const uint64_t p = b + lane;
            const uint64_t nz = __ballot(p < e && buf[p] != '0');
            if (nz) return b + (uint64_t)(__ffsll((unsigned long long)nz) - 1);
        }
        return e;
    }
    __device__ __forceinline__ bool any_nonzero(uint64_t b, uint64_t e) const { return first_nonzero(b, e) < e; }
};

__global__ __launch_bounds__(kThreads) void num_long(const uint8_t *__restrict__ buf, uint64_t len, const uint32_t *__restrict__ idx,
                                                     msj_number *__restrict__ out, uint64_t capacity, msj_numbers_result *__restrict__ result,
                                                     const Counters *__restrict__ counters, const uint2 *__restrict__ long_list,
                                                     uint32_t long_cap) {
    const uint32_t cnt = min(counters->long_count, long_cap);
    const uint32_t waves = gridDim.x * (kThreads / 64);
    const WaveRuns r{buf, len};
    for (uint32_t j = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); j < cnt; j += waves) {
        const uint2 e = long_list[j];
        const Scan sc = scan_number(r, idx[e.x]);
        Result res = convert_fast(r, sc);
        if (res.kind == kPending) res = convert_exact(r, sc, res);
        if ((threadIdx.x & 63) == 0) emit(out, capacity, e.y, e.x, res, result);
    }
}

}  // namespace msj_nums

extern "C" uint32_t msj_number_fallback_capacity(uint64_t n) { return (uint32_t)(n / 16 + 4096); }
extern "C" uint32_t msj_number_long_capacity(uint64_t len) { return (uint32_t)(len / 1025 + 1); }

namespace msj_nums {
struct Work {
    Counters *counters;
    uint32_t *block_cnt, *block_off;  // per block
    uint2 *fb_list, *long_list;
};
static inline Work layout(msj_carver &c, uint64_t n, uint64_t len) {
    const uint64_t nb = (n + kBlock - 1) / kBlock;
    Work w;
    w.counters = c.take<Counters>(1, 4);
    w.block_cnt = c.take<uint32_t>(nb ? nb : 1, 4);
    w.block_off = c.take<uint32_t>(nb ? nb : 1, 4);
    w.fb_list = c.take<uint2>(msj_number_fallback_capacity(n), 8);  // 16 + 8 * nb bytes in: 8-byte aligned
    w.long_list = c.take<uint2>(msj_number_long_capacity(len), 8);
    return w;
}
}  // namespace msj_nums

extern "C" uint64_t msj_number_values_workspace_bytes(uint64_t n, uint64_t len) { return msj_measure(msj_nums::layout, n, len) + 64; }

extern "C" int msj_launch_number_values(const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n, const uint8_t *d_flags,
                                        msj_number *d_numbers, uint64_t capacity, msj_numbers_result *d_result, void *d_ws, void *stream) {
    using namespace msj_nums;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t nb = (uint32_t)((n + kBlock - 1) / kBlock);
    const Work w = msj_place(layout, d_ws, n, len);
    const uint32_t fb_cap = msj_number_fallback_capacity(n), long_cap = msj_number_long_capacity(len);
    if (nb) hipLaunchKernelGGL(num_count, dim3(nb), dim3(kThreads), 0, s, d_flags, n, w.block_cnt);
    hipLaunchKernelGGL(num_scan, dim3(1), dim3(kScanThreads), 0, s, w.block_cnt, nb, w.block_off, d_result, w.counters);
    if (nb) {
        hipLaunchKernelGGL(num_convert<false>, dim3(nb), dim3(kThreads), 0, s, d_buf, len, d_idx, n, d_flags, w.block_off, d_numbers, capacity,
                           d_result, w.counters, w.fb_list, fb_cap, w.long_list, long_cap);
        hipLaunchKernelGGL(num_long, dim3(kListBlocks / 4), dim3(kThreads), 0, s, d_buf, len, d_idx, d_numbers, capacity, d_result, w.counters,
                           w.long_list, long_cap);
        hipLaunchKernelGGL(num_fallback, dim3(kListBlocks), dim3(kThreads), 0, s, d_buf, len, d_idx, d_numbers, capacity, d_result, w.counters,
                           w.fb_list, fb_cap);
        hipLaunchKernelGGL(num_convert<true>, dim3(nb), dim3(kThreads), 0, s, d_buf, len, d_idx, n, d_flags, w.block_off, d_numbers, capacity,
                           d_result, w.counters, w.fb_list, fb_cap, w.long_list, long_cap);
    }
    return (int)hipGetLastError();
}
