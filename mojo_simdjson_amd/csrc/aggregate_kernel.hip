// Count, sum, min, max per group -- msj_aggregate_device (include/msj_stage1.h): from msj_field records with their
// msj_select_documents_result and an int32 code per row, one 48-byte msj_aggregate per (column, group).  The arithmetic --
// the value test, the exponents, a value's limbs, the 128-bit sum and its one rounding, the min / max rule, the record of a
// group -- is aggregate_math.h, host + device and checked on the CPU by tests/test_aggregate_math.py.  R and G are read on
// the device by every kernel: the host sizes the launches by the capacities.
//
// Every accumulator (aggregate_math.h: Acc, one per (column, group) in the workspace) starts at zero and grows by 64-bit
// integer adds and integer maxima alone -- a minimum is the maximum of the inverted key -- so the words a launch leaves
// do not depend on which lane ran when: the records are the same bytes from run to run and for any order of the rows.
// Launches, all on the caller's stream, behind a memset of the call's counters; no lane ever waits for another lane:
//   ag_init    zeroes the accumulators of the groups below G
//   ag_pass1   a lane per row, blockIdx.y the column: the code (a wave's loads consecutive), one 16-byte record load, and
//              into the row's group: n_rows, n_values, the count of doubles, the largest exponent, the int and the double
//              minimum and maximum as keys
//   ag_pass2   the same rows again: the value's limbs for what pass 1 found -- the int64's two limbs while the group holds
//              no double, else the three limbs of trunc(v * 2^(95 - E)) -- added into three 64-bit sums
//   ag_finish  a lane per (column, group): the record (aggregate_math.h: finish_group), three 16-byte stores
//   ag_result  one lane: the result
// Two ways into a group's words (kLds; DESIGN.md section 5b has both rates).  G at or below the limit: a block keeps the G
// groups in LDS over all the rows it owns and adds what it touched to the global words once, at its end -- with few groups
// every lane of the grid would otherwise queue on the same few addresses.  G above it: global atomics from the lanes, which
// then spread over many addresses.  In both a wave whose 64 rows share one group (always so without codes) reduces by
// shuffles first and lets lane 0 add.  The choice is uniform over the grid, made from G, and changes no bit of the output.
// Safety: a record and a code are read only at k < R <= stride; a group's words only at g < G <= groups_capacity, in LDS
// only at g < G <= the limit <= kMaxLdsGroups.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "aggregate_math.h"
#include "bytes_block.h"
#include "launch.h"

namespace msj_agg {

using namespace msj::agg;
using namespace msj::wave;
using msj_bytes::kRows, msj_bytes::most_rows;
using msj_tape::kThreads, msj_tape::kWaves;
using msj_tdocs::load_field;

static_assert(sizeof(msj_aggregate) == 48 && sizeof(msj_aggregate_result) == 48 && sizeof(msj_field) == 16, "ABI");
static_assert(kRows == (uint32_t)kThreads && kWaves == 4, "geometry");

constexpr uint32_t kMaxLdsGroups = kAggregateMaxLdsGroups;
constexpr uint32_t kRowBlocks = 2048;    // most blocks of a pass per column (they loop over what R needs)
constexpr uint32_t kGroupBlocks = 4096;  // most blocks of ag_init / ag_finish per column

struct State {  // cleared by a memset per call
    unsigned long long n_ungrouped, n_values, n_skipped;
    uint32_t flags, reserved[9];
};
static_assert(sizeof(State) == 64, "layout");
struct Work {
    State *st;
    Acc *acc;  // [c * groups_capacity + g]
};
struct Call {
    const msj_field *fields;
    uint64_t stride;
    const msj_select_documents_result *sel;
    const int32_t *codes;
    uint64_t n_groups;
    const uint64_t *d_n_groups;
    uint64_t groups_capacity;
    uint32_t lds_groups;
};

static inline Work layout(msj_carver &c, uint64_t groups_capacity, uint32_t n_columns) {
    Work w;
    w.st = c.take<State>(1);
    w.acc = c.take<Acc>(groups_capacity * n_columns);
    return w;
}

// what every kernel reads of the call: R rows in `blocks` blocks, G groups.  stop: nothing but the result is written
struct Head {
    uint64_t R, G, blocks;
    int32_t code;
    bool skip, over, stop, lds;
};
__device__ __forceinline__ Head load_head(const Call &call) {
    Head h;
    h.code = call.sel->code;
    h.R = call.sel->n_documents;
    h.G = call.d_n_groups ? *call.d_n_groups : call.n_groups;
    h.skip = h.code != 0;
    h.over = !h.skip && (rows_over(h.R, call.stride) || groups_over(h.G, call.groups_capacity));
    h.stop = h.skip || h.over;
    h.blocks = h.stop ? 0 : (h.R + kRows - 1) / kRows;
    h.lds = h.G <= call.lds_groups;
    return h;
}

__device__ __forceinline__ unsigned long long wave_max64(unsigned long long v) {
    return wave_reduce(v, [](unsigned long long a, unsigned long long b) { return b > a ? b : a; });
}
__device__ __forceinline__ void add_to(uint64_t *p, uint64_t v) {
    if (v) atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}
__device__ __forceinline__ void add_to(int64_t *p, int64_t v) {
    if (v) atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);  // (two's complement: the sum wraps as the twin's does)
}
__device__ __forceinline__ void max_to(uint64_t *p, uint64_t v) {
    if (v) atomicMax(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}

// a block's groups in LDS: pass 1's eight words of Acc, and pass 2's sums with what pass 1 found
struct Lds1 {
    uint64_t n_rows, n_values, n_double, ekey, int_min_inv, int_max, dbl_min_inv, dbl_max;
};
struct Lds2 {
    int64_t a[3];
    uint64_t n_double, ekey;
};

// one row of pass 1 as the words it adds: all 0 for a row without a value, and 0 changes nothing
struct Note {
    uint64_t ekey, int_min_inv, int_max, dbl_min_inv, dbl_max;
    uint32_t value, dbl;
};
__device__ __forceinline__ Note note_of(bool value, uint32_t type, uint64_t bits) {
    Note n{0, 0, 0, 0, 0, 0, 0};
    if (!value) return n;
    n.value = 1, n.ekey = exp_key(type, bits);
    if (type == 'l') {
        const uint64_t k = int_key((int64_t)bits);
        n.int_min_inv = ~k, n.int_max = k;
    } else {
        const uint64_t k = double_key(bits);
        n.dbl = 1, n.dbl_min_inv = ~k, n.dbl_max = k;
    }
    return n;
}
// (a key and its inverse cannot both be 0, so a value always leaves a mark in the two words of its type; a key of 0 itself
// -- INT64_MIN as a maximum -- is the word's start value)
template <class T>
__device__ __forceinline__ void note_into(T *x, uint64_t rows, uint64_t values, uint64_t doubles, const Note &n) {
    add_to(&x->n_rows, rows), add_to(&x->n_values, values), add_to(&x->n_double, doubles);
    max_to(&x->ekey, n.ekey);
    max_to(&x->int_min_inv, n.int_min_inv), max_to(&x->int_max, n.int_max);
    max_to(&x->dbl_min_inv, n.dbl_min_inv), max_to(&x->dbl_max, n.dbl_max);
}
// a wave's rows into their groups' words at `base`: all 64 in one group -> shuffles and lane 0; else a lane per row
template <class T>
__device__ __forceinline__ void wave_note(T *base, int64_t g, Note n) {
    const int g32 = (int)g, g0 = __shfl(g32, 0);
    if (g0 >= 0 && __all(g32 == g0)) {
        const uint32_t cnt = wave_sum(1u | n.value << 8 | n.dbl << 16);
        n.ekey = wave_max64(n.ekey);
        n.int_min_inv = wave_max64(n.int_min_inv), n.int_max = wave_max64(n.int_max);
        n.dbl_min_inv = wave_max64(n.dbl_min_inv), n.dbl_max = wave_max64(n.dbl_max);
        if ((threadIdx.x & 63) == 0) note_into(base + g0, cnt & 0xFFu, (cnt >> 8) & 0xFFu, cnt >> 16, n);
    } else if (g >= 0) {
        note_into(base + g, 1, n.value, n.dbl, n);
    }
}
template <class T>
__device__ __forceinline__ void wave_add(T *base, int64_t g, int64_t l[3]) {
    const int g32 = (int)g, g0 = __shfl(g32, 0);
    if (g0 >= 0 && __all(g32 == g0)) {
#pragma unroll
        for (int i = 0; i < 3; i++) l[i] = (int64_t)wave_sum64((uint64_t)l[i]);
        if ((threadIdx.x & 63) == 0) add_to(&base[g0].a[0], l[0]), add_to(&base[g0].a[1], l[1]), add_to(&base[g0].a[2], l[2]);
    } else if (g >= 0) {
        add_to(&base[g].a[0], l[0]), add_to(&base[g].a[1], l[1]), add_to(&base[g].a[2], l[2]);
    }
}

__global__ __launch_bounds__(kThreads) void ag_init(const Call call, const Work w) {
    const Head h = load_head(call);
    if (h.stop) return;
    uint4 *words = reinterpret_cast<uint4 *>(w.acc + (uint64_t)blockIdx.y * call.groups_capacity);  // (column c's G accumulators lie back to back)
    const uint64_t n = h.G * (sizeof(Acc) / 16);
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) words[i] = make_uint4(0, 0, 0, 0);
}

template <bool kLds>
__device__ __forceinline__ void pass1(const Call &call, const Work &w, const Head &h, Lds1 *s_acc, uint32_t (&s_a)[kWaves], uint32_t (&s_b)[kWaves],
                                      uint32_t (&s_c)[kWaves]) {
    const msj_field *col = call.fields + (uint64_t)blockIdx.y * call.stride;
    Acc *acc = w.acc + (uint64_t)blockIdx.y * call.groups_capacity;
    if (kLds) {
        for (uint64_t g = threadIdx.x; g < h.G; g += kThreads) s_acc[g] = Lds1{0, 0, 0, 0, 0, 0, 0, 0};
        __syncthreads();
    }
    uint32_t ungrouped = 0, values = 0, skipped = 0;
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t k = v * kRows + threadIdx.x;
        int64_t g = -1;
        bool value = false;
        msj_field f{};
        if (k < h.R) {
            g = group_of(call.codes, k, h.G);
            ungrouped += g < 0;
            if (g >= 0) {
                f = load_field(col, k);
                const uint32_t kind = value_kind(f);
                value = kind == kValue, skipped += kind == kSkipped;
            }
        }
        values += value;
        const Note n = note_of(value, f.type, f.bits);
        if (kLds) wave_note(s_acc, g, n);
        else wave_note(acc, g, n);
    }
    (void)block_counter_add(blockIdx.y == 0 ? ungrouped : 0u, s_a, reinterpret_cast<uint64_t *>(&w.st->n_ungrouped));
    (void)block_counter_add(values, s_b, reinterpret_cast<uint64_t *>(&w.st->n_values));
    (void)block_counter_add(skipped, s_c, reinterpret_cast<uint64_t *>(&w.st->n_skipped));
    if (kLds) {  // (behind the counters' barriers: every lane's LDS atomics are done)
        for (uint64_t g = threadIdx.x; g < h.G; g += kThreads) {
            const Lds1 x = s_acc[g];
            if (x.n_rows == 0) continue;
            note_into(acc + g, x.n_rows, x.n_values, x.n_double, Note{x.ekey, x.int_min_inv, x.int_max, x.dbl_min_inv, x.dbl_max, 0, 0});
        }
    }
}

__global__ __launch_bounds__(kThreads) void ag_pass1(const Call call, const Work w) {
    __shared__ Lds1 s_acc[kMaxLdsGroups];
    __shared__ uint32_t s_a[kWaves], s_b[kWaves], s_c[kWaves];
    const Head h = load_head(call);
    if (h.stop) return;
    if (h.lds) pass1<true>(call, w, h, s_acc, s_a, s_b, s_c);  // (uniform over the grid)
    else pass1<false>(call, w, h, s_acc, s_a, s_b, s_c);
}

template <bool kLds>
__device__ __forceinline__ void pass2(const Call &call, const Work &w, const Head &h, Lds2 *s_acc) {
    const msj_field *col = call.fields + (uint64_t)blockIdx.y * call.stride;
    Acc *acc = w.acc + (uint64_t)blockIdx.y * call.groups_capacity;
    if (kLds) {
        for (uint64_t g = threadIdx.x; g < h.G; g += kThreads) s_acc[g] = Lds2{{0, 0, 0}, acc[g].n_double, acc[g].ekey};
        __syncthreads();
    }
    for (uint64_t v = blockIdx.x; v < h.blocks; v += gridDim.x) {
        const uint64_t k = v * kRows + threadIdx.x;
        int64_t g = -1;
        int64_t l[3] = {0, 0, 0};
        if (k < h.R) {
            g = group_of(call.codes, k, h.G);
            if (g >= 0) {
                const msj_field f = load_field(col, k);
                if (value_kind(f) == kValue) {
                    const uint64_t n_double = kLds ? s_acc[g].n_double : acc[g].n_double, ekey = kLds ? s_acc[g].ekey : acc[g].ekey;
                    pass2_limbs(n_double, ekey, f.type, f.bits, l);
                }
            }
        }
        if (kLds) wave_add(s_acc, g, l);
        else wave_add(acc, g, l);
    }
    if (kLds) {
        __syncthreads();
        for (uint64_t g = threadIdx.x; g < h.G; g += kThreads) add_to(&acc[g].a[0], s_acc[g].a[0]), add_to(&acc[g].a[1], s_acc[g].a[1]), add_to(&acc[g].a[2], s_acc[g].a[2]);
    }
}

__global__ __launch_bounds__(kThreads) void ag_pass2(const Call call, const Work w) {
    __shared__ Lds2 s_acc[kMaxLdsGroups];
    const Head h = load_head(call);
    if (h.stop) return;
    if (h.lds) pass2<true>(call, w, h, s_acc);
    else pass2<false>(call, w, h, s_acc);
}

__global__ __launch_bounds__(kThreads) void ag_finish(const Call call, const Work w, msj_aggregate *__restrict__ groups) {
    const Head h = load_head(call);
    if (h.stop) return;
    const Acc *acc = w.acc + (uint64_t)blockIdx.y * call.groups_capacity;
    uint4 *out = reinterpret_cast<uint4 *>(groups + (uint64_t)blockIdx.y * call.groups_capacity);
    uint32_t flags = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x; g < h.G; g += (uint64_t)gridDim.x * kThreads) {
        const msj_aggregate r = finish_group<msj_aggregate>(acc[g]);
        flags |= r.flags;
        const uint32_t tail = (uint32_t)r.sum_type | (uint32_t)r.min_type << 8 | (uint32_t)r.max_type << 16 | (uint32_t)r.flags << 24;
        out[3 * g] = make_uint4((uint32_t)r.n_rows, (uint32_t)(r.n_rows >> 32), (uint32_t)r.n_values, (uint32_t)(r.n_values >> 32));
        out[3 * g + 1] = make_uint4((uint32_t)r.sum_bits, (uint32_t)(r.sum_bits >> 32), (uint32_t)r.min_bits, (uint32_t)(r.min_bits >> 32));
        out[3 * g + 2] = make_uint4((uint32_t)r.max_bits, (uint32_t)(r.max_bits >> 32), tail, 0u);
    }
    if (flags) atomicOr(&w.st->flags, flags);
}

__global__ void ag_result(const Call call, const Work w, msj_aggregate_result *__restrict__ result) {
    const Head h = load_head(call);
    msj_aggregate_result r;
    r.code = h.skip ? h.code : h.over ? MSJ_CAPACITY : 0;
    r.flags = h.stop ? 0 : w.st->flags;
    r.n_rows = h.skip ? 0 : h.R;
    r.n_groups = h.skip ? 0 : h.G;
    r.n_ungrouped = h.stop ? 0 : w.st->n_ungrouped;
    r.n_values = h.stop ? 0 : w.st->n_values;
    r.n_skipped = h.stop ? 0 : w.st->n_skipped;
    *result = r;
}

}  // namespace msj_agg

extern "C" uint64_t msj_aggregate_workspace_bytes(uint64_t capacity, uint64_t groups_capacity, uint32_t n_columns) {
    (void)capacity;  // (nothing is kept per row)
    return msj_measure(msj_agg::layout, groups_capacity, n_columns) + 64;
}

extern "C" int msj_launch_aggregate(const msj_field *d_fields, uint64_t stride, uint32_t n_columns, const msj_select_documents_result *d_rows_select,
                                    const int32_t *d_codes, uint64_t n_groups, const uint64_t *d_n_groups, msj_aggregate *d_groups,
                                    uint64_t groups_capacity, uint32_t lds_groups, msj_aggregate_result *d_result, void *d_ws, void *stream) {
    using namespace msj_agg;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Call call{d_fields, stride, d_rows_select, d_codes, n_groups, d_n_groups, groups_capacity, lds_groups < kMaxLdsGroups ? lds_groups : kMaxLdsGroups};
    const Work w = msj_place(layout, d_ws, groups_capacity, n_columns);
    const hipError_t cleared = hipMemsetAsync(w.st, 0, sizeof(State), s);
    if (cleared != hipSuccess) return (int)cleared;
    const uint64_t most = most_rows(stride), nb = (most + kRows - 1) / kRows;
    const uint64_t gb = (groups_capacity * (sizeof(Acc) / 16) + kThreads - 1) / kThreads, fb = (groups_capacity + kThreads - 1) / kThreads;
    const dim3 rows_grid((uint32_t)(nb > kRowBlocks ? kRowBlocks : nb), n_columns);
    if (groups_capacity) hipLaunchKernelGGL(ag_init, dim3((uint32_t)(gb > kGroupBlocks ? kGroupBlocks : gb), n_columns), dim3(kThreads), 0, s, call, w);
    if (most) {  // (without a group's room too: the rows are counted in n_ungrouped)
        hipLaunchKernelGGL(ag_pass1, rows_grid, dim3(kThreads), 0, s, call, w);
        hipLaunchKernelGGL(ag_pass2, rows_grid, dim3(kThreads), 0, s, call, w);
    }
    if (groups_capacity) hipLaunchKernelGGL(ag_finish, dim3((uint32_t)(fb > kGroupBlocks ? kGroupBlocks : fb), n_columns), dim3(kThreads), 0, s, call, w, d_groups);
    hipLaunchKernelGGL(ag_result, dim3(1), dim3(1), 0, s, call, w, d_result);
    return (int)hipGetLastError();
}
