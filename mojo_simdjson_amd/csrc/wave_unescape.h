// wave_unescape.h -- the checked byte writer and the wave's walk over a long escaped string body, shared by the tape
// kernels (tape_block.h: tape_kernel.hip, tape_docs_kernel.hip) and string_column_kernel.hip.  Device code only; the
// per-byte arithmetic is tape_math.h (unescape_step is the host's form of the walk).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tape_math.h"
#include "wave_ops.h"

namespace msj_tape {

using namespace msj::tape;
using namespace msj::wave;
using msj::val::ByteReader;

constexpr uint32_t kLaneBody = 1024;           // bodies up to this many bytes are measured and written by their lane

struct BufWriter {  // byte o of a string's record (its length prefix included): checked against the capacity
    uint8_t *out;
    uint64_t base, cap;
    __device__ __forceinline__ void put(uint64_t o, uint32_t byte) const {
        const uint64_t a = base + o;
        if (out && a < cap) out[a] = (uint8_t)byte;
    }
};

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

}  // namespace msj_tape
