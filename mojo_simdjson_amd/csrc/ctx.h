// ctx.h -- struct msj_ctx and what the three host files of the C ABI share: api.cpp (context, stage 1), host_pipe.cpp (the
// pinned-ring pipeline of the host-pointer entry point) and stage2_api.cpp (every device call behind stage 1).
// Internal: nothing declared here is exported from the library.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "../../include/msj_stage1.h"
#include "launch.h"
#include "stage1_kernel.h"

#pragma GCC visibility push(hidden)

inline bool hip_ok(hipError_t e) { return e == hipSuccess; }
inline bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }  // (null is aligned)

// Device memory a context keeps between calls, grown on demand.  Every buffer of a context is one of these: none has a
// free of its own to forget, and the old block is never freed under a kernel that may still be using it.
struct DeviceBuffer {
    void *p = nullptr;
    uint64_t bytes = 0;
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    ~DeviceBuffer() { release(); }  // (msj_ctx_destroy has selected the context's device)
    // need <= bytes: nothing.  Otherwise the device is synchronised, the old block freed and need (headroom: + need / 4, so
    // that calls of similar size do not re-allocate) bytes allocated; false, and the buffer empty, when that fails
    bool reserve(uint64_t need, bool headroom) {
        if (need <= bytes) return true;
        release();
        const uint64_t want = headroom ? need + need / 4 : need;
        if (!hip_ok(hipMalloc(&p, want))) {
            p = nullptr;
            return false;
        }
        bytes = want;
        return true;
    }
    void release() {
        if (p) {
            (void)hipDeviceSynchronize();  // nothing of ours may still be using the block
            (void)hipFree(p);
        }
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T *as() const { return static_cast<T *>(p); }
};

// from here on msj_stage1 stages through pinned rings in chunks (host_pipeline)
constexpr uint64_t kPipelineMinDefault = 64u << 20;  // (below that plain staging is as fast or faster; test hook: msj_debug_set_pipeline_min_bytes)

struct HostPipe;  // pinned rings, streams and copy workers of the host-pointer entry point (host_pipe.cpp)

struct msj_ctx {
    int device = 0;
    HostPipe *pipe = nullptr;     // created by the first large msj_stage1 call
    // Two workspace buffers (tickets + descriptors) used alternately.  A launch needs its
    // buffer zeroed; instead of a memset in front of every launch, each launch zeroes the
    // OTHER buffer word for word when that one was dirtied with the same layout (same ntiles).
    DeviceBuffer ws;
    uint64_t ws_words = 0;        // words per buffer
    uint32_t ws_toggle = 0;
    uint32_t ws_dirty[2] = {0, 0}; // ntiles of the launch that last used the buffer; 0 = clean, ~0 = all of it
    msj_carry *carries = nullptr; // [0] = zero carry, [1..] chained segment carries
    uint32_t n_carries = 0;
    DeviceBuffer d_in, d_idx;     // staging for the host-pointer entry points
    msj_carry *d_result = nullptr;
    uint8_t *h_pin = nullptr;     // pinned host staging of the small-input path of msj_stage1 (kPinBytes)
    uint8_t *d_small = nullptr;   // ... and the msj_carry of that path (device memory: the kernel updates it with atomics)
    uint32_t grid = 0;            // persistent workgroups per launch (CUs x resident blocks per CU)
    uint32_t wait_ticks = msj::kWaitTicksDefault;  // bound of the kernel's waits (10 ns ticks)
    uint64_t seg_bytes = msj::kSegmentBytes;  // longest segment of one launch (test hook: msj_debug_set_segment_bytes)
    uint64_t pipeline_min = kPipelineMinDefault;  // host-pointer inputs from this size on take the chunked pipeline
    bool pipe_unavailable = false;  // the pipeline's pinned memory / streams could not be had: plain staging from then on
    bool pipe_fail_setup = false;   // test hook: msj_debug_fail_pipeline_setup
    DeviceBuffer tp;              // workspace of the two-pass path (2 words per tile), allocated on first use
    uint64_t fallbacks = 0;       // calls re-issued through the two-pass path after an expired wait
    // the last shard call, so that msj_carry_fetch can re-issue it (one in-flight call per context)
    struct {
        bool valid = false;
        const uint8_t *d_buf; uint64_t len; uint32_t *d_idx; uint64_t idx_capacity;
        const msj_carry *d_carry_in; msj_carry *d_carry_out; msj_segment *d_segments; uint32_t max_segments;
        bool has_prefix, is_final, no_emit; uint64_t trailer_len; hipStream_t stream; uint32_t flags;
        bool by_value; uint32_t carry_bits;  // msj_stage1_shard_device_cv
    } last;
    struct HostRange { const uint8_t *base; uint64_t bytes; };
    std::vector<HostRange> pinned;  // msj_host_register: caller-owned host ranges the DMA engines can reach directly
    bool is_pinned(const void *p, uint64_t n) const {
        const uint8_t *q = static_cast<const uint8_t *>(p);
        for (const HostRange &r : pinned)
            if (q >= r.base && n <= r.bytes && (uint64_t)(q - r.base) <= r.bytes - n) return true;
        return false;
    }
    DeviceBuffer span_fix;        // work list of the span kernel's fix-up pass (tokens_kernel.hip), allocated and zeroed once
    DeviceBuffer tok_ws;          // block aggregates of the token pre-pass
    uint64_t tok_doc_n = ~0ull;   // the token count whose document aggregates tok_ws holds (~0: none)
    DeviceBuffer seg_idx;         // msj_stage2_prep_segments: 16-byte aligned copy of a segment's index slice that is not aligned
    uint8_t *types_out = nullptr; // msj_stage1_types_device (prototype): where the launch being enqueued writes the type bytes
    DeviceBuffer resid;           // msj_stage2_prep_segments with d_match: MSJ_RESID_WORDS per segment (the brackets a segment could not pair)
    msj_token_opts tok_opts;      // test hooks of the token calls (msj_debug_set_span_limits / _span_mode): per context
    DeviceBuffer doc_ws;          // block counts of the document split
    DeviceBuffer num_ws;          // msj_number_values_device: block counts / offsets, the fallback and long-number lists
    DeviceBuffer val_ws;          // msj_validate_device: the call's state, the lists of long and huge escaped strings
    DeviceBuffer vdoc_ws;         // msj_validate_documents_device: the same for a window (the documents' error words live in d_verdicts)
    DeviceBuffer tape_ws;         // msj_tape_device: pos[], element counts, block sums, the table of long strings
    DeviceBuffer tdoc_ws;         // msj_tape_documents_device: the same for a window, and 8 bytes per document
    DeviceBuffer sel_ws;          // msj_select_documents_device: two state words per (path, document)
    DeviceBuffer scol_ws;         // msj_string_column_device: the counts, a sum per block of rows, a length per row
    DeviceBuffer acol_ws;         // msj_array_column_device: the counts, a descriptor per row, a count per block of tokens
    DeviceBuffer selem_ws;        // msj_select_elements_device: two state words per (path, row), a start token per row
    DeviceBuffer aelem_ws;        // msj_array_elements_device: the state, a word and a start token per row, a descriptor and an offset per dense row, the block counts
    DeviceBuffer oent_ws;         // msj_object_entries_device: the same state and arrays (rows_block.h)
    DeviceBuffer rcol_ws;         // msj_raw_column_device: lengths per row, the list of long rows, P per token (compact)
    DeviceBuffer dict_ws;         // msj_dictionary_device: a hash and a slot per row, the table of rows, the block sums, the list of long rows
    DeviceBuffer dictx_ws;        // msj_dictionary_extend_device: the same per ITEM (prior entries + rows), the table of items
    DeviceBuffer frow_ws;         // msj_filter_rows_device: the counters, a count per block of rows, a rank per row
    DeviceBuffer take_ws;         // msj_take_rows_device: the counters
    DeviceBuffer cast_ws;         // msj_cast_strings_device: the counters, the list of the rows the lane path leaves over
    uint32_t cast_fetch = 0;      // msj_debug_set_cast_fetch: MSJ_CAST_FETCH_*
    DeviceBuffer agg_ws;          // msj_aggregate_device: the counters, the accumulators of every (column, group)
    uint32_t agg_lds_groups = kAggregateMaxLdsGroups;  // msj_debug_set_aggregate_limits: the most groups the LDS path takes
    DeviceBuffer sort_ws;         // msj_sort_rows_device: the state and the plan, two buffers of two key words per row, the tiles' bucket counts
    DeviceBuffer join_ws;         // msj_join_rows_device: the counters, count / start per key, two buffers of (key, row) per right row, a run and an offset per left row
    DeviceBuffer order_ws;        // msj_dictionary_order_device: the counters, and per entry the tied entries' keys, entries and places twice over
    DeviceBuffer match_ws;        // msj_match_strings_device: the state, per (pattern, row) the word the places compete on and the cursor
    DeviceBuffer bucket_ws;       // msj_bucket_rows_device: the counters
    DeviceBuffer gkeys_ws;        // msj_group_keys_device: the counters
    uint32_t order_mode = 0;      // msj_debug_set_order_mode: 0 the path by capacity, 1 always the grid path, 2 the one-workgroup path wherever it fits
    uint32_t sort_mode = 0;       // msj_debug_set_sort_mode: 0 chosen on the device, 1 always the full sort, 2 always the selection
};

// ---- api.cpp ----
// Enqueue the kernels for one shard: a chain of <= kSegmentBytes launches whose carry structs stay in device memory
int32_t enqueue_shard(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, uint32_t *d_idx, uint64_t idx_capacity,
                      const msj_carry *d_carry_in, msj_carry *d_carry_out, msj_segment *d_segments, uint32_t max_segments,
                      uint32_t *n_segments_out, bool has_prefix, bool is_final, bool no_emit, uint64_t trailer_len, hipStream_t stream,
                      uint32_t flags, uint32_t index_bias = 0, const uint32_t *carry_bits = nullptr);
extern std::mutex g_default_mutex;  // guards the default context (the entry points that take ctx == NULL)
msj_ctx *default_ctx_locked();      // g_default_mutex held; null without a device

// ---- host_pipe.cpp ----
// The pipelined form of msj_stage1_ctx's device staging.  Returns kPipeUnavailable when the machinery cannot be
// set up (pinned memory, streams, events: e.g. a memlock limit in a container) -- nothing has been enqueued then
// and the caller takes the plain path, for this call and every later one; any other failure is the call's
// result.  Otherwise fills *res with the final carry.
constexpr int32_t kPipeUnavailable = -100;
int32_t host_pipeline(msj_ctx *ctx, const uint8_t *buf, uint64_t len, uint32_t *idx_out, uint64_t dev_cap, uint32_t flags, msj_carry *res);
void host_pipe_destroy(HostPipe *pipe);
bool knob_set(const char *name);  // measurement build (-DMSJ_DEBUG_KNOBS): the environment variable is set; else false

#pragma GCC visibility pop
