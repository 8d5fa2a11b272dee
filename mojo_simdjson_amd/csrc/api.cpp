// api.cpp -- extern "C" entry points declared in include/msj_stage1.h: the context and stage 1.  (The pinned-ring
// pipeline of the host-pointer entry point is host_pipe.cpp, the device calls behind stage 1 are stage2_api.cpp.)
//
// Host-side counterpart of DomParserImplementation.stage1 / allocate
// (src/mojo_simdjson/include/generic/dom_parser_implementation.mojo:59-69,85-89):
// argument checks, workspace management and kernel launches.  There is no CPU
// implementation behind this ABI: without a usable HIP device every entry
// point returns MSJ_ERR_NO_DEVICE.
#include <cstring>
#include <new>

#include "ctx.h"

// small-input path of msj_stage1: input, result and len + 3 indices fit the pinned staging buffer, which the kernel
// reads and writes itself over PCIe (no DMA calls; measured against staged copies: 77 B 24 -> 22 us, 13 KB 33 -> 23,
// 62 KB 45 -> 30, 258 KB 76 -> 42, 1 MB 136 -> 104; 4 MB 242 -> 371, hence the limit)
constexpr uint64_t kSmallInput = 1u << 20;
constexpr uint64_t kPinBytes = kSmallInput + 64 + (kSmallInput + 3) * sizeof(uint32_t) + 64;

static_assert(sizeof(msj_carry) == 64, "the small-input staging layout assumes a 64-byte carry");

namespace {

uint64_t *g_stamps = nullptr;  // diagnostic builds (-DMSJ_STAMPS) only: msj_debug_set_stamps
constexpr uint32_t kMaxChain = 64;  // segments per shard call (64 x ~4 GiB)

constexpr uint32_t kAllDirty = 0xFFFFFFFFu;

int32_t ensure_workspace(msj_ctx *ctx, uint32_t ntiles) {
    const uint64_t need = msj::workspace_words(ntiles);
    if (need <= ctx->ws_words) return MSJ_SUCCESS;
    ctx->ws_words = 0;
    // grow with head-room so repeated calls of similar size do not re-allocate (its own rounding, hence none of the buffer's)
    const uint64_t words = (need + need / 4 + 64 + 511) & ~511ull;
    if (!ctx->ws.reserve(2 * words * sizeof(uint64_t), false)) return MSJ_MEMALLOC;
    ctx->ws_words = words;
    ctx->ws_toggle = 0;
    ctx->ws_dirty[0] = ctx->ws_dirty[1] = kAllDirty;  // fresh memory: zeroed before first use
    return MSJ_SUCCESS;
}

// Zero what a previous launch (or nothing known) left in workspace buffer b.
bool scrub(msj_ctx *ctx, uint32_t b, hipStream_t stream) {
    const uint32_t d = ctx->ws_dirty[b];
    if (d == 0) return true;
    const uint64_t words = (d == kAllDirty) ? ctx->ws_words : msj::workspace_words(d);
    if (!hip_ok(hipMemsetAsync(ctx->ws.as<uint64_t>() + (uint64_t)b * ctx->ws_words, 0, words * sizeof(uint64_t), stream)))
        return false;
    ctx->ws_dirty[b] = 0;
    return true;
}

}  // namespace

// Enqueue the kernels for one shard: a chain of <= kSegmentBytes launches whose
// carry structs stay in device memory (no host synchronisation in between).
int32_t enqueue_shard(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, uint32_t *d_idx,
                      uint64_t idx_capacity, const msj_carry *d_carry_in, msj_carry *d_carry_out,
                      msj_segment *d_segments, uint32_t max_segments, uint32_t *n_segments_out,
                      bool has_prefix, bool is_final, bool no_emit, uint64_t trailer_len,
                      hipStream_t stream, uint32_t flags, uint32_t index_bias, const uint32_t *carry_bits) {
    // carry_bits: the state at the shard's first byte by value (bit 0 in_string, 1 next_is_escaped, 2 prev_scalar;
    // counts and sticky flags zero) instead of d_carry_in
    if (!ctx || !d_buf || (!d_carry_in && !carry_bits) || !d_carry_out || len == 0) return MSJ_ERR_BAD_ARGUMENT;
    if (!aligned(d_buf, 16)) return MSJ_ERR_BAD_ARGUMENT;
    if (!no_emit && !d_idx) return MSJ_ERR_BAD_ARGUMENT;
    if (!aligned(d_idx, 16)) return MSJ_ERR_BAD_ARGUMENT;  // 16-B stores
    const uint64_t seg_bytes = ctx->seg_bytes;
    const uint64_t nseg = (len + seg_bytes - 1) / seg_bytes;
    if (nseg > kMaxChain) return MSJ_CAPACITY;
    if (d_segments && nseg > max_segments) return MSJ_CAPACITY;
    if (!hip_ok(hipSetDevice(ctx->device))) return MSJ_ERR_HIP;
    ctx->last.valid = true;
    ctx->last.d_buf = d_buf; ctx->last.len = len; ctx->last.d_idx = d_idx; ctx->last.idx_capacity = idx_capacity;
    ctx->last.d_carry_in = d_carry_in; ctx->last.d_carry_out = d_carry_out; ctx->last.d_segments = d_segments;
    ctx->last.max_segments = max_segments; ctx->last.has_prefix = has_prefix; ctx->last.is_final = is_final;
    ctx->last.no_emit = no_emit; ctx->last.trailer_len = trailer_len; ctx->last.stream = stream; ctx->last.flags = flags;
    ctx->last.by_value = carry_bits != nullptr; ctx->last.carry_bits = carry_bits ? *carry_bits : 0u;

    const uint64_t first_len = len < seg_bytes ? len : seg_bytes;
    const uint32_t max_tiles = (uint32_t)((first_len + msj::kTileBytes - 1) / msj::kTileBytes);
    int32_t rc = ensure_workspace(ctx, max_tiles);
    if (rc != MSJ_SUCCESS) return rc;

    for (uint64_t s = 0; s < nseg; s++) {
        const uint64_t base = s * seg_bytes;
        const uint64_t seg_len = (len - base) < seg_bytes ? (len - base) : seg_bytes;
        msj::KernelArgs a;
        a.buf = d_buf + base;
        a.len = seg_len;
        a.idx = d_idx;
        a.capacity = idx_capacity;
        const uint32_t wb = ctx->ws_toggle, wo = wb ^ 1u;
        uint64_t *const ws = ctx->ws.as<uint64_t>();
        a.ws = ws + (uint64_t)wb * ctx->ws_words;
        a.carry_in = (s == 0) ? d_carry_in : &ctx->carries[s];
        a.carry_bits = 0;
        a.reserved0 = 0;
        a.carry_out = (s + 1 == nseg) ? d_carry_out : &ctx->carries[s + 1];
        a.segment = d_segments ? &d_segments[s] : nullptr;
        a.segment_byte_base = base;
        a.trailer_len = trailer_len;
        a.ntiles = (uint32_t)((seg_len + msj::kTileBytes - 1) / msj::kTileBytes);
        a.flags = flags & (msj::kFlagStrictUtf8 | msj::kFlagNoUtf8);
        if (is_final && s + 1 == nseg) a.flags |= msj::kFlagFinal;
        if (has_prefix || s > 0) a.flags |= msj::kFlagHasPrefix;
        if (no_emit) a.flags |= msj::kFlagNoEmit;
        if (s == 0) a.flags |= flags & (15u << msj::kFlagSkipShift);
        if (s > 0) a.flags |= msj::kFlagEchoThrough;
        if (s == 0 && carry_bits) {
            a.flags |= msj::kFlagCarryByValue;
            a.carry_bits = *carry_bits & 7u;
            a.carry_in = nullptr;
        }
        a.stamps = g_stamps;
        a.types = ctx->types_out;
        if (a.types) a.flags |= msj::kFlagEmitTypes;
        a.wait_ticks = ctx->wait_ticks;
        // without a segment table nothing tells the caller where a later segment's offsets start: they stay
        // relative to the call's buffer (wrapping like the reference's UInt32 would, json_structural_indexer.mojo:138)
        a.index_bias = index_bias + (d_segments ? 0u : (uint32_t)base);
        a.tp = nullptr;
        if (flags & MSJ_FLAG_DEBUG_STALL) a.flags |= msj::kFlagDebugStall;
        if (flags & MSJ_FLAG_TWO_PASS) {
            // three plain kernels, no inter-workgroup waiting, own workspace (need not be zeroed)
            if (!ctx->tp.reserve(2ull * max_tiles * sizeof(uint64_t), false)) return MSJ_MEMALLOC;
            a.tp = ctx->tp.as<uint64_t>();
            a.ws = nullptr;
            a.ws_clean = nullptr;
            if (msj_launch_stage1_twopass(&a, stream) != 0) return MSJ_ERR_HIP;
            continue;
        }
        // ticket + descriptors must read as "not ready" at launch: this launch's buffer is clean
        // already in the steady state; the other one is cleaned by this launch if its dirt has
        // this launch's layout, by a memset otherwise
        a.ws_clean = nullptr;
        if (ctx->ws_dirty[wo] == a.ntiles) a.ws_clean = ws + (uint64_t)wo * ctx->ws_words;
        if (!scrub(ctx, wb, stream) || (!a.ws_clean && !scrub(ctx, wo, stream))) {
            ctx->ws_dirty[0] = ctx->ws_dirty[1] = kAllDirty;
            return MSJ_ERR_HIP;
        }
        // (Tried in round 3: a grid sized so that every workgroup gets the same number of ranges -- 993 x 33 instead of
        // 1 023 workers with 31 stragglers in a 33rd round at 1 GiB -- loses 3-4 %: 30 empty workgroup slots cost more
        // than the stragglers' ~5 us.  The grid fills every CU.)
        if (msj_launch_stage1(&a, stream, ctx->grid) != 0) {
            ctx->ws_dirty[0] = ctx->ws_dirty[1] = kAllDirty;
            return MSJ_ERR_HIP;
        }
        ctx->ws_dirty[wb] = a.ntiles;
        ctx->ws_dirty[wo] = 0;
        ctx->ws_toggle = wo;
    }
    if (n_segments_out) *n_segments_out = (uint32_t)nseg;
    return MSJ_SUCCESS;
}
std::mutex g_default_mutex;
static msj_ctx *g_default_ctx = nullptr;
msj_ctx *default_ctx_locked() {  // g_default_mutex held
    if (!g_default_ctx && msj_ctx_create(0, &g_default_ctx) != MSJ_SUCCESS) return nullptr;
    return g_default_ctx;
}

extern "C" {

#ifndef MSJ_SOURCE_HASH
#define MSJ_SOURCE_HASH "unknown"
#endif
// "... src:<hash>": the first 12 hex digits of the SHA-256 of the stage-1 kernel's sources (csrc/Makefile), so that
// measurements kept beside the code (profiles/traffic.json) can say which kernel they were taken with
const char *msj_version(void) { return "mojo-simdjson_amd stage1 0.4 (gfx950) src:" MSJ_SOURCE_HASH; }

uint32_t msj_tile_bytes(void) { return msj::kTileBytes; }

int32_t msj_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int32_t msj_ctx_create(int32_t device, msj_ctx **out) {
    if (!out) return MSJ_ERR_BAD_ARGUMENT;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return MSJ_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return MSJ_ERR_BAD_ARGUMENT;
    if (!hip_ok(hipSetDevice(device))) return MSJ_ERR_HIP;
    msj_ctx *ctx = new (std::nothrow) msj_ctx();
    if (!ctx) return MSJ_MEMALLOC;
    ctx->device = device;
    {
        // persistent grid: fill every CU to the kernel's occupancy
        hipDeviceProp_t prop;
        int per_cu = 0;
        if (hip_ok(hipGetDeviceProperties(&prop, device)) && msj_stage1_occupancy(&per_cu) == 0 &&
            per_cu > 0)
            ctx->grid = (uint32_t)prop.multiProcessorCount * (uint32_t)per_cu;
        else
            ctx->grid = 1024;
    }
    ctx->n_carries = kMaxChain + 2;
    if (!hip_ok(hipMalloc(reinterpret_cast<void **>(&ctx->carries),
                          ctx->n_carries * sizeof(msj_carry))) ||
        !hip_ok(hipMemset(ctx->carries, 0, ctx->n_carries * sizeof(msj_carry))) ||
        !hip_ok(hipMalloc(reinterpret_cast<void **>(&ctx->d_result), sizeof(msj_carry)))) {
        msj_ctx_destroy(ctx);
        return MSJ_MEMALLOC;
    }
    *out = ctx;
    return MSJ_SUCCESS;
}

int32_t msj_ctx_device(const msj_ctx *ctx) { return ctx ? ctx->device : -1; }

void msj_ctx_destroy(msj_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->carries) (void)hipFree(ctx->carries);
    if (ctx->d_result) (void)hipFree(ctx->d_result);
    host_pipe_destroy(ctx->pipe);
    for (const msj_ctx::HostRange &r : ctx->pinned) (void)hipHostUnregister(const_cast<uint8_t *>(r.base));
    if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
    if (ctx->d_small) (void)hipFree(ctx->d_small);
    delete ctx;  // (every DeviceBuffer member releases itself)
}

int32_t msj_stage1_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, uint32_t *d_idx,
                          uint64_t idx_capacity, msj_carry *d_result, void *stream,
                          uint32_t flags) {
    if (!ctx || !d_result) return MSJ_ERR_BAD_ARGUMENT;
    if (len == 0) return MSJ_EMPTY;  // json_structural_indexer.mojo:91-92
    if (len > MSJ_MAX_SEGMENT_BYTES) return MSJ_CAPACITY;  // include/base.mojo:2
    // carries[0] is the all-zero state at the start of a document (:74-79)
    return enqueue_shard(ctx, d_buf, len, d_idx, idx_capacity, &ctx->carries[0], d_result, nullptr,
                         0, nullptr, false, true, false, len, static_cast<hipStream_t>(stream),
                         flags);
}

int32_t msj_stage1_shard_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, uint32_t *d_idx,
                                uint64_t idx_capacity, const msj_carry *d_carry_in,
                                msj_carry *d_carry_out, msj_segment *d_segments,
                                uint32_t max_segments, uint32_t *n_segments_out,
                                int32_t has_prefix, int32_t is_final, int32_t no_emit,
                                uint64_t trailer_len, void *stream, uint32_t flags) {
    return enqueue_shard(ctx, d_buf, len, d_idx, idx_capacity, d_carry_in, d_carry_out, d_segments,
                         max_segments, n_segments_out, has_prefix != 0, is_final != 0, no_emit != 0,
                         trailer_len, static_cast<hipStream_t>(stream), flags);
}

int32_t msj_stage1_shard_device_cv(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, uint32_t *d_idx,
                                   uint64_t idx_capacity, uint32_t carry_bits, msj_carry *d_carry_out,
                                   msj_segment *d_segments, uint32_t max_segments, uint32_t *n_segments_out,
                                   int32_t has_prefix, int32_t is_final, int32_t no_emit, uint64_t trailer_len,
                                   void *stream, uint32_t flags) {
    if (carry_bits > 7u) return MSJ_ERR_BAD_ARGUMENT;
    return enqueue_shard(ctx, d_buf, len, d_idx, idx_capacity, nullptr, d_carry_out, d_segments, max_segments,
                         n_segments_out, has_prefix != 0, is_final != 0, no_emit != 0, trailer_len,
                         static_cast<hipStream_t>(stream), flags, 0, &carry_bits);
}

int32_t msj_device_alloc(msj_ctx *ctx, uint64_t bytes, void **d_out) {
    if (!ctx || !d_out) return MSJ_ERR_BAD_ARGUMENT;
    *d_out = nullptr;
    if (!hip_ok(hipSetDevice(ctx->device))) return MSJ_ERR_HIP;
    return hip_ok(hipMalloc(d_out, bytes ? bytes : 1)) ? MSJ_SUCCESS : MSJ_MEMALLOC;
}

int32_t msj_device_free(msj_ctx *ctx, void *d_ptr) {
    if (!ctx) return MSJ_ERR_BAD_ARGUMENT;
    if (!d_ptr) return MSJ_SUCCESS;
    if (!hip_ok(hipSetDevice(ctx->device))) return MSJ_ERR_HIP;
    return hip_ok(hipFree(d_ptr)) ? MSJ_SUCCESS : MSJ_ERR_HIP;
}

static int32_t blocking_copy(msj_ctx *ctx, void *dst, const void *src, uint64_t bytes, void *stream, hipMemcpyKind kind) {
    if (!ctx || (bytes && (!dst || !src))) return MSJ_ERR_BAD_ARGUMENT;
    if (bytes == 0) return MSJ_SUCCESS;
    if (!hip_ok(hipSetDevice(ctx->device))) return MSJ_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!hip_ok(hipMemcpyAsync(dst, src, bytes, kind, s))) return MSJ_ERR_HIP;
    return hip_ok(hipStreamSynchronize(s)) ? MSJ_SUCCESS : MSJ_ERR_HIP;
}

int32_t msj_copy_to_device(msj_ctx *ctx, void *d_dst, const void *src, uint64_t bytes, void *stream) {
    return blocking_copy(ctx, d_dst, src, bytes, stream, hipMemcpyHostToDevice);
}

int32_t msj_copy_to_host(msj_ctx *ctx, void *dst, const void *d_src, uint64_t bytes, void *stream) {
    return blocking_copy(ctx, dst, d_src, bytes, stream, hipMemcpyDeviceToHost);
}

int32_t msj_carry_fetch(msj_ctx *ctx, const msj_carry *d_carry, msj_carry *host_out, void *stream) {
    if (!ctx || !d_carry || !host_out) return MSJ_ERR_BAD_ARGUMENT;
    if (!hip_ok(hipSetDevice(ctx->device))) return MSJ_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!hip_ok(hipMemcpyAsync(host_out, d_carry, sizeof(msj_carry), hipMemcpyDeviceToHost, s)))
        return MSJ_ERR_HIP;
    if (!hip_ok(hipStreamSynchronize(s))) return MSJ_ERR_HIP;
    if (host_out->internal_error && ctx->last.valid && ctx->last.d_carry_out == d_carry &&
        !(ctx->last.flags & MSJ_FLAG_TWO_PASS)) {
        // a wait inside the single-pass kernel ran into its bound (a starved GPU, a stalled resolver): the
        // result is poisoned.  Run the call again through the two-pass kernels, which wait for nothing.
        const auto L = ctx->last;
        ctx->fallbacks++;
        ctx->ws_dirty[0] = ctx->ws_dirty[1] = kAllDirty;  // the poisoned launch may have left anything behind
        const int32_t rc = enqueue_shard(ctx, L.d_buf, L.len, L.d_idx, L.idx_capacity, L.d_carry_in, L.d_carry_out,
                                         L.d_segments, L.max_segments, nullptr, L.has_prefix, L.is_final, L.no_emit,
                                         L.trailer_len, L.stream, L.flags | MSJ_FLAG_TWO_PASS, 0,
                                         L.by_value ? &L.carry_bits : nullptr);
        if (rc != MSJ_SUCCESS) return rc;
        if (!hip_ok(hipStreamSynchronize(L.stream))) return MSJ_ERR_HIP;
        if (!hip_ok(hipMemcpyAsync(host_out, d_carry, sizeof(msj_carry), hipMemcpyDeviceToHost, s)) ||
            !hip_ok(hipStreamSynchronize(s)))
            return MSJ_ERR_HIP;
    }
    return MSJ_SUCCESS;
}

int32_t msj_debug_set_wait_ticks(msj_ctx *ctx, uint32_t ticks) {
    if (!ctx) return MSJ_ERR_BAD_ARGUMENT;
    ctx->wait_ticks = ticks;
    return MSJ_SUCCESS;
}

int32_t msj_host_register(msj_ctx *ctx, void *ptr, uint64_t bytes) {
    if (!ptr || bytes == 0) return MSJ_ERR_BAD_ARGUMENT;
    std::unique_lock<std::mutex> lock(g_default_mutex, std::defer_lock);
    if (!ctx) {
        lock.lock();
        ctx = default_ctx_locked();
        if (!ctx) return MSJ_ERR_NO_DEVICE;
    }
    if (!hip_ok(hipSetDevice(ctx->device))) return MSJ_ERR_HIP;
    if (!hip_ok(hipHostRegister(ptr, bytes, hipHostRegisterDefault))) {
        (void)hipGetLastError();
        return MSJ_ERR_HIP;
    }
    ctx->pinned.push_back({static_cast<const uint8_t *>(ptr), bytes});
    return MSJ_SUCCESS;
}

int32_t msj_host_unregister(msj_ctx *ctx, void *ptr) {
    if (!ptr) return MSJ_ERR_BAD_ARGUMENT;
    std::unique_lock<std::mutex> lock(g_default_mutex, std::defer_lock);
    if (!ctx) {
        lock.lock();
        ctx = g_default_ctx;
        if (!ctx) return MSJ_ERR_BAD_ARGUMENT;
    }
    for (size_t i = 0; i < ctx->pinned.size(); i++)
        if (ctx->pinned[i].base == ptr) {
            ctx->pinned.erase(ctx->pinned.begin() + (long)i);
            (void)hipSetDevice(ctx->device);
            (void)hipDeviceSynchronize();  // nothing of ours may still be moving bytes of the range
            return hip_ok(hipHostUnregister(ptr)) ? MSJ_SUCCESS : MSJ_ERR_HIP;
        }
    return MSJ_ERR_BAD_ARGUMENT;
}

uint64_t msj_fallback_count(const msj_ctx *ctx) { return ctx ? ctx->fallbacks : 0; }

int32_t msj_debug_set_pipeline_min_bytes(msj_ctx *ctx, uint64_t bytes) {
    std::unique_lock<std::mutex> lock(g_default_mutex, std::defer_lock);
    if (!ctx) {
        lock.lock();
        ctx = default_ctx_locked();
        if (!ctx) return MSJ_ERR_NO_DEVICE;
    }
    ctx->pipeline_min = bytes ? bytes : kPipelineMinDefault;
    return MSJ_SUCCESS;
}

int32_t msj_debug_fail_pipeline_setup(msj_ctx *ctx, int32_t on) {
    std::unique_lock<std::mutex> lock(g_default_mutex, std::defer_lock);
    if (!ctx) {
        lock.lock();
        ctx = default_ctx_locked();
        if (!ctx) return MSJ_ERR_NO_DEVICE;
    }
    ctx->pipe_fail_setup = on != 0;
    if (!on) ctx->pipe_unavailable = false;
    return ctx->pipe_unavailable ? 1 : 0;
}

int32_t msj_debug_set_segment_bytes(msj_ctx *ctx, uint64_t bytes) {
    if (!ctx || bytes == 0 || bytes % msj::kTileBytes != 0 || bytes > msj::kSegmentBytes) return MSJ_ERR_BAD_ARGUMENT;
    ctx->seg_bytes = bytes;
    return MSJ_SUCCESS;
}

int32_t msj_stage1_ctx(msj_ctx *ctx, const uint8_t *buf, uint64_t len, uint32_t *idx_out,
                       uint64_t idx_capacity, uint64_t *n_out, int32_t *utf8_verdict_out,
                       uint32_t flags) {
    if (!ctx) return MSJ_ERR_BAD_ARGUMENT;
    if (len == 0) return MSJ_EMPTY;  // json_structural_indexer.mojo:91-92
    if (!buf || !idx_out || !n_out) return MSJ_ERR_BAD_ARGUMENT;
    if (len > MSJ_MAX_SEGMENT_BYTES) return MSJ_CAPACITY;
    if (!hip_ok(hipSetDevice(ctx->device))) return MSJ_ERR_HIP;

    // Small inputs: latency, not bandwidth.  Through pinned staging everything is enqueued at once -- input up,
    // kernel, result and ALL len + 3 index slots down in one copy (n is not known yet; 4 bytes per input byte
    // is cheap at this size) -- and the host waits once instead of three times (pageable copies are synchronous).
    if (len <= kSmallInput && idx_capacity >= len + 3) {
        if (!ctx->h_pin && !hip_ok(hipHostMalloc(reinterpret_cast<void **>(&ctx->h_pin), kPinBytes, hipHostMallocDefault))) ctx->h_pin = nullptr;
        if (!ctx->d_small && !hip_ok(hipMalloc(reinterpret_cast<void **>(&ctx->d_small), sizeof(msj_carry)))) ctx->d_small = nullptr;
    }
    if (len <= kSmallInput && idx_capacity >= len + 3 && ctx->h_pin && ctx->d_small) {
        // pinned: [0, kSmallInput): input | [kSmallInput, +64): msj_carry | then len + 3 indices.  The kernel reads the
        // input from there and writes the indices there; the 64-byte result lives in device memory (the kernel
        // updates it with atomics) and comes down by the one copy of the call
        std::memcpy(ctx->h_pin, buf, len);
        msj_carry *d_res = reinterpret_cast<msj_carry *>(ctx->d_small);
        uint32_t *h_ix = reinterpret_cast<uint32_t *>(ctx->h_pin + kSmallInput + 64);
        int32_t rc = msj_stage1_device(ctx, ctx->h_pin, len, h_ix, len + 3, d_res, nullptr, flags);
        if (rc != MSJ_SUCCESS) return rc;
        if (!hip_ok(hipMemcpyAsync(ctx->h_pin + kSmallInput, d_res, sizeof(msj_carry), hipMemcpyDeviceToHost, nullptr)) ||
            !hip_ok(hipStreamSynchronize(nullptr)))
            return MSJ_ERR_HIP;
        const msj_carry res = *reinterpret_cast<const msj_carry *>(ctx->h_pin + kSmallInput);
        if (res.internal_error && !(flags & MSJ_FLAG_TWO_PASS)) {
            // an expired wait in the single-pass kernel: once more through the two-pass kernels
            ctx->fallbacks++;
            ctx->ws_dirty[0] = ctx->ws_dirty[1] = kAllDirty;
            return msj_stage1_ctx(ctx, buf, len, idx_out, idx_capacity, n_out, utf8_verdict_out, flags | MSJ_FLAG_TWO_PASS);
        }
        if (utf8_verdict_out) *utf8_verdict_out = res.utf8_error ? MSJ_UTF8_ERROR : MSJ_SUCCESS;
        if (res.code == MSJ_UNCLOSED_STRING || res.code == MSJ_UNESCAPED_CHARS || res.code == MSJ_UNEXPECTED_ERROR ||
            res.code == MSJ_CAPACITY)
            return res.code;  // the reference returns before it sets n or the trailer (:151-158)
        std::memcpy(idx_out, ctx->h_pin + kSmallInput + 64, (res.count + 3) * sizeof(uint32_t));
        *n_out = res.count;
        return res.code;
    }
    // device staging (the reference's allocate(len), dom_parser_implementation.mojo:85-89)
    if (!ctx->d_in.reserve((len + 63u) & ~63ull, false)) return MSJ_MEMALLOC;
    const uint64_t dev_cap = idx_capacity < len + 3 ? idx_capacity : len + 3;
    if (!ctx->d_idx.reserve(dev_cap * sizeof(uint32_t), false)) return MSJ_MEMALLOC;
    uint8_t *const d_in = ctx->d_in.as<uint8_t>();
    uint32_t *const d_idx = ctx->d_idx.as<uint32_t>();
    msj_carry res;
    int32_t rc;
    static const bool pipe_off = knob_set("MSJ_PIPE_DISABLE");  // measurement build: the plain staging path
    bool piped = len >= ctx->pipeline_min && !(flags & MSJ_FLAG_TWO_PASS) && !pipe_off && !ctx->pipe_unavailable;
    if (piped) {
        // large inputs: pinned rings, chunks, both PCIe directions and the kernel at once
        try {
            rc = host_pipeline(ctx, buf, len, idx_out, dev_cap, flags, &res);
        } catch (...) {  // std::thread / std::vector could not get what they need: nothing of ours crosses the C boundary
            rc = MSJ_MEMALLOC;
        }
        if (rc == kPipeUnavailable) {
            // the machinery cannot be had on this host: the plain staging path below, now and from now on
            (void)hipGetLastError();
            ctx->pipe_unavailable = true;
            piped = false;
        } else if (rc != MSJ_SUCCESS) {
            return rc;
        }
    }
    if (piped) {
        if (res.internal_error) {  // an expired wait somewhere in the chain: once more, two-pass, plain staging
            ctx->fallbacks++;
            ctx->ws_dirty[0] = ctx->ws_dirty[1] = kAllDirty;
            return msj_stage1_ctx(ctx, buf, len, idx_out, idx_capacity, n_out, utf8_verdict_out, flags | MSJ_FLAG_TWO_PASS);
        }
    } else {
        if (!hip_ok(hipMemcpy(d_in, buf, len, hipMemcpyHostToDevice))) return MSJ_ERR_HIP;
        rc = msj_stage1_device(ctx, d_in, len, d_idx, dev_cap, ctx->d_result, nullptr, flags);
        if (rc != MSJ_SUCCESS) return rc;
        rc = msj_carry_fetch(ctx, ctx->d_result, &res, nullptr);
        if (rc != MSJ_SUCCESS) return rc;
    }
    if (utf8_verdict_out) *utf8_verdict_out = res.utf8_error ? MSJ_UTF8_ERROR : MSJ_SUCCESS;
    // On UNCLOSED_STRING / UNESCAPED_CHARS the reference returns before it sets
    // n_structural_indexes or the trailer (json_structural_indexer.mojo:151-158).
    if (res.code == MSJ_UNCLOSED_STRING || res.code == MSJ_UNESCAPED_CHARS ||
        res.code == MSJ_UNEXPECTED_ERROR || res.code == MSJ_CAPACITY) {
        // The pipeline has brought down what its chunks found before the code was known: the indices, clipped to the
        // capacity, and no trailer.  Plain staging leaves the caller the same words (tests/test_host_pointer_borders.py)
        const uint64_t have = res.count < dev_cap ? res.count : dev_cap;
        if (!piped && have && !hip_ok(hipMemcpy(idx_out, d_idx, have * sizeof(uint32_t), hipMemcpyDeviceToHost))) return MSJ_ERR_HIP;
        return res.code;
    }
    const uint64_t n = res.count;
    if (!piped && !hip_ok(hipMemcpy(idx_out, d_idx, (n + 3) * sizeof(uint32_t), hipMemcpyDeviceToHost)))
        return MSJ_ERR_HIP;  // (the pipeline has brought the indices and the trailer down already)
    *n_out = n;
    return res.code;
}

#ifdef MSJ_STAMPS
void msj_debug_set_stamps(uint64_t *d_stamps) { g_stamps = d_stamps; }
#endif

int32_t msj_stage1(const uint8_t *buf, uint64_t len, uint32_t *idx_out, uint64_t idx_capacity,
                   uint64_t *n_out, int32_t *utf8_verdict_out, uint32_t flags) {
    std::lock_guard<std::mutex> lock(g_default_mutex);
    if (!g_default_ctx) {
        const int32_t rc = msj_ctx_create(0, &g_default_ctx);
        if (rc != MSJ_SUCCESS) return rc;
    }
    return msj_stage1_ctx(g_default_ctx, buf, len, idx_out, idx_capacity, n_out, utf8_verdict_out,
                          flags);
}

}  // extern "C"
