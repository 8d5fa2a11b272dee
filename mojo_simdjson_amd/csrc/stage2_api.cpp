// stage2_api.cpp -- extern "C" entry points of everything that runs behind stage 1 (include/msj_stage1.h): tokens, spans,
// the fused prep, segments, documents, number values, the verdict and the tape (one document, or every document of a
// window), fields by path, a path's strings as a column and its arrays as a list column, fields by path inside list
// elements, the arrays inside list rows, an object's members as a map column, a selected value's JSON text as a column, a byte column as codes plus distinct
// values (in one window, or against a dictionary carried across windows), rows by predicate, strings cast to numbers, count / sum / min / max per group, rows by numeric order, the equi-join of two code columns, a dictionary's values in byte order, the rank records of a code column, substring patterns over a byte column, numbers floored to buckets and byte keys from several columns.  Every call is the same few steps: check the arguments (the order of the checks is part of the ABI: callers
// see which error wins; tests/test_check_order.py), select the device, grow the call's workspace, launch.
#include <memory>
#include <new>

#include "ctx.h"
#include "aggregate_math.h"
#include "cast_strings_math.h"
#include "dictionary_order_math.h"
#include "filter_rows_math.h"
#include "group_keys_math.h"
#include "join_rows_math.h"
#include "match_strings_math.h"
#include "select_math.h"

// msj_paths_create's object: the compiled paths (select_math.h: Paths) in device memory, and what the host needs of them
struct msj_paths {
    int device = 0;
    uint32_t n_paths = 0, max_levels = 0;
    DeviceBuffer blob;
};

// msj_predicates_create's object: the compiled predicates (filter_rows_math.h: Predicates) in device memory, and what the
// host needs of them
struct msj_predicates {
    int device = 0;
    uint32_t max_column = 0;
    DeviceBuffer blob;
};

// msj_patterns_create's object: the compiled patterns (match_strings_math.h: Patterns) in device memory, and what the host
// needs of them
struct msj_patterns {
    int device = 0;
    uint32_t n_patterns = 0, max_pieces = 0;
    DeviceBuffer blob;
};

namespace {

constexpr uint64_t kMaxTokens = 1ull << 31;  // token numbers are uint32 with the top bit spare
bool too_big(uint64_t len, uint64_t n) { return len > MSJ_MAX_SEGMENT_BYTES || n >= kMaxTokens; }
template <class... P>
bool all_aligned(uintptr_t a, P... p) { return (aligned(p, a) && ...); }  // (null pointers are aligned)

// what the calls over a window ask of their views (launch.h): the entry point decides the code and the order
bool arrays_present(const msj_token_view &t) { return t.d_idx && t.d_type && t.d_depth && t.d_match && t.d_end && t.d_flags; }
bool all_present(const msj_token_view &t) { return t.d_buf && arrays_present(t); }
bool too_big(const msj_token_view &t) { return too_big(t.len, t.n); }
bool is_aligned(const msj_token_view &t) { return all_aligned(16, t.d_idx, t.d_depth, t.d_match, t.d_end) && all_aligned(8, t.d_type, t.d_flags); }
bool is_aligned(const msj_split_view &sp) { return aligned(sp.d_docs, 8) && aligned(sp.d_doc_first, 4); }
bool records_present(const msj_number_view &nv) { return nv.numbers_capacity == 0 || nv.d_numbers; }
bool is_aligned(const msj_number_view &nv) { return aligned(nv.d_numbers, 16) && aligned(nv.d_numbers_result, 8); }

// behind the argument checks of a device call: its device selected, its workspace at least `need` bytes
int32_t begin_call(msj_ctx *ctx, DeviceBuffer &ws, uint64_t need) {
    if (!hip_ok(hipSetDevice(ctx->device))) return MSJ_ERR_HIP;
    return ws.reserve(need, true) ? MSJ_SUCCESS : MSJ_MEMALLOC;
}
int32_t launched(int hip_error) { return hip_error == 0 ? MSJ_SUCCESS : MSJ_ERR_HIP; }

// the span kernel's fix-up list: allocated once, zeroed once
bool ensure_span_fix(msj_ctx *ctx) {
    if (ctx->span_fix.p) return true;
    if (!ctx->span_fix.reserve(msj_span_fix_bytes(), false)) return false;
    if (!hip_ok(hipMemset(ctx->span_fix.p, 0, msj_span_fix_bytes()))) {
        ctx->span_fix.release();
        return false;
    }
    return true;
}

// The token calls (spans = false: msj_launch_tokens; d_end / d_flags unused) and the fused prep calls (spans = true:
// msj_launch_stage2_prep).  match_bias / d_resid: msj_stage2_prep_segments (partners as positions in the shard's arrays,
// the call's unpaired brackets kept).  tok_doc_n says whose document aggregates the workspace holds: none while a launch
// may have failed half-way.
int32_t chain_impl(msj_ctx *ctx, bool spans, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n, uint8_t *d_type,
                   int32_t *d_depth, uint32_t *d_match, uint32_t *d_end, uint8_t *d_flags, msj_tokens_result *d_result,
                   const msj_tokens_result *d_prev, void *stream, uint32_t match_bias, uint32_t *d_resid, msj_bracket_pair *d_pairs) {
    if (!ctx || !d_result || d_prev == d_result) return MSJ_ERR_BAD_ARGUMENT;
    if (n > 0 && (!d_buf || !d_idx || !d_type || !d_depth || (spans && (!d_end || !d_flags)))) return MSJ_ERR_BAD_ARGUMENT;
    if (too_big(len, n)) return MSJ_CAPACITY;
    if (!all_aligned(16, d_idx, d_depth, d_match) || !aligned(d_type, 8)) return MSJ_ERR_BAD_ARGUMENT;  // match[] leaves as 16-byte stores
    // (the workspace includes the fused kernel's chunk aggregates and group table)
    const int32_t rc = begin_call(ctx, ctx->tok_ws, msj_stage2_prep_workspace_bytes(n, len, d_pairs ? 2 : (d_match != nullptr ? 1 : 0)));
    if (rc != MSJ_SUCCESS) return rc;
    ctx->tok_doc_n = ~0ull;
    if (spans && !ensure_span_fix(ctx)) return MSJ_MEMALLOC;
    msj_token_opts o = ctx->tok_opts;
    o.d_prev = d_prev;
    o.match_bias = match_bias;
    o.d_resid = d_match ? d_resid : nullptr;
    o.d_pairs = d_pairs;
    int32_t *ws = ctx->tok_ws.as<int32_t>();
    const int e = spans ? msj_launch_stage2_prep(d_buf, len, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_result, ws,
                                                 ctx->span_fix.as<uint32_t>(), stream, o)
                        : msj_launch_tokens(d_buf, len, d_idx, n, d_type, d_depth, d_match, d_result, ws, stream, o);
    if (e != 0) return MSJ_ERR_HIP;
    ctx->tok_doc_n = n;
    return MSJ_SUCCESS;
}

}  // namespace

extern "C" {

int32_t msj_stage1_types_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, uint32_t *d_idx, uint64_t idx_capacity,
                                uint8_t *d_types, msj_carry *d_result, void *stream, uint32_t flags) {
    if (!ctx || !d_result || !d_types || !aligned(d_types, 4)) return MSJ_ERR_BAD_ARGUMENT;
    if (len == 0) return MSJ_EMPTY;
    if (len > ctx->seg_bytes || (flags & MSJ_FLAG_TWO_PASS)) return MSJ_CAPACITY;  // one single-pass launch (prototype)
    ctx->types_out = d_types;
    const int32_t rc = enqueue_shard(ctx, d_buf, len, d_idx, idx_capacity, &ctx->carries[0], d_result, nullptr, 0, nullptr, false, true, false,
                                     len, static_cast<hipStream_t>(stream), flags);
    ctx->types_out = nullptr;
    ctx->last.valid = false;  // (no two-pass fallback for this form: a poisoned launch stays poisoned)
    return rc;
}

int32_t msj_depth_from_types_device(msj_ctx *ctx, const uint8_t *d_type, uint64_t n, int32_t *d_depth, uint32_t *d_match,
                                    msj_tokens_result *d_result, const msj_tokens_result *d_prev, void *stream) {
    if (!ctx || !d_result || d_prev == d_result) return MSJ_ERR_BAD_ARGUMENT;
    if (n > 0 && (!d_type || !d_depth)) return MSJ_ERR_BAD_ARGUMENT;
    if (n >= kMaxTokens) return MSJ_CAPACITY;
    if (!all_aligned(16, d_depth, d_match) || !aligned(d_type, 8)) return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->tok_ws, msj_stage2_prep_workspace_bytes(n, 0, d_match != nullptr));
    if (rc != MSJ_SUCCESS) return rc;
    ctx->tok_doc_n = ~0ull;
    msj_token_opts o = ctx->tok_opts;
    o.d_prev = d_prev;
    if (msj_launch_depth_from_types(d_type, n, d_depth, d_match, d_result, ctx->tok_ws.as<int32_t>(), stream, o) != 0) return MSJ_ERR_HIP;
    ctx->tok_doc_n = n;
    return MSJ_SUCCESS;
}

int32_t msj_tokens_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                          uint8_t *d_type, int32_t *d_depth, uint32_t *d_match, msj_tokens_result *d_result,
                          void *stream) {
    return msj_tokens_chain_device(ctx, d_buf, len, d_idx, n, d_type, d_depth, d_match, d_result, nullptr, stream);
}

int32_t msj_tokens_chain_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                                uint8_t *d_type, int32_t *d_depth, uint32_t *d_match, msj_tokens_result *d_result,
                                const msj_tokens_result *d_prev, void *stream) {
    return chain_impl(ctx, false, d_buf, len, d_idx, n, d_type, d_depth, d_match, nullptr, nullptr, d_result, d_prev, stream, 0u, nullptr, nullptr);
}

int32_t msj_tokens_pairs_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n, uint8_t *d_type,
                                int32_t *d_depth, msj_bracket_pair *d_pairs, msj_tokens_result *d_result,
                                const msj_tokens_result *d_prev, void *stream) {
    if (!d_pairs || !aligned(d_pairs, 8)) return MSJ_ERR_BAD_ARGUMENT;
    return chain_impl(ctx, false, d_buf, len, d_idx, n, d_type, d_depth, nullptr, nullptr, nullptr, d_result, d_prev, stream, 0u, nullptr, d_pairs);
}

int32_t msj_token_spans_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                               uint32_t *d_end, uint8_t *d_flags, void *stream) {
    if (!ctx) return MSJ_ERR_BAD_ARGUMENT;
    if (n > 0 && (!d_buf || !d_idx || !d_end || !d_flags)) return MSJ_ERR_BAD_ARGUMENT;
    if (too_big(len, n)) return MSJ_CAPACITY;
    const int32_t rc = begin_call(ctx, ctx->tok_ws, msj_stage2_prep_workspace_bytes(n, len, 0));  // the group table lives there
    if (rc != MSJ_SUCCESS) return rc;
    if (!ensure_span_fix(ctx)) return MSJ_MEMALLOC;
    ctx->tok_doc_n = ~0ull;
    return launched(msj_launch_token_spans(d_buf, len, d_idx, n, d_end, d_flags, ctx->tok_ws.as<int32_t>(), ctx->span_fix.as<uint32_t>(), stream,
                                           ctx->tok_opts));
}

int32_t msj_stage2_prep_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                               uint8_t *d_type, int32_t *d_depth, uint32_t *d_match, uint32_t *d_end, uint8_t *d_flags,
                               msj_tokens_result *d_result, void *stream) {
    return msj_stage2_prep_chain_device(ctx, d_buf, len, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_result, nullptr, stream);
}

int32_t msj_stage2_prep_pairs_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                                     uint8_t *d_type, int32_t *d_depth, msj_bracket_pair *d_pairs, uint32_t *d_end, uint8_t *d_flags,
                                     msj_tokens_result *d_result, const msj_tokens_result *d_prev, void *stream) {
    if (!d_pairs || !aligned(d_pairs, 8)) return MSJ_ERR_BAD_ARGUMENT;
    return chain_impl(ctx, true, d_buf, len, d_idx, n, d_type, d_depth, nullptr, d_end, d_flags, d_result, d_prev, stream, 0u, nullptr, d_pairs);
}

int32_t msj_stage2_prep_chain_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                                     uint8_t *d_type, int32_t *d_depth, uint32_t *d_match, uint32_t *d_end, uint8_t *d_flags,
                                     msj_tokens_result *d_result, const msj_tokens_result *d_prev, void *stream) {
    return chain_impl(ctx, true, d_buf, len, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_result, d_prev, stream, 0u, nullptr, nullptr);
}

int32_t msj_stage2_prep_segments(msj_ctx *ctx, const uint8_t *d_buf, const msj_segment *segments, uint32_t n_segments,
                                 const uint32_t *d_idx, uint8_t *d_type, int32_t *d_depth, uint32_t *d_match, uint32_t *d_end,
                                 uint8_t *d_flags, msj_tokens_result *d_results, const msj_tokens_result *d_prev,
                                 uint64_t *offsets_out, void *stream) {
    if (!ctx || !segments || n_segments == 0 || !d_results || !d_buf) return MSJ_ERR_BAD_ARGUMENT;
    if (!hip_ok(hipSetDevice(ctx->device))) return MSJ_ERR_HIP;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t begin0 = segments[0].index_begin, base0 = segments[0].byte_base;
    // the whole table is checked before the first launch: a bad entry k must not leave segments 0 .. k-1 on the stream
    for (uint32_t s = 0; s < n_segments; s++) {
        const msj_segment &sg = segments[s];
        if (sg.byte_len == 0 || too_big(sg.byte_len, sg.count)) return MSJ_CAPACITY;
        if (s > 0) {  // segments of one shard follow each other without gaps, in bytes and in indices
            const msj_segment &pv = segments[s - 1];
            if (sg.byte_base != pv.byte_base + pv.byte_len || sg.index_begin != pv.index_begin + pv.count) return MSJ_ERR_BAD_ARGUMENT;
        }
    }
    // bracket partners over the whole shard: match[] holds positions in the shard's output arrays (uint32), every
    // segment leaves its unpaired brackets in a residual list of the context's, a stitch pairs them at the end
    msj_stitch_args st_args;
    st_args.n_segments = n_segments;
    if (d_match) {
        if (n_segments > MSJ_STITCH_MAX_SEGMENTS) return MSJ_CAPACITY;
        uint64_t total = 0;
        for (uint32_t s = 0; s < n_segments; s++) total = (((total + segments[s].count + 3u) & ~3ull) + 7u) & ~7ull;
        if (total >= 0xFFFFFFFFull) return MSJ_CAPACITY;  // (0xFFFFFFFF is "no partner")
        const uint64_t need = (uint64_t)n_segments * MSJ_RESID_WORDS * sizeof(uint32_t);
        if (!ctx->resid.reserve(need, false)) return MSJ_MEMALLOC;
        if (!hip_ok(hipMemsetAsync(ctx->resid.p, 0, need, st))) return MSJ_ERR_HIP;
    }
    uint64_t off = 0;
    // the result each segment goes on from: that of the LAST segment with tokens (d_prev in front of them).  A segment
    // without tokens carries the stream's depth, minimum and maximum on unchanged, but with n = 0 the call behind it
    // could not tell it from the start of a stream and would drop the minimum and maximum of the tokens in front.
    const msj_tokens_result *prev = d_prev;
    for (uint32_t s = 0; s < n_segments; s++) {
        const msj_segment &sg = segments[s];
        const uint64_t n = sg.count;
        // (a segment without tokens -- inside a long string -- reads no index: its slice may start anywhere)
        const uint32_t *idx = n ? d_idx + (sg.index_begin - begin0) : nullptr;
        if (n && !aligned(idx, 16)) {
            // stage 1 writes a shard's indices densely, so a later segment's slice starts wherever the one in front
            // ended: the token kernels read index quads, so it is copied to an aligned buffer first (4 bytes per token
            // each way, on the stream; the first segment of a shard never needs it)
            if (!ctx->seg_idx.reserve((n + 4) * sizeof(uint32_t), false)) return MSJ_MEMALLOC;
            if (!hip_ok(hipMemcpyAsync(ctx->seg_idx.p, idx, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st))) return MSJ_ERR_HIP;
            idx = ctx->seg_idx.as<uint32_t>();
        }
        if (offsets_out) offsets_out[s] = off;
        uint32_t *resid = d_match ? ctx->resid.as<uint32_t>() + (uint64_t)s * MSJ_RESID_WORDS : nullptr;
        if (d_match) {
            st_args.offsets[s] = (uint32_t)off;
            st_args.resid[s] = resid;
        }
        const int32_t rc = chain_impl(ctx, true, d_buf + (sg.byte_base - base0), sg.byte_len, idx, n, d_type ? d_type + off : nullptr,
                                      d_depth ? d_depth + off : nullptr, d_match ? d_match + off : nullptr, d_end ? d_end + off : nullptr,
                                      d_flags ? d_flags + off : nullptr, &d_results[s], prev, stream, (uint32_t)off, resid, nullptr);
        if (rc != MSJ_SUCCESS) return rc;
        if (n) prev = &d_results[s];
        off += (n + 3u) & ~3ull;  // every segment's slices start 16-byte aligned (8 for the byte arrays: n rounded to 4 ... 8 below)
        off = (off + 7u) & ~7ull;
    }
    if (d_match && msj_launch_stitch_partners(st_args, d_match, d_results, d_prev, stream) != 0) return MSJ_ERR_HIP;
    return MSJ_SUCCESS;
}

int32_t msj_documents_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, int32_t is_final, const uint32_t *d_idx,
                             uint64_t n, const uint8_t *d_type, const int32_t *d_depth, const msj_carry *d_carry,
                             uint32_t *d_doc_first, uint64_t capacity, msj_documents_result *d_result, void *stream) {
    if (!ctx || !d_result) return MSJ_ERR_BAD_ARGUMENT;
    if (n > 0 && (!d_buf || !d_idx || !d_type || !d_depth)) return MSJ_ERR_BAD_ARGUMENT;
    if (capacity > 0 && !d_doc_first) return MSJ_ERR_BAD_ARGUMENT;
    if (too_big(len, n)) return MSJ_CAPACITY;
    if (!aligned(d_depth, 16) || !aligned(d_type, 8)) return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->doc_ws, msj_documents_workspace_bytes(n));
    if (rc != MSJ_SUCCESS) return rc;
    // MSJ_DOCS_AFTER_TOKENS: the block aggregates the token pre-pass left in its workspace are for these arrays
    const void *pre = ((is_final & MSJ_DOCS_AFTER_TOKENS) && ctx->tok_ws.p && ctx->tok_doc_n == n && n > 0)
                          ? msj_tokens_doc_aggregates(ctx->tok_ws.as<int32_t>(), n)
                          : nullptr;
    return launched(msj_launch_documents(d_buf, len, is_final & MSJ_DOCS_FINAL, d_idx, n, d_type, d_depth, d_carry, d_doc_first, capacity, d_result,
                                         ctx->doc_ws.p, pre, stream));
}

int32_t msj_number_values_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                                 const uint8_t *d_flags, msj_number *d_numbers, uint64_t capacity,
                                 msj_numbers_result *d_result, void *stream) {
    if (!ctx || !d_result) return MSJ_ERR_BAD_ARGUMENT;
    if (n > 0 && (!d_buf || !d_idx || !d_flags)) return MSJ_ERR_BAD_ARGUMENT;
    if (capacity > 0 && !d_numbers) return MSJ_ERR_BAD_ARGUMENT;
    if (too_big(len, n)) return MSJ_CAPACITY;
    if (!all_aligned(16, d_idx, d_numbers) || !all_aligned(8, d_flags, d_result)) return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->num_ws, msj_number_values_workspace_bytes(n, len));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_number_values(d_buf, len, d_idx, n, d_flags, d_numbers, capacity, d_result, ctx->num_ws.p, stream));
}

int32_t msj_validate_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                            const uint8_t *d_type, const int32_t *d_depth, const uint32_t *d_match,
                            const uint32_t *d_end, const uint8_t *d_flags, const msj_numbers_result *d_numbers,
                            uint32_t max_depth, msj_validate_result *d_result, void *stream) {
    const msj_token_view t{d_buf, len, d_idx, n, d_type, d_depth, d_match, d_end, d_flags};
    const msj_number_view nv{nullptr, 0, d_numbers};
    if (!ctx || !d_result || !all_present(t)) return MSJ_ERR_BAD_ARGUMENT;
    if (n == 0 || max_depth == 0) return MSJ_ERR_BAD_ARGUMENT;
    if (too_big(t)) return MSJ_CAPACITY;
    if (!is_aligned(t) || !is_aligned(nv) || !aligned(d_result, 8)) return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->val_ws, msj_validate_workspace_bytes(n, len));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_validate(t, nv, max_depth, d_result, ctx->val_ws.p, stream));
}

int32_t msj_validate_documents_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                                      const uint8_t *d_type, const int32_t *d_depth, const uint32_t *d_match, const uint32_t *d_end,
                                      const uint8_t *d_flags, const uint32_t *d_doc_first, const msj_documents_result *d_docs,
                                      const msj_number *d_numbers, uint64_t numbers_capacity, const msj_numbers_result *d_numbers_result,
                                      uint32_t max_depth, msj_document_verdict *d_verdicts, uint64_t capacity,
                                      msj_validate_documents_result *d_result, void *stream) {
    const msj_token_view t{d_buf, len, d_idx, n, d_type, d_depth, d_match, d_end, d_flags};
    const msj_split_view sp{d_doc_first, d_docs};
    const msj_number_view nv{d_numbers, numbers_capacity, d_numbers_result};
    if (!ctx || !d_result || !d_docs || max_depth == 0) return MSJ_ERR_BAD_ARGUMENT;
    if (n > 0 && (!all_present(t) || !d_doc_first)) return MSJ_ERR_BAD_ARGUMENT;
    if ((capacity > 0 && !d_verdicts) || !records_present(nv)) return MSJ_ERR_BAD_ARGUMENT;
    if (too_big(t)) return MSJ_CAPACITY;
    if (!is_aligned(t) || !is_aligned(sp) || !is_aligned(nv) || !all_aligned(8, d_verdicts, d_result)) return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->vdoc_ws, msj_validate_documents_workspace_bytes(n, len, capacity));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_validate_documents(t, sp, nv, max_depth, d_verdicts, capacity, d_result, ctx->vdoc_ws.p, stream));
}

int32_t msj_tape_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n, const uint8_t *d_type,
                        const int32_t *d_depth, const uint32_t *d_match, const uint32_t *d_end, const uint8_t *d_flags,
                        const msj_number *d_numbers, uint64_t numbers_capacity, const msj_numbers_result *d_numbers_result,
                        const msj_validate_result *d_verdict, uint64_t *d_tape, uint64_t tape_capacity, uint8_t *d_string_buf,
                        uint64_t string_capacity, msj_tape_result *d_result, void *stream) {
    const msj_token_view t{d_buf, len, d_idx, n, d_type, d_depth, d_match, d_end, d_flags};
    const msj_number_view nv{d_numbers, numbers_capacity, d_numbers_result};
    if (!ctx || !d_result || !all_present(t)) return MSJ_ERR_BAD_ARGUMENT;
    if ((tape_capacity > 0 && !d_tape) || !records_present(nv)) return MSJ_ERR_BAD_ARGUMENT;
    if (n == 0) return MSJ_ERR_BAD_ARGUMENT;
    if (too_big(t)) return MSJ_CAPACITY;
    if (!is_aligned(t) || !is_aligned(nv) || !aligned(d_tape, 16) || !all_aligned(8, d_verdict, d_result)) return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->tape_ws, msj_tape_workspace_bytes(n, len));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_tape(t, nv, d_verdict, d_tape, tape_capacity, d_string_buf, string_capacity, d_result, ctx->tape_ws.p, stream));
}

int32_t msj_tape_documents_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n, const uint8_t *d_type,
                                  const int32_t *d_depth, const uint32_t *d_match, const uint32_t *d_end, const uint8_t *d_flags,
                                  const uint32_t *d_doc_first, const msj_documents_result *d_docs, const msj_number *d_numbers,
                                  uint64_t numbers_capacity, const msj_numbers_result *d_numbers_result,
                                  const msj_document_verdict *d_verdicts, uint64_t *d_tape, uint64_t tape_capacity, uint8_t *d_string_buf,
                                  uint64_t string_capacity, msj_document_tape *d_doc_tapes, uint64_t capacity,
                                  msj_tape_documents_result *d_result, void *stream) {
    const msj_token_view t{d_buf, len, d_idx, n, d_type, d_depth, d_match, d_end, d_flags};
    const msj_split_view sp{d_doc_first, d_docs};
    const msj_number_view nv{d_numbers, numbers_capacity, d_numbers_result};
    if (!ctx || !d_result || !d_docs) return MSJ_ERR_BAD_ARGUMENT;
    if (n > 0 && (!all_present(t) || !d_doc_first)) return MSJ_ERR_BAD_ARGUMENT;
    if ((tape_capacity > 0 && !d_tape) || (capacity > 0 && !d_doc_tapes) || !records_present(nv)) return MSJ_ERR_BAD_ARGUMENT;
    if (too_big(t)) return MSJ_CAPACITY;
    if (!is_aligned(t) || !is_aligned(sp) || !is_aligned(nv) || !aligned(d_tape, 16) || !all_aligned(8, d_verdicts, d_doc_tapes, d_result))
        return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->tdoc_ws, msj_tape_documents_workspace_bytes(n, len, capacity));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_tape_documents(t, sp, nv, d_verdicts, d_tape, tape_capacity, d_string_buf, string_capacity, d_doc_tapes, capacity,
                                              d_result, ctx->tdoc_ws.p, stream));
}

int32_t msj_paths_create(msj_ctx *ctx, const char *const *pointers, uint32_t n_paths, msj_paths **out) {
    using namespace msj::sel;
    if (!ctx || !out) return MSJ_ERR_BAD_ARGUMENT;
    std::vector<Paths> host(1);  // (33 KiB: not on the stack)
    Paths &h = host[0];
    const int parsed = compile_paths(pointers, n_paths, h);
    if (parsed != 0) return parsed < 0 ? MSJ_ERR_BAD_ARGUMENT : parsed;
    if (!hip_ok(hipSetDevice(ctx->device))) return MSJ_ERR_HIP;
    msj_paths *obj = new (std::nothrow) msj_paths;
    if (!obj) return MSJ_MEMALLOC;
    obj->device = ctx->device, obj->n_paths = n_paths, obj->max_levels = h.max_levels;
    if (!obj->blob.reserve(sizeof h, false)) {
        delete obj;
        return MSJ_MEMALLOC;
    }
    if (!hip_ok(hipMemcpy(obj->blob.p, &h, sizeof h, hipMemcpyHostToDevice))) {  // synchronous: usable on any stream from here on
        delete obj;
        return MSJ_ERR_HIP;
    }
    *out = obj;
    return MSJ_SUCCESS;
}

void msj_paths_destroy(msj_paths *paths) {
    if (!paths) return;
    (void)hipSetDevice(paths->device);
    delete paths;
}

int32_t msj_select_documents_device(msj_ctx *ctx, const msj_paths *paths, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                                    const uint8_t *d_type, const int32_t *d_depth, const uint32_t *d_match, const uint32_t *d_end,
                                    const uint8_t *d_flags, const uint32_t *d_doc_first, const msj_documents_result *d_docs,
                                    const msj_number *d_numbers, uint64_t numbers_capacity, const msj_numbers_result *d_numbers_result,
                                    const msj_document_verdict *d_verdicts, msj_field *d_fields, uint64_t capacity,
                                    msj_select_documents_result *d_result, void *stream) {
    const msj_token_view t{d_buf, len, d_idx, n, d_type, d_depth, d_match, d_end, d_flags};
    const msj_split_view sp{d_doc_first, d_docs};
    const msj_number_view nv{d_numbers, numbers_capacity, d_numbers_result};
    if (!ctx || !paths || paths->device != ctx->device || !d_result || !d_docs) return MSJ_ERR_BAD_ARGUMENT;
    if (n > 0 && (!all_present(t) || !d_doc_first)) return MSJ_ERR_BAD_ARGUMENT;
    if ((capacity > 0 && !d_fields) || !records_present(nv)) return MSJ_ERR_BAD_ARGUMENT;
    if (too_big(t)) return MSJ_CAPACITY;
    if (!is_aligned(t) || !is_aligned(sp) || !is_aligned(nv) || !aligned(d_fields, 16) || !all_aligned(8, d_verdicts, d_result))
        return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->sel_ws, msj_select_documents_workspace_bytes(n, len, capacity, paths->n_paths));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_select_documents(paths->blob.p, paths->n_paths, paths->max_levels, t, sp, nv, d_verdicts, d_fields, capacity,
                                                d_result, ctx->sel_ws.p, stream));
}

int32_t msj_string_column_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const msj_field *d_column,
                                 const msj_select_documents_result *d_select, uint64_t *d_offsets, uint8_t *d_valid, uint64_t capacity,
                                 uint8_t *d_bytes, uint64_t bytes_capacity, msj_string_column_result *d_result, void *stream) {
    if (!ctx || !d_result || !d_select || !d_buf) return MSJ_ERR_BAD_ARGUMENT;
    if (capacity > 0 && (!d_column || !d_offsets || !d_valid)) return MSJ_ERR_BAD_ARGUMENT;
    if (bytes_capacity > 0 && !d_bytes) return MSJ_ERR_BAD_ARGUMENT;
    if (len > MSJ_MAX_SEGMENT_BYTES) return MSJ_CAPACITY;
    if (!aligned(d_column, 16) || !all_aligned(8, d_offsets, d_select, d_result)) return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->scol_ws, msj_string_column_workspace_bytes(capacity));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_string_column(d_buf, len, d_column, d_select, d_offsets, d_valid, capacity, d_bytes, bytes_capacity, d_result,
                                             ctx->scol_ws.p, stream));
}

int32_t msj_array_column_device(msj_ctx *ctx, const uint32_t *d_idx, uint64_t n, const uint8_t *d_type, const int32_t *d_depth,
                                const uint32_t *d_match, const uint32_t *d_end, const uint8_t *d_flags, const uint32_t *d_doc_first,
                                const msj_documents_result *d_docs, const msj_number *d_numbers, uint64_t numbers_capacity,
                                const msj_numbers_result *d_numbers_result, const msj_field *d_column,
                                const msj_select_documents_result *d_select, uint64_t *d_offsets, uint8_t *d_valid, uint64_t capacity,
                                msj_field *d_elements, uint64_t elements_capacity, msj_array_column_result *d_result,
                                msj_select_documents_result *d_elements_select, void *stream) {
    const msj_token_view t{nullptr, 0, d_idx, n, d_type, d_depth, d_match, d_end, d_flags};  // (the call reads no byte of the window)
    const msj_split_view sp{d_doc_first, d_docs};
    const msj_number_view nv{d_numbers, numbers_capacity, d_numbers_result};
    if (!ctx || !d_result || !d_select || !d_docs) return MSJ_ERR_BAD_ARGUMENT;
    if (n > 0 && (!arrays_present(t) || !d_doc_first)) return MSJ_ERR_BAD_ARGUMENT;
    if (capacity > 0 && (!d_column || !d_offsets || !d_valid)) return MSJ_ERR_BAD_ARGUMENT;
    if ((elements_capacity > 0 && !d_elements) || !records_present(nv)) return MSJ_ERR_BAD_ARGUMENT;
    if (too_big(t)) return MSJ_CAPACITY;
    if (!is_aligned(t) || !is_aligned(sp) || !is_aligned(nv) || !all_aligned(16, d_column, d_elements) ||
        !all_aligned(8, d_select, d_offsets, d_result, d_elements_select))
        return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->acol_ws, msj_array_column_workspace_bytes(n, capacity));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_array_column(t, sp, nv, d_column, d_select, d_offsets, d_valid, capacity, d_elements, elements_capacity, d_result,
                                            d_elements_select, ctx->acol_ws.p, stream));
}

int32_t msj_select_elements_device(msj_ctx *ctx, const msj_paths *paths, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                                   const uint8_t *d_type, const int32_t *d_depth, const uint32_t *d_match, const uint32_t *d_end,
                                   const uint8_t *d_flags, const msj_number *d_numbers, uint64_t numbers_capacity,
                                   const msj_numbers_result *d_numbers_result, const msj_field *d_rows,
                                   const msj_select_documents_result *d_rows_select, msj_field *d_fields, uint64_t capacity,
                                   msj_select_documents_result *d_result, void *stream) {
    const msj_token_view t{d_buf, len, d_idx, n, d_type, d_depth, d_match, d_end, d_flags};
    const msj_number_view nv{d_numbers, numbers_capacity, d_numbers_result};
    if (!ctx || !paths || paths->device != ctx->device || !d_result || !d_rows_select || d_result == d_rows_select) return MSJ_ERR_BAD_ARGUMENT;
    if (n > 0 && !all_present(t)) return MSJ_ERR_BAD_ARGUMENT;
    if ((capacity > 0 && (!d_rows || !d_fields)) || !records_present(nv)) return MSJ_ERR_BAD_ARGUMENT;
    if (too_big(t)) return MSJ_CAPACITY;
    if (!is_aligned(t) || !is_aligned(nv) || !all_aligned(16, d_rows, d_fields) || !all_aligned(8, d_rows_select, d_result))
        return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->selem_ws, msj_select_elements_workspace_bytes(n, capacity, paths->n_paths));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_select_elements(paths->blob.p, paths->n_paths, paths->max_levels, t, nv, d_rows, d_rows_select, d_fields, capacity,
                                               d_result, ctx->selem_ws.p, stream));
}

int32_t msj_array_elements_device(msj_ctx *ctx, const uint32_t *d_idx, uint64_t n, const uint8_t *d_type, const int32_t *d_depth,
                                  const uint32_t *d_match, const uint32_t *d_end, const uint8_t *d_flags, const msj_number *d_numbers,
                                  uint64_t numbers_capacity, const msj_numbers_result *d_numbers_result, const msj_field *d_rows,
                                  const msj_select_documents_result *d_rows_select, uint64_t *d_offsets, uint8_t *d_valid, uint64_t capacity,
                                  msj_field *d_elements, uint64_t elements_capacity, msj_array_column_result *d_result,
                                  msj_select_documents_result *d_elements_select, void *stream) {
    const msj_token_view t{nullptr, 0, d_idx, n, d_type, d_depth, d_match, d_end, d_flags};  // (the call reads no byte of the window)
    const msj_number_view nv{d_numbers, numbers_capacity, d_numbers_result};
    if (!ctx || !d_result || !d_rows_select) return MSJ_ERR_BAD_ARGUMENT;
    if (n > 0 && !arrays_present(t)) return MSJ_ERR_BAD_ARGUMENT;
    if (capacity > 0 && (!d_rows || !d_offsets || !d_valid)) return MSJ_ERR_BAD_ARGUMENT;
    if ((elements_capacity > 0 && !d_elements) || !records_present(nv)) return MSJ_ERR_BAD_ARGUMENT;
    if (too_big(t)) return MSJ_CAPACITY;
    if (d_elements_select == d_rows_select || (d_elements && d_elements == d_rows)) return MSJ_ERR_BAD_ARGUMENT;
    if (!is_aligned(t) || !is_aligned(nv) || !all_aligned(16, d_rows, d_elements) ||
        !all_aligned(8, d_rows_select, d_offsets, d_result, d_elements_select))
        return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->aelem_ws, msj_array_elements_workspace_bytes(n, capacity));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_array_elements(t, nv, d_rows, d_rows_select, d_offsets, d_valid, capacity, d_elements, elements_capacity, d_result,
                                              d_elements_select, ctx->aelem_ws.p, stream));
}

int32_t msj_object_entries_device(msj_ctx *ctx, const uint32_t *d_idx, uint64_t n, const uint8_t *d_type, const int32_t *d_depth,
                                  const uint32_t *d_match, const uint32_t *d_end, const uint8_t *d_flags, const msj_number *d_numbers,
                                  uint64_t numbers_capacity, const msj_numbers_result *d_numbers_result, const msj_field *d_rows,
                                  const msj_select_documents_result *d_rows_select, uint64_t *d_offsets, uint8_t *d_valid, uint64_t capacity,
                                  msj_field *d_keys, msj_field *d_values, uint64_t entries_capacity, msj_object_entries_result *d_result,
                                  msj_select_documents_result *d_keys_select, msj_select_documents_result *d_values_select, void *stream) {
    const msj_token_view t{nullptr, 0, d_idx, n, d_type, d_depth, d_match, d_end, d_flags};  // (the call reads no byte of the window)
    const msj_number_view nv{d_numbers, numbers_capacity, d_numbers_result};
    if (!ctx || !d_result || !d_rows_select) return MSJ_ERR_BAD_ARGUMENT;
    if (n > 0 && !arrays_present(t)) return MSJ_ERR_BAD_ARGUMENT;
    if (capacity > 0 && (!d_rows || !d_offsets || !d_valid)) return MSJ_ERR_BAD_ARGUMENT;
    if ((entries_capacity > 0 && !d_keys) || (d_keys == nullptr) != (d_values == nullptr) || !records_present(nv)) return MSJ_ERR_BAD_ARGUMENT;
    if (too_big(t)) return MSJ_CAPACITY;
    if (d_keys_select == d_rows_select || d_values_select == d_rows_select || (d_keys_select && d_keys_select == d_values_select))
        return MSJ_ERR_BAD_ARGUMENT;
    if (d_keys && (d_keys == d_rows || d_values == d_rows || d_keys == d_values)) return MSJ_ERR_BAD_ARGUMENT;
    if (!is_aligned(t) || !is_aligned(nv) || !all_aligned(16, d_rows, d_keys, d_values) ||
        !all_aligned(8, d_rows_select, d_offsets, d_result, d_keys_select, d_values_select))
        return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->oent_ws, msj_object_entries_workspace_bytes(n, capacity));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_object_entries(t, nv, d_rows, d_rows_select, d_offsets, d_valid, capacity, d_keys, d_values, entries_capacity,
                                              d_result, d_keys_select, d_values_select, ctx->oent_ws.p, stream));
}

int32_t msj_raw_column_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n, const uint8_t *d_type,
                              const uint32_t *d_match, const uint32_t *d_end, const uint8_t *d_flags, const msj_field *d_rows,
                              const msj_select_documents_result *d_rows_select, uint64_t *d_offsets, uint8_t *d_valid, uint64_t capacity,
                              uint8_t *d_bytes, uint64_t bytes_capacity, uint32_t flags, msj_raw_column_result *d_result, void *stream) {
    const msj_token_view t{d_buf, len, d_idx, n, d_type, nullptr, d_match, d_end, d_flags};  // (d_match is not read: the record's bits name the partner)
    if (!ctx || !d_result || !d_rows_select || !d_buf) return MSJ_ERR_BAD_ARGUMENT;
    if (n > 0 && (!d_idx || !d_type || !d_end || !d_flags)) return MSJ_ERR_BAD_ARGUMENT;
    if (capacity > 0 && (!d_rows || !d_offsets || !d_valid)) return MSJ_ERR_BAD_ARGUMENT;
    if ((bytes_capacity > 0 && !d_bytes) || (flags & ~MSJ_RAW_COMPACT) != 0) return MSJ_ERR_BAD_ARGUMENT;
    if (too_big(t)) return MSJ_CAPACITY;
    if (!aligned(d_rows, 16) || !all_aligned(8, d_offsets, d_rows_select, d_result) || !all_aligned(4, d_idx, d_match, d_end))
        return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->rcol_ws, msj_raw_column_workspace_bytes(n, capacity, flags));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_raw_column(t, d_rows, d_rows_select, d_offsets, d_valid, capacity, d_bytes, bytes_capacity, flags, d_result,
                                          ctx->rcol_ws.p, stream));
}

int32_t msj_dictionary_device(msj_ctx *ctx, const uint64_t *d_offsets, const uint8_t *d_valid, uint64_t rows, const uint64_t *d_n_rows,
                              const uint8_t *d_bytes, uint64_t bytes_len, int32_t *d_codes, uint64_t *d_dict_offsets, uint32_t *d_dict_first,
                              uint64_t dict_capacity, uint8_t *d_dict_bytes, uint64_t dict_bytes_capacity, uint32_t flags,
                              msj_dictionary_result *d_result, void *stream) {
    if (!ctx || !d_result) return MSJ_ERR_BAD_ARGUMENT;
    if (rows > 0 && (!d_offsets || !d_valid || !d_codes)) return MSJ_ERR_BAD_ARGUMENT;
    if (bytes_len > 0 && !d_bytes) return MSJ_ERR_BAD_ARGUMENT;
    if (dict_capacity > 0 && (!d_dict_offsets || !d_dict_first)) return MSJ_ERR_BAD_ARGUMENT;
    if ((dict_bytes_capacity > 0 && !d_dict_bytes) || (flags & ~MSJ_DICTIONARY_WEAK_HASH) != 0) return MSJ_ERR_BAD_ARGUMENT;
    if (!all_aligned(8, d_offsets, d_n_rows, d_dict_offsets, d_result) || !all_aligned(4, d_codes, d_dict_first)) return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->dict_ws, msj_dictionary_workspace_bytes(rows));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_dictionary(d_offsets, d_valid, rows, d_n_rows, d_bytes, bytes_len, d_codes, d_dict_offsets, d_dict_first,
                                          dict_capacity, d_dict_bytes, dict_bytes_capacity, flags, d_result, ctx->dict_ws.p, stream));
}

int32_t msj_dictionary_extend_device(msj_ctx *ctx, const uint64_t *d_offsets, const uint8_t *d_valid, uint64_t rows, const uint64_t *d_n_rows,
                                     const uint8_t *d_bytes, uint64_t bytes_len, uint64_t n_prior, const uint64_t *d_n_prior, int32_t *d_codes,
                                     uint64_t *d_dict_offsets, uint32_t *d_dict_first, uint64_t dict_capacity, uint8_t *d_dict_bytes,
                                     uint64_t dict_bytes_capacity, uint32_t flags, msj_dictionary_extend_result *d_result, void *stream) {
    const bool layout_only = !d_dict_offsets && !d_dict_first && !d_dict_bytes;
    if (!ctx || !d_result) return MSJ_ERR_BAD_ARGUMENT;
    if (rows > 0 && (!d_offsets || !d_valid || !d_codes)) return MSJ_ERR_BAD_ARGUMENT;
    if (bytes_len > 0 && !d_bytes) return MSJ_ERR_BAD_ARGUMENT;
    if (dict_capacity > 0 && (!d_dict_offsets || !d_dict_first)) return MSJ_ERR_BAD_ARGUMENT;
    if (dict_bytes_capacity > 0 && !d_dict_bytes) return MSJ_ERR_BAD_ARGUMENT;
    if ((n_prior > 0 || d_n_prior) && layout_only) return MSJ_ERR_BAD_ARGUMENT;
    if ((flags & ~(MSJ_DICTIONARY_WEAK_HASH | MSJ_DICTIONARY_FROZEN)) != 0) return MSJ_ERR_BAD_ARGUMENT;
    if ((flags & MSJ_DICTIONARY_FROZEN) && layout_only) return MSJ_ERR_BAD_ARGUMENT;
    if (!all_aligned(8, d_offsets, d_n_rows, d_n_prior, d_dict_offsets, d_result) || !all_aligned(4, d_codes, d_dict_first)) return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->dictx_ws, msj_dictionary_extend_workspace_bytes(rows, dict_capacity));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_dictionary_extend(d_offsets, d_valid, rows, d_n_rows, d_bytes, bytes_len, n_prior, d_n_prior, d_codes,
                                                 d_dict_offsets, d_dict_first, dict_capacity, d_dict_bytes, dict_bytes_capacity, flags, d_result,
                                                 ctx->dictx_ws.p, stream));
}

int32_t msj_predicates_create(msj_ctx *ctx, const msj_predicate *predicates, uint32_t n_predicates, uint32_t flags, msj_predicates **out) {
    using namespace msj::frows;
    if (!ctx || !out) return MSJ_ERR_BAD_ARGUMENT;
    std::vector<Predicates> host(1);  // (4 KiB: not on the stack)
    Predicates &h = host[0];
    if (compile_predicates(predicates, n_predicates, flags, h) != 0) return MSJ_ERR_BAD_ARGUMENT;
    if (!hip_ok(hipSetDevice(ctx->device))) return MSJ_ERR_HIP;
    msj_predicates *obj = new (std::nothrow) msj_predicates;
    if (!obj) return MSJ_MEMALLOC;
    obj->device = ctx->device, obj->max_column = h.max_column;
    if (!obj->blob.reserve(sizeof h, false)) {
        delete obj;
        return MSJ_MEMALLOC;
    }
    if (!hip_ok(hipMemcpy(obj->blob.p, &h, sizeof h, hipMemcpyHostToDevice))) {  // synchronous: usable on any stream from here on
        delete obj;
        return MSJ_ERR_HIP;
    }
    *out = obj;
    return MSJ_SUCCESS;
}

void msj_predicates_destroy(msj_predicates *predicates) {
    if (!predicates) return;
    (void)hipSetDevice(predicates->device);
    delete predicates;
}

int32_t msj_filter_rows_device(msj_ctx *ctx, const msj_predicates *predicates, const uint8_t *d_buf, uint64_t len, const msj_field *d_fields,
                               uint64_t stride, uint32_t n_columns, const msj_select_documents_result *d_rows_select, uint8_t *d_keep,
                               uint32_t *d_kept, uint64_t capacity, const uint64_t *d_list_offsets, uint64_t list_rows,
                               const uint64_t *d_list_n_rows, uint64_t *d_list_offsets_out, msj_filter_rows_result *d_result,
                               msj_select_documents_result *d_kept_select, void *stream) {
    if (!ctx || !predicates || predicates->device != ctx->device || !d_result || !d_rows_select || !d_buf) return MSJ_ERR_BAD_ARGUMENT;
    if (capacity > 0 && (!d_fields || !d_keep)) return MSJ_ERR_BAD_ARGUMENT;
    if ((d_list_offsets == nullptr) != (d_list_offsets_out == nullptr)) return MSJ_ERR_BAD_ARGUMENT;
    if (n_columns == 0 || n_columns > msj::frows::kMaxColumns || predicates->max_column >= n_columns || (n_columns > 1 && stride < capacity))
        return MSJ_ERR_BAD_ARGUMENT;
    if (len > MSJ_MAX_SEGMENT_BYTES) return MSJ_CAPACITY;
    if ((const void *)d_result == (const void *)d_rows_select || (const void *)d_result == (const void *)d_kept_select ||
        d_kept_select == d_rows_select)
        return MSJ_ERR_BAD_ARGUMENT;
    if (!aligned(d_fields, 16) || !aligned(d_kept, 4) ||
        !all_aligned(8, d_list_offsets, d_list_n_rows, d_list_offsets_out, d_rows_select, d_result, d_kept_select))
        return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->frow_ws, msj_filter_rows_workspace_bytes(capacity));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_filter_rows(predicates->blob.p, d_buf, len, d_fields, stride, d_rows_select, d_keep, d_kept, capacity, d_list_offsets,
                                           list_rows, d_list_n_rows, d_list_offsets_out, d_result, d_kept_select, ctx->frow_ws.p, stream));
}

int32_t msj_take_rows_device(msj_ctx *ctx, const uint32_t *d_take, const msj_select_documents_result *d_take_select, const msj_field *d_fields,
                             uint64_t stride, uint32_t n_columns, const msj_select_documents_result *d_rows_select, msj_field *d_out,
                             uint64_t out_stride, uint64_t out_capacity, msj_take_rows_result *d_result,
                             msj_select_documents_result *d_out_select, void *stream) {
    if (!ctx || !d_result || !d_take_select || !d_rows_select) return MSJ_ERR_BAD_ARGUMENT;
    if ((out_capacity > 0 && (!d_take || !d_out)) || (stride > 0 && !d_fields)) return MSJ_ERR_BAD_ARGUMENT;
    if (n_columns == 0 || n_columns > msj::frows::kMaxColumns || (n_columns > 1 && out_stride < out_capacity)) return MSJ_ERR_BAD_ARGUMENT;
    if (stride >= (1ull << 40) || out_stride >= (1ull << 40) || out_capacity >= (1ull << 40)) return MSJ_CAPACITY;  // (the extents below: no overflow)
    if (d_out && d_fields) {  // the two sets of records may not share a byte
        const uintptr_t a = reinterpret_cast<uintptr_t>(d_fields), b = reinterpret_cast<uintptr_t>(d_out);
        const uint64_t a_bytes = 16 * (uint64_t)n_columns * stride, b_bytes = 16 * ((uint64_t)(n_columns - 1) * out_stride + out_capacity);
        if (a < b + b_bytes && b < a + a_bytes) return MSJ_ERR_BAD_ARGUMENT;
    }
    if ((const void *)d_result == (const void *)d_take_select || (const void *)d_result == (const void *)d_rows_select ||
        (const void *)d_result == (const void *)d_out_select || d_out_select == d_take_select || d_out_select == d_rows_select)
        return MSJ_ERR_BAD_ARGUMENT;
    if (!all_aligned(16, d_fields, d_out) || !aligned(d_take, 4) || !all_aligned(8, d_take_select, d_rows_select, d_result, d_out_select))
        return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->take_ws, msj_filter_rows_workspace_bytes(0));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_take_rows(d_take, d_take_select, d_fields, stride, n_columns, d_rows_select, d_out, out_stride, out_capacity, d_result,
                                         d_out_select, ctx->take_ws.p, stream));
}

int32_t msj_cast_strings_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const msj_field *d_rows,
                                const msj_select_documents_result *d_rows_select, uint32_t kind, uint32_t unit, uint32_t flags, msj_field *d_out,
                                uint64_t capacity, msj_cast_strings_result *d_result, msj_select_documents_result *d_out_select, void *stream) {
    if (!ctx || !d_result || !d_rows_select || !d_buf) return MSJ_ERR_BAD_ARGUMENT;
    if (capacity > 0 && (!d_rows || !d_out)) return MSJ_ERR_BAD_ARGUMENT;
    if (msj::cast::check_kind(kind, unit, flags) != 0) return MSJ_ERR_BAD_ARGUMENT;
    if (len > MSJ_MAX_SEGMENT_BYTES || capacity >= (1ull << 40)) return MSJ_CAPACITY;  // (the extent below: no overflow)
    if (d_out && d_rows && d_out != d_rows) {  // in place, or no byte shared
        const uintptr_t a = reinterpret_cast<uintptr_t>(d_rows), b = reinterpret_cast<uintptr_t>(d_out);
        if (a < b + 16 * capacity && b < a + 16 * capacity) return MSJ_ERR_BAD_ARGUMENT;
    }
    if ((const void *)d_result == (const void *)d_rows_select || (const void *)d_result == (const void *)d_out_select ||
        d_out_select == d_rows_select)
        return MSJ_ERR_BAD_ARGUMENT;
    if (!all_aligned(16, d_rows, d_out) || !all_aligned(8, d_rows_select, d_result, d_out_select)) return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->cast_ws, msj_cast_strings_workspace_bytes(capacity));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_cast_strings(d_buf, len, d_rows, d_rows_select, kind, unit, flags, ctx->cast_fetch, d_out, capacity, d_result,
                                            d_out_select, ctx->cast_ws.p, stream));
}
int32_t msj_debug_set_cast_fetch(msj_ctx *ctx, uint32_t fetch) {
    if (!ctx || fetch > MSJ_CAST_FETCH_BYTES) return MSJ_ERR_BAD_ARGUMENT;
    ctx->cast_fetch = fetch;
    return MSJ_SUCCESS;
}

int32_t msj_aggregate_device(msj_ctx *ctx, const msj_field *d_fields, uint64_t stride, uint32_t n_columns,
                             const msj_select_documents_result *d_rows_select, const int32_t *d_codes, uint64_t n_groups,
                             const uint64_t *d_n_groups, msj_aggregate *d_groups, uint64_t groups_capacity, msj_aggregate_result *d_result,
                             void *stream) {
    if (!ctx || !d_result || !d_rows_select) return MSJ_ERR_BAD_ARGUMENT;
    if ((stride > 0 && !d_fields) || (groups_capacity > 0 && !d_groups)) return MSJ_ERR_BAD_ARGUMENT;
    if (n_columns == 0 || n_columns > msj::agg::kMaxColumns) return MSJ_ERR_BAD_ARGUMENT;
    if (stride >= (1ull << 40) || groups_capacity >= (1ull << 40)) return MSJ_CAPACITY;  // (the workspace's size below: no overflow)
    if ((const void *)d_result == (const void *)d_rows_select) return MSJ_ERR_BAD_ARGUMENT;
    if (!all_aligned(16, d_fields, d_groups) || !aligned(d_codes, 4) || !all_aligned(8, d_n_groups, d_rows_select, d_result))
        return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->agg_ws, msj_aggregate_workspace_bytes(stride, groups_capacity, n_columns));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_aggregate(d_fields, stride, n_columns, d_rows_select, d_codes, n_groups, d_n_groups, d_groups, groups_capacity,
                                         ctx->agg_lds_groups, d_result, ctx->agg_ws.p, stream));
}
int32_t msj_debug_set_aggregate_limits(msj_ctx *ctx, uint32_t lds_groups) {
    if (!ctx || lds_groups > kAggregateMaxLdsGroups) return MSJ_ERR_BAD_ARGUMENT;
    ctx->agg_lds_groups = lds_groups;
    return MSJ_SUCCESS;
}

int32_t msj_sort_rows_device(msj_ctx *ctx, const msj_field *d_fields, uint64_t stride, const msj_select_documents_result *d_rows_select,
                             const uint32_t *d_rows_in, const msj_select_documents_result *d_rows_in_select, uint32_t flags, uint64_t limit,
                             uint32_t *d_order, uint64_t capacity, msj_sort_rows_result *d_result, msj_select_documents_result *d_order_select,
                             void *stream) {
    if (!ctx || !d_result || !d_rows_select) return MSJ_ERR_BAD_ARGUMENT;
    if ((d_rows_in == nullptr) != (d_rows_in_select == nullptr)) return MSJ_ERR_BAD_ARGUMENT;
    if ((stride > 0 && !d_fields) || (capacity > 0 && !d_order)) return MSJ_ERR_BAD_ARGUMENT;
    if (flags & ~(MSJ_SORT_DESCENDING | MSJ_SORT_VALUES_ONLY)) return MSJ_ERR_BAD_ARGUMENT;
    if (stride >= (1ull << 40) || capacity >= (1ull << 40)) return MSJ_CAPACITY;  // (the extents below: no overflow)
    if ((const void *)d_result == (const void *)d_rows_select || (const void *)d_result == (const void *)d_rows_in_select ||
        (const void *)d_result == (const void *)d_order_select)
        return MSJ_ERR_BAD_ARGUMENT;
    if (d_order_select && (d_order_select == d_rows_select || d_order_select == d_rows_in_select)) return MSJ_ERR_BAD_ARGUMENT;
    if (d_order && d_rows_in) {  // the order may not be written over the rows it is read from
        const uintptr_t a = reinterpret_cast<uintptr_t>(d_rows_in), b = reinterpret_cast<uintptr_t>(d_order);
        const uint64_t b_rows = limit > 0 && limit < capacity ? limit : capacity;
        if (a < b + 4 * b_rows && b < a + 4 * capacity) return MSJ_ERR_BAD_ARGUMENT;
    }
    if (!aligned(d_fields, 16) || !all_aligned(4, d_order, d_rows_in) || !all_aligned(8, d_rows_select, d_rows_in_select, d_result, d_order_select))
        return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->sort_ws, msj_sort_rows_workspace_bytes(capacity));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_sort_rows(d_fields, stride, d_rows_select, d_rows_in, d_rows_in_select, flags, limit, ctx->sort_mode, d_order, capacity,
                                         d_result, d_order_select, ctx->sort_ws.p, stream));
}
int32_t msj_debug_set_sort_mode(msj_ctx *ctx, uint32_t mode) {
    if (!ctx || mode > 2u) return MSJ_ERR_BAD_ARGUMENT;
    ctx->sort_mode = mode;
    return MSJ_SUCCESS;
}

int32_t msj_join_rows_device(msj_ctx *ctx, const int32_t *d_left_keys, uint64_t left_rows, const uint64_t *d_n_left, const int32_t *d_right_keys,
                             uint64_t right_rows, const uint64_t *d_n_right, uint64_t n_keys, const uint64_t *d_n_keys, uint64_t keys_capacity,
                             uint32_t flags, uint32_t *d_left_rows, uint32_t *d_right_rows, uint64_t pairs_capacity, uint64_t *d_offsets,
                             msj_join_rows_result *d_result, msj_select_documents_result *d_left_select,
                             msj_select_documents_result *d_right_select, void *stream) {
    if (!ctx || !d_result) return MSJ_ERR_BAD_ARGUMENT;
    if ((left_rows > 0 && !d_left_keys) || (right_rows > 0 && !d_right_keys)) return MSJ_ERR_BAD_ARGUMENT;
    if (pairs_capacity > 0 && !d_left_rows) return MSJ_ERR_BAD_ARGUMENT;
    if (flags & ~msj::jrows::kKnownFlags) return MSJ_ERR_BAD_ARGUMENT;
    if (d_offsets) {  // the offsets may not be written over what the call reads (128 bits: no room is too large to compare)
        const auto overlaps = [&](const void *p, uint64_t count, uint64_t size) {
            const unsigned __int128 a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(d_offsets);
            return p && a < b + ((unsigned __int128)left_rows + 1) * 8 && b < a + (unsigned __int128)count * size;
        };
        if (overlaps(d_left_keys, left_rows, 4) || overlaps(d_right_keys, right_rows, 4) || overlaps(d_n_left, 1, 8) || overlaps(d_n_right, 1, 8) ||
            overlaps(d_n_keys, 1, 8))
            return MSJ_ERR_BAD_ARGUMENT;
    }
    if (left_rows >= (1ull << 40) || right_rows >= (1ull << 40) || keys_capacity >= (1ull << 40) || pairs_capacity >= (1ull << 40)) return MSJ_CAPACITY;
    if (!all_aligned(4, d_left_keys, d_right_keys, d_left_rows, d_right_rows) ||
        !all_aligned(8, d_offsets, d_n_left, d_n_right, d_n_keys, d_result, d_left_select, d_right_select))
        return MSJ_ERR_BAD_ARGUMENT;
    if ((const void *)d_result == (const void *)d_left_select || (const void *)d_result == (const void *)d_right_select) return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->join_ws, msj_join_rows_workspace_bytes(left_rows, right_rows, keys_capacity));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_join_rows(d_left_keys, left_rows, d_n_left, d_right_keys, right_rows, d_n_right, n_keys, d_n_keys, keys_capacity, flags,
                                         d_left_rows, d_right_rows, pairs_capacity, d_offsets, d_result, d_left_select, d_right_select,
                                         ctx->join_ws.p, stream));
}

int32_t msj_dictionary_order_device(msj_ctx *ctx, const uint64_t *d_dict_offsets, const uint8_t *d_dict_bytes, uint64_t dict_bytes_capacity,
                                    uint64_t n_entries, const uint64_t *d_n_entries, uint64_t capacity, uint64_t depth, uint32_t max_rounds,
                                    uint32_t flags, uint32_t *d_sorted, uint32_t *d_rank, msj_dictionary_order_result *d_result, void *stream) {
    if (!ctx || !d_result) return MSJ_ERR_BAD_ARGUMENT;
    if ((capacity > 0 && (!d_dict_offsets || !d_sorted || !d_rank)) || (dict_bytes_capacity > 0 && !d_dict_bytes)) return MSJ_ERR_BAD_ARGUMENT;
    if (msj::dord::bad_numbers(depth, max_rounds, flags)) return MSJ_ERR_BAD_ARGUMENT;
    if (capacity >= (1ull << 40)) return MSJ_CAPACITY;  // (the workspace's size below: no overflow)
    if (!all_aligned(8, d_dict_offsets, d_n_entries, d_result) || !all_aligned(4, d_sorted, d_rank)) return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->order_ws, msj_dictionary_order_workspace_bytes(capacity));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_dictionary_order(d_dict_offsets, d_dict_bytes, dict_bytes_capacity, n_entries, d_n_entries, capacity, depth, max_rounds,
                                                flags, ctx->order_mode, d_sorted, d_rank, d_result, ctx->order_ws.p, stream));
}
int32_t msj_debug_set_order_mode(msj_ctx *ctx, uint32_t mode) {
    if (!ctx || mode > 2u) return MSJ_ERR_BAD_ARGUMENT;
    ctx->order_mode = mode;
    return MSJ_SUCCESS;
}

int32_t msj_rank_rows_device(msj_ctx *ctx, const int32_t *d_codes, uint64_t rows, const uint64_t *d_n_rows, const uint32_t *d_rank,
                             uint64_t rank_capacity, const msj_dictionary_order_result *d_order_result, msj_field *d_fields, uint64_t capacity,
                             msj_rank_rows_result *d_result, msj_select_documents_result *d_select, void *stream) {
    if (!ctx || !d_result || !d_select || !d_order_result) return MSJ_ERR_BAD_ARGUMENT;
    if ((rows > 0 && !d_codes) || (capacity > 0 && !d_fields) || (rank_capacity > 0 && !d_rank)) return MSJ_ERR_BAD_ARGUMENT;
    if (rows >= (1ull << 40) || capacity >= (1ull << 40)) return MSJ_CAPACITY;
    if ((const void *)d_result == (const void *)d_select) return MSJ_ERR_BAD_ARGUMENT;
    if (!aligned(d_fields, 16) || !all_aligned(4, d_codes, d_rank) || !all_aligned(8, d_n_rows, d_order_result, d_result, d_select))
        return MSJ_ERR_BAD_ARGUMENT;
    if (!hip_ok(hipSetDevice(ctx->device))) return MSJ_ERR_HIP;
    return launched(msj_launch_rank_rows(d_codes, rows, d_n_rows, d_rank, rank_capacity, d_order_result, d_fields, capacity, d_result, d_select, stream));
}

int32_t msj_patterns_create(msj_ctx *ctx, const msj_pattern *patterns, uint32_t n_patterns, uint32_t flags, msj_patterns **out) {
    using namespace msj::mstr;
    if (!ctx || !out) return MSJ_ERR_BAD_ARGUMENT;
    const std::unique_ptr<Patterns> host(new (std::nothrow) Patterns);  // (17 KiB: not on the stack; no exception leaves the C ABI)
    if (!host) return MSJ_MEMALLOC;
    Patterns &h = *host;
    if (compile_patterns(patterns, n_patterns, flags, h) != 0) return MSJ_ERR_BAD_ARGUMENT;
    if (!hip_ok(hipSetDevice(ctx->device))) return MSJ_ERR_HIP;
    msj_patterns *obj = new (std::nothrow) msj_patterns;
    if (!obj) return MSJ_MEMALLOC;
    obj->device = ctx->device, obj->n_patterns = h.n, obj->max_pieces = h.max_pieces;
    if (!obj->blob.reserve(sizeof h, false)) {
        delete obj;
        return MSJ_MEMALLOC;
    }
    if (!hip_ok(hipMemcpy(obj->blob.p, &h, sizeof h, hipMemcpyHostToDevice))) {  // synchronous: usable on any stream from here on
        delete obj;
        return MSJ_ERR_HIP;
    }
    *out = obj;
    return MSJ_SUCCESS;
}

void msj_patterns_destroy(msj_patterns *patterns) {
    if (!patterns) return;
    (void)hipSetDevice(patterns->device);
    delete patterns;
}

int32_t msj_match_strings_device(msj_ctx *ctx, const msj_patterns *patterns, const uint64_t *d_offsets, const uint8_t *d_valid, uint64_t rows,
                                 const uint64_t *d_n_rows, const uint8_t *d_bytes, uint64_t bytes_len, msj_field *d_fields, uint64_t capacity,
                                 msj_match_strings_result *d_result, msj_select_documents_result *d_select, void *stream) {
    if (!ctx || !patterns || !d_result || !d_select || patterns->device != ctx->device) return MSJ_ERR_BAD_ARGUMENT;
    if ((rows > 0 && (!d_offsets || !d_valid)) || (capacity > 0 && !d_fields)) return MSJ_ERR_BAD_ARGUMENT;
    if (bytes_len > 0 && !d_bytes) return MSJ_ERR_BAD_ARGUMENT;
    if (rows >= (1ull << 40) || capacity >= (1ull << 40) || bytes_len >= msj::mstr::kMaxBytes) return MSJ_CAPACITY;
    if ((const void *)d_result == (const void *)d_select) return MSJ_ERR_BAD_ARGUMENT;
    if (!aligned(d_fields, 16) || !all_aligned(8, d_offsets, d_n_rows, d_result, d_select)) return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->match_ws, msj_match_strings_workspace_bytes(rows, patterns->n_patterns));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_match_strings(patterns->blob.p, patterns->n_patterns, patterns->max_pieces, d_offsets, d_valid, rows, d_n_rows,
                                             d_bytes, bytes_len, d_fields, capacity, d_result, d_select, ctx->match_ws.p, stream));
}

int32_t msj_bucket_rows_device(msj_ctx *ctx, const msj_field *d_rows, const msj_select_documents_result *d_rows_select, int64_t width, int64_t origin,
                               uint32_t flags, msj_field *d_out, uint64_t capacity, msj_bucket_rows_result *d_result,
                               msj_select_documents_result *d_out_select, void *stream) {
    if (!ctx || !d_result || !d_rows_select) return MSJ_ERR_BAD_ARGUMENT;
    if (capacity > 0 && (!d_rows || !d_out)) return MSJ_ERR_BAD_ARGUMENT;
    if (msj::gkeys::bad_bucket(width, flags)) return MSJ_ERR_BAD_ARGUMENT;
    if (capacity >= (1ull << 40)) return MSJ_CAPACITY;  // (the extent below: no overflow)
    if (d_out && d_rows && d_out != d_rows) {           // in place, or no byte shared
        const uintptr_t a = reinterpret_cast<uintptr_t>(d_rows), b = reinterpret_cast<uintptr_t>(d_out);
        if (a < b + 16 * capacity && b < a + 16 * capacity) return MSJ_ERR_BAD_ARGUMENT;
    }
    if ((const void *)d_result == (const void *)d_rows_select || (const void *)d_result == (const void *)d_out_select ||
        d_out_select == d_rows_select)
        return MSJ_ERR_BAD_ARGUMENT;
    if (!all_aligned(16, d_rows, d_out) || !all_aligned(8, d_rows_select, d_result, d_out_select)) return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->bucket_ws, msj_bucket_rows_workspace_bytes(capacity));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_bucket_rows(d_rows, d_rows_select, width, origin, d_out, capacity, d_result, d_out_select, ctx->bucket_ws.p, stream));
}

int32_t msj_group_keys_device(msj_ctx *ctx, const msj_key_part *parts, uint32_t n_parts, uint64_t stride,
                              const msj_select_documents_result *d_rows_select, uint64_t *d_offsets, uint8_t *d_valid, uint8_t *d_bytes,
                              uint64_t capacity, uint64_t bytes_capacity, msj_group_keys_result *d_result, void *stream) {
    if (!ctx || !d_result || !d_rows_select || !parts) return MSJ_ERR_BAD_ARGUMENT;
    if (n_parts == 0 || n_parts > msj::gkeys::kMaxParts) return MSJ_ERR_BAD_ARGUMENT;
    for (uint32_t j = 0; j < n_parts; j++)
        if (msj::gkeys::bad_part(parts[j].kind, parts[j].flags)) return MSJ_ERR_BAD_ARGUMENT;
    for (uint32_t j = 0; j < n_parts; j++)
        if (stride > 0 && !parts[j].d_column) return MSJ_ERR_BAD_ARGUMENT;
    if (capacity > 0 && (!d_offsets || !d_valid || !d_bytes)) return MSJ_ERR_BAD_ARGUMENT;
    if ((const void *)d_result == (const void *)d_rows_select) return MSJ_ERR_BAD_ARGUMENT;
    for (uint32_t j = 0; j < n_parts; j++)
        if (!aligned(parts[j].d_column, parts[j].kind == MSJ_KEY_NUMBER ? 16 : 4)) return MSJ_ERR_BAD_ARGUMENT;
    if (!aligned(d_bytes, 16) || !all_aligned(8, d_offsets, d_rows_select, d_result)) return MSJ_ERR_BAD_ARGUMENT;
    const int32_t rc = begin_call(ctx, ctx->gkeys_ws, msj_group_keys_workspace_bytes(capacity));
    if (rc != MSJ_SUCCESS) return rc;
    return launched(msj_launch_group_keys(parts, n_parts, stride, d_rows_select, d_offsets, d_valid, d_bytes, capacity, bytes_capacity, d_result,
                                          ctx->gkeys_ws.p, stream));
}

int32_t msj_debug_set_span_limits(msj_ctx *ctx, uint32_t lds_limit_bytes, uint32_t fix_capacity) {
    if (!ctx) return MSJ_ERR_BAD_ARGUMENT;
    ctx->tok_opts.lds_limit = lds_limit_bytes;
    ctx->tok_opts.fix_cap = fix_capacity;
    return MSJ_SUCCESS;
}
int32_t msj_debug_set_span_mode(msj_ctx *ctx, uint32_t mode) {
    if (!ctx || mode > 2u) return MSJ_ERR_BAD_ARGUMENT;
    ctx->tok_opts.span_mode = mode;
    return MSJ_SUCCESS;
}

}  // extern "C"
