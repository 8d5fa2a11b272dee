// launch.h -- launch interface between stage2_api.cpp and the kernel files behind stage 1: tokens_kernel.hip (rows f1 /
// f2 / f4 of SURVEY.md section 8), documents_kernel.hip, numbers_kernel.hip, validate_kernel.hip,
// validate_docs_kernel.hip, tape_kernel.hip, tape_docs_kernel.hip, select_kernel.hip, string_column_kernel.hip,
// array_column_kernel.hip, select_elements_kernel.hip, array_elements_kernel.hip, object_entries_kernel.hip, raw_column_kernel.hip, dictionary_kernel.hip, dictionary_extend_kernel.hip, filter_rows_kernel.hip, cast_strings_kernel.hip, aggregate_kernel.hip, sort_rows_kernel.hip, join_rows_kernel.hip, dictionary_order_kernel.hip (the last three over
// radix_block.h's one radix pass), match_strings_kernel.hip, group_keys_kernel.hip.  Every launcher and every internal workspace size is declared
// here and nowhere else; the file that defines one and the file that calls it both include this header, so the compiler
// compares the two signatures (C linkage alone would not).  The calls over a window take what they read as named views
// (msj_token_view, msj_split_view, msj_number_view): two arrays of one type cannot change places on the way.
// (stage 1 has stage1_kernel.h; the exported *_workspace_bytes are declared in include/msj_stage1.h.)
#pragma once
#include <stdint.h>

#include "../../include/msj_stage1.h"

// ---- how every call behind stage 1 carves its one device workspace (host only) ----
// A call has ONE function that takes its arrays from a carver, in order.  The launcher runs it over the workspace and gets
// the pointers; the exported msj_*_workspace_bytes runs it over no base at all and gets the size, to which it adds the
// call's tail slack.  So a size cannot disagree with the layout it reserves room for ("A call's size is its
// layout, measured").  The offset is an integer: measuring forms no pointer.
struct msj_carver {
    uint8_t *base;       // null: measure only
    uint64_t bytes = 0;  // carved so far
    explicit msj_carver(void *ws) : base(static_cast<uint8_t *>(ws)) {}
    // `count` elements of T from here on; what comes next starts at the next multiple of `round` bytes (a power of two)
    template <class T>
    T *take(uint64_t count, uint64_t round = 16) {
        const uint64_t at = bytes;
        bytes = (at + count * sizeof(T) + round - 1) & ~(round - 1);
        return base ? reinterpret_cast<T *>(base + at) : nullptr;
    }
};
// a layout function over a workspace: what it returns; and over none: the bytes it carves
template <class Layout, class... Args>
auto msj_place(Layout layout, void *ws, Args... args) {
    msj_carver c(ws);
    return layout(c, args...);
}
template <class Layout, class... Args>
uint64_t msj_measure(Layout layout, Args... args) {
    msj_carver c(nullptr);
    layout(c, args...);
    return c.bytes;
}

// What a token call takes besides its arrays.  The first three are TEST HOOKS kept per context
// (msj_debug_set_span_limits / msj_debug_set_span_mode; 0xFFFFFFFF / 0 = the built-in behaviour): a hook left set by
// one test or tool cannot change the data path of another context.
struct msj_token_opts {
    uint32_t span_mode = 0;             // 0 by the density of the index, 1 the kernel organised by tokens, 2 by tiles
    uint32_t lds_limit = 0xFFFFFFFFu;   // stretches over this many bytes take the span kernels' global-memory path
    uint32_t fix_cap = 0xFFFFFFFFu;     // entries of the fix-up list
    // the msj_tokens_result (device) of the call that covered the tokens IN FRONT of this call's, or null at the start of
    // a stream: the running depth walk_document keeps (json_iterator.mojo:84-90,173-180) goes on from its final_depth,
    // and this call's min / max / final are those of the stream so far
    const msj_tokens_result *d_prev = nullptr;
    // msj_stage2_prep_segments (bracket partners over a whole shard): match[] values are positions in the SHARD's output
    // arrays -- this call's token index + match_bias -- and the brackets this call could not pair (their container is cut
    // by the call's border) are left in d_resid for the stitch behind the last segment (tokens_kernel.hip, "residuals")
    uint32_t match_bias = 0;
    uint32_t *d_resid = nullptr;
    // msj_*_pairs_device: the containers as {open, close} records in the order of their opening brackets (msj_bracket_pair),
    // instead of a partner index per token
    msj_bracket_pair *d_pairs = nullptr;
};

// residual brackets of one call (device, uint32 words): [0] unclosed opening brackets, [1] closing brackets without a
// partner, [2] the call's minimum running depth m (int32; its start depth included), [3] spare; then MSJ_RESID_CAP
// positions of the former -- entry j = the one at depth m + j -- and MSJ_RESID_CAP of the latter -- entry k = the one at
// depth m + k (token indices local to the call)
#define MSJ_RESID_CAP 65536u
#define MSJ_RESID_WORDS (4u + 2u * MSJ_RESID_CAP)
#define MSJ_STITCH_MAX_SEGMENTS 32u
struct msj_stitch_args {
    uint32_t n_segments;
    uint32_t offsets[MSJ_STITCH_MAX_SEGMENTS];       // element offset of every segment's slices in the shard's output arrays
    const uint32_t *resid[MSJ_STITCH_MAX_SEGMENTS];  // its residual brackets
};
int msj_launch_stitch_partners(const msj_stitch_args &a, uint32_t *d_match, msj_tokens_result *d_results, const msj_tokens_result *d_prev,
                               void *stream);

extern "C" uint64_t msj_tokens_workspace_bytes(uint64_t n, int with_match);
extern "C" uint64_t msj_stage2_prep_workspace_bytes(uint64_t n, uint64_t len, int with_match);
extern "C" uint64_t msj_span_fix_bytes(void);
extern "C" void *msj_tokens_doc_aggregates(int32_t *d_ws, uint64_t n);
extern "C" int msj_launch_depth_from_types(const uint8_t *d_type, uint64_t n, int32_t *d_depth, uint32_t *d_match, msj_tokens_result *d_result,
                                           int32_t *d_ws, void *stream, const msj_token_opts &o);
int msj_launch_tokens(const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n, uint8_t *d_type, int32_t *d_depth,
                      uint32_t *d_match, msj_tokens_result *d_result, int32_t *d_ws, void *stream, const msj_token_opts &o);
int msj_launch_token_spans(const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n, uint32_t *d_end, uint8_t *d_flags,
                           int32_t *d_ws, uint32_t *d_fix, void *stream, const msj_token_opts &o);
int msj_launch_stage2_prep(const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n, uint8_t *d_type, int32_t *d_depth,
                           uint32_t *d_match, uint32_t *d_end, uint8_t *d_flags, msj_tokens_result *d_result, int32_t *d_ws,
                           uint32_t *d_fix, void *stream, const msj_token_opts &o);

// ---- documents_kernel.hip ----
extern "C" uint64_t msj_documents_workspace_bytes(uint64_t n);
// d_block_agg: the block aggregates the token pre-pass left for exactly these arrays (msj_tokens_doc_aggregates), or null
extern "C" int msj_launch_documents(const uint8_t *d_buf, uint64_t len, int is_final, const uint32_t *d_idx, uint64_t n,
                                    const uint8_t *d_type, const int32_t *d_depth, const msj_carry *d_carry, uint32_t *d_doc_first, uint64_t capacity,
                                    msj_documents_result *d_result, void *d_ws, const void *d_block_agg, void *stream);

// ---- numbers_kernel.hip ----
extern "C" int msj_launch_number_values(const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n, const uint8_t *d_flags,
                                        msj_number *d_numbers, uint64_t capacity, msj_numbers_result *d_result, void *d_ws, void *stream);

// ---- what the calls over a window read, members in the ABI's order: the token arrays (msj_stage2_prep_device's outputs
// over d_buf / d_idx), the split into documents (msj_documents_device), the number records (msj_number_values_device) ----
struct msj_token_view {
    const uint8_t *d_buf;
    uint64_t len;
    const uint32_t *d_idx;
    uint64_t n;
    const uint8_t *d_type;
    const int32_t *d_depth;
    const uint32_t *d_match, *d_end;
    const uint8_t *d_flags;
};
struct msj_split_view {
    const uint32_t *d_doc_first;
    const msj_documents_result *d_docs;
};
struct msj_number_view {
    const msj_number *d_numbers;
    uint64_t numbers_capacity;
    const msj_numbers_result *d_numbers_result;
};

// ---- validate_kernel.hip ----
extern "C" int msj_launch_validate(const msj_token_view &t, const msj_number_view &nv, uint32_t max_depth, msj_validate_result *d_result,
                                   void *d_ws, void *stream);

// ---- validate_docs_kernel.hip ----
extern "C" int msj_launch_validate_documents(const msj_token_view &t, const msj_split_view &sp, const msj_number_view &nv, uint32_t max_depth,
                                             msj_document_verdict *d_verdicts, uint64_t capacity, msj_validate_documents_result *d_result,
                                             void *d_ws, void *stream);

// ---- tape_kernel.hip ----
extern "C" int msj_launch_tape(const msj_token_view &t, const msj_number_view &nv, const msj_validate_result *d_verdict, uint64_t *d_tape,
                               uint64_t tape_capacity, uint8_t *d_string_buf, uint64_t string_capacity, msj_tape_result *d_result,
                               void *d_ws, void *stream);

// ---- tape_docs_kernel.hip ----
extern "C" int msj_launch_tape_documents(const msj_token_view &t, const msj_split_view &sp, const msj_number_view &nv,
                                         const msj_document_verdict *d_verdicts, uint64_t *d_tape, uint64_t tape_capacity,
                                         uint8_t *d_string_buf, uint64_t string_capacity, msj_document_tape *d_doc_tapes, uint64_t capacity,
                                         msj_tape_documents_result *d_result, void *d_ws, void *stream);

// ---- select_kernel.hip ----
// d_paths: the compiled paths (select_math.h: Paths) in device memory; n_paths / max_levels: what the host knows of them
extern "C" int msj_launch_select_documents(const void *d_paths, uint32_t n_paths, uint32_t max_levels, const msj_token_view &t,
                                           const msj_split_view &sp, const msj_number_view &nv, const msj_document_verdict *d_verdicts,
                                           msj_field *d_fields, uint64_t capacity, msj_select_documents_result *d_result, void *d_ws,
                                           void *stream);

// ---- string_column_kernel.hip ----
extern "C" int msj_launch_string_column(const uint8_t *d_buf, uint64_t len, const msj_field *d_column, const msj_select_documents_result *d_select,
                                        uint64_t *d_offsets, uint8_t *d_valid, uint64_t capacity, uint8_t *d_bytes, uint64_t bytes_capacity,
                                        msj_string_column_result *d_result, void *d_ws, void *stream);

// ---- array_column_kernel.hip ----
// (t.d_buf / t.len are not read)
extern "C" int msj_launch_array_column(const msj_token_view &t, const msj_split_view &sp, const msj_number_view &nv, const msj_field *d_column,
                                       const msj_select_documents_result *d_select, uint64_t *d_offsets, uint8_t *d_valid, uint64_t capacity,
                                       msj_field *d_elements, uint64_t elements_capacity, msj_array_column_result *d_result,
                                       msj_select_documents_result *d_elements_select, void *d_ws, void *stream);

// ---- select_elements_kernel.hip ----
// d_paths / n_paths / max_levels as for msj_launch_select_documents; d_rows / d_rows_select: the element records of an
// array column
extern "C" int msj_launch_select_elements(const void *d_paths, uint32_t n_paths, uint32_t max_levels, const msj_token_view &t,
                                          const msj_number_view &nv, const msj_field *d_rows, const msj_select_documents_result *d_rows_select,
                                          msj_field *d_fields, uint64_t capacity, msj_select_documents_result *d_result, void *d_ws,
                                          void *stream);

// ---- array_elements_kernel.hip ----
// (t.d_buf / t.len are not read); d_rows / d_rows_select: the element records of an array column, or one path's records of
// msj_launch_select_elements
extern "C" int msj_launch_array_elements(const msj_token_view &t, const msj_number_view &nv, const msj_field *d_rows,
                                         const msj_select_documents_result *d_rows_select, uint64_t *d_offsets, uint8_t *d_valid,
                                         uint64_t capacity, msj_field *d_elements, uint64_t elements_capacity, msj_array_column_result *d_result,
                                         msj_select_documents_result *d_elements_select, void *d_ws, void *stream);

// ---- object_entries_kernel.hip ----
// (t.d_buf / t.len are not read); d_rows / d_rows_select: any ascending records with their select result, as for
// msj_launch_array_elements; d_keys / d_values: both or neither
extern "C" int msj_launch_object_entries(const msj_token_view &t, const msj_number_view &nv, const msj_field *d_rows,
                                         const msj_select_documents_result *d_rows_select, uint64_t *d_offsets, uint8_t *d_valid,
                                         uint64_t capacity, msj_field *d_keys, msj_field *d_values, uint64_t entries_capacity,
                                         msj_object_entries_result *d_result, msj_select_documents_result *d_keys_select,
                                         msj_select_documents_result *d_values_select, void *d_ws, void *stream);

// ---- raw_column_kernel.hip ----
// (t.d_depth and t.d_match are not read); d_rows / d_rows_select: any records with their select result, in any order;
// flags: MSJ_RAW_COMPACT or 0
extern "C" int msj_launch_raw_column(const msj_token_view &t, const msj_field *d_rows, const msj_select_documents_result *d_rows_select,
                                     uint64_t *d_offsets, uint8_t *d_valid, uint64_t capacity, uint8_t *d_bytes, uint64_t bytes_capacity,
                                     uint32_t flags, msj_raw_column_result *d_result, void *d_ws, void *stream);

// ---- dictionary_kernel.hip ----
// the (d_offsets, d_valid, d_bytes) layout of a byte column; d_n_rows: the rows on the device, or null for `rows`; the three
// dictionary arrays null: the layout-only form; flags: MSJ_DICTIONARY_WEAK_HASH or 0
extern "C" int msj_launch_dictionary(const uint64_t *d_offsets, const uint8_t *d_valid, uint64_t rows, const uint64_t *d_n_rows,
                                     const uint8_t *d_bytes, uint64_t bytes_len, int32_t *d_codes, uint64_t *d_dict_offsets,
                                     uint32_t *d_dict_first, uint64_t dict_capacity, uint8_t *d_dict_bytes, uint64_t dict_bytes_capacity,
                                     uint32_t flags, msj_dictionary_result *d_result, void *d_ws, void *stream);

// ---- dictionary_extend_kernel.hip ----
// the same column; n_prior / d_n_prior: P, the entries the dictionary arrays hold already (the word on the device wins); the
// three dictionary arrays null: the layout-only form (P = 0); flags: MSJ_DICTIONARY_WEAK_HASH | MSJ_DICTIONARY_FROZEN
extern "C" int msj_launch_dictionary_extend(const uint64_t *d_offsets, const uint8_t *d_valid, uint64_t rows, const uint64_t *d_n_rows,
                                            const uint8_t *d_bytes, uint64_t bytes_len, uint64_t n_prior, const uint64_t *d_n_prior,
                                            int32_t *d_codes, uint64_t *d_dict_offsets, uint32_t *d_dict_first, uint64_t dict_capacity,
                                            uint8_t *d_dict_bytes, uint64_t dict_bytes_capacity, uint32_t flags,
                                            msj_dictionary_extend_result *d_result, void *d_ws, void *stream);

// ---- filter_rows_kernel.hip ----
// d_predicates: the compiled predicates (filter_rows_math.h: Predicates) in device memory; d_fields: column c at c * stride;
// d_kept null: the mask-only form; the two list arrays: both or neither; d_list_n_rows: the list rows on the device, or null
// for `list_rows`
extern "C" int msj_launch_filter_rows(const void *d_predicates, const uint8_t *d_buf, uint64_t len, const msj_field *d_fields, uint64_t stride,
                                      const msj_select_documents_result *d_rows_select, uint8_t *d_keep, uint32_t *d_kept, uint64_t capacity,
                                      const uint64_t *d_list_offsets, uint64_t list_rows, const uint64_t *d_list_n_rows,
                                      uint64_t *d_list_offsets_out, msj_filter_rows_result *d_result,
                                      msj_select_documents_result *d_kept_select, void *d_ws, void *stream);
// d_take / d_take_select: any row numbers with the select result that counts them; `stride` is also the room of a column
extern "C" int msj_launch_take_rows(const uint32_t *d_take, const msj_select_documents_result *d_take_select, const msj_field *d_fields,
                                    uint64_t stride, uint32_t n_columns, const msj_select_documents_result *d_rows_select, msj_field *d_out,
                                    uint64_t out_stride, uint64_t out_capacity, msj_take_rows_result *d_result,
                                    msj_select_documents_result *d_out_select, void *d_ws, void *stream);

// ---- cast_strings_kernel.hip ----
// d_rows / d_rows_select: any records with their select result; kind / unit / flags: checked by the caller
// (cast_strings_math.h: check_kind); fetch: MSJ_CAST_FETCH_*; d_out == d_rows: in place
extern "C" int msj_launch_cast_strings(const uint8_t *d_buf, uint64_t len, const msj_field *d_rows, const msj_select_documents_result *d_rows_select,
                                       uint32_t kind, uint32_t unit, uint32_t flags, uint32_t fetch, msj_field *d_out, uint64_t capacity,
                                       msj_cast_strings_result *d_result, msj_select_documents_result *d_out_select, void *d_ws, void *stream);

// ---- aggregate_kernel.hip ----
// d_fields: column c at c * stride, `stride` also the room of a column and of d_codes (null: every row is group 0);
// d_n_groups: G on the device, or null for `n_groups`; d_groups: column c's records at c * groups_capacity; lds_groups: the
// most groups the LDS path takes (at most kAggregateMaxLdsGroups)
constexpr uint32_t kAggregateMaxLdsGroups = 256;
extern "C" int msj_launch_aggregate(const msj_field *d_fields, uint64_t stride, uint32_t n_columns, const msj_select_documents_result *d_rows_select,
                                    const int32_t *d_codes, uint64_t n_groups, const uint64_t *d_n_groups, msj_aggregate *d_groups,
                                    uint64_t groups_capacity, uint32_t lds_groups, msj_aggregate_result *d_result, void *d_ws, void *stream);

// ---- sort_rows_kernel.hip ----
// d_fields: ONE column, `stride` its room; d_rows_in / d_rows_in_select: both or neither; flags: checked by the caller;
// mode: 0 the path chosen on the device, 1 always the full sort, 2 always the selection (msj_debug_set_sort_mode)
extern "C" int msj_launch_sort_rows(const msj_field *d_fields, uint64_t stride, const msj_select_documents_result *d_rows_select,
                                    const uint32_t *d_rows_in, const msj_select_documents_result *d_rows_in_select, uint32_t flags, uint64_t limit,
                                    uint32_t mode, uint32_t *d_order, uint64_t capacity, msj_sort_rows_result *d_result,
                                    msj_select_documents_result *d_order_select, void *d_ws, void *stream);

// ---- join_rows_kernel.hip ----
// the two key columns with their rooms and the counts on the device (or null for the room); n_keys / d_n_keys: G; flags:
// MSJ_JOIN_*, checked by the caller; d_right_rows, d_offsets and the two select results: each may be null
extern "C" int msj_launch_join_rows(const int32_t *d_left_keys, uint64_t left_rows, const uint64_t *d_n_left, const int32_t *d_right_keys,
                                    uint64_t right_rows, const uint64_t *d_n_right, uint64_t n_keys, const uint64_t *d_n_keys,
                                    uint64_t keys_capacity, uint32_t flags, uint32_t *d_left_rows, uint32_t *d_right_rows, uint64_t pairs_capacity,
                                    uint64_t *d_offsets, msj_join_rows_result *d_result, msj_select_documents_result *d_left_select,
                                    msj_select_documents_result *d_right_select, void *d_ws, void *stream);

// ---- dictionary_order_kernel.hip ----
// the (d_dict_offsets, d_dict_bytes) layout of a dictionary; n_entries / d_n_entries: V (the word on the device wins); depth,
// max_rounds, flags: checked by the caller (dictionary_order_math.h: bad_numbers); mode: 0 the path by capacity, 1 always the
// grid path, 2 the one-workgroup path wherever it fits (msj_debug_set_order_mode)
extern "C" int msj_launch_dictionary_order(const uint64_t *d_dict_offsets, const uint8_t *d_dict_bytes, uint64_t dict_bytes_capacity,
                                           uint64_t n_entries, const uint64_t *d_n_entries, uint64_t capacity, uint64_t depth, uint32_t max_rounds,
                                           uint32_t flags, uint32_t mode, uint32_t *d_sorted, uint32_t *d_rank,
                                           msj_dictionary_order_result *d_result, void *d_ws, void *stream);
// `rows` / `capacity`: the rooms of d_codes / d_fields; the two results are cleared on the stream in front of the one kernel
extern "C" int msj_launch_rank_rows(const int32_t *d_codes, uint64_t rows, const uint64_t *d_n_rows, const uint32_t *d_rank, uint64_t rank_capacity,
                                    const msj_dictionary_order_result *d_order_result, msj_field *d_fields, uint64_t capacity,
                                    msj_rank_rows_result *d_result, msj_select_documents_result *d_select, void *stream);

// ---- match_strings_kernel.hip ----
// d_patterns: the compiled patterns (match_strings_math.h: Patterns) in device memory; n_patterns / max_pieces: what the host
// knows of them; the (d_offsets, d_valid, d_bytes) layout of a byte column; d_n_rows: the rows on the device, or null for
// `rows`; d_fields: pattern p's records at p * capacity; the two results are cleared on the stream in front of the kernels
extern "C" int msj_launch_match_strings(const void *d_patterns, uint32_t n_patterns, uint32_t max_pieces, const uint64_t *d_offsets,
                                        const uint8_t *d_valid, uint64_t rows, const uint64_t *d_n_rows, const uint8_t *d_bytes, uint64_t bytes_len,
                                        msj_field *d_fields, uint64_t capacity, msj_match_strings_result *d_result,
                                        msj_select_documents_result *d_select, void *d_ws, void *stream);

// ---- group_keys_kernel.hip ----
// d_rows / d_rows_select: any records with their select result; width >= 1; d_out == d_rows: in place
extern "C" int msj_launch_bucket_rows(const msj_field *d_rows, const msj_select_documents_result *d_rows_select, int64_t width, int64_t origin,
                                      msj_field *d_out, uint64_t capacity, msj_bucket_rows_result *d_result,
                                      msj_select_documents_result *d_out_select, void *d_ws, void *stream);
// parts: the HOST array, kinds and flags checked by the caller (group_keys_math.h: bad_part); `stride` the room of every column
extern "C" int msj_launch_group_keys(const msj_key_part *parts, uint32_t n_parts, uint64_t stride, const msj_select_documents_result *d_rows_select,
                                     uint64_t *d_offsets, uint8_t *d_valid, uint8_t *d_bytes, uint64_t capacity, uint64_t bytes_capacity,
                                     msj_group_keys_result *d_result, void *d_ws, void *stream);
