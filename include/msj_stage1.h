/*
 * msj_stage1.h -- C ABI of the MI355X-native stage-1 JSON structural indexer.
 *
 * This is the drop-in boundary for ONE path of gabrieldemarmiesse/mojo-simdjson:
 * the call
 *     JsonStructuralIndexer.index[128](buffer, self)
 * made by DomParserImplementation.stage1(Span[UInt8])
 * (reference: src/mojo_simdjson/include/generic/dom_parser_implementation.mojo:65-69,
 *  callee src/mojo_simdjson/generic/stage1/json_structural_indexer.mojo:81-108,147-186).
 * The reference has no FFI of its own (it is a plain Mojo static-method call);
 * the entry points below are what a Mojo `sys.ffi.DLHandle` binding for that
 * call site binds (INTEGRATION.md shows the shim).  Plain pointers and sizes
 * only; no torch / HIP types appear in any signature (`stream` is an opaque
 * hipStream_t passed as void*).
 *
 * Contract left behind by a successful call (what stage 2 reads,
 * generic/stage2/json_iterator.mojo:28-38,256-288, and what the reference's
 * own test asserts, tests/test_stage_1.mojo:43-82):
 *   idx[0..n)   strictly increasing uint32 byte offsets of structural starts
 *   idx[n]   = (uint32) len      \
 *   idx[n+1] = (uint32) len       } json_structural_indexer.mojo:167-173
 *   idx[n+2] = 0                 /
 *   *n_out   = n                   (parser.n_structural_indexes, :160-165)
 * Return value: the reference's integer error code (errors.mojo:2-36):
 *   0 SUCCESS, 1 CAPACITY, 13 EMPTY, 14 UNESCAPED_CHARS, 15 UNCLOSED_STRING,
 *   24 UNEXPECTED_ERROR; 11 UTF8_ERROR only when MSJ_FLAG_STRICT_UTF8 is set
 *   (the reference's UTF-8 checker is an empty stub that always succeeds,
 *   json_structural_indexer.mojo:16-30, so reference parity ignores UTF-8).
 * Error precedence follows finish() (:147-186): 15, then 14, then (trailer
 * written) 13, then 11.  On 14/15 the reference returns before writing n and
 * the trailer; the host-pointer entry points do the same (n_out untouched).
 *
 * Capacity: the reference allocates exactly `len` slots (allocate(len),
 * dom_parser_implementation.mojo:85-89) but writes up to n+3 <= len+3 words.
 * Callers of this ABI must provide idx_capacity >= n + 3; len + 3 is always
 * enough.  A smaller buffer is accepted: writes are clipped and CAPACITY (1)
 * is returned if n + 3 > idx_capacity.
 *
 * HIP backend only: every entry point fails with MSJ_ERR_NO_DEVICE (-2) when no
 * gfx950 device / HIP runtime is usable.  There is no CPU fallback.
 */
#ifndef MSJ_STAGE1_H
#define MSJ_STAGE1_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* reference error codes, src/mojo_simdjson/errors.mojo:2-26 */
#define MSJ_SUCCESS 0
#define MSJ_CAPACITY 1
#define MSJ_MEMALLOC 2
#define MSJ_UTF8_ERROR 11
#define MSJ_EMPTY 13
#define MSJ_UNESCAPED_CHARS 14
#define MSJ_UNCLOSED_STRING 15
#define MSJ_UNEXPECTED_ERROR 24
/* library-level failures (negative: never collide with reference codes) */
#define MSJ_ERR_BAD_ARGUMENT (-1)
#define MSJ_ERR_NO_DEVICE (-2)
#define MSJ_ERR_HIP (-3)

/* flags */
#define MSJ_FLAG_STRICT_UTF8 1u /* return 11 when the input is not valid UTF-8 */
#define MSJ_FLAG_NO_UTF8 2u     /* skip UTF-8 validation entirely (verdict = 0) */
/* Index through the two-pass kernels (summary, scan, emission: no workgroup ever waits for another one)
 * instead of the single-pass kernel.  Slower; what the library itself falls back to when a single-pass
 * launch reports internal_error (an inter-workgroup wait ran into its 2 s bound), so that a valid document
 * never comes back as UNEXPECTED_ERROR (24).  Same results bit for bit. */
#define MSJ_FLAG_TWO_PASS 0x100u
/* Test hook: the single-pass kernel's resolver idles ~2 ms before it starts (with msj_debug_set_wait_ticks
 * this forces the wait-expiry path). */
#define MSJ_FLAG_DEBUG_STALL 0x200u
/* The first n (0..15) bytes of the buffer read as blanks: a window of a document stream starts at
 * a document, its 16-byte aligned base a few bytes earlier (msj_documents_device, resume_offset). */
#define MSJ_FLAG_SKIP(n) (((uint32_t)(n) & 15u) << 24)

/* SIMDJSON_MAXSIZE_BYTES, src/mojo_simdjson/include/base.mojo:2: indices are
 * uint32, so one segment of input is limited to this many bytes. */
#define MSJ_MAX_SEGMENT_BYTES 0xFFFFFFFFull

/*
 * Carry state at a byte boundary of the input stream: everything the
 * reference's scanners carry from one 64-byte block to the next
 * (JsonEscapeScanner.next_is_escaped json_escape_scanner.mojo:13,
 *  JsonStringScanner.prev_in_string json_string_scanner.mojo:49,
 *  JsonScanner.prev_scalar json_scanner.mojo:57,
 *  JsonStructuralIndexer.unescaped_chars_error json_structural_indexer.mojo:72,
 *  BitIndexer.tail :34) plus the UTF-8 verdict so far.  Lives in device
 * memory; 64 bytes.
 */
typedef struct msj_carry {
    uint64_t count;           /* structurals emitted so far (BitIndexer.tail - base) */
    uint64_t bytes;           /* input bytes consumed so far */
    uint32_t in_string;       /* 1 = inside a string (prev_in_string != 0) */
    uint32_t next_is_escaped; /* 1 = next byte is escaped */
    uint32_t prev_scalar;     /* 1 = previous byte was a non-quote scalar */
    uint32_t unescaped_error; /* sticky: control char seen inside a string */
    uint32_t utf8_error;      /* sticky: invalid UTF-8 seen */
    uint32_t internal_error;  /* sticky: a wait inside the single-pass kernel ran into its bound */
    int32_t code;             /* reference return code, valid after a FINAL segment */
    uint32_t capacity_error;  /* sticky: the index buffer could not hold every index so far (+ the 3 trailer words
                                 on a FINAL segment); writes were clipped.  A FINAL segment also reports it as
                                 code = MSJ_CAPACITY, a non-final shard only here (msj_shard_global_code reads it) */
    uint32_t reserved[4];     /* [0], written by every shard call into its carry_out: bit 31 set, bits 0..2 the in_string /
                                 next_is_escaped / prev_scalar the call STARTED from (handed down the chain of a shard of
                                 several segments): what a rank of a sharded stream reports as the carry it used; [1..3] 0 */
} msj_carry;
#define MSJ_CARRY_ECHO_VALID 0x80000000u

/* One <= 4 GiB piece of a larger input: offsets in
 * idx[index_begin .. index_begin+count) are relative to byte_base. */
typedef struct msj_segment {
    uint64_t byte_base;
    uint64_t byte_len;
    uint64_t index_begin;
    uint64_t count;
} msj_segment;

typedef struct msj_ctx msj_ctx;

/* Library / device probes.  msj_device_count() returns the number of HIP
 * devices (0 when none or no runtime); never initialises a context. */
int32_t msj_device_count(void);
/* "mojo-simdjson_amd stage1 <version> (gfx950) src:<12 hex digits>": the digits are a hash of the stage-1 kernel's
 * sources; measurements kept beside the code (profiles/traffic.json) name the kernel they were taken with. */
const char *msj_version(void);

/* Context: owns the per-device workspace (tile descriptors, carry structs,
 * staging buffers).  Not re-entrant on the host: one thread per context at a
 * time, matching the reference (one parser = one synchronous call).  On the
 * device (tests/test_stream_order.py):
 *  - any number of calls of one context may be in flight on ONE stream: a
 *    call's workspace is reused by the next call in stream order, and no call
 *    waits for the one in front of it;
 *  - calls of one context on DIFFERENT streams share those workspaces: the
 *    caller orders them (an event, or a synchronisation in between);
 *  - a call that has to grow a workspace synchronises the device first, once
 *    per size (nothing of the context may still be using the old block): a
 *    chain that has run once over its largest window never waits again. */
int32_t msj_ctx_create(int32_t device, msj_ctx **out);
void msj_ctx_destroy(msj_ctx *ctx);
int32_t msj_ctx_device(const msj_ctx *ctx); /* the HIP device the context was created on (-1: NULL) */

/*
 * msj_stage1 -- host-pointer form; replaces
 *   JsonStructuralIndexer.index[128](buffer, self)   (json_structural_indexer.mojo:81-108)
 * `buf`/`idx_out` are host memory; the library copies the input to the device,
 * runs the HIP kernels, and copies back idx[0..n+3).  Uses a process-wide
 * default context on device 0 (created on first use).
 * utf8_verdict_out (optional): 0 valid, 11 invalid -- reported separately from
 * the return code unless MSJ_FLAG_STRICT_UTF8.
 * On CAPACITY, UNCLOSED_STRING, UNESCAPED_CHARS and UNEXPECTED_ERROR n_out is
 * not set and no trailer is written (as in the reference); inputs past the
 * small-input path then leave min(n, idx_capacity) indices in idx_out, the
 * same words whether the call staged plainly or through the pinned pipeline.
 */
int32_t msj_stage1(const uint8_t *buf, uint64_t len, uint32_t *idx_out, uint64_t idx_capacity,
                   uint64_t *n_out, int32_t *utf8_verdict_out, uint32_t flags);

/* Same, on an explicit context. */
int32_t msj_stage1_ctx(msj_ctx *ctx, const uint8_t *buf, uint64_t len, uint32_t *idx_out,
                       uint64_t idx_capacity, uint64_t *n_out, int32_t *utf8_verdict_out,
                       uint32_t flags);

/*
 * Optional: pin a caller-owned host range once (hipHostRegister) and remember it.  msj_stage1 / msj_stage1_ctx
 * calls whose input and / or index array lie inside a registered range move that side by DMA straight from / into
 * the caller's memory instead of staging it through the library's pinned rings (two host copies less per byte).
 * For buffers the host reuses: the reference allocates structural_indexes once per parser, in allocate()
 * (include/generic/dom_parser_implementation.mojo:85-89) -- the shim registers it there and unregisters it where the
 * parser is destroyed.  Pinning costs ~50 us per MiB, once.  The range must stay allocated until
 * msj_host_unregister (msj_ctx_destroy unregisters what is left).  ctx NULL: the default context of msj_stage1.
 * Returns MSJ_SUCCESS, MSJ_ERR_BAD_ARGUMENT (null / empty / ptr not the start of a registered range), MSJ_ERR_HIP.
 */
int32_t msj_host_register(msj_ctx *ctx, void *ptr, uint64_t bytes);
/*
 * msj_host_placement -- where the host side of msj_stage1's pipeline lives, as one line of JSON in `out` (MSJ_CAPACITY if it
 * does not fit): the GPU's PCI address and NUMA node, how many CPUs of that node the process may use, whether the
 * pipeline exists yet (the first large call creates it), how many of its copy workers are bound to the GPU's node, the
 * node its pinned rings were placed on, the PCIe link's speed and width (sysfs; -1 / "" = the kernel does not say).
 * ctx NULL = the default context of msj_stage1.  A measurement aid: bench.py records it beside `end_to_end`.
 */
int32_t msj_host_placement(msj_ctx *ctx, char *out, uint64_t capacity);
/* the NUMA node the page under a host address lies on (-1: unknown); measurement aid like the above */
int32_t msj_debug_numa_node_of(const void *host_ptr);
int32_t msj_host_unregister(msj_ctx *ctx, void *ptr);

/*
 * msj_stage1_device -- device-resident form (what bench.py times).
 * d_buf: device pointer, 16-byte aligned, len < 2^32 bytes.
 * d_idx: device pointer (16-byte aligned) to idx_capacity uint32 slots.
 * d_result: device pointer to one msj_carry; after the stream drains it holds
 *   count (= n), code (reference return code), utf8_error, ...
 * Enqueues on `stream` (hipStream_t as void*, NULL = default stream) and
 * returns immediately; the return value only reports argument / launch errors.
 */
int32_t msj_stage1_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, uint32_t *d_idx,
                          uint64_t idx_capacity, msj_carry *d_result, void *stream,
                          uint32_t flags);

/* Blocking read-back of a device msj_carry (synchronises `stream`).  If it is the result of the context's last
 * msj_stage1_device / msj_stage1_shard_device call and reports internal_error (a wait inside the single-pass
 * kernel expired), that call is issued again through the two-pass kernels first (MSJ_FLAG_TWO_PASS), so the
 * caller gets the document's real result. */
int32_t msj_carry_fetch(msj_ctx *ctx, const msj_carry *d_carry, msj_carry *host_out, void *stream);

/* Test hook: bound of every inter-workgroup wait of the single-pass kernel, in 10 ns ticks (default 2 s). */
int32_t msj_debug_set_wait_ticks(msj_ctx *ctx, uint32_t ticks);
/* Number of times this context fell back to the two-pass kernels after an expired wait. */
uint64_t msj_fallback_count(const msj_ctx *ctx);

/*
 * msj_stage1_shard_device -- one byte-range shard of a larger stream
 * (multi-GPU sharding and > 4 GiB inputs).
 * The shard is cut into <= MSJ_MAX_SEGMENT_BYTES segments; indices are written
 * densely to d_idx (relative to each segment's byte_base, see msj_segment) and
 * the segment table to d_segments (device, max_segments entries; count is
 * filled in on the device).
 *   d_carry_in : device msj_carry with the exact state at the shard's first
 *                byte (zeroed for the start of the document).
 *   d_carry_out: device msj_carry receiving the state after the last byte (a shard may end
 *                anywhere, also inside a multi-byte character or right after a backslash; only its
 *                base must be 16-byte aligned).
 *   has_prefix : non-zero when d_buf[-64..0) is readable and holds the 64
 *                stream bytes preceding the shard (used for the UTF-8
 *                continuation check across the shard boundary).
 *   is_final   : non-zero for the last shard of the stream: writes the trailer
 *                (with trailer_len) and the reference return code into
 *                d_carry_out->code.
 *   no_emit    : non-zero = summary pass only (no index writes): used to get
 *                the shard's quote parity before the RCCL stitch.
 * *n_segments_out receives the number of segments used.
 */
int32_t msj_stage1_shard_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, uint32_t *d_idx,
                                uint64_t idx_capacity, const msj_carry *d_carry_in,
                                msj_carry *d_carry_out, msj_segment *d_segments,
                                uint32_t max_segments, uint32_t *n_segments_out,
                                int32_t has_prefix, int32_t is_final, int32_t no_emit,
                                uint64_t trailer_len, void *stream, uint32_t flags);

/* The same with the state at the shard's first byte given BY VALUE -- carry_bits: bit 0 in_string, bit 1
 * next_is_escaped, bit 2 prev_scalar; structurals, bytes and the sticky flags start at zero -- instead of a device
 * msj_carry: the start of a shard whose carries the host knows (or assumes: msj_shard_speculate).  Nothing has to be
 * copied to the device in front of the launch. */
int32_t msj_stage1_shard_device_cv(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, uint32_t *d_idx,
                                   uint64_t idx_capacity, uint32_t carry_bits, msj_carry *d_carry_out,
                                   msj_segment *d_segments, uint32_t max_segments, uint32_t *n_segments_out,
                                   int32_t has_prefix, int32_t is_final, int32_t no_emit, uint64_t trailer_len,
                                   void *stream, uint32_t flags);

/*
 * ---- N-GPU form: one contiguous byte-range shard of one stream per rank (SURVEY.md section 8b
 * `msj_stage1_sharded`, section 8e; one process per GPU) ----------------------------------------
 * The reference is single-threaded (no parallelism of any kind); what a Mojo host
 * calling DomParserImplementation.stage1 (include/generic/dom_parser_implementation.mojo:65-69) on a stream
 * that is spread over the GPUs of a node binds is the pair msj_stage1_sharded_submit / _result below.
 * Protocol (csrc/sharded.cpp): every rank assumes the carries at its shard's first byte from its own bytes
 * (msj_shard_speculate), runs the single-pass kernel once, and ONE all-gather of a 128-byte report per rank
 * lets every rank replay the chain (msj_shard_verify); only ranks whose assumption was refuted index again.
 * Index arrays stay shard-local (offsets relative to the shard, or to its segments: msj_segment); the
 * trailer is written by the last rank with `total_len`.
 */
typedef struct msj_shard_report {
    msj_carry used; /* the carry this rank's launch assumed at its first byte */
    msj_carry out;  /* the state after its last byte, its count and sticky errors */
} msj_shard_report;

/* Carries a shard may assume from its own bytes: halo = the <= 64 stream bytes in front of it (halo_len 0 at the
 * start of the stream), head = its first <= 4096 bytes.  next_is_escaped / prev_scalar are exact unless a run of
 * backslashes reaches halo[0]; in_string is a guess: the head is followed under both hypotheses until one meets a byte
 * it cannot hold (a control character inside a string; outside of strings anything but blanks, operators, number
 * characters and the letters of true / false / null), else the neighbours of the first unescaped quote decide. */
int32_t msj_shard_speculate(const uint8_t *halo, uint64_t halo_len, const uint8_t *head, uint64_t head_len,
                            msj_carry *out);
/* The same; *decided_out (optional) = 1 when one hypothesis was contradicted by the head (or there is no halo: the
 * start of the stream), 0 when the in_string guess rests on the quote-neighbour rule or on nothing at all -- a caller
 * with more bytes at hand then asks again with a longer head (msj_stage1_sharded_submit does: 4 KiB, 64 KiB, 1 MiB). */
int32_t msj_shard_speculate_ex(const uint8_t *halo, uint64_t halo_len, const uint8_t *head, uint64_t head_len,
                               msj_carry *out, int32_t *decided_out);
/* Replays the chain of all ranks' reports.  exact_in[g] (world entries) receives the exact carry at the start of
 * shard g for every g < return value -- in_string / next_is_escaped / prev_scalar, and the STITCHED OFFSETS:
 * exact_in[g].count = structurals of the stream in front of shard g (the position of its first index in the
 * stream-wide array that the reference's BitIndexer.tail / n_structural_indexes define,
 * json_structural_indexer.mojo:34-37,160-165), exact_in[g].bytes = stream bytes in front of it.  The counts of
 * ranks named in *rerun_mask are not final yet (they index again), so the offsets are final when the mask is 0.
 * *rerun_mask gets bit g set for every rank that has to index again with exact_in[g] (wrong in_string guess,
 * wrong escape carries, or a poisoned launch -- the chain cannot be followed past the latter two).  Returns world
 * and mask 0 when every report stands; < 0 on bad arguments. */
int32_t msj_shard_verify(const msj_shard_report *reports, uint32_t world, msj_carry *exact_in, uint64_t *rerun_mask);
/* The reference's return code for the whole stream (finish(), json_structural_indexer.mojo:147-186) and the
 * total structural count, from reports that msj_shard_verify accepted.  MSJ_CAPACITY when any rank's index
 * buffer was too small for its shard (out.capacity_error), in the place the single-GPU path gives it (after
 * 15 and 14, before 13 and 11). */
int32_t msj_shard_global_code(const msj_shard_report *reports, uint32_t world, uint32_t flags, uint64_t *total_count);

/* The one collective: all-gather of `bytes_per_rank` bytes per rank, device memory, enqueued on `stream`
 * (or completed before returning).  Returns MSJ_SUCCESS or a negative library error. */
typedef int32_t (*msj_allgather_fn)(void *comm, const void *d_send, void *d_recv, uint64_t bytes_per_rank, void *stream);
typedef struct msj_exchange {
    void *comm;                 /* passed to allgather as is */
    msj_allgather_fn allgather;
    uint32_t rank, world;       /* world <= 64 */
    uint32_t owns_comm;         /* set by msj_exchange_rccl: `comm` is freed by msj_sharded_destroy */
    uint32_t reserved;
} msj_exchange;
/* RCCL over xGMI: fills *out with an all-gather that calls ncclAllGather(..., ncclUint8, nccl_comm, stream).
 * nccl_comm is the caller's ncclComm_t (passed as void*; it stays the caller's: create it with
 * ncclCommInitRank, destroy it with ncclCommDestroy after msj_sharded_destroy).  The library does not link RCCL:
 * the symbol is taken from `librccl_path` (NULL: "librccl.so") at run time -- pass the RCCL the communicator
 * was created with. */
int32_t msj_exchange_rccl(void *nccl_comm, uint32_t rank, uint32_t world, const char *librccl_path, msj_exchange *out);

/* Device operations behind the protocol.  NULL in msj_sharded_create = HIP on the context's device; tests
 * substitute host memory and a CPU shard runner to run the protocol without a GPU. */
typedef struct msj_sharded_ops {
    void *user;
    int32_t (*alloc)(void *user, uint64_t bytes, int pinned_host, void **out);
    void (*free)(void *user, void *p, int pinned_host);
    int32_t (*copy)(void *user, void *dst, const void *src, uint64_t bytes, int to_host, void *stream);
    int32_t (*sync)(void *user, void *stream);
    int32_t (*run_shard)(void *user, const uint8_t *d_shard, uint64_t len, uint32_t *d_idx, uint64_t idx_capacity,
                         const msj_carry *d_carry_in, msj_carry *d_carry_out, msj_segment *d_segments,
                         uint32_t max_segments, int32_t has_prefix, int32_t is_final, uint64_t trailer_len,
                         void *stream, uint32_t flags);
    /* Optional -- the first five together or not at all (all NULL: operations that complete before they return, the
     * CPU tests' kind; msj_stage1_sharded_result then drains the submission's stream with `sync`).  With them a
     * result waits for the event behind ITS submission's read-back only, so that later submissions keep the GPU
     * busy meanwhile, and the exchange + read-back go to `side_stream` behind an event at the end of the kernel,
     * so that the next kernel starts behind the kernel, not behind the collective.  The default HIP operations have
     * all of them (hipEvent_t, a non-blocking stream of the highest priority). */
    int32_t (*event_create)(void *user, void **event_out);
    void (*event_destroy)(void *user, void *event);
    int32_t (*event_record)(void *user, void *event, void *stream);
    int32_t (*event_wait)(void *user, void *event);                /* the host blocks until the event has happened */
    int32_t (*stream_wait)(void *user, void *stream, void *event); /* what is enqueued on `stream` from now on waits */
    int32_t (*event_query)(void *user, void *event);               /* optional: 1 happened, 0 not yet, < 0 error */
    int32_t (*event_elapsed_ns)(void *user, void *from, void *to, uint64_t *ns_out); /* optional: statistics only */
    void *side_stream; /* custom operations: the stream of the exchange and the read-back (NULL: the submission's) */
} msj_sharded_ops;

typedef struct msj_sharded msj_sharded;
int32_t msj_sharded_create(msj_ctx *ctx, const msj_exchange *xchg, const msj_sharded_ops *ops, msj_sharded **out);
void msj_sharded_destroy(msj_sharded *sh);
uint64_t msj_sharded_reruns(const msj_sharded *sh); /* shard launches repeated by this rank (refuted guesses) */
uint64_t msj_sharded_rounds(const msj_sharded *sh); /* all-gathers so far */
/* Where the time of the stitch goes (cumulative since msj_sharded_create; device figures only with the default HIP
 * operations, 0 otherwise): results = msj_stage1_sharded_result calls completed; stitch_device_ns = HIP-event time
 * from the end of a round's kernel to the arrival of the gathered reports in pinned host memory (the all-gather
 * and the read-back, per round); result_wait_ns = host time spent blocked inside msj_stage1_sharded_result. */
typedef struct msj_sharded_stats {
    uint64_t results, rounds, reruns;
    uint64_t stitch_device_ns, result_wait_ns;
    uint64_t kernel_device_ns;    /* cumulative event time of this rank's shard launches alone (the carry's 64-byte upload
                                     + the kernel chain), no exchange in it: the rank's kernel-only time */
    uint64_t last_kernel_ns;      /* ... of the last completed result's launch */
    uint64_t last_stitch_ns;      /* end of that launch -> gathered reports in pinned memory.  The rank whose kernel ends
                                     last sees the exchange's bare latency here, every other rank that + its lead: the
                                     spread of this figure over the ranks of one step is the ranks' skew */
    uint64_t reruns_behind_queue; /* second launches (refuted guesses) that were enqueued behind the kernels of LATER
                                     submissions on the same stream (launches of one context are stream-ordered) */
    uint64_t reserved[3];
} msj_sharded_stats;
int32_t msj_sharded_get_stats(const msj_sharded *sh, msj_sharded_stats *out);
/* Where a submission is, without waiting: a set of MSJ_SHARDED_* bits (both set with operations that have no events:
 * everything completed inside submit), < 0 on error / a ticket that is not in flight. */
#define MSJ_SHARDED_KERNEL_DONE 1 /* the round's kernel (and what was in front of it on its stream) has finished */
#define MSJ_SHARDED_REPORTS_IN 2  /* the gathered reports have arrived: msj_stage1_sharded_result will not block */
int32_t msj_sharded_ticket_state(msj_sharded *sh, uint32_t ticket);
/* Gives back what msj_exchange_rccl allocated when the exchange is NOT handed to msj_sharded_create after all. */
void msj_exchange_release(msj_exchange *x);

/* Enqueue this rank's shard: the kernel on `stream`; the all-gather of the reports and the pinned read-back on the
 * library's own high-priority stream behind an event at the kernel's end (so the kernel of the NEXT submission on
 * `stream` runs beside them); returns at once with a ticket (up to 3 submissions may be in flight, all launches of
 * one msj_sharded on ONE stream: a context's launches are stream-ordered).  d_shard: 16-byte aligned device pointer;
 * with has_prefix the 64 bytes in front of it must be readable stream bytes.  speculation: the carry to assume (what
 * msj_shard_speculate gave for host copies of the bytes, or -- resubmitting an unchanged shard -- the carry its last
 * result reported as used: then nothing is read here).  NULL = derived here from the device bytes: one blocking
 * 4 KiB read of `stream` per call, plus a 64 KiB and a 1 MiB read while the bytes decide nothing (strings of digits
 * or literals) unless the shard's last verified result already settled it for the same bytes.
 * d_segments / max_segments as in msj_stage1_shard_device. */
int32_t msj_stage1_sharded_submit(msj_sharded *sh, const uint8_t *d_shard, uint64_t shard_len, uint32_t *d_idx,
                                  uint64_t idx_capacity, uint64_t total_len, int32_t has_prefix,
                                  const msj_carry *speculation, msj_segment *d_segments, uint32_t max_segments,
                                  void *stream, uint32_t flags, uint32_t *ticket_out);
/* Where a shard's results sit in the stream: the stitch's offsets (every rank folds the
 * ranks below it).  Local index k of this shard is index (index_begin + k) of the stream-wide array; a local
 * offset (plus its segment's byte_base, msj_segment) + byte_base is the offset in the stream. */
typedef struct msj_shard_placement {
    uint64_t index_begin; /* structurals of the stream in front of this shard: BitIndexer.tail - base at its first byte
                             (json_structural_indexer.mojo:34-37); the exclusive sum of the lower ranks' counts */
    uint64_t byte_base;   /* stream bytes in front of this shard */
    uint64_t count;       /* this shard's structurals */
    uint64_t bytes;       /* this shard's bytes */
} msj_shard_placement;
/* Wait for a submission -- for ITS gathered reports only: later submissions keep running on the GPU meanwhile
 * (msj_sharded_ticket_state tells) -- ; collective (every rank calls it for its matching ticket).  *code_out: the reference's
 * return code for the whole stream; *total_count_out: structurals of the whole stream (n_structural_indexes,
 * json_structural_indexer.mojo:160-165); *local_out: this shard's msj_carry (count = its own structurals);
 * *used_out: the exact carry at its first byte; *placement_out: the stitched offsets.  Any out pointer may be NULL.
 * A failure of the exchange or of a launch while ranks index again is returned as is and frees the ticket; the
 * collective is then broken for that submission on every rank (they fail or time out in their own exchange). */
int32_t msj_stage1_sharded_result(msj_sharded *sh, uint32_t ticket, int32_t *code_out, uint64_t *total_count_out,
                                  msj_carry *local_out, msj_carry *used_out, msj_shard_placement *placement_out);
/* Test hook: host-pointer inputs of at least this many bytes go through the chunked pinned pipeline of msj_stage1
 * (default 64 MiB; 0 restores it).  ctx NULL: the default context. */
int32_t msj_debug_set_pipeline_min_bytes(msj_ctx *ctx, uint64_t bytes);
/* Test hook: on != 0 makes the pipeline's set-up fail as it does on a host that cannot give it pinned memory; the
 * call (and every later one) then goes through the plain staging path.  on == 0 clears that state.  Returns 1 while
 * the context has given the pipeline up, 0 otherwise, < 0 on error.  ctx NULL: the default context. */
int32_t msj_debug_fail_pipeline_setup(msj_ctx *ctx, int32_t on);
/* Test hook: longest segment (bytes, multiple of 4096) one launch indexes; default MSJ_MAX_SEGMENT_BYTES rounded
 * down to the tile. */
int32_t msj_debug_set_segment_bytes(msj_ctx *ctx, uint64_t bytes);

/*
 * ---- token stream for stage 2 (DERIVED, see below) -------------
 * msj_tokens_device -- from the structural indices of one segment, two coalesced arrays:
 *   d_type[i]  = buf[idx[i]]: the byte JsonIterator.advance / peek / last_structural dereference
 *                one structural at a time (generic/stage2/json_iterator.mojo:256-288);
 *   d_depth[i] = nesting depth of token i, the running count walk_document keeps by hand
 *                (+1 at '{' '[', -1 at '}' ']', json_iterator.mojo:84-90,173-180): a bracket
 *                carries the depth of the container it sits in, so an opening bracket and its
 *                closing bracket have the same value and everything between them is deeper.
 *   d_match[i] (optional, may be NULL) = for a bracket, the index of the other end of its
 *                container -- what start_container / end_container keep on a stack
 *                (generic/stage2/tape_builder.mojo:235-272); 0xFFFFFFFF for every other token and
 *                for a bracket without a partner.
 * d_result: n, the final / minimum / maximum running depth (after each token): final != 0 is an
 * unclosed document, minimum < 0 a closing bracket without an opening one, maximum is what the
 * reference compares with max_depth (DEPTH_ERROR).
 * These are derived quantities: the reference has no such arrays and no fixture for them, so
 * the CPU statement the tests compare with is a definition, not a pin.
 * d_buf / d_idx as produced by msj_stage1_device (offsets < len < 2^32, n < 2^31); d_idx,
 * d_depth and (when given) d_match 16-byte aligned, d_type 8-byte aligned: anything else is
 * MSJ_ERR_BAD_ARGUMENT (the arrays leave as 16-byte stores).  Asynchronous on `stream`.
 */
typedef struct msj_tokens_result {
    uint64_t n;
    int32_t final_depth;
    int32_t min_depth;
    int32_t max_depth;
    uint32_t reserved; /* number of opening brackets */
} msj_tokens_result;

int32_t msj_tokens_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                          uint8_t *d_type, int32_t *d_depth, uint32_t *d_match, msj_tokens_result *d_result,
                          void *stream);
/* The same for tokens that are NOT the start of their stream -- the next uint32 segment of a shard (msj_segment: a
 * 64 GiB stream is 8 GiB per GPU, two segments), the next window of a document stream: d_prev (device, or NULL =
 * msj_tokens_device) is the msj_tokens_result of the call that covered the tokens in front.  The running depth
 * walk_document keeps (generic/stage2/json_iterator.mojo:84-90,173-180) goes on from d_prev->final_depth -- that
 * int32 is the whole carry -- and d_result's final / min / max are those of the stream so far (n: this call's).
 * Read on the device, in stream order: calls chain without a host round trip.  d_match stays LOCAL to the call: a
 * container that closes in a later call keeps 0xFFFFFFFF at both ends (its opening bracket is found again from the
 * depths: the first later token at its depth). */
int32_t msj_tokens_chain_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                                uint8_t *d_type, int32_t *d_depth, uint32_t *d_match, msj_tokens_result *d_result,
                                const msj_tokens_result *d_prev, void *stream);

/*
 * msj_token_spans_device -- per structural (DERIVED like the token
 * stream): for a string token the offset of its closing quote and whether the body holds a backslash
 * (the scan parse_string does first, generic/stage2/string_parsing.mojo:334-386); for a number token the
 * offset one past its last character and whether it is written as a float (number_parsing.mojo:22-80).
 *   d_end[i]:   string: offset of the closing quote (len if never closed); number: the end parse_number's scan finds
 *               (number_parsing.mojo:41-59: '-'? digits, then . e E makes it a float that ends at the first
 *               structural or blank byte; bytes past the buffer read as blanks); 0 if longer than 1024 characters;
 *               0 for every other token
 *   d_flags[i]: MSJ_SPAN_* bits
 */
#define MSJ_SPAN_STRING 1u   /* the token opens a string */
#define MSJ_SPAN_ESCAPED 2u  /* ... whose body holds at least one backslash */
#define MSJ_SPAN_NUMBER 4u   /* the token starts a number */
#define MSJ_SPAN_FLOAT 8u    /* ... written with '.', 'e' or 'E' */
#define MSJ_SPAN_OPEN 16u    /* string not closed before the end of the buffer (d_end = len) */
#define MSJ_SPAN_BAD 32u     /* number: the byte behind its digits is neither . e E nor structural / blank: the
                                reference's parse_number returns NUMBER_ERROR here (number_parsing.mojo:56-57) */
#define MSJ_SPAN_LONG 128u   /* number of more than 1024 characters: not scanned (d_end = 0).  Never set on a string: the
                                closing quote and MSJ_SPAN_ESCAPED are exact at any body length (round 5: bodies over 1024
                                bytes are scanned by a wave each behind the span kernel, over 1 MiB by the whole grid) */
int32_t msj_token_spans_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                               uint32_t *d_end, uint8_t *d_flags, void *stream);

/*
 * Bracket partners as a COMPACT LIST (round 5): d_pairs[k] = {token index of the k-th opening bracket of the call, token
 * index of the bracket that closes its container, 0xFFFFFFFF if it is never closed inside the call}, k in the order of
 * the opening brackets; d_result->reserved is their number, the array needs room for as many (n at most).  Eight bytes per
 * CONTAINER instead of the four bytes per TOKEN of d_match -- brackets are 12 % of the minified workload's tokens -- for
 * the consumer that walks the tokens in order and takes one record at every opening bracket, the way the reference's
 * stage 2 pushes in start_container and pops in end_container (generic/stage2/tape_builder.mojo:235-272).  Same arguments
 * and results otherwise as msj_tokens_chain_device / msj_stage2_prep_chain_device without d_match; d_pairs 8-byte aligned.
 * The faster of the two partner forms (1 GiB minified: 1.00 ms per call against 1.17 with d_match): the call keeps the
 * brackets of its tokens as a compact list in the context's workspace (8 more bytes per token of capacity) and pairs them
 * there.
 */
typedef struct msj_bracket_pair {
    uint32_t open, close;
} msj_bracket_pair;
int32_t msj_tokens_pairs_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n, uint8_t *d_type,
                                int32_t *d_depth, msj_bracket_pair *d_pairs, msj_tokens_result *d_result,
                                const msj_tokens_result *d_prev, void *stream);
int32_t msj_stage2_prep_pairs_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                                     uint8_t *d_type, int32_t *d_depth, msj_bracket_pair *d_pairs, uint32_t *d_end, uint8_t *d_flags,
                                     msj_tokens_result *d_result, const msj_tokens_result *d_prev, void *stream);

/*
 * PROTOTYPE (round 5; SURVEY.md section 8 row f1 from ONE pass over the bytes; measured and decided in DESIGN.md section 5b):
 * msj_stage1_types_device -- msj_stage1_device that also writes d_types[k] = d_buf[d_idx[k]], the type byte stage 2's
 *   JsonIterator.advance dereferences (generic/stage2/json_iterator.mojo:256-262), beside every index from the same
 *   emission (one uint32 segment, single-pass kernel only: MSJ_CAPACITY otherwise; d_types 4-byte aligned, same
 *   capacity as d_idx);
 * msj_depth_from_types_device -- depth (and, d_match given, bracket partners) of every token from such type bytes:
 *   msj_tokens_chain_device without the pass over the buffer.
 */
int32_t msj_stage1_types_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, uint32_t *d_idx, uint64_t idx_capacity,
                                uint8_t *d_types, msj_carry *d_result, void *stream, uint32_t flags);
int32_t msj_depth_from_types_device(msj_ctx *ctx, const uint8_t *d_type, uint64_t n, int32_t *d_depth, uint32_t *d_match,
                                    msj_tokens_result *d_result, const msj_tokens_result *d_prev, void *stream);

/* Test hook (per context, like msj_debug_set_segment_bytes): stretches of more than lds_limit_bytes take the span
 * kernels' global-memory path, the fix-up list holds fix_capacity entries; 0xFFFFFFFF = the built-in value of either. */
int32_t msj_debug_set_span_limits(msj_ctx *ctx, uint32_t lds_limit_bytes, uint32_t fix_capacity);
/* Test hook (per context): which of their two kernels the token calls run -- 0 (default) by the density of the index
 * (the kernel organised by tiles of the buffer from one structural per 11 bytes on, the one organised by tokens below
 * that), 1 = by tokens, 2 = by tiles whatever the density.  Identical results; the tests run both. */
int32_t msj_debug_set_span_mode(msj_ctx *ctx, uint32_t mode);
/* Test hook: bytes of the buffer per workgroup of the kernel organised by tiles (which = 0) and of its halo (which = 1):
 * what the tests move their tokens across. */
uint32_t msj_debug_tile_group(int32_t which);

/*
 * msj_stage2_prep_device -- msj_tokens_device and msj_token_spans_device in one go (rows f1 + f2 + f4), with
 * identical results: the span kernel holds every token's first byte already, so it writes the type bytes and
 * the depth aggregates too and the buffer is read once instead of twice.  Same arguments, alignment and limits
 * as the two calls (d_match optional).  Asynchronous on `stream`.
 */
int32_t msj_stage2_prep_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                               uint8_t *d_type, int32_t *d_depth, uint32_t *d_match, uint32_t *d_end, uint8_t *d_flags,
                               msj_tokens_result *d_result, void *stream);
/* ... continuing a stream (d_prev as in msj_tokens_chain_device). */
int32_t msj_stage2_prep_chain_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                                     uint8_t *d_type, int32_t *d_depth, uint32_t *d_match, uint32_t *d_end, uint8_t *d_flags,
                                     msj_tokens_result *d_result, const msj_tokens_result *d_prev, void *stream);
/*
 * msj_stage2_prep_segments -- rows f1 + f2 + f4 for a whole SHARD of several uint32 segments (what
 * msj_stage1_shard_device leaves behind for more than MSJ_MAX_SEGMENT_BYTES: BASELINE config 5's 8 GiB per GPU), in
 * one call: one msj_stage2_prep_chain_device per segment, the depth handed from segment to segment on the device.
 *   segments: HOST copy of the shard's msj_segment table (n_segments entries; their counts size the launches)
 *   d_buf: the shard's first byte; d_idx and all output arrays: the shard's token arrays, segment s at
 *          [index_begin_s - index_begin_0, + count_s) of d_idx (dense, as stage 1 wrote them; a slice that does not
 *          start on the 16-byte grid is copied to an aligned buffer of the library's before the kernels read it).  The
 *          OUTPUT arrays are not dense: see offsets below; pass them with 8 elements of slack per segment.
 *   The table is checked as a whole before anything is launched: segments must follow each other without gaps
 *   (byte_base_s = byte_base_{s-1} + byte_len_{s-1}, index_begin likewise: MSJ_ERR_BAD_ARGUMENT), 0 < byte_len <=
 *   MSJ_MAX_SEGMENT_BYTES and count < 2^31 (MSJ_CAPACITY).
 *   d_results: n_segments msj_tokens_result (device); the last one describes the shard
 *   d_prev: the result in front of the shard, or NULL
 * Outputs of segment s start at element offsets[s] = the sum of the counts in front of it, each rounded up to a multiple of 8
 * elements (so that every slice keeps the single calls' alignment); offsets_out (host, n_segments entries, may be NULL) receives them.
 * d_end is relative to the SEGMENT's bytes (like the indices).
 * d_match (round 5) is valid over the WHOLE SHARD: for a bracket, the position IN THE SHARD'S OUTPUT ARRAYS (offsets[s] +
 * the token's index inside its segment: the element at which that token's type / depth / end / flags / match are
 * stored) of the other end of its container -- also when the container is opened in one segment and closed in a later
 * one (the stack of start_container / end_container, generic/stage2/tape_builder.mojo:235-272, has no such border):
 * every segment leaves the brackets it could not pair in a residual list of the context's (their depth above the
 * segment's minimum running depth is their place in it), and a stitch behind the last segment pairs them.  0xFFFFFFFF:
 * not a bracket, or no partner inside the shard.
 * Limits with d_match: at most 32 segments and fewer than 2^32 - 1 output elements (MSJ_CAPACITY otherwise); at a segment
 * border, every container less than 65 536 levels above the shard's minimum running depth is stitched.  With d_prev =
 * NULL and a well-formed document, that means depth < 65 536.  Further above, a container cut by a border may keep
 * 0xFFFFFFFF at both ends; bit 31 of d_results[n_segments - 1].reserved is then set.  The single calls (msj_stage2_prep_chain_device,
 * msj_tokens_chain_device) write into arrays of the caller's for each call and keep their partners local to the call.
 */
int32_t msj_stage2_prep_segments(msj_ctx *ctx, const uint8_t *d_buf, const msj_segment *segments, uint32_t n_segments,
                                 const uint32_t *d_idx, uint8_t *d_type, int32_t *d_depth, uint32_t *d_match, uint32_t *d_end,
                                 uint8_t *d_flags, msj_tokens_result *d_results, const msj_tokens_result *d_prev,
                                 uint64_t *offsets_out, void *stream);

/*
 * ---- multi-document mode (DERIVED) -----------------------------
 * The reference left upstream simdjson's streaming modes out
 * (generic/stage1/json_structural_indexer.mojo:153,169; generic/stage2/tape_builder.mojo:25 "TODO: add
 * streaming").  msj_documents_device splits the token stream of one window of a stream of concatenated
 * documents (NDJSON, or no separator at all) into documents: a document starts at every token that sits
 * at depth 0 and is not a closing bracket.
 *   d_doc_first[k] = token index (into d_idx / d_type / d_depth) of the first token of document k,
 *                    ascending; at most `capacity` are stored, n_documents counts all of them
 *   d_result:  n_documents      documents that START in the window
 *              n_complete       ... of which complete: all, or all but the last.  The last one is
 *                               complete if it is a container closed before the window ends; a closed
 *                               string (d_carry->in_string tells); any other scalar when is_final, or
 *                               when the window ends in a blank -- a number or literal that touches
 *                               the end of a window may go on in the next one
 *              tokens_complete  tokens covered by the complete documents: n, or the index of the first
 *                               token of the cut document (what upstream's find_next_document_index
 *                               returns for the window)
 *              resume_offset    byte offset (relative to the window) of that token = where the next
 *                               window has to start; len when nothing is cut
 * d_buf / len: the window; is_final: MSJ_DOCS_* bits -- MSJ_DOCS_FINAL: the window is the end of the stream;
 * MSJ_DOCS_AFTER_TOKENS: d_type / d_depth are exactly what the LAST msj_tokens_device / msj_stage2_prep_device call
 * on this context wrote (same n, same stream order) and have not been changed since: the per-block counts that call
 * left in the context's workspace are used instead of a pass over the two arrays.  d_type / d_depth as written by
 * msj_tokens_device for the same d_idx; d_carry (optional, may be NULL):
 * the carry_out of the window's msj_stage1_shard_device call, read on the device.  A window of a
 * stream is indexed with msj_stage1_shard_device(..., is_final = 0): nothing is an error yet at its end.
 * Asynchronous on `stream`.
 */
#define MSJ_DOCS_FINAL 1
#define MSJ_DOCS_AFTER_TOKENS 2
typedef struct msj_documents_result {
    uint64_t n_documents;
    uint64_t n_complete;
    uint64_t tokens_complete;
    uint64_t resume_offset;
} msj_documents_result;

int32_t msj_documents_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, int32_t is_final, const uint32_t *d_idx,
                             uint64_t n, const uint8_t *d_type, const int32_t *d_depth, const msj_carry *d_carry,
                             uint32_t *d_doc_first, uint64_t capacity, msj_documents_result *d_result, void *stream);

/*
 * ---- number values for stage 2 (after row f4; DERIVED) ---------------------------------------
 * msj_number_values_device -- the reference's Int(span) / Float64(span) (number_parsing.mojo:60-78, what feeds
 * TapeWriter.append_s64 / append_double) for every number token of one segment, as a COMPACT LIST: one 16-byte record
 * per token whose d_flags (from any span call for the same d_idx) has MSJ_SPAN_NUMBER, in token order.  A consumer that
 * walks the tokens in order takes the next record at every number token; `token` serves random access.
 * The definition (RFC 8259 plus the value Python's json gives):
 *   text       -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)? starting at idx[i], followed by a structural byte ({}[]:,), a
 *              blank (space, tab, LF, CR), or the end of the buffer (bytes at or past len read as blanks).  Anything else
 *              is MSJ_NUMBER_ERR_SYNTAX (01, -, 1., 1.e5, 1e, 1e+, 1.5x, 12a; every token flagged MSJ_SPAN_BAD)
 *   integer    no fraction and no exponent: MSJ_NUMBER_INT64, the exact value in [-2^63, 2^63 - 1]; outside that range
 *              MSJ_NUMBER_ERR_RANGE (the reference's Int is 64-bit too); -0 is the integer 0
 *   float      anything else: MSJ_NUMBER_DOUBLE, the binary64 nearest to the exact decimal value, ties to even (CPython's
 *              float()), for any number of digits and any exponent; underflow gives +-0 or a correctly rounded subnormal,
 *              sign kept (-1e-400 is -0.0); a value whose correct rounding is +-infinity is MSJ_NUMBER_ERR_RANGE
 * d_result: n_numbers counts every number token, also those beyond `capacity` (only the first `capacity` records are
 * stored); first_error is the token index of the first erroneous number in token order (where the reference's stage 2
 * stops with NUMBER_ERROR), UINT64_MAX if none.  Arguments and limits as msj_token_spans_device: one uint32 segment,
 * n < 2^31 (MSJ_CAPACITY otherwise); d_idx 16-byte aligned, d_flags and d_result 8-byte, d_numbers 16-byte (MSJ_ERR_BAD_ARGUMENT,
 * nothing launched).  n = 0 writes a zero result with first_error = UINT64_MAX.  Asynchronous on `stream`, no host round
 * trip on any path (chains behind msj_stage2_prep_pairs_device in one stream).  Workspace: the context's own, see
 * msj_number_values_workspace_bytes.
 */
#define MSJ_NUMBER_INT64 1u      /* bits = the int64 value */
#define MSJ_NUMBER_DOUBLE 2u     /* bits = the IEEE-754 binary64 bit pattern */
#define MSJ_NUMBER_ERR_SYNTAX 3u /* bits = 0 */
#define MSJ_NUMBER_ERR_RANGE 4u  /* bits = 0 */
typedef struct msj_number {      /* 16 bytes: one record per number token, in token order */
    uint64_t bits;
    uint32_t token;              /* index of the token in d_idx / d_type / d_flags */
    uint32_t kind;               /* MSJ_NUMBER_* */
} msj_number;
typedef struct msj_numbers_result {
    uint64_t n_numbers;   /* number tokens in the call, also those beyond capacity */
    uint64_t n_errors;    /* records of an ERR kind */
    uint64_t first_error; /* token index of the first erroneous number in token order; UINT64_MAX: none */
    uint64_t n_slow;      /* numbers the exact fallback resolved (diagnostic) */
} msj_numbers_result;
int32_t msj_number_values_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                                 const uint8_t *d_flags, msj_number *d_numbers, uint64_t capacity,
                                 msj_numbers_result *d_result, void *stream);
/* Device workspace of one msj_number_values_device call over n tokens of a len-byte segment (the context keeps it). */
uint64_t msj_number_values_workspace_bytes(uint64_t n, uint64_t len);

/*
 * ---- stage 2's verdict for one document (DERIVED) ---------------------------------------------
 * msj_validate_device -- the code and the token at which the reference's walk_document
 * (generic/stage2/json_iterator.mojo:40-254) with TapeBuilder's visitors (tape_builder.mojo, atom_parsing.mojo,
 * string_parsing.mojo:267-386) would stop, for ONE document in ONE uint32 segment whose stage 1 returned MSJ_SUCCESS (so
 * n >= 1 and every string is closed), with d_depth from a call that started at depth 0 (d_prev == NULL).  The reference
 * cannot run here, so this text is the definition; it follows the reference line by line except where listed below.
 * The walk is not done serially: the state in which the walker meets token i follows from at most three tokens in front
 * of i and one hop through d_match, provided no earlier token is in error, and the walker returns the code of the FIRST
 * token in error -- so every token is judged on its own and the verdict is a minimum over positions.
 * Per token i in [0, n] (token n is the end of the stream: a token that matches nothing), in a valid prefix:
 *   structure  the walker's state machine as written: after '{' a key string or '}'; after a key ':'; after ':', '[', or
 *              a ',' inside an array, a value ('{', '[', '"', '-', 0-9, t, f, n; any other first byte is TAPE_ERROR 3, as
 *              in visit_primitive :309-329); after a ',' inside an object a key string; after a value ',' or the closing
 *              bracket of the container's own kind; after the root value nothing (i == n), else TAPE_ERROR at i
 *              (:248-253).  At token 0: a root '{' / '[' whose LAST token is not '}' / ']' is TAPE_ERROR at token 0 (:54-59)
 *   depth      a non-empty container (its next token is not its own closing bracket; {} and [] never count, :62-76,
 *              :114-130, :193-211) opened at token i has walker depth d_depth[i] + 1.  '{': DEPTH_ERROR 4 if that is
 *              > max_depth (:87); '[': if it is >= max_depth (:176).  Both comparisons as the reference writes them
 *   atoms      t / f / n must spell true / false / null and be followed by one of {}[]:, space, tab, LF, CR or the end of
 *              the buffer (bytes at or past len read as blanks, atom_parsing.mojo:34-80): else code 6 / 7 / 8
 *   strings    (keys too, visit_key), only where d_flags has MSJ_SPAN_ESCAPED: walking the body up to d_end[i], every
 *              backslash that starts an escape is followed by one of " \ / b f n r t, or by u and four hex digits; a code
 *              unit in D800-DBFF must be followed at once by \u and four hex digits in DC00-DFFF (the pair is one escape);
 *              a code unit in DC00-DFFF on its own is an error (handle_unicode_codepoint with allow_replacement = False,
 *              :267-327; parse_string :353-381).  Else STRING_ERROR 5.  Exact at any body length
 *   numbers    not re-parsed: d_numbers (optional) is the device msj_numbers_result of a msj_number_values_device call over
 *              the same tokens; its first_error token competes as NUMBER_ERROR 9.  NULL: numbers are not checked and
 *              MSJ_VALIDATE_NUMBERS_UNCHECKED is set in the result
 *   count      a container whose 1 + (commas directly inside it) exceeds 0xFFFFFF is MSJ_CAPACITY at its closing bracket
 *              (end_container, tape_builder.mojo:257-264).  Only a container with at least 2 * 0xFFFFFF + 1 tokens between
 *              its brackets can reach that: the direct commas (type == ',' and d_depth == d_depth[open] + 1 between the
 *              brackets) of up to MSJ_VALIDATE_BIG_CONTAINERS such containers are counted exactly; a call that finds none
 *              does no second read of the arrays.  More than that: no count is checked, MSJ_VALIDATE_COUNTS_CLIPPED is
 *              set, and with that flag a code of 0 does not rule out MSJ_CAPACITY
 *   one code per token, first token wins: at a token a structure or depth error comes before a content error (string /
 *              atom / number / count).  The result is the smallest i with a code, and that code.
 * Deviations from the reference: (1) a root {} / [] is valid: the reference forgets the advance() at :61-76 (the three
 * other empty-container sites have it) and returns TAPE_ERROR for these two documents; upstream simdjson advances.
 * (2) the number grammar is msj_number_values_device's (RFC 8259), not Mojo's Int() / Float64().  (3) for '{' at walker
 * depth == max_depth the reference's comparison passes and then indexes its lists one past the end; here it just passes.
 * Inputs are exactly what msj_stage2_prep_device(..., d_match != NULL, ...) wrote for the same d_idx.  Alignment and limits
 * as that call (d_idx, d_depth, d_match, d_end 16-byte, d_type, d_flags, d_numbers, d_result 8-byte: MSJ_ERR_BAD_ARGUMENT;
 * len > MSJ_MAX_SEGMENT_BYTES or n >= 2^31: MSJ_CAPACITY; nothing launched); n == 0 or max_depth == 0 is
 * MSJ_ERR_BAD_ARGUMENT.  Asynchronous on `stream`, no host round trip on any path, workspace in the context.  Safe on ANY
 * token arrays stage 1 + prep can produce from arbitrary bytes: a neighbour that cannot be resolved (no partner, a token in
 * front of token 0) means an earlier token is already in error, so the token reports nothing; no index derived from
 * d_match is used unchecked.
 */
#define MSJ_VALIDATE_NUMBERS_UNCHECKED 1u
#define MSJ_VALIDATE_COUNTS_CLIPPED 2u
#define MSJ_VALIDATE_BIG_CONTAINERS 64u
typedef struct msj_validate_result {
    int32_t code;          /* reference code: 0, 1, 3..9 */
    uint32_t flags;        /* MSJ_VALIDATE_* */
    uint64_t error_token;  /* token index in [0, n]; UINT64_MAX when code == 0 */
    uint64_t error_offset; /* d_idx[error_token], len for token n; UINT64_MAX when code == 0 */
    uint64_t n_escaped;    /* strings whose escapes were walked (diagnostic) */
} msj_validate_result;
int32_t msj_validate_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
                            const uint8_t *d_type, const int32_t *d_depth, const uint32_t *d_match,
                            const uint32_t *d_end, const uint8_t *d_flags, const msj_numbers_result *d_numbers,
                            uint32_t max_depth, msj_validate_result *d_result, void *stream);
/* Device workspace of one msj_validate_device call over n tokens of a len-byte segment (the context keeps it). */
uint64_t msj_validate_workspace_bytes(uint64_t n, uint64_t len);

/*
 * ---- the document: tape and string buffer (DERIVED) --------------------------------------------
 * msj_tape_device -- what the reference's stage 2 exists to produce: Document.tape (uint64 words) and Document.string_buf,
 * as TapeBuilder (generic/stage2/tape_builder.mojo) builds them and dump_raw_tape / DocumentEntryIterator
 * (include/dom/document.mojo) read them, for ONE document in ONE uint32 segment.  The reference cannot run here, so this
 * text is the definition.  Inputs are exactly what msj_stage2_prep_device(..., d_match != NULL, ...), started at depth 0,
 * and msj_number_values_device (capacity >= n_numbers) wrote for the same d_idx.
 * The tape is SPECIFIED ONLY for a document whose msj_validate_device code is 0 with flags == 0.  On any other token arrays
 * the call stays inside the capacities it was given and returns; the contents are then unspecified (no index derived from
 * d_match or d_end is used unchecked).
 *   words     w(i) per token: 1 for { } [ ], for a string (key or value) and for t f n; 2 for a token with MSJ_SPAN_NUMBER;
 *             0 for : , and any other byte
 *   positions pos(i) = 1 + the sum of w(j) over j < i; E = pos(n); the tape has E + 1 words (< 2^32 because n < 2^31)
 *   root      tape[0] = 'r' << 56 | (E + 1), tape[E] = 'r' << 56 (visit_document_start / _end, tape_builder.mojo:62-66,94-105)
 *   opening bracket i with partner j = d_match[i]: type << 56 | count << 32 | (pos(j) + 1); count = min(elements, 0xFFFFFF),
 *             elements = 0 if j == i + 1 (empty_container :227-233: start_index + 2), else 1 + the number of k in (i, j) with
 *             d_type[k] == ',' and d_depth[k] == d_depth[i] + 1 (what increment_count keeps, :245-272; read back at
 *             document.mojo:194-202)
 *   closing bracket j with partner i: type << 56 | pos(i)
 *   string    '"' << 56 | soff(i), soff(i) = the sum over string tokens k < i of 4 + ulen(k): the record in the string buffer
 *             is a 4-byte little-endian length, then the bytes, NO NUL terminator (on_string_start / on_string_end :274-301)
 *   number    the next record of d_numbers in token order: 'l' << 56 then the int64 bits, or 'd' << 56 then the binary64 bit
 *             pattern.  'u' (UINT64) is never produced: a value above 2^63 - 1 is ERR_RANGE in the number call
 *   atoms     't', 'f' or 'n' << 56
 *   ulen(k)   without MSJ_SPAN_ESCAPED d_end[k] - d_idx[k] - 1.  With it the body is walked: a byte outside an escape counts 1
 *             and is copied unchanged; \" \\ \/ \b \f \n \r \t give 1 byte; \uXXXX gives the UTF-8 of its code point (1, 2 or
 *             3 bytes); a high surrogate followed at once by a \u low surrogate gives the pair's 4 bytes (parse_string,
 *             string_parsing.mojo:334-386, handle_unicode_codepoint :267-327).  string_bytes = the sum of 4 + ulen
 * Deviations from the reference: (1) the END word of a non-empty container is written: end_container (:245-272) says "Write
 * the ending tape element" and has no append for it, but its own dump_raw_tape and upstream simdjson expect the word, and
 * without it empty_container and end_container disagree about the layout.  (2) A double is stored as its bit pattern:
 * append_double does a numeric cast under a "TODO: is this type cast correct?", the reader bitcasts (document.mojo:251).
 * (3) A count above 0xFFFFFF saturates in the word; the reference's CAPACITY for it is msj_validate_device's to report.
 * (4) The number grammar and the root {} / [] are as in msj_validate_device.
 * d_verdict (optional): the device msj_validate_result of the document.  When its code is not 0 the kernels read that on the
 * device and write only d_result, with that code and zero sizes: index -> prep -> numbers -> validate -> tape needs no host
 * round trip.  d_string_buf may be NULL: the tape and string_bytes are still exact (the layout-only form).  Capacities are
 * never written past; on overflow (tape, string buffer, or fewer number records than number tokens) code = MSJ_CAPACITY and
 * the true sizes are reported.  Arguments as msj_validate_device: NULL (other than d_verdict, d_string_buf, and d_numbers
 * with numbers_capacity == 0) or off-grid pointers (d_idx, d_depth, d_match, d_end, d_numbers, d_tape 16-byte; d_type, d_flags,
 * d_numbers_result, d_verdict, d_result 8-byte; d_string_buf any) are MSJ_ERR_BAD_ARGUMENT, len > MSJ_MAX_SEGMENT_BYTES or
 * n >= 2^31 MSJ_CAPACITY, n == 0 MSJ_ERR_BAD_ARGUMENT; nothing is launched on an error.  d_numbers_result (optional) is
 * accepted for symmetry with the chain; the number tokens are counted from d_flags.  Asynchronous on `stream`, workspace in
 * the context.
 */
typedef struct msj_tape_result {
    int32_t code;          /* 0; MSJ_CAPACITY if tape / string buffer / d_numbers is too small; d_verdict's code if that is not 0 */
    uint32_t flags;        /* 0 */
    uint64_t tape_words;   /* E + 1, also when clipped */
    uint64_t string_bytes; /* also when clipped, and when d_string_buf == NULL */
    uint64_t n_strings;
} msj_tape_result;
int32_t msj_tape_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n, const uint8_t *d_type,
                        const int32_t *d_depth, const uint32_t *d_match, const uint32_t *d_end, const uint8_t *d_flags,
                        const msj_number *d_numbers, uint64_t numbers_capacity, const msj_numbers_result *d_numbers_result,
                        const msj_validate_result *d_verdict, uint64_t *d_tape, uint64_t tape_capacity, uint8_t *d_string_buf,
                        uint64_t string_capacity, msj_tape_result *d_result, void *stream);
/* Device workspace of one msj_tape_device call over n tokens of a len-byte segment (the context keeps it). */
uint64_t msj_tape_workspace_bytes(uint64_t n, uint64_t len);

/*
 * ---- stage 2's verdict for every document of a window (DERIVED) --------------------------------
 * msj_validate_documents_device -- msj_validate_device's verdict for EVERY complete document of a window that
 * msj_documents_device has split, in one pass over the window's token arrays: no launch per document and no host round
 * trip.  Read on the device: D = d_docs->n_complete and T = d_docs->tokens_complete (the device msj_documents_result of the
 * split over the same arrays; d_doc_first holds at least D entries).  Document k covers the tokens [f_k, e_k), f_k =
 * d_doc_first[k], e_k = d_doc_first[k + 1], e_(D-1) = T.  d_verdicts[k] is what the definition of msj_validate_device gives for
 * the token sub-arrays [f_k, e_k) -- d_type, d_depth, d_match, d_end, d_flags from f_k on, e_k - f_k tokens -- with
 *   buffer     the same d_buf / len and the same d_idx values: content checks look at the window's bytes, not at a slice of
 *              them.  A `true` or a `12` directly followed by the next document's `"` is therefore an atom / number error,
 *              exactly as the span and number calls already see it
 *   partners   rebased: d_match[i] - f_k; a partner outside [f_k, e_k) counts as no partner
 *   in front   a token in front of f_k matches nothing (it is "a token in front of token 0")
 *   the end    token e_k is that document's end of the stream: a token that matches nothing, judged for document k
 *   error_token is reported as an index into the WINDOW's arrays, in [f_k, e_k]
 * Why this is exact: the per-token rule is local (three tokens in front, one hop through d_match) and the split starts a
 * document at every depth-0 token that is not a closing bracket, so d_depth needs no rebase and the only thing to hide from
 * a token is the other documents.  Tokens at or past T belong to the cut document: they are never judged and never read as
 * anything but "nothing"; tokens in front of d_doc_first[0] (a window that starts below depth 0) belong to no document.
 * d_verdicts[k] for k >= D is not written.
 *   numbers    d_numbers_result == NULL: numbers are not checked, MSJ_VALIDATE_NUMBERS_UNCHECKED is set.  n_errors == 0 (read
 *              on the device): nothing more is needed, d_numbers may be NULL with numbers_capacity 0 -- the usual case, no
 *              record is ever written.  n_errors > 0 and n_numbers <= numbers_capacity: every record of an ERR kind whose
 *              token is below T competes in its document as NUMBER_ERROR 9 (the first one of a document wins, as first_error
 *              does in msj_validate_device).  n_errors > 0 and not every record stored: MSJ_VALIDATE_NUMBERS_UNCHECKED is set
 *              (run the number call again with n_numbers records, then this call)
 *   count      as msj_validate_device: up to MSJ_VALIDATE_BIG_CONTAINERS wide containers per CALL are counted exactly, a
 *              MSJ_CAPACITY goes to the document that holds the container; more sets MSJ_VALIDATE_COUNTS_CLIPPED
 * d_result: code 0, or MSJ_CAPACITY when D > capacity (then n_documents = D and nothing else is specified; no verdict is
 * written); flags for the whole call; n_documents = D; n_invalid the verdicts with a code, first_invalid the smallest such k
 * (UINT64_MAX: none); n_escaped as msj_validate_result's.  n == 0 or D == 0 writes a zero result with first_invalid =
 * UINT64_MAX.  Arguments: alignment and limits of msj_validate_device (d_idx, d_depth, d_match, d_end, d_numbers 16-byte;
 * d_type, d_flags, d_docs, d_numbers_result, d_verdicts, d_result 8-byte; d_doc_first 4-byte); NULL d_result / d_docs, NULL
 * arrays with n > 0, NULL d_verdicts with capacity > 0, NULL d_numbers with numbers_capacity > 0 or max_depth == 0:
 * MSJ_ERR_BAD_ARGUMENT; len > MSJ_MAX_SEGMENT_BYTES or n >= 2^31: MSJ_CAPACITY; nothing is launched on either.  Asynchronous on
 * `stream`, no host round trip on any path, workspace in the context.  Safe on ANY arrays stage 1 + prep + split can produce
 * from arbitrary bytes: no index from d_match or d_doc_first is used unchecked, D and T are clipped to n, and a window whose
 * depth goes negative stays in bounds (its later tokens fall into one document, judged by the same rule).
 */
typedef struct msj_document_verdict {   /* 16 bytes, one per complete document */
    int32_t  code;         /* reference code 0, 1, 3..9 -- as msj_validate_result.code */
    uint32_t reserved;     /* 0 */
    uint64_t error_token;  /* index into the WINDOW's token arrays, in [first_k, end_k]; UINT64_MAX when code == 0 */
} msj_document_verdict;
typedef struct msj_validate_documents_result {  /* 48 bytes */
    int32_t  code;          /* 0, or MSJ_CAPACITY: more complete documents than `capacity`, nothing else specified */
    uint32_t flags;         /* MSJ_VALIDATE_NUMBERS_UNCHECKED / MSJ_VALIDATE_COUNTS_CLIPPED, meaning as today, for the whole call */
    uint64_t n_documents;   /* verdicts written = d_docs->n_complete */
    uint64_t n_invalid;     /* verdicts with code != 0 */
    uint64_t first_invalid; /* smallest such document index, UINT64_MAX if none */
    uint64_t n_escaped;     /* diagnostic, as today */
    uint64_t reserved;
} msj_validate_documents_result;
int32_t msj_validate_documents_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
        const uint8_t *d_type, const int32_t *d_depth, const uint32_t *d_match, const uint32_t *d_end, const uint8_t *d_flags,
        const uint32_t *d_doc_first, const msj_documents_result *d_docs,
        const msj_number *d_numbers, uint64_t numbers_capacity, const msj_numbers_result *d_numbers_result,
        uint32_t max_depth, msj_document_verdict *d_verdicts, uint64_t capacity,
        msj_validate_documents_result *d_result, void *stream);
/* Device workspace of one msj_validate_documents_device call (the context keeps it; the documents' error words live in d_verdicts). */
uint64_t msj_validate_documents_workspace_bytes(uint64_t n, uint64_t len, uint64_t capacity);

/*
 * ---- a tape for every document of a window (DERIVED) -------------------------------------------
 * msj_tape_documents_device -- msj_tape_device's tape and string buffer for EVERY complete document of a window that
 * msj_documents_device has split, in one pass over the window's tokens: no launch per document and no host round trip.
 * Inputs as for msj_validate_documents_device: the window's d_buf / len, and d_idx, d_type, d_depth, d_match, d_end, d_flags
 * from msj_stage2_prep_device(..., d_match != NULL, ...) started at depth 0; d_doc_first and the device
 * msj_documents_result of the split; d_numbers / numbers_capacity / d_numbers_result from msj_number_values_device over the
 * WHOLE window's tokens; optionally d_verdicts, the msj_document_verdict array of msj_validate_documents_device (D entries;
 * none is read when D > capacity).  D = d_docs->n_complete and T = d_docs->tokens_complete are read on the device and clipped to n.  Document k
 * covers the tokens [f_k, e_k), f_k = d_doc_first[k], e_k = d_doc_first[k + 1], e_(D-1) = T.
 * Document k's tape and string buffer are exactly what the definition of msj_tape_device gives for the token sub-arrays
 * [f_k, e_k), with these four conventions:
 *   buffer     the same d_buf / len and the same d_idx / d_end values are used, as in the verdict call
 *   partners   rebased (d_match[i] - f_k); a partner outside [f_k, e_k) is no partner
 *   numbers    the records are those whose token lies in [f_k, e_k), in order
 *   local      positions in bracket words, tape[0]'s word count and string offsets are LOCAL to the document
 * Each document's slice is therefore a self-contained Document(tape, string_buf).  It is specified for a document whose
 * verdict is 0, as for the single call.  d_depth needs no rebase, because f_k sits at depth 0.
 * Layout in the window's output arrays, in closed form.  Let W(i), S(i), N(i) be the sums over window tokens j < i of the
 * words per token (W), of 4 + ulen at strings (S) and of the number tokens (N).  Then
 *   document k's tape starts at word tape_first[k] = W(f_k) - W(f_0) + 2k of d_tape and has W(e_k) - W(f_k) + 2 words
 *   its string records start at byte string_first[k] = S(f_k) - S(f_0) of d_string_buf
 *   token i of document k writes at word W(i) - W(f_0) + 2k + 1; a string's word holds S(i) - S(f_k)
 *   a number takes record N(i), the global rank in the window, not rebased
 *   the end root word of document k - 1 and the first root word of document k are adjacent, at tape_first[k] - 1 and
 *   tape_first[k]
 * Word addresses are 64-bit: W(T) + 2D can pass 2^32 although every local position stays below it.  No scan over documents
 * is needed.  The price is that a document with a verdict code still occupies its slot: its record reports the verdict's
 * code with tape_words = string_bytes = 0, and the contents of its slot are unspecified but stay inside it and inside the
 * capacities.  Tokens in front of f_0 and at or past T write nothing and are read only as "nothing".
 * Results: one 32-byte msj_document_tape per complete document in d_doc_tapes, and one 64-byte msj_tape_documents_result:
 * code 0, or MSJ_CAPACITY when the tape, the string buffer, the records (D > capacity: nothing else is written then) or the
 * number records (fewer than the number tokens below T: n_numbers > numbers_capacity) do not fit; tape_words and
 * string_bytes are the window's true totals, also when clipped, n_numbers the records the call reads.  Capacities are never
 * written past.  d_string_buf == NULL is the layout-only form, as in msj_tape_device.  d_verdicts == NULL builds every
 * document (unspecified where one is invalid, still in bounds).  n == 0 or D == 0 writes a zero result.
 * Arguments, alignments and limits follow msj_validate_documents_device / msj_tape_device: d_idx, d_depth, d_match, d_end,
 * d_numbers, d_tape 16-byte; d_type, d_flags, d_docs, d_numbers_result, d_verdicts, d_doc_tapes, d_result 8-byte;
 * d_doc_first 4-byte; d_string_buf any.  NULL d_result / d_docs, NULL arrays with n > 0, NULL d_tape / d_doc_tapes / d_numbers
 * with a capacity > 0: MSJ_ERR_BAD_ARGUMENT; len > MSJ_MAX_SEGMENT_BYTES or n >= 2^31: MSJ_CAPACITY; nothing is launched on
 * either.  d_numbers_result (optional) is accepted for symmetry with the chain; the number tokens are counted from d_flags.
 * Asynchronous on `stream`, workspace in the context.  Safe on ANY arrays stage 1 + prep + split can produce from arbitrary
 * bytes: no index from d_match, d_end or d_doc_first is used unchecked and every store is checked against its capacity.
 */
typedef struct msj_document_tape {   /* 32 bytes, one per complete document */
    uint64_t tape_first;    /* word offset of the document's tape in d_tape */
    uint64_t string_first;  /* byte offset of its records in d_string_buf */
    uint32_t tape_words;    /* 0 when code != 0 */
    int32_t  code;          /* 0, or d_verdicts[k].code */
    uint64_t string_bytes;  /* 0 when code != 0 */
} msj_document_tape;
typedef struct msj_tape_documents_result {  /* 64 bytes */
    int32_t  code;          /* 0, or MSJ_CAPACITY: tape / string buffer / records / number records too small */
    uint32_t flags;         /* 0 */
    uint64_t n_documents;   /* D */
    uint64_t n_built;       /* records with code 0 */
    uint64_t tape_words;    /* W(T) - W(f_0) + 2D, also when clipped */
    uint64_t string_bytes;  /* S(T) - S(f_0), also when clipped, and when d_string_buf == NULL */
    uint64_t n_strings;
    uint64_t n_numbers;     /* number tokens below T = the records of d_numbers the call reads */
    uint64_t reserved;
} msj_tape_documents_result;
int32_t msj_tape_documents_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
        const uint8_t *d_type, const int32_t *d_depth, const uint32_t *d_match, const uint32_t *d_end, const uint8_t *d_flags,
        const uint32_t *d_doc_first, const msj_documents_result *d_docs,
        const msj_number *d_numbers, uint64_t numbers_capacity, const msj_numbers_result *d_numbers_result,
        const msj_document_verdict *d_verdicts, uint64_t *d_tape, uint64_t tape_capacity, uint8_t *d_string_buf,
        uint64_t string_capacity, msj_document_tape *d_doc_tapes, uint64_t capacity,
        msj_tape_documents_result *d_result, void *stream);
/* Device workspace of one msj_tape_documents_device call (the context keeps it): msj_tape_device's plus 8 bytes per document. */
uint64_t msj_tape_documents_workspace_bytes(uint64_t n, uint64_t len, uint64_t capacity);

/*
 * ---- fields by path for every document of a window (DERIVED) ------------------------------------
 * msj_select_documents_device -- upstream simdjson's at_key / at_pointer, restricted to object keys, for up to 16 paths and
 * EVERY complete document of a window in one call: one 16-byte msj_field per (path, document), path-major, so that each path
 * is a contiguous column.  The reference stops in front of this (its dom/element, object and array files are empty; the
 * three codes below sit in its errors file unused).
 * Paths: msj_paths_create compiles n_paths RFC 6901 JSON pointers, synchronously, into device memory the object owns.  ""
 * is the document's root value; otherwise /seg/seg..., with ~1 for '/' and ~0 for '~'.  Every segment is an OBJECT KEY,
 * compared as bytes with the UNESCAPED key of the document; a numeric segment is a key like any other (array indices are
 * not supported; a key that holds a NUL byte cannot be named, the pointers being C strings).  1 to 16 paths, at most 8 segments per path, each of 0 to 255 bytes (the empty key is legal JSON):
 * MSJ_ERR_BAD_ARGUMENT beyond that or on NULL; 22 (INVALID_JSON_POINTER) for a non-empty pointer that does not start with
 * '/' or a '~' not followed by 0 or 1.  The object is immutable and may be used by any number of later calls on any stream
 * of its context's device; msj_paths_destroy(NULL) does nothing.
 * The call: inputs, D, T, [f_k, e_k), clipping, alignments, argument checks, "asynchronous on `stream`, no host round trip,
 * workspace in the context" and "safe on ANY arrays" are those of msj_tape_documents_device, with d_fields (16-byte aligned,
 * n_paths * capacity records; NULL only with capacity 0) in the place of its outputs and NULL `paths`, or paths of another
 * device, MSJ_ERR_BAD_ARGUMENT.  d_numbers_result is READ here: the records searched are the first min(n_numbers,
 * numbers_capacity); without it no record is available.
 * Lookup of path p (segments s_0 .. s_(L-1)) in document k with verdict 0: start with v = f_k; for l = 0 .. L-1:
 *   if d_type[v] != '{', or m = d_match[v] is not in (v, e_k): code 17 (INCORRECT_TYPE), stop
 *   the members of v are the tokens i in (v, m) with d_type[i] == '"', d_depth[i] == d_depth[v] + 1 and d_type[i + 1] == ':'
 *   (any token strictly between partners is at least that deep, so these are exactly the direct keys; f_k sits at depth 0,
 *   so they are the keys at depth l + 1)
 *   the match is the SMALLEST such i whose unescaped body equals s_l: the first duplicate wins, as in at_key (json.loads
 *   keeps the last); none: code 20 (NO_SUCH_FIELD), stop; else v = i + 2
 * and the value is token v with code 0.  A key with MSJ_SPAN_ESCAPED is unescaped as msj_tape_device does it; it can only
 * match when its raw length lies in [len(s), 6 * len(s)].
 * d_fields[p * capacity + k] for k < D; records for k >= D are not written.  A number's bits are those of the msj_number
 * record whose token is v (binary search: the records are in token order); with no record available (d_numbers or
 * d_numbers_result NULL, the record not stored, or of an ERR kind) type is 'd' / 'l' from MSJ_SPAN_FLOAT -- exact in a
 * document with verdict 0 -- and MSJ_FIELD_NO_BITS is set.  d_verdicts == NULL looks every document up (unspecified where
 * one is invalid, still in bounds).  d_result: code 0, or MSJ_CAPACITY when D > capacity (then n_documents = D and no record
 * is written).  n == 0 or D == 0 writes a zero result (n_paths kept).
 */
#define MSJ_FIELD_NO_BITS 64u   /* msj_field.flags: a number without a record: bits = 0, type from MSJ_SPAN_FLOAT */
typedef struct msj_paths msj_paths;
typedef struct msj_field {   /* 16 bytes, one per (path, document) */
    uint64_t bits;   /* 'l': the int64; 'd': the binary64 bit pattern; '"': (d_idx[v] + 1) | (d_end[v] - d_idx[v] - 1) << 32, the
                        raw body's window offset and length; '{' '[': d_match[v], a window token; 't' 'f' 'n' and code != 0: 0 */
    uint32_t token;  /* v as a window index; 0xFFFFFFFF when code != 0 */
    uint8_t  type;   /* the tape's tag of the value: '{' '[' '"' 'l' 'd' 't' 'f' 'n'; 0 when code != 0 */
    uint8_t  flags;  /* MSJ_SPAN_ESCAPED of a string value; MSJ_FIELD_NO_BITS on a number when no record was available */
    uint16_t code;   /* 0; 20 NO_SUCH_FIELD; 17 INCORRECT_TYPE; or d_verdicts[k].code when that is not 0 (nothing is looked up) */
} msj_field;
typedef struct msj_select_documents_result {  /* 48 bytes */
    int32_t  code;         /* 0, or MSJ_CAPACITY: more complete documents than `capacity`, no record written */
    uint32_t flags;        /* 0 */
    uint64_t n_documents;  /* D */
    uint64_t n_paths;
    uint64_t n_found;      /* records with code 0, over all paths */
    uint64_t n_no_bits;    /* records with MSJ_FIELD_NO_BITS */
    uint64_t reserved;
} msj_select_documents_result;
int32_t msj_paths_create(msj_ctx *ctx, const char *const *pointers, uint32_t n_paths, msj_paths **out);
void msj_paths_destroy(msj_paths *paths);
int32_t msj_select_documents_device(msj_ctx *ctx, const msj_paths *paths,
        const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
        const uint8_t *d_type, const int32_t *d_depth, const uint32_t *d_match, const uint32_t *d_end, const uint8_t *d_flags,
        const uint32_t *d_doc_first, const msj_documents_result *d_docs,
        const msj_number *d_numbers, uint64_t numbers_capacity, const msj_numbers_result *d_numbers_result,
        const msj_document_verdict *d_verdicts,
        msj_field *d_fields, uint64_t capacity, msj_select_documents_result *d_result, void *stream);
/* Device workspace of one msj_select_documents_device call (the context keeps it): two state words per (path, document). */
uint64_t msj_select_documents_workspace_bytes(uint64_t n, uint64_t len, uint64_t capacity, uint32_t n_paths);

/*
 * ---- a selected path's strings as one column (DERIVED) ------------------------------------------
 * msj_string_column_device -- for ONE path of msj_select_documents_device, the string values of every document in the
 * standard variable-length layout: d_offsets[D + 1], the unescaped bytes back to back in d_bytes, a validity byte per row in
 * d_valid.  (A numeric column needs no call: an msj_field carries the int64 / binary64 in `bits`, so it is a strided view of
 * d_fields.)  All on the device, on the caller's stream, no host round trip.
 * Inputs: d_buf / len, the window the select call ran over; d_column = d_fields + p * (the select call's capacity), path p's
 * records; d_select, the device msj_select_documents_result of that call.  D = d_select->n_documents is read on the device.
 * d_select->code != 0: d_result is a zero result with that code and nothing else is written.  D > capacity: MSJ_CAPACITY with
 * n_rows = D and nothing else is written (a window has fewer than 2^31 tokens: D >= 2^31, which no call writes, is treated
 * the same whatever the capacity).
 * Row k (k < D) is a string, d_valid[k] = 1, iff its record has code == 0, type == '"' and its span b = bits & 0xFFFFFFFF,
 * r = bits >> 32 satisfies b + r <= len: a record whose span does not lie inside the window is no string and is never
 * dereferenced.  A row that is no string has d_valid[k] = 0 and length 0.  A string's length ulen(k) is r without
 * MSJ_SPAN_ESCAPED in the record's flags, else what msj_tape_device's ulen gives for the body [b, b + r): the same escapes,
 * the same UTF-8 of \u, the same surrogate pairs.
 *   d_offsets[0] = 0, d_offsets[k + 1] = d_offsets[k] + ulen(k) for k < D; uint64, so that no input -- records from anywhere
 *                included -- has an overflow case.  capacity + 1 entries; those past D are not written
 *   d_valid      capacity entries; those at or past D are not written
 *   d_bytes      [d_offsets[k], d_offsets[k + 1]) is row k's unescaped body: no length prefix, no terminator.  Bytes at or past
 *                min(total_bytes, bytes_capacity) are not written: with total_bytes > bytes_capacity the offsets and d_valid are
 *                complete, the bytes clipped, the code MSJ_CAPACITY, and total_bytes says what to allocate.  d_bytes == NULL
 *                (with bytes_capacity 0) is the layout-only form: offsets, d_valid and total_bytes exact, code 0
 * d_result: code; n_rows = D; n_strings the rows with d_valid = 1, n_escaped those of them that were unescaped; total_bytes =
 * d_offsets[D]; n_other the rows whose record has code 0 and that are no string (a number, a container, true / false / null);
 * a row whose record has a code (NO_SUCH_FIELD, INCORRECT_TYPE, an invalid document's) is in neither count.  D == 0 writes
 * d_offsets[0] = 0 and a zero result.
 * Arguments: d_column 16-byte aligned; d_offsets, d_select, d_result 8-byte; d_valid, d_bytes any.  NULL d_result / d_select /
 * d_buf, NULL d_column / d_offsets / d_valid with capacity > 0, NULL d_bytes with bytes_capacity > 0, or an off-grid pointer:
 * MSJ_ERR_BAD_ARGUMENT; len > MSJ_MAX_SEGMENT_BYTES: MSJ_CAPACITY; nothing is launched on either.  Asynchronous on `stream`,
 * workspace in the context.  Safe on ANY records: the window is read only inside [0, len), every store to d_bytes is checked
 * against bytes_capacity, and rows at or past D are not touched.
 */
typedef struct msj_string_column_result {   /* 48 bytes */
    int32_t  code;         /* 0; MSJ_CAPACITY (rows > capacity: nothing else written; or total_bytes > bytes_capacity:
                              offsets / valid complete, bytes clipped); or d_select->code when that is not 0 */
    uint32_t flags;        /* 0 */
    uint64_t n_rows;       /* D */
    uint64_t n_strings;    /* rows with valid = 1 */
    uint64_t n_escaped;    /* ... of which were unescaped */
    uint64_t total_bytes;  /* offsets[D], exact also when clipped and when d_bytes == NULL */
    uint64_t n_other;      /* rows with code 0 whose value is not a string (number, container, true/false/null) */
} msj_string_column_result;
int32_t msj_string_column_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len,
        const msj_field *d_column, const msj_select_documents_result *d_select,
        uint64_t *d_offsets, uint8_t *d_valid, uint64_t capacity,
        uint8_t *d_bytes, uint64_t bytes_capacity,
        msj_string_column_result *d_result, void *stream);
/* Device workspace of one msj_string_column_device call (the context keeps it): 4 bytes per row of capacity, 8 per 256 rows. */
uint64_t msj_string_column_workspace_bytes(uint64_t capacity);

/*
 * ---- a selected path's arrays as a list column (DERIVED) ----------------------------------------
 * msj_array_column_device -- for ONE path of msj_select_documents_device, the arrays of every document as a list column:
 * d_offsets[D + 1], a validity byte per row in d_valid, and the elements back to back in d_elements, each an msj_field.  So a
 * list<int64 / double> is a strided view of d_elements, a list<string> one msj_string_column_device call over the element
 * records, and element j of row k is d_elements[d_offsets[k] + j] -- which also covers what an array index at the end of a
 * pointer would have given (the pointer grammar is unchanged: a numeric segment stays a key).  All on the device, on the
 * caller's stream, no host round trip.
 * Inputs: the token arrays, the split (d_doc_first, d_docs) and the number records with their result, exactly those the
 * select call ran over; d_column = d_fields + p * (the select call's capacity), path p's records; d_select, the device
 * msj_select_documents_result of that call.  D, T, [f_k, e_k) and clipping are msj_select_documents_device's, read on the
 * device from d_docs.  d_select cross-checks and is never trusted: d_select->code != 0: d_result is a zero result with that
 * code and nothing else is written; d_select->n_documents != D (a result of another window): a zero result with code
 * MSJ_ERR_BAD_ARGUMENT in d_result, nothing else written; D > capacity: MSJ_CAPACITY with n_rows = D, nothing else written.
 * Row k (k < D) is an array, d_valid[k] = 1, iff all of the following hold, each checked on the arrays and not believed from
 * the record: the record has code == 0 and type == '['; v = token lies in [f_k, e_k); d_type[v] == '['; m = d_match[v] lies in
 * (v, e_k).  Anything else gives d_valid[k] = 0 and no elements.
 * The elements of row k are the tokens i in (v, m) with d_depth[i] == d_depth[v] + 1 (a direct child: everything between
 * partners is deeper), d_type[i - 1] '[' or ',' (the start of a value, not the comma) and d_type[i] neither ']' nor '}' (the
 * ']' of a nested [] has '[' in front of it and carries its container's depth), in token order.
 *   d_offsets    d_offsets[k] = the number of elements of the rows in front of k, d_offsets[D] = n_elements; uint64, capacity
 *                + 1 entries; those past D are not written
 *   d_valid      capacity entries; those at or past D are not written
 *   d_elements   d_elements[d_offsets[k] + j] = the record of the j-th element token i of row k as the select call would write
 *                it for a value at token i: the same tags, spans, number bits (the record found by token, MSJ_FIELD_NO_BITS
 *                without one), container partners, code 0.  Records at or past min(n_elements, elements_capacity) are not
 *                written: with n_elements > elements_capacity the offsets and d_valid are complete, the elements clipped, the
 *                code MSJ_CAPACITY, and n_elements says what to allocate.  d_elements == NULL (with elements_capacity 0) is the
 *                layout-only form: offsets, d_valid and n_elements exact, code 0
 *   d_elements_select  NULL, or a msj_select_documents_result for the element records: code = this call's code, n_documents =
 *                n_found = n_elements, n_paths = 1, n_no_bits as in d_result.  msj_string_column_device(d_buf, len, d_elements,
 *                d_elements_select, ...) then runs unchanged on the elements, and refuses a clipped list by its code
 * d_result: code; n_rows = D; n_arrays the rows with d_valid = 1; n_elements; n_other the rows whose record has code 0 and that
 * are no array; n_no_bits the element records WRITTEN with MSJ_FIELD_NO_BITS (0 in the layout-only form).  D == 0 writes
 * d_offsets[0] = 0 and a zero result.
 * Arguments: d_idx, d_depth, d_match, d_end, d_numbers, d_column, d_elements 16-byte aligned; d_type, d_flags, d_docs,
 * d_numbers_result, d_select, d_offsets, d_result, d_elements_select 8-byte; d_doc_first 4-byte; d_valid any.  NULL d_result /
 * d_select / d_docs, a NULL token array with n > 0, NULL d_column / d_offsets / d_valid with capacity > 0, NULL d_elements with
 * elements_capacity > 0, NULL d_numbers with numbers_capacity > 0, or an off-grid pointer: MSJ_ERR_BAD_ARGUMENT; n >= 2^31:
 * MSJ_CAPACITY; nothing is launched on either.  Asynchronous on `stream`, workspace in the context.  Safe on ANY arrays and
 * records: every index from a record, d_match or d_doc_first is checked before it is used, every store to d_elements is checked
 * against elements_capacity, and rows at or past D are not touched.  For a d_doc_first that is not what the split writes the
 * outputs are unspecified, still in bounds.
 * Out of scope: rows other than a select column's (so no list of lists in one step -- a nested array is an element record of
 * type '[', which msj_array_elements_device takes as a row), and any change to the pointer grammar.
 */
typedef struct msj_array_column_result {   /* 48 bytes */
    int32_t  code;        /* 0; MSJ_CAPACITY (rows > capacity: nothing else written; or n_elements > elements_capacity: offsets /
                             valid complete, elements clipped); d_select->code when that is not 0; MSJ_ERR_BAD_ARGUMENT when
                             d_select is of another window */
    uint32_t flags;       /* 0 */
    uint64_t n_rows;      /* D */
    uint64_t n_arrays;    /* rows with valid = 1 */
    uint64_t n_elements;  /* offsets[D]; exact also when clipped and when d_elements == NULL */
    uint64_t n_other;     /* rows whose record has code 0 and that are no array */
    uint64_t n_no_bits;   /* element records written with MSJ_FIELD_NO_BITS */
} msj_array_column_result;
int32_t msj_array_column_device(msj_ctx *ctx,
        const uint32_t *d_idx, uint64_t n, const uint8_t *d_type, const int32_t *d_depth, const uint32_t *d_match,
        const uint32_t *d_end, const uint8_t *d_flags, const uint32_t *d_doc_first, const msj_documents_result *d_docs,
        const msj_number *d_numbers, uint64_t numbers_capacity, const msj_numbers_result *d_numbers_result,
        const msj_field *d_column, const msj_select_documents_result *d_select,
        uint64_t *d_offsets, uint8_t *d_valid, uint64_t capacity,
        msj_field *d_elements, uint64_t elements_capacity,
        msj_array_column_result *d_result, msj_select_documents_result *d_elements_select, void *stream);
/* Device workspace of one msj_array_column_device call (the context keeps it): 16 bytes per row, 4 per 1 024 tokens. */
uint64_t msj_array_column_workspace_bytes(uint64_t n, uint64_t capacity);

/*
 * ---- fields by path inside the elements of a list column (DERIVED) ------------------------------
 * msj_select_elements_device -- msj_select_documents_device with ELEMENTS as the rows instead of documents: for up to 16
 * paths and every element record of an array column, one msj_field per (path, row), path-major.  For "items":[{"sku":..,
 * "qty":..,"dims":{"w":..}}, ...] the paths /sku, /qty and /dims/w are columns on the device, aligned with the list
 * column's d_offsets: a list of structs.  Everything downstream composes as it does for a document column: a numeric column
 * is a strided view of d_fields, a string column one msj_string_column_device call, a nested array one more
 * msj_array_column_device-style record of type '['.  The pointer grammar is unchanged (msj_paths_create; no '*', no indices).
 * Inputs: the window, the token arrays and the number records with their result, exactly those the array-column call ran
 * over; d_rows = that call's d_elements, d_rows_select = its d_elements_select.  R = d_rows_select->n_documents is read on
 * the device.  The window's n stands where a document's e_k stood.
 *   d_rows_select->code != 0 (a clipped element list arrives this way): d_result is a zero result with that code and nothing
 *                else is written
 *   R > capacity: MSJ_CAPACITY with n_documents = R (n_paths kept), no record written
 *   order:       the records' `token` fields must ascend strictly over r = 0 .. R-1, compared as uint32 (array-column output
 *                always does).  Checked on the device, not believed: on a violation code = MSJ_ERR_BAD_ARGUMENT, n_documents = R
 *                (n_paths kept), no record written
 * Row r is USABLE iff all of the following hold, each re-checked on the arrays: its record has code == 0 and type == '{'; v =
 * token < n; d_type[v] == '{'; m = d_match[v] lies in (v, n).
 * Lookup of path p (segments s_0 .. s_(L-1)) in row r:
 *   the record has a code != 0: that code is copied (an array-column record never has one)
 *   L == 0 and v < n: the record is that of the value at token v, re-derived from the arrays (the row's own value)
 *   otherwise a row that is not usable: code 17 (INCORRECT_TYPE)
 *   otherwise the loop of msj_select_documents_device from lo = v, with n in the place of e_k: the members of the object lo
 *   are the tokens i in (lo, d_match[lo]) with d_type[i] == '"', d_depth[i] == d_depth[lo] + 1 and d_type[i + 1] == ':' -- the
 *   depth is that of the OBJECT, rows sit at whatever depth their array does -- the SMALLEST i whose unescaped body equals
 *   s_l wins, none: code 20 (NO_SUCH_FIELD); the value is token i + 2, which before the last segment must be a '{' with its
 *   partner in (i + 2, n), else code 17
 * Which row a key can belong to: key token i belongs to the LAST row r with token_r < i, and is a member for that row alone.
 * For true element records that is the enclosing element (siblings are disjoint and ascending); for any other records --
 * one row inside another, say -- it makes the output a function of the input: row r sees the keys i <= token_(r+1) only.
 * The key compare, the unescape, the raw-length rule, the number-record search and MSJ_FIELD_NO_BITS are
 * msj_select_documents_device's, unchanged.
 * d_fields[p * capacity + r] for r < R; records at or past R are not written.  d_result: a msj_select_documents_result with
 * code, n_documents = R, n_paths, n_found, n_no_bits -- so msj_string_column_device(d_buf, len, d_fields + p * capacity,
 * d_result, ...) runs unchanged on any of the new columns.  R == 0 and n == 0 need no special case: with n == 0 no row is
 * usable.
 * Arguments: d_idx, d_depth, d_match, d_end, d_numbers, d_rows, d_fields 16-byte aligned; d_type, d_flags, d_numbers_result,
 * d_rows_select, d_result 8-byte.  NULL ctx / paths / d_result / d_rows_select, paths of another device, d_result ==
 * d_rows_select, a NULL window or token array with n > 0, NULL d_rows / d_fields with capacity > 0, NULL d_numbers with
 * numbers_capacity > 0, or an off-grid pointer: MSJ_ERR_BAD_ARGUMENT; n >= 2^31 or len > MSJ_MAX_SEGMENT_BYTES: MSJ_CAPACITY;
 * nothing is launched on either.  Asynchronous on `stream`, no host round trip, workspace in the context.  Safe on ANY arrays
 * and records: every index from a record, d_match or d_end is checked before it is used, the window is read only inside
 * [0, len), and rows at or past R are not touched.
 * Out of scope: a list of lists in one step (msj_array_elements_device opens a column of '[' records), rows other than
 * ascending element records, any change to the pointer grammar.
 */
int32_t msj_select_elements_device(msj_ctx *ctx, const msj_paths *paths,
        const uint8_t *d_buf, uint64_t len, const uint32_t *d_idx, uint64_t n,
        const uint8_t *d_type, const int32_t *d_depth, const uint32_t *d_match, const uint32_t *d_end, const uint8_t *d_flags,
        const msj_number *d_numbers, uint64_t numbers_capacity, const msj_numbers_result *d_numbers_result,
        const msj_field *d_rows, const msj_select_documents_result *d_rows_select,
        msj_field *d_fields, uint64_t capacity, msj_select_documents_result *d_result, void *stream);
/* Device workspace of one msj_select_elements_device call (the context keeps it): two state words per (path, row) and 4 bytes
 * per row, for min(n, capacity) rows. */
uint64_t msj_select_elements_workspace_bytes(uint64_t n, uint64_t capacity, uint32_t n_paths);

/*
 * ---- the arrays inside list rows as a list column (DERIVED) --------------------------------------
 * msj_array_elements_device -- msj_array_column_device with ANY ascending msj_field records as the rows instead of one record
 * per document: the arrays among the elements of a list column -- a list of lists, "coordinates":[[x,y],[x,y],...] -- or one
 * path's records of msj_select_elements_device -- a list inside a list of structs, items[*].tags.  The output is again
 * d_offsets[R + 1], a validity byte per row, the element records back to back and a msj_select_documents_result for them, so
 * msj_string_column_device, msj_select_elements_device and this call itself run on it unchanged, to any depth.  All on the
 * device, on the caller's stream, no host round trip.
 * Inputs: the token arrays and the number records with their result, exactly those the call that wrote the rows ran over;
 * d_rows / d_rows_select = an array-column call's (or this call's) d_elements / d_elements_select, or d_fields + p * capacity /
 * d_result of a select-elements call.  R = d_rows_select->n_documents is read on the device.  There is no split and no d_docs:
 * the window's n stands where a document's e_k stood.
 *   d_rows_select->code != 0 (a clipped element list arrives this way): d_result is a zero result with that code and nothing
 *                else is written
 *   R > capacity: MSJ_CAPACITY with n_rows = R, nothing else written
 *   order:       a select-elements column holds records with a code (20, 17), whose token is 0xFFFFFFFF.  The rows whose
 *                record has code == 0 are the LIVE rows; their tokens must ascend strictly over r, compared as uint32
 *                (array-column output does; so does select-elements output over true element rows: a found value lies inside
 *                its own element).  Checked on the device, not believed: on a violation code = MSJ_ERR_BAD_ARGUMENT, n_rows = R,
 *                every count 0, nothing else written -- neither d_valid nor d_offsets
 * Row r (r < R) is an array, d_valid[r] = 1, iff all of the following hold, each re-checked on the arrays: its record has
 * code == 0 and type == '['; v = token < n; d_type[v] == '['; m = d_match[v] lies in (v, n).  A row with a code and a row of
 * any other kind are both invalid and have no elements.
 * Which row a token belongs to: token i belongs to the LAST live row whose token lies below i, and to that row alone.  For
 * true rows that is no restriction (siblings are disjoint and ascending); for any other records -- one row inside another,
 * say -- it makes the output a function of the input: row r sees the tokens i <= the next live row's token only.
 * The elements of row r are the tokens i that belong to r, in token order, with v < i < m, d_depth[i] == d_depth[v] + 1,
 * d_type[i - 1] '[' or ',' and d_type[i] neither ']' nor '}': msj_array_column_device's element test.
 *   d_offsets    d_offsets[r] = the number of elements of the rows in front of r, d_offsets[R] = n_elements; a row with a code,
 *                or with token >= n, has the next row's offset.  uint64, capacity + 1 entries; those past R are not written
 *   d_valid      capacity entries; those at or past R are not written
 *   d_elements   as in msj_array_column_device: the record of the value at token i (MSJ_FIELD_NO_BITS and the number-record
 *                search unchanged), clipped at elements_capacity -- then the offsets and d_valid are complete, the code is
 *                MSJ_CAPACITY and n_elements is exact.  d_elements == NULL (with elements_capacity 0) is the layout-only form
 *   d_elements_select  NULL, or written wherever d_result is: code = this call's code, n_documents = n_found = n_elements (0 on
 *                a stop), n_paths = 1, n_no_bits as in d_result
 * d_result: a msj_array_column_result -- code; n_rows = R; n_arrays the rows with d_valid = 1; n_elements; n_other the rows
 * whose record has code 0 and that are no array; n_no_bits the element records written with MSJ_FIELD_NO_BITS.  R == 0 writes
 * d_offsets[0] = 0 and a zero result; with n == 0 no row is valid.
 * Arguments: d_idx, d_depth, d_match, d_end, d_numbers, d_rows, d_elements 16-byte aligned; d_type, d_flags, d_numbers_result,
 * d_rows_select, d_offsets, d_result, d_elements_select 8-byte; d_valid any.  NULL ctx / d_result / d_rows_select, a NULL token
 * array with n > 0, NULL d_rows / d_offsets / d_valid with capacity > 0, NULL d_elements with elements_capacity > 0, NULL
 * d_numbers with numbers_capacity > 0, d_elements_select == d_rows_select, d_elements == d_rows, or an off-grid pointer:
 * MSJ_ERR_BAD_ARGUMENT; n >= 2^31: MSJ_CAPACITY.  The checks come in msj_array_column_device's order -- missing arrays, the
 * size, then outputs and alignment -- and nothing is launched on either.  Asynchronous on `stream`, no host round trip,
 * workspace in the context.  Safe on ANY arrays and records: every index from a record or from d_match is checked before it is
 * used, every store to d_elements is checked against elements_capacity, and rows at or past R are not touched.
 * Out of scope: any change to the pointer grammar (no '*', no indices), typed numeric columns.  (An object's members as
 * rows: msj_object_entries_device.)
 */
int32_t msj_array_elements_device(msj_ctx *ctx,
        const uint32_t *d_idx, uint64_t n, const uint8_t *d_type, const int32_t *d_depth, const uint32_t *d_match,
        const uint32_t *d_end, const uint8_t *d_flags,
        const msj_number *d_numbers, uint64_t numbers_capacity, const msj_numbers_result *d_numbers_result,
        const msj_field *d_rows, const msj_select_documents_result *d_rows_select,
        uint64_t *d_offsets, uint8_t *d_valid, uint64_t capacity,
        msj_field *d_elements, uint64_t elements_capacity,
        msj_array_column_result *d_result, msj_select_documents_result *d_elements_select, void *stream);
/* Device workspace of one msj_array_elements_device call (the context keeps it): 8 bytes per row of capacity and 8 per 256 of
 * them, 24 per row of min(n, capacity), 4 per 1 024 tokens. */
uint64_t msj_array_elements_workspace_bytes(uint64_t n, uint64_t capacity);

/*
 * ---- an object's members as a map column (DERIVED) ------------------------------------------------
 * msj_object_entries_device -- msj_array_elements_device with OBJECTS as the rows and two records per entry: an object whose
 * keys are data, not schema -- "attrs":{"color":"red","size":"L"}, "counts":{"2024-01-01":3,...}, a map of maps -- as
 * d_offsets[R + 1], a validity byte per row and, back to back, the key's record in d_keys and the value's in d_values at the
 * same position.  Both record arrays come with a msj_select_documents_result, so msj_string_column_device runs on the keys
 * and msj_array_elements_device, msj_select_elements_device and this call itself on the values, unchanged.  All on the
 * device, on the caller's stream, no host round trip.
 * Inputs: the token arrays and the number records with their result, exactly those the call that wrote the rows ran over;
 * d_rows / d_rows_select = ANY msj_field records with their select result: one path's column of msj_select_documents_device
 * (d_fields + p * capacity, its d_result: the rows are the documents), the d_elements / d_elements_select of an array call,
 * one path of msj_select_elements_device, or this call's own d_values / d_values_select.  R = d_rows_select->n_documents is
 * read on the device.  There is no split and no d_docs: the window's n stands where a document's e_k stood.
 *   d_rows_select->code != 0: d_result is a zero result with that code and nothing else is written
 *   R > capacity: MSJ_CAPACITY with n_rows = R, nothing else written
 *   order:       the rows whose record has code == 0 are the LIVE rows; their tokens must ascend strictly over r, compared as
 *                uint32.  Checked on the device, not believed: on a violation code = MSJ_ERR_BAD_ARGUMENT, n_rows = R, every
 *                count 0, nothing else written -- neither d_valid nor d_offsets
 *   on every stop only d_result and the two select results (when given) are written
 * Row r (r < R) is an object, d_valid[r] = 1, iff all of the following hold, each re-checked on the arrays: its record has
 * code == 0 and type == '{'; v = token < n; d_type[v] == '{'; m = d_match[v] lies in (v, n).  Every other row is invalid and
 * has no entries.
 * Which row a token belongs to: token i belongs to the LAST live row whose token lies below i, and to that row alone.
 * The entries of row r are the tokens i that belong to r, in token order, with v < i, i + 2 < m, d_depth[i] == d_depth[v] + 1,
 * d_type[i] == '"' and d_type[i + 1] == ':'.  For entry number e, counted over the window, d_keys[e] is the record of the value
 * at token i -- a string record: the raw span, MSJ_SPAN_ESCAPED in flags -- and d_values[e] the record of the value at token
 * i + 2, both as msj_select_documents_device writes a value (MSJ_FIELD_NO_BITS and the number-record search unchanged).
 * Duplicate keys are all kept, in document order; {} is a valid row without entries.  Rows in a document with a verdict code
 * and malformed members ({"a":}) give unspecified, in-bounds output.
 *   d_offsets    d_offsets[r] = the number of entries in front of row r -- for a live row with token < n the entries whose key
 *                token is at or below the row's token --, d_offsets[R] = n_entries; a row with a code, or with token >= n, has
 *                the next row's offset.  uint64, capacity + 1 entries; those past R are not written
 *   d_valid      capacity entries; those at or past R are not written
 *   d_keys, d_values  records at or past min(n_entries, entries_capacity) are not written; with n_entries > entries_capacity the
 *                offsets and d_valid are complete, the code is MSJ_CAPACITY and n_entries is exact.  Both NULL (with
 *                entries_capacity 0) is the layout-only form
 *   d_keys_select, d_values_select  each NULL, or written wherever d_result is: code = this call's code, n_documents = n_found =
 *                n_entries (0 on a stop), n_paths = 1, n_no_bits 0 for the keys and d_result's for the values
 * d_result: a msj_object_entries_result -- code; n_rows = R; n_objects the rows with d_valid = 1; n_entries; n_other the live
 * rows that are no object; n_no_bits the value records written with MSJ_FIELD_NO_BITS.  R == 0 writes d_offsets[0] = 0 and a
 * zero result; with n == 0 no row is valid.
 * Arguments: d_idx, d_depth, d_match, d_end, d_numbers, d_rows, d_keys, d_values 16-byte aligned; d_type, d_flags,
 * d_numbers_result, d_rows_select, d_offsets, d_result, d_keys_select, d_values_select 8-byte; d_valid any.  NULL ctx /
 * d_result / d_rows_select, a NULL token array with n > 0, NULL d_rows / d_offsets / d_valid with capacity > 0, NULL d_keys with
 * entries_capacity > 0, exactly one of d_keys / d_values NULL, NULL d_numbers with numbers_capacity > 0, d_keys, d_values or a
 * select result that is the rows, their select result or each other, or an off-grid pointer: MSJ_ERR_BAD_ARGUMENT; n >= 2^31:
 * MSJ_CAPACITY.  The checks come in msj_array_elements_device's order -- missing arrays, the size, then outputs and alignment
 * -- and nothing is launched on either.  Asynchronous on `stream`, no host round trip, workspace in the context.  Safe on ANY
 * arrays and records: every index from a record or from d_match is checked before it is used, tokens i + 1 and i + 2 are read
 * only below n, every store to d_keys / d_values is checked against entries_capacity, and rows at or past R are not touched.
 * Out of scope: any change to the pointer grammar, lookup of a run-time key, de-duplicating keys (the distinct keys of a map
 * column are msj_dictionary_device over msj_string_column_device over d_keys), typed numeric columns.
 */
typedef struct msj_object_entries_result {   /* 48 bytes; the layout of msj_array_column_result */
    int32_t  code;          /* 0, MSJ_CAPACITY, MSJ_ERR_BAD_ARGUMENT (the order), or the code of d_rows_select */
    uint32_t flags;         /* 0 */
    uint64_t n_rows;        /* R */
    uint64_t n_objects;     /* rows with d_valid = 1 */
    uint64_t n_entries;     /* entries of all rows, exact also when they were clipped */
    uint64_t n_other;       /* live rows that are no object */
    uint64_t n_no_bits;     /* value records written with MSJ_FIELD_NO_BITS */
} msj_object_entries_result;
int32_t msj_object_entries_device(msj_ctx *ctx,
        const uint32_t *d_idx, uint64_t n, const uint8_t *d_type, const int32_t *d_depth, const uint32_t *d_match,
        const uint32_t *d_end, const uint8_t *d_flags,
        const msj_number *d_numbers, uint64_t numbers_capacity, const msj_numbers_result *d_numbers_result,
        const msj_field *d_rows, const msj_select_documents_result *d_rows_select,
        uint64_t *d_offsets, uint8_t *d_valid, uint64_t capacity,
        msj_field *d_keys, msj_field *d_values, uint64_t entries_capacity,
        msj_object_entries_result *d_result,
        msj_select_documents_result *d_keys_select, msj_select_documents_result *d_values_select, void *stream);
/* Device workspace of one msj_object_entries_device call (the context keeps it): msj_array_elements_workspace_bytes' sizes. */
uint64_t msj_object_entries_workspace_bytes(uint64_t n, uint64_t capacity);

/*
 * ---- a selected value's JSON text as a column (DERIVED) ---------------------------------------------
 * msj_raw_column_device -- simdjson's raw_json(), get_json_object of the dataframe engines: the value ITSELF, as JSON text,
 * for every row of any msj_field records, in the standard variable-length layout: d_offsets[R + 1], the bytes back to back
 * in d_bytes, a validity byte per row in d_valid.  It is the column for a field whose shape differs from line to line, for a
 * subtree that is handed on unparsed, and for re-emitting a window as minified NDJSON.  All on the device, on the caller's
 * stream, no host round trip.
 * Inputs: d_buf / len and the token arrays of the window the records were written over (d_depth is not among them; d_match
 * may be NULL: it is not read, a container's closing token is its record's bits); d_rows / d_rows_select = ANY msj_field
 * records with their select result: a path of msj_select_documents_device (d_fields + p * capacity, its d_result), the
 * d_elements / d_elements_select of an array call, a path of msj_select_elements_device, the d_keys or d_values of
 * msj_object_entries_device with their select result.  The rows need NOT ascend: every row is treated on its own, and two
 * rows may name the same value.  R = d_rows_select->n_documents is read on the device.
 *   d_rows_select->code != 0: d_result is a zero result with that code (flags kept) and nothing else is written
 *   R > capacity, or R >= 2^31: MSJ_CAPACITY with n_rows = R, nothing else written
 * Token text: lim(i) = d_idx[i + 1] for i + 1 < n, else len, and never more than len.  te(i) =
 *   d_end[i] + 1                                  d_flags[i] has MSJ_SPAN_STRING
 *   d_end[i]                                      MSJ_SPAN_NUMBER without MSJ_SPAN_LONG
 *   lim(i) minus the blanks (space \t \n \r) directly in front of it    MSJ_SPAN_NUMBER with MSJ_SPAN_LONG
 *   d_idx[i] + 4 / + 5 / + 1                      d_type[i] 't' or 'n' / 'f' / anything else
 * clipped to lim(i), and tl(i) = te(i) - d_idx[i], 0 when that is negative.  On any arrays the text of a token then lies in
 * [0, len) and ends at or in front of lim(i).
 * Row k (k < R) is a value, d_valid[k] = 1, iff its record has code == 0 and token < n and, for type '{' or '[', last = bits
 * satisfies token < last < n; for every other type last = token.  A record with code 0 that fails the test is counted in
 * n_other, has d_valid[k] = 0 and length 0 and is never dereferenced; a record with a code has d_valid[k] = 0 and length 0
 * and is in neither count.
 *   flags 0, verbatim:   row k's bytes are d_buf[d_idx[token] .. te(last)) -- the source's text, blanks and escapes included;
 *                        no byte when the arrays put te(last) in front of d_idx[token].  No pass over the tokens runs
 *   MSJ_RAW_COMPACT:     row k's bytes are the texts of the tokens token .. last back to back: the blanks BETWEEN tokens are
 *                        dropped, those inside a string stay.  The length is P[last + 1] - P[token], P the exclusive sum of
 *                        tl over the window's tokens (one pass and a scan, 64-bit throughout).  A pretty-printed window gives
 *                        the bytes of its minified twin
 *   d_offsets    d_offsets[0] = 0, d_offsets[k + 1] = d_offsets[k] + the length of row k; uint64; capacity + 1 entries,
 *                those past R are not written
 *   d_valid      capacity entries; those at or past R are not written
 *   d_bytes      bytes at or past min(total_bytes, bytes_capacity) are not written: with total_bytes > bytes_capacity the
 *                offsets and d_valid are complete, the bytes clipped, the code MSJ_CAPACITY and total_bytes exact.
 *                d_bytes == NULL (with bytes_capacity 0) is the layout-only form: code 0
 * d_result: code; flags, the call's; n_rows = R; n_values the rows with d_valid = 1; n_containers those of them of type '{'
 * or '['; total_bytes = d_offsets[R]; n_other.  R == 0 writes d_offsets[0] = 0 and a zero result (flags kept).
 * Arguments, checked in this order: NULL ctx / d_result / d_rows_select / d_buf; NULL d_idx / d_type / d_end / d_flags with
 * n > 0; NULL d_rows / d_offsets / d_valid with capacity > 0; NULL d_bytes with bytes_capacity > 0 or a flag other than
 * MSJ_RAW_COMPACT: MSJ_ERR_BAD_ARGUMENT.  len > MSJ_MAX_SEGMENT_BYTES or n >= 2^31: MSJ_CAPACITY.  Then alignment: d_rows
 * 16-byte; d_offsets, d_rows_select, d_result 8-byte; d_idx, d_match, d_end 4-byte; the others any: MSJ_ERR_BAD_ARGUMENT.
 * Nothing is launched on any of them.  Asynchronous on `stream`, no host round trip, workspace in the context.  Safe on ANY
 * arrays and records: a token from a record is used only below n, every read of the window lies in [0, len), every store
 * to d_bytes is below min(total_bytes, bytes_capacity), and rows at or past R are not touched.
 * Out of scope: array indices in pointers, re-serialising numbers or strings, pretty-printing.
 */
#define MSJ_RAW_COMPACT 1u   /* msj_raw_column_device flags: the tokens' texts back to back, blanks between tokens dropped */
typedef struct msj_raw_column_result {   /* 48 bytes */
    int32_t  code;          /* 0; MSJ_CAPACITY (rows > capacity: nothing else written; or total_bytes > bytes_capacity:
                               offsets / valid complete, bytes clipped); or d_rows_select->code when that is not 0 */
    uint32_t flags;         /* the call's flags */
    uint64_t n_rows;        /* R */
    uint64_t n_values;      /* rows with valid = 1 */
    uint64_t n_containers;  /* ... of which are of type '{' or '[' */
    uint64_t total_bytes;   /* offsets[R], exact also when clipped and when d_bytes == NULL */
    uint64_t n_other;       /* rows with code 0 that fail the row test */
} msj_raw_column_result;
int32_t msj_raw_column_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len,
        const uint32_t *d_idx, uint64_t n, const uint8_t *d_type, const uint32_t *d_match,
        const uint32_t *d_end, const uint8_t *d_flags,
        const msj_field *d_rows, const msj_select_documents_result *d_rows_select,
        uint64_t *d_offsets, uint8_t *d_valid, uint64_t capacity,
        uint8_t *d_bytes, uint64_t bytes_capacity, uint32_t flags,
        msj_raw_column_result *d_result, void *stream);
/* Device workspace of one msj_raw_column_device call (the context keeps it): 8 bytes per row of capacity, 8 per 256 rows, a
 * list of 1 024 long rows; with MSJ_RAW_COMPACT also 8 bytes per token and 8 per 1 024 tokens. */
uint64_t msj_raw_column_workspace_bytes(uint64_t n, uint64_t capacity, uint32_t flags);

/*
 * ---- a byte column as codes plus distinct values (DERIVED) ------------------------------------------
 * msj_dictionary_device -- the dictionary layout of a variable-length byte column: an int32 code per row and the distinct
 * values back to back.  It answers, without moving a byte to the host: which distinct values does the column have, which
 * rows are equal, and -- over the keys of a map column of the root objects -- which fields do the documents have at all.
 * All on the device, on the caller's stream, no host round trip.
 * Inputs: the (d_offsets, d_bytes, d_valid) layout that msj_string_column_device and msj_raw_column_device write -- a path's
 * strings, a list's strings, a map's keys, raw JSON texts (on a compact raw column: whole sub-objects) -- or any arrays of
 * that shape: d_offsets[rows + 1], d_valid[rows], d_bytes[bytes_len].  R, the number of rows, is `rows` when d_n_rows == NULL,
 * else *d_n_rows read on the device (for example &string_result->n_rows: the call follows a column call without a
 * synchronisation).  R > rows, or R >= 2^31: MSJ_CAPACITY with n_rows = R and nothing else written.
 * Row k (k < R) has a value iff d_valid[k] != 0 and d_offsets[k] <= d_offsets[k + 1] <= bytes_len -- checked on the arrays,
 * never believed; the value is the bytes [d_offsets[k], d_offsets[k + 1]), the empty string is a value.  Any other row is
 * null.  Two rows are equal iff their values are byte for byte equal: no normalisation (the string column has unescaped
 * already, so an A written as the escape u0041 and a plain "A" arrive equal).
 *   d_codes      rows entries, those at or past R not written.  -1 for a null row; else the number of distinct values whose
 *                first occurrence lies in a row in front of the first occurrence of row k's value: the order of first
 *                appearance, what dict.setdefault(v, len(d)) gives over the rows in order
 *   d_dict_first    dict_capacity entries: d_dict_first[c] is the row of code c's first occurrence
 *   d_dict_offsets  dict_capacity + 1 entries: d_dict_offsets[0] = 0, d_dict_offsets[c + 1] - d_dict_offsets[c] the length of
 *                   code c's value
 *   d_dict_bytes    the distinct values back to back in code order, no prefix, no terminator
 * Entries at or past min(n_distinct, dict_capacity) (offsets: one further) and bytes at or past min(d_dict_offsets[that],
 * dict_bytes_capacity) are not written: with n_distinct > dict_capacity or dict_bytes > dict_bytes_capacity the codes are
 * complete, n_distinct and dict_bytes exact, what does not fit is not written, and the code is MSJ_CAPACITY.  All three
 * dictionary arrays NULL with both capacities 0 is the layout-only form: codes and counts, code 0.  (One of them NULL with
 * its capacity 0 writes the others, clipped as above.)
 * Every output but max_probe is a pure function of the input, bit-identical from run to run whatever the scheduling;
 * max_probe is a diagnostic of the hash table's state, which depends on which row reached a slot first.
 * d_result: code; flags, the call's; n_rows = R; n_values the rows that are not null; n_distinct; dict_bytes the total bytes
 * of the distinct values; max_probe the longest probe sequence any row walked.  R == 0 writes d_dict_offsets[0] = 0 and a zero
 * result (flags kept).
 * MSJ_DICTIONARY_WEAK_HASH is a TEST AID, like the forced span kernels: the hash of every row becomes 2^64 - 1 - (length mod
 * 4), so that every chain starts in the table's last four slots and wraps through slot 0, and every slot is decided by the
 * byte compare.  The result is by definition the same as without it.
 * Arguments, checked in this order: NULL ctx / d_result; NULL d_offsets / d_valid / d_codes with rows > 0; NULL d_bytes with
 * bytes_len > 0; NULL d_dict_offsets / d_dict_first with dict_capacity > 0; NULL d_dict_bytes with dict_bytes_capacity > 0; a
 * flag other than MSJ_DICTIONARY_WEAK_HASH: MSJ_ERR_BAD_ARGUMENT.  Then alignment: d_offsets, d_n_rows, d_dict_offsets,
 * d_result 8-byte; d_codes, d_dict_first 4-byte; d_bytes, d_valid, d_dict_bytes any: MSJ_ERR_BAD_ARGUMENT.  Nothing is launched on any of them.  Asynchronous on `stream`, no host round trip, workspace in the
 * context.  Safe on ANY arrays: d_bytes is read only inside [0, bytes_len), every store to the dictionary arrays is checked
 * against its capacity, nothing at or past R is touched.
 * Out of scope: counts per value (bincount of the codes; the Python layer does that), ordering the dictionary by value
 * (msj_dictionary_order_device, below, orders its entries without rewriting it),
 * case or Unicode folding.  One dictionary across windows is msj_dictionary_extend_device, below.
 */
#define MSJ_DICTIONARY_WEAK_HASH 1u   /* msj_dictionary_device flags: TEST AID, every chain in the table's last four slots */
typedef struct msj_dictionary_result {   /* 48 bytes */
    int32_t  code;        /* 0; MSJ_CAPACITY (R > rows or R >= 2^31: nothing else written; or the dictionary clipped: codes
                             complete, counts exact); MSJ_UNEXPECTED_ERROR: a row walked the whole table (never) */
    uint32_t flags;       /* the call's flags */
    uint64_t n_rows;      /* R */
    uint64_t n_values;    /* rows that are not null */
    uint64_t n_distinct;  /* distinct values */
    uint64_t dict_bytes;  /* total bytes of the distinct values, exact also when clipped and in the layout-only form */
    uint64_t max_probe;   /* the longest probe sequence any row walked (a diagnostic; not a function of the input alone) */
} msj_dictionary_result;
int32_t msj_dictionary_device(msj_ctx *ctx,
        const uint64_t *d_offsets, const uint8_t *d_valid, uint64_t rows, const uint64_t *d_n_rows,
        const uint8_t *d_bytes, uint64_t bytes_len,
        int32_t *d_codes,
        uint64_t *d_dict_offsets, uint32_t *d_dict_first, uint64_t dict_capacity,
        uint8_t *d_dict_bytes, uint64_t dict_bytes_capacity,
        uint32_t flags, msj_dictionary_result *d_result, void *stream);
/* Device workspace of one msj_dictionary_device call (the context keeps it): 8 + 4 bytes per row (hash, slot), 4 bytes per
 * table slot (the power of two >= 2 * rows, at least 1 024), 16 per 256 rows (block sums), a list of 1 024 long rows. */
uint64_t msj_dictionary_workspace_bytes(uint64_t rows);

/*
 * ---- one dictionary across windows (DERIVED) -----------------------------------------------------------
 * msj_dictionary_extend_device -- msj_dictionary_device against the P entries the dictionary arrays hold already: a value
 * keeps its code from window to window, so counts per code add, msj_aggregate_device's group g is the same value in every
 * window, and a filter or a sort by code means the same everywhere.  With MSJ_DICTIONARY_FROZEN it encodes against a FIXED
 * vocabulary -- a reference table's codes, a model's categories, an IN-list: the semi-join on the device.
 * The column, R, the row test (checked, never believed) and equality byte for byte are msj_dictionary_device's.
 * The prior dictionary: P = d_n_prior ? *d_n_prior : n_prior, read on the device (&previous_result->n_distinct chains window
 * after window without a host wait).  It is d_dict_offsets[0 .. P] and the bytes below base = d_dict_offsets[P], as an earlier
 * call of either dictionary call wrote them into these arrays; with P = 0 the call writes d_dict_offsets[0] = 0 itself and
 * base = 0.  Prior entry c < P has a value iff d_dict_offsets[c] <= d_dict_offsets[c + 1] <= dict_bytes_capacity -- checked
 * on the array; an entry without a value equals no row and stays where it is.
 *   d_codes      with d = {entry c's bytes: c} over the prior entries in ascending c (the lowest c wins among equal
 *                entries), what `for v in rows: d.setdefault(v, len(d))` gives: a row with a prior value gets that entry's
 *                code, a new value P plus the number of new values whose first row lies in front of its own first row, a
 *                null row -1
 *   appended     the new values in code order: d_dict_offsets[c + 1] for c >= P, d_dict_first[c] the row of THIS column
 *                that first holds the value, the bytes behind base
 * NOTHING OF THE PRIOR DICTIONARY IS WRITTEN: no entry of d_dict_offsets at or below P (but [0] when P = 0), no
 * d_dict_first[c] for c < P, no byte below base -- the first piece of the byte copy starts at base itself, whatever its
 * alignment.  Clipping is msj_dictionary_device's rule: the codes are complete, n_distinct (= P + new values) and dict_bytes
 * (= base + new bytes) exact, what does not fit is not written, and the code is MSJ_CAPACITY.  Because nothing below P / base
 * is ever written, a caller who gets MSJ_CAPACITY copies the prior part into larger arrays and REPEATS THE CALL WITH THE SAME
 * P for the complete answer; repeating any call with the same P gives the same bytes.
 * All three dictionary arrays NULL with both capacities 0 is the layout-only form, legal only with P = 0: codes and counts.
 * R > rows, P > dict_capacity, base > dict_bytes_capacity or P + R >= 2^31: MSJ_CAPACITY, and nothing but code, flags,
 * n_rows and n_prior is written (the other members are 0) -- so a clipped previous call chained through d_n_prior stops
 * the chain by itself.
 * MSJ_DICTIONARY_FROZEN: the three dictionary arrays are read only; a row whose value is no prior entry's gets code -2;
 * n_distinct = P, dict_bytes = base; the code is 0 unless one of the four conditions above holds.
 * MSJ_DICTIONARY_WEAK_HASH keeps its meaning as a test aid, for prior entries and rows alike.
 * Every output but max_probe is a pure function of the input, bit-identical from run to run.
 * Arguments, checked in this order: NULL ctx / d_result; NULL d_offsets / d_valid / d_codes with rows > 0; NULL d_bytes with
 * bytes_len > 0; NULL d_dict_offsets / d_dict_first with dict_capacity > 0; NULL d_dict_bytes with dict_bytes_capacity > 0;
 * n_prior > 0 or d_n_prior != NULL with all three dictionary arrays NULL; a flag other than the two; MSJ_DICTIONARY_FROZEN
 * with all three dictionary arrays NULL: MSJ_ERR_BAD_ARGUMENT.  Then alignment as in msj_dictionary_device, and d_n_prior
 * 8-byte: MSJ_ERR_BAD_ARGUMENT.  Nothing is launched on any of them.  Asynchronous on `stream`, no host round trip, workspace
 * in the context.  Safe on ANY arrays: prior offsets are used only after the entry test, nothing at or past a capacity is
 * written, nothing at or past R is touched.
 * Out of scope: merging msj_aggregate records on the device (two 'd' sums do not merge exactly; that needs the 96-bit
 * accumulators exposed); removing values from a dictionary; ordering it by value (msj_dictionary_order_device); a dictionary over more than 2^31 - 1
 * items (P + R); a hash table kept between calls -- the prior entries are hashed again per call, one read of the
 * dictionary's bytes.
 */
#define MSJ_DICTIONARY_FROZEN 2u   /* look up only: nothing is appended, a value that is not in the dictionary gets code -2 */
typedef struct msj_dictionary_extend_result {   /* 64 bytes; the first 48 are msj_dictionary_result's members, in its order */
    int32_t  code;        /* 0; MSJ_CAPACITY (one of the four conditions: nothing else written; or the dictionary clipped:
                             codes complete, counts exact); MSJ_UNEXPECTED_ERROR: an item walked the whole table (never) */
    uint32_t flags;       /* the call's flags */
    uint64_t n_rows;      /* R */
    uint64_t n_values;    /* rows that are not null */
    uint64_t n_distinct;  /* P + the new values; frozen: P */
    uint64_t dict_bytes;  /* base + the bytes of the new values, exact also when clipped; frozen: base */
    uint64_t max_probe;   /* the longest probe sequence any item walked (a diagnostic; not a function of the input alone) */
    uint64_t n_prior;     /* P */
    uint64_t n_matched;   /* rows whose value is a prior entry's */
} msj_dictionary_extend_result;
int32_t msj_dictionary_extend_device(msj_ctx *ctx,
        const uint64_t *d_offsets, const uint8_t *d_valid, uint64_t rows, const uint64_t *d_n_rows,
        const uint8_t *d_bytes, uint64_t bytes_len,
        uint64_t n_prior, const uint64_t *d_n_prior,
        int32_t *d_codes,
        uint64_t *d_dict_offsets, uint32_t *d_dict_first, uint64_t dict_capacity,
        uint8_t *d_dict_bytes, uint64_t dict_bytes_capacity,
        uint32_t flags, msj_dictionary_extend_result *d_result, void *stream);
/* Device workspace of one msj_dictionary_extend_device call (the context keeps it): msj_dictionary_workspace_bytes' terms
 * per ITEM, rows + dict_capacity of them (at most 2^31). */
uint64_t msj_dictionary_extend_workspace_bytes(uint64_t rows, uint64_t dict_capacity);

/*
 * ---- rows by predicate (DERIVED) --------------------------------------------------------------------
 * msj_filter_rows_device chooses rows, msj_take_rows_device gathers them: "keep the lines where /status == "error" and
 * /latency_ms > 250" without a copy to the host, without a host wait for the count, without building the string column
 * first and without casting an int64 to a double.  Both write msj_field records WITH a msj_select_documents_result, which
 * is all that msj_string_column_device, msj_raw_column_device, msj_array_elements_device, msj_object_entries_device,
 * msj_select_elements_device and (behind a column call) msj_dictionary_device ask of their rows: the whole chain runs on
 * filtered rows unchanged.  A filtered window as minified NDJSON is filter -> take -> msj_raw_column_device(MSJ_RAW_COMPACT)
 * over the "" path; a take by msj_dictionary_device's d_dict_first is one row per distinct value.
 *
 * Predicates: msj_predicates_create compiles 1 to 16 msj_predicate, synchronously, into device memory the object owns -- the
 * twin of msj_paths_create: immutable, usable by any number of later calls on any stream of its context's device;
 * msj_predicates_destroy(NULL) does nothing.  A predicate names a column c (0..15), an op, flags and an operand, and looks at
 * ONE record f, that of its column in the row:
 *   MSJ_PRED_FOUND        f.code == 0
 *   MSJ_PRED_TYPE         f.code == 0 and f.type is in operand_bits, an 8-bit mask over the tape's tags in the order
 *                         { [ " l d t f n (MSJ_TYPE_*); a mask of 0 or with other bits set: MSJ_ERR_BAD_ARGUMENT
 *   MSJ_PRED_NUM_EQ / _LT / _LE / _GT / _GE
 *                         f.code == 0, f.type is 'l' or 'd', MSJ_FIELD_NO_BITS is not set, and value OP operand holds between
 *                         the two AS REAL NUMBERS, EXACTLY.  operand_bits is an int64, or with MSJ_PRED_DOUBLE the pattern of
 *                         a finite binary64 (not finite: MSJ_ERR_BAD_ARGUMENT).  Neither side is cast to the other's type:
 *                         an int64 i against a double d is decided by the sign when d >= 2^63 or d < -2^63 (-2^63 itself is
 *                         an int64), else by i against trunc(d) as int64 and on equality by 0 against d - trunc(d), which
 *                         is exact.  So 9007199254740993 > 9007199254740992.0 holds, and -0.0 == 0.  A record whose double
 *                         is a NaN (no number call writes one) fails all five.  A number without bits fails all five and
 *                         its row is counted in n_no_bits
 *   MSJ_PRED_STR_EQ / MSJ_PRED_STR_PREFIX
 *                         the operand is operand_len (0..255) bytes at operand_bytes, NUL allowed.  The string value of a
 *                         row is BY DEFINITION the bytes msj_string_column_device would write for the record, and the row's
 *                         validity is that call's too: code == 0, type == '"', the span inside the window; the value
 *                         unescaped as the tape does it when MSJ_SPAN_ESCAPED is set.  STR_EQ: the value equals the
 *                         operand.  STR_PREFIX: the value starts with it; an empty operand holds for every string row.  A
 *                         row that is no string fails both.  At most 6 * 255 raw bytes are read per row
 * MSJ_PRED_NOT inverts the predicate's truth value, INCLUDING for rows that have no value: a record with a code fails
 * NUM_GT, so it passes NOT NUM_GT.  This is two-valued logic, not SQL's three-valued logic; ask for MSJ_PRED_FOUND as well
 * where that matters.  MSJ_PREDICATES_ANY on the object: a row is kept when any predicate holds; default: when all hold.
 * Every predicate is evaluated on every row, whatever the others said: the counts do not depend on an order.
 * msj_predicates_create returns MSJ_ERR_BAD_ARGUMENT on NULL, a count outside 1..16, a column above 15, an operand over 255
 * bytes (or without its pointer), an unknown op, an unknown flag (MSJ_PRED_DOUBLE on an op that is not numeric is one).
 *
 * msj_filter_rows_device.  Column c is d_fields + c * stride -- the path-major layout the two select calls write; a single
 * column is n_columns = 1.  R = d_rows_select->n_documents is read on the device.  d_rows_select->code != 0: a zero result
 * with that code, d_kept_select likewise, nothing else written.  R > capacity or R >= 2^31: MSJ_CAPACITY with n_rows = R,
 * nothing else written.  A predicate naming a column at or past n_columns: MSJ_ERR_BAD_ARGUMENT on the host.
 *   d_keep          capacity bytes: d_keep[k] = 1 iff row k is kept, else 0, for k < R
 *   d_kept          capacity uint32: the kept row numbers ascending, n_kept of them -- the selection vector.  NULL: the
 *                   mask-only form
 *   d_kept_select   NULL, or a msj_select_documents_result: code = this call's, n_documents = n_found = n_kept, n_paths = 1,
 *                   n_no_bits = 0: a later call reads the count on the device
 *   d_list_offsets / d_list_offsets_out   both NULL, or the offsets of a list column WHOSE ELEMENTS ARE THESE ROWS and their
 *                   re-based form: P + 1 uint64 each, P = list_rows, or *d_list_n_rows read on the device when that is not
 *                   NULL.  d_list_offsets_out[r] = the number of kept rows k < min(d_list_offsets[r], R), for r <= P: a
 *                   gather in the exclusive rank, so defined on any input array; items[*] stays a list column behind
 *                   items[*].qty > 1.  P > list_rows or P >= 2^31: MSJ_CAPACITY, d_list_offsets_out not written, the rest
 *                   complete
 * d_result: code; flags, the object's; n_rows = R; n_kept; n_no_bits, the rows where at least one numeric predicate met a
 * number without bits; n_missing, the rows where at least one predicate met a record with a code.  R == 0 writes a zero
 * result (flags kept) and d_list_offsets_out all 0.  Every output is a pure function of the input.
 * Arguments, checked in this order: NULL ctx / predicates (or predicates of another device) / d_result / d_rows_select /
 * d_buf; NULL d_fields / d_keep with capacity > 0; one of d_list_offsets / d_list_offsets_out without the other; n_columns
 * outside 1..16, a predicate's column at or past n_columns, stride < capacity with n_columns > 1: MSJ_ERR_BAD_ARGUMENT.
 * len > MSJ_MAX_SEGMENT_BYTES: MSJ_CAPACITY.  Then d_result == a select result, d_kept_select == d_rows_select, and alignment
 * -- d_fields 16-byte; d_kept 4-byte; the offsets, d_list_n_rows, the results and select results 8-byte:
 * MSJ_ERR_BAD_ARGUMENT.  Nothing is launched on any of them.  Asynchronous on `stream`, no host round trip, workspace in the
 * context.  Safe on ANY records: the window is read only inside [0, len), nothing at or past R or capacity is touched.
 *
 * msj_take_rows_device gathers records by a selection vector: d_out[c * out_stride + j] = d_fields[c * stride + d_take[j]]
 * for j < K and c < n_columns, K = d_take_select->n_documents read on the device.  d_take: any uint32 row numbers -- d_kept,
 * d_dict_first -- in any order, with repeats; K is known on the device only, so the array holds min(K, out_capacity) entries
 * at least.  `stride` is also the room of a column: R = d_rows_select->n_documents > stride
 * is MSJ_CAPACITY.  An index at or past R writes the record of a missing value -- code 20, token 0xFFFFFFFF, everything else 0
 * -- and is counted in n_out_of_range.  K > out_capacity (or K >= 2^31): MSJ_CAPACITY with n_rows = K, nothing else written.
 * A code in d_take_select (it wins) or d_rows_select: a zero result with that code.  d_out_select: NULL, or a
 * msj_select_documents_result with code = this call's, n_documents = K, n_paths = n_columns, n_found and n_no_bits RECOUNTED
 * over what was written, so that any downstream call runs on d_out as on a select call's output.  Rows taken in ascending
 * order stay ascending, which msj_array_elements_device, msj_object_entries_device and msj_select_elements_device ask for;
 * their on-device order check catches any other vector.
 * Arguments, in this order: NULL ctx / d_result / d_take_select / d_rows_select; NULL d_take / d_out with out_capacity > 0,
 * NULL d_fields with stride > 0; n_columns outside 1..16, out_stride < out_capacity with n_columns > 1: MSJ_ERR_BAD_ARGUMENT;
 * a stride or capacity of 2^40 records or more: MSJ_CAPACITY; d_out overlapping
 * d_fields, d_result == a select result, d_out_select == d_take_select or d_rows_select; alignment (d_fields, d_out 16-byte,
 * d_take 4-byte, the results 8-byte): MSJ_ERR_BAD_ARGUMENT.  Asynchronous on `stream`, safe on ANY arrays.
 * Out of scope: contains / suffix / LIKE (msj_match_strings_device, below: its records under MSJ_PRED_FOUND), regex,
 * predicates on dictionary codes, nested boolean expressions (a second call over
 * the taken rows is AND).  (Order: msj_sort_rows_device, which takes d_kept as it is.)
 */
#define MSJ_PRED_FOUND 0u
#define MSJ_PRED_TYPE 1u
#define MSJ_PRED_NUM_EQ 2u
#define MSJ_PRED_NUM_LT 3u
#define MSJ_PRED_NUM_LE 4u
#define MSJ_PRED_NUM_GT 5u
#define MSJ_PRED_NUM_GE 6u
#define MSJ_PRED_STR_EQ 7u
#define MSJ_PRED_STR_PREFIX 8u
#define MSJ_PRED_NOT 1u        /* msj_predicate.flags: the truth value inverted, also for a row without a value */
#define MSJ_PRED_DOUBLE 2u     /* msj_predicate.flags, numeric ops: operand_bits is a binary64 pattern, not an int64 */
#define MSJ_PREDICATES_ANY 1u  /* msj_predicates_create flags: any predicate keeps a row; default: all must hold */
#define MSJ_TYPE_OBJECT 1u     /* MSJ_PRED_TYPE's mask: { [ " l d t f n */
#define MSJ_TYPE_ARRAY 2u
#define MSJ_TYPE_STRING 4u
#define MSJ_TYPE_INT64 8u
#define MSJ_TYPE_DOUBLE 16u
#define MSJ_TYPE_TRUE 32u
#define MSJ_TYPE_FALSE 64u
#define MSJ_TYPE_NULL 128u
typedef struct msj_predicates msj_predicates;
typedef struct msj_predicate {   /* 32 bytes */
    uint32_t column;         /* 0..15 */
    uint32_t op;             /* MSJ_PRED_* */
    uint32_t flags;          /* MSJ_PRED_NOT, MSJ_PRED_DOUBLE */
    uint32_t operand_len;    /* string ops: 0..255 */
    uint64_t operand_bits;   /* numeric ops: the int64, or the binary64 pattern; MSJ_PRED_TYPE: the mask */
    const uint8_t *operand_bytes;  /* string ops; read during the create call only */
} msj_predicate;
typedef struct msj_filter_rows_result {   /* 48 bytes */
    int32_t  code;       /* 0; MSJ_CAPACITY; or the code of d_rows_select */
    uint32_t flags;      /* the predicates object's flags */
    uint64_t n_rows;     /* R */
    uint64_t n_kept;
    uint64_t n_no_bits;  /* rows where a numeric predicate met a number with MSJ_FIELD_NO_BITS */
    uint64_t n_missing;  /* rows where at least one predicate met a record with a code */
    uint64_t reserved;
} msj_filter_rows_result;
typedef struct msj_take_rows_result {   /* 48 bytes */
    int32_t  code;            /* 0; MSJ_CAPACITY; or the code of d_take_select / d_rows_select */
    uint32_t flags;           /* 0 */
    uint64_t n_rows;          /* K */
    uint64_t n_out_of_range;  /* indices at or past R */
    uint64_t n_found;         /* records written with code 0, over all columns */
    uint64_t n_no_bits;       /* records written with MSJ_FIELD_NO_BITS */
    uint64_t reserved;
} msj_take_rows_result;
int32_t msj_predicates_create(msj_ctx *ctx, const msj_predicate *predicates, uint32_t n_predicates, uint32_t flags, msj_predicates **out);
void msj_predicates_destroy(msj_predicates *predicates);
int32_t msj_filter_rows_device(msj_ctx *ctx, const msj_predicates *predicates, const uint8_t *d_buf, uint64_t len,
        const msj_field *d_fields, uint64_t stride, uint32_t n_columns, const msj_select_documents_result *d_rows_select,
        uint8_t *d_keep, uint32_t *d_kept, uint64_t capacity,
        const uint64_t *d_list_offsets, uint64_t list_rows, const uint64_t *d_list_n_rows, uint64_t *d_list_offsets_out,
        msj_filter_rows_result *d_result, msj_select_documents_result *d_kept_select, void *stream);
int32_t msj_take_rows_device(msj_ctx *ctx, const uint32_t *d_take, const msj_select_documents_result *d_take_select,
        const msj_field *d_fields, uint64_t stride, uint32_t n_columns, const msj_select_documents_result *d_rows_select,
        msj_field *d_out, uint64_t out_stride, uint64_t out_capacity,
        msj_take_rows_result *d_result, msj_select_documents_result *d_out_select, void *stream);
/* Device workspace of one msj_filter_rows_device call (the context keeps it): 4 bytes per row (the rank), 8 per 256 rows
 * (block counts).  msj_take_rows_device needs the counters alone. */
uint64_t msj_filter_rows_workspace_bytes(uint64_t capacity);

/*
 * ---- timestamps and numbers written as strings (DERIVED) ----------------------------------------------
 * JSON has no type for a timestamp, and producers quote numbers to protect them from double-only readers: "ts":
 * "2024-05-01T12:34:56.789Z", "id":"9007199254740993", "price":"12.50".  msj_cast_strings_device reads such a column of
 * strings and writes msj_field records of type 'l' or 'd' WITH a msj_select_documents_result, which is all that
 * msj_filter_rows_device, msj_take_rows_device and a number column ask of a column: "/ts >= T0 and /ts < T1" is two
 * MSJ_PRED_NUM_* predicates on an exact int64, on the device, without building the string column first.
 *
 * R = d_rows_select->n_documents is read on the device.  The output record of row k < R:
 *   the input has a code       the input record, unchanged
 *   a string row               a string by msj_string_column_device's test: code == 0, type == '"', the span inside the window
 *                              (a record whose span leaves the window is no string and is never dereferenced).  The row's
 *                              VALUE is by definition the bytes the string column would write, escapes resolved as the tape
 *                              does: "\u0032024-05-01" is 2024-05-01.  The value is of the kind's grammar and in range: bits =
 *                              the value, token = the input's token (ascending rows stay ascending, and the raw text is still
 *                              found), type 'l' or 'd', flags 0, code 0.  Otherwise: code 9 (NUMBER_ERROR of the reference's
 *                              error table), token 0xFFFFFFFF, everything else 0, and the row is counted in n_syntax (the
 *                              value is not of the grammar) or n_range (it is, and has no int64 / binary64)
 *   no string, code 0          with MSJ_CAST_KEEP_NUMBERS an 'l' / 'd' record is copied as it is, MSJ_FIELD_NO_BITS included,
 *                              and counted in n_cast; every other record becomes code 17 (INCORRECT_TYPE), token 0xFFFFFFFF,
 *                              everything else 0, and is counted in n_other
 * MSJ_CAST_NUMBER: the value, WHOLE, is one JSON number -- no blank in front of it or behind it, no '+' -- and the record is
 * exactly what msj_number_values_device gives for the same text as a token: MSJ_NUMBER_INT64 'l', MSJ_NUMBER_DOUBLE 'd',
 * MSJ_NUMBER_ERR_SYNTAX n_syntax, MSJ_NUMBER_ERR_RANGE n_range.  "9007199254740993" stays an exact int64; "-0" is the int64
 * 0; "1e400" is n_range.  LIMIT: a value of more than 128 bytes is n_syntax without being read (an escaped body of more than
 * 6 * 128 raw bytes likewise) -- where MSJ_SPAN_LONG starts at 1 024 characters for a number token, a quoted number ends at
 * 128.  `unit` must be 0.
 * MSJ_CAST_TIMESTAMP: RFC 3339 with the relaxations real producers need:
 *   date      = YYYY "-" MM "-" DD                      year 0000..9999, proleptic Gregorian, the day valid for month and leap year
 *   time      = hh ":" mm [ ":" ss [ ("." | ",") 1*9DIGIT ] ]     hh 00..23, mm 00..59, ss 00..59 (a leap second 60 is n_syntax)
 *   offset    = "Z" | "z" | ("+" | "-") hh [ [":"] mm ]           hh 00..23, mm 00..59; none: UTC
 *   timestamp = date [ ("T" | "t" | " ") time [offset] ]          a date alone is its midnight UTC
 * The longest member has 35 bytes: a longer value is n_syntax without being read, an escaped body of more than 6 * 35 raw
 * bytes likewise.  The value is (days_from_civil(date) * 86400 + hh * 3600 + mm * 60 + ss - offset_seconds) * U + the fraction
 * CUT to the unit's digits (a floor: the fraction is not negative), U = 1, 10^3, 10^6, 10^9 for MSJ_CAST_UNIT_S / _MS / _US /
 * _NS, as an int64 ('l').  0000-01-01T00:00:00Z is -62167219200 s, 9999-12-31T23:59:59Z is 253402300799 s; an offset may
 * push the instant outside that span, which is a value like any other.  A result outside int64 is n_range, which only
 * MSJ_CAST_UNIT_NS can meet: 2262-04-11T23:47:16.854775807Z is 2^63 - 1, 1677-09-21T00:12:43.145224192Z is -2^63, one step
 * further is n_range -- decided without a multiply that wraps.
 *
 * d_result: code; flags = kind | unit << 8 | flags << 16; n_rows = R; n_cast the records written with code 0, kept numbers
 * included; n_syntax; n_range; n_other.  d_rows_select->code != 0: a zero result with that code (flags kept), d_out_select
 * likewise, nothing else written.  R > capacity or R >= 2^31: MSJ_CAPACITY with n_rows = R, nothing else written.  R == 0
 * writes zero results, flags kept.  d_out_select: NULL, or a msj_select_documents_result with code = this call's,
 * n_documents = R, n_paths = 1, n_found = n_cast and n_no_bits RECOUNTED over what was written, so that any downstream call
 * runs on d_out as on a select call's output.  d_out == d_rows exactly is allowed, a cast in place: a row is read by the lane
 * that writes it, before it writes.  Every output is a pure function of the input.
 * Arguments, checked in this order: NULL ctx / d_result / d_rows_select / d_buf; NULL d_rows / d_out with capacity > 0; an
 * unknown kind, unit or flag, a unit other than 0 with MSJ_CAST_NUMBER: MSJ_ERR_BAD_ARGUMENT.  len > MSJ_MAX_SEGMENT_BYTES or
 * a capacity of 2^40 records or more: MSJ_CAPACITY.  Then d_out overlapping d_rows in any way but d_out == d_rows, d_result ==
 * a select result, d_out_select == d_rows_select, and alignment -- d_rows, d_out 16-byte; the result and select results
 * 8-byte: MSJ_ERR_BAD_ARGUMENT.  Nothing is launched on any of them.  Asynchronous on `stream`, no host round trip, workspace
 * in the context.  Safe on ANY records: the window is read only inside [0, len), nothing at or past R or capacity is touched.
 * Out of scope: format strings (%d/%m/%Y), time-zone names, week and ordinal dates, the basic format without dashes, leap
 * seconds; durations; booleans in strings; casting to a dictionary code; numbers of more than 128 bytes.
 */
#define MSJ_CAST_TIMESTAMP 1u
#define MSJ_CAST_NUMBER    2u
#define MSJ_CAST_UNIT_S  0u   /* timestamps: the int64 counts seconds / milli / micro / nanoseconds since 1970-01-01T00:00:00Z */
#define MSJ_CAST_UNIT_MS 1u
#define MSJ_CAST_UNIT_US 2u
#define MSJ_CAST_UNIT_NS 3u
#define MSJ_CAST_KEEP_NUMBERS 1u   /* flags: a row that already is a number ('l' / 'd') is copied as it is instead of code 17 */
typedef struct msj_cast_strings_result {   /* 48 bytes */
    int32_t  code;      /* 0; MSJ_CAPACITY (R > capacity or R >= 2^31: n_rows = R, nothing else written); or d_rows_select->code */
    uint32_t flags;     /* kind | unit << 8 | flags << 16 */
    uint64_t n_rows;    /* R */
    uint64_t n_cast;    /* records written with code 0 (kept numbers included) */
    uint64_t n_syntax;  /* string rows whose value is not of the kind's grammar */
    uint64_t n_range;   /* string rows of the grammar whose value has no int64 / binary64 */
    uint64_t n_other;   /* rows with code 0 that are neither a string nor a kept number */
} msj_cast_strings_result;
int32_t msj_cast_strings_device(msj_ctx *ctx, const uint8_t *d_buf, uint64_t len,
        const msj_field *d_rows, const msj_select_documents_result *d_rows_select,
        uint32_t kind, uint32_t unit, uint32_t flags,
        msj_field *d_out, uint64_t capacity,
        msj_cast_strings_result *d_result, msj_select_documents_result *d_out_select, void *stream);
/* Device workspace of one msj_cast_strings_device call (the context keeps it): the counters and 4 bytes per row (the list of
 * the rows whose body is escaped or whose number needs the exact path). */
uint64_t msj_cast_strings_workspace_bytes(uint64_t capacity);
/* Measurement only (scripts/cast_strings_rate.py): how the kernel fetches a body's bytes.  Both forms write the same records. */
#define MSJ_CAST_FETCH_WINDOW 0u   /* the aligned 16-byte words that cover the body, through LDS (the default) */
#define MSJ_CAST_FETCH_BYTES  1u   /* byte loads from the window */
int32_t msj_debug_set_cast_fetch(msj_ctx *ctx, uint32_t fetch);

/*
 * ---- count, sum, min, max per group (DERIVED) ---------------------------------------------------------
 * msj_aggregate_device answers "how many lines, what total, smallest and largest /latency_ms per /status" on the device:
 * one 48-byte msj_aggregate per (column, group) over msj_field records of type 'l' / 'd' -- a path of a select call, cast
 * strings, taken rows, list elements -- grouped by any int32 codes, msj_dictionary_device's d_codes first of all.  EXACT and
 * REPRODUCIBLE: an int64 is never cast to a double, and every output is a pure function of the input, bit for bit from run
 * to run and under any permutation of the rows (codes permuted with them): the kernels use integer atomics alone.
 *
 * Column c is d_fields + c * stride, as msj_filter_rows_device takes them; `stride` is also the room of a column.
 * R = d_rows_select->n_documents and G = d_n_groups ? *d_n_groups : n_groups are read on the device (d_n_groups =
 * &dictionary_result->n_distinct groups by a dictionary without a host wait).  d_groups[c * groups_capacity + g] is the
 * record of column c and group g < G; nothing at or past G is written.
 *   Grouping      row k < R belongs to group d_codes[k] when that lies in [0, G); otherwise it is counted in n_ungrouped and
 *                 in no group.  d_codes == NULL: every row is group 0.  d_codes holds `stride` entries
 *   Number value  a record is a number value iff its code == 0, its type is 'l' or 'd', MSJ_FIELD_NO_BITS is not set and,
 *                 for 'd', its bits are finite.  Any other record of a grouped row adds to its group's n_rows only; one
 *                 with code == 0 and type 'l' / 'd' but no usable bits (MSJ_FIELD_NO_BITS; a NaN or an infinity, which no
 *                 number call writes) is counted in n_skipped
 *   min / max     the values compared AS REAL NUMBERS, an int64 against a double exactly (the compare of
 *                 MSJ_PRED_NUM_*): 9007199254740993 lies above 9007199254740992.0.  Between equal reals the 'l' record wins,
 *                 for the minimum and for the maximum; among doubles -0.0 lies below +0.0.  min_type / max_type say what
 *                 min_bits / max_bits hold
 *   sum, 'l'      every value of the group is an 'l' and the exact integer sum fits an int64: sum_bits is that sum.  The
 *                 running sum is never clipped: INT64_MAX, 1, -1 sum to the exact 'l' INT64_MAX
 *   sum, 'd'      otherwise.  Let E be the largest floor(log2|v|) over the group's non-zero values.  Every value becomes
 *                 the integer t = trunc(v * 2^(95 - E)), exact for every value whose lowest set bit lies at or above
 *                 2^(E - 95): every int64 while E <= 95, every double within 2^42 of the largest.  S = the sum of the t,
 *                 exact (R < 2^31: |S| < 2^127).  sum_bits is S * 2^(E - 95) rounded ONCE to the nearest binary64, ties to
 *                 even, subnormals included; beyond DBL_MAX it is +-infinity with MSJ_AGG_INFINITE.  A group of 'l' alone
 *                 that left the int path sets MSJ_AGG_INT_OVERFLOW (its sum is the exact integer sum, rounded once).  No
 *                 non-zero value, or S == 0: +0.0.  The error is below R * 2^(E - 95), that of a double sum up to
 *                 R * 2^(E - 52), and it is the same for every order of the rows: 2^53, 1.0, 1.0 gives 2^53 + 2.  What
 *                 lies more than 95 binary places below the group's largest value is cut: 1e308, -1e308, 1.0 gives +0.0
 *                 (the double sum in that order 1.0, in another 0.0)
 * A group without a value: n_rows, and every other member 0.  sum_type == 0 says so.
 * d_result: code; flags, the OR of every record's; n_rows = R; n_groups = G; n_ungrouped; n_values and n_skipped over all
 * columns (grouped rows only: n_values is the sum of the records').  d_rows_select->code != 0: a zero result with that code,
 * nothing else written.  R > stride or R >= 2^31, or G > groups_capacity: MSJ_CAPACITY with n_rows = R and n_groups = G,
 * nothing else written.  R == 0 or G == 0: the same definition -- zeroed records for g < G, n_ungrouped = R.
 * Merging two windows' records: n_rows and n_values add, min and max merge by the rule above, an 'l' sum adds to an 'l' sum
 * while it fits; two 'd' sums do NOT merge exactly (each was rounded): aggregate the windows' rows in one call for that.
 * Arguments, checked in this order: NULL ctx / d_result / d_rows_select; NULL d_fields with stride > 0, NULL d_groups with
 * groups_capacity > 0; n_columns outside 1..16: MSJ_ERR_BAD_ARGUMENT.  A stride or groups_capacity of 2^40 or more:
 * MSJ_CAPACITY.  Then d_result == d_rows_select, and alignment -- d_fields, d_groups 16-byte;
 * d_codes 4-byte; d_n_groups, the result and the select result 8-byte: MSJ_ERR_BAD_ARGUMENT.  Nothing is launched on any of
 * them.  Asynchronous on `stream`, no host round trip, workspace in the context (96 bytes per (column, group) of
 * groups_capacity).  Safe on ANY arrays: a record is read only at k < R <= stride, a code only there, nothing at or past G
 * or groups_capacity is written.
 * Two paths, chosen on the device from G: up to the context's limit (256 groups) a block sums its rows in LDS and adds what
 * it touched to the group's words once; above it every lane adds to the group's words directly.  Both give the same bytes.
 * msj_debug_set_aggregate_limits moves the limit (0: never LDS; at most 256) so that tests run both on small inputs.
 * Out of scope: mean and variance (the caller divides); making the codes -- a numeric key, a time bucket and more than one
 * key are msj_bucket_rows_device and msj_group_keys_device in front of a dictionary call (below), the groups in key order
 * msj_dictionary_order_device over that dictionary --; argmin / argmax rows; sums across windows (above).
 */
#define MSJ_AGG_INT_OVERFLOW 1u   /* msj_aggregate.flags: every value an 'l', the exact sum outside int64: sum_type 'd' */
#define MSJ_AGG_INFINITE 2u       /* the sum lies beyond DBL_MAX: sum_bits is +-infinity */
typedef struct msj_aggregate {      /* 48 bytes, 16-byte aligned, one per (column, group) */
    uint64_t n_rows;    /* rows of the group */
    uint64_t n_values;  /* of them, rows whose record is a number value */
    uint64_t sum_bits;  /* 'l': the int64; 'd': the binary64 pattern */
    uint64_t min_bits, max_bits;
    uint8_t  sum_type, min_type, max_type;   /* 'l' / 'd'; 0 when n_values == 0 */
    uint8_t  flags;     /* MSJ_AGG_INT_OVERFLOW, MSJ_AGG_INFINITE */
    uint32_t reserved;
} msj_aggregate;
typedef struct msj_aggregate_result {   /* 48 bytes */
    int32_t  code;         /* 0; MSJ_CAPACITY; or the code of d_rows_select */
    uint32_t flags;        /* the OR of every written record's flags */
    uint64_t n_rows;       /* R */
    uint64_t n_groups;     /* G */
    uint64_t n_ungrouped;  /* rows whose code lies outside [0, G) */
    uint64_t n_values;     /* number values, over all columns */
    uint64_t n_skipped;    /* 'l' / 'd' records without usable bits, over all columns */
} msj_aggregate_result;
int32_t msj_aggregate_device(msj_ctx *ctx,
        const msj_field *d_fields, uint64_t stride, uint32_t n_columns,
        const msj_select_documents_result *d_rows_select,
        const int32_t *d_codes,
        uint64_t n_groups, const uint64_t *d_n_groups,
        msj_aggregate *d_groups, uint64_t groups_capacity,
        msj_aggregate_result *d_result, void *stream);
/* Device workspace of one msj_aggregate_device call (the context keeps it): the counters and 96 bytes per (column, group). */
uint64_t msj_aggregate_workspace_bytes(uint64_t capacity, uint64_t groups_capacity, uint32_t n_columns);
/* TEST AID: the most groups the LDS path takes (0: none; more than 256: MSJ_ERR_BAD_ARGUMENT).  Both paths write the same bytes. */
int32_t msj_debug_set_aggregate_limits(msj_ctx *ctx, uint32_t lds_groups);

/*
 * msj_sort_rows_device answers "the ten slowest lines" and "these lines in time order" on the device: the row numbers of
 * ONE column of msj_field records in the exact numeric order of their values, stable, optionally only the first `limit`.
 * What it writes is a selection vector -- msj_take_rows_device gathers any columns by it -- so no column, no count and no
 * key reaches the host.  A cast to double would order 9007199254740993 and 9007199254740992.0 as equal and an int64 above
 * 2^53 wrongly; this call compares as real numbers.
 * d_fields: the column (column c of a set of records: d_fields + c * stride); stride: its room; R = d_rows_select->
 * n_documents, read on the device.  d_rows_in == NULL: the input sequence is the rows 0 .. R-1, N = R.  Otherwise (both
 * d_rows_in pointers given) it is d_rows_in[0 .. N), N = d_rows_in_select->n_documents read on the device, repeats and any
 * order allowed -- a filter's d_kept, an earlier call's d_order; an entry at or past R is a row without a value, counted in
 * n_out_of_range.  A sort by two keys is two calls, the minor key first: the second takes the first's d_order as d_rows_in.
 * Number value: msj_aggregate_device's rule -- code == 0, type 'l' or 'd', MSJ_FIELD_NO_BITS not set, a 'd' finite.  Every
 * other record is a row without a value; one with code == 0 and type 'l' / 'd' but no usable bits is counted in n_skipped.
 * Order: the rows with a value first, ascending by value AS REAL NUMBERS, an int64 against a double exactly (the compare of
 * MSJ_PRED_NUM_*): 9007199254740993 lies between 9007199254740992.0 and 9007199254740994.0; -0.0, +0.0 and the int64 0 are
 * equal, 3 and 3.0 are equal.  Equal values keep the order of the input sequence (stable).  MSJ_SORT_DESCENDING reverses
 * the order of the values only: equal values still keep input order and the rows without a value still come last, in input
 * order; with MSJ_SORT_VALUES_ONLY they are left out.  The answer is unique, and every output is the same bytes from run
 * to run.
 * Outputs: M = n_values with MSJ_SORT_VALUES_ONLY, else N; K = M for limit == 0, else min(limit, M).  d_order[0 .. K): the
 * first K row numbers of the order (entries of the input sequence, not positions in it); nothing at or past K is written.
 * d_order_select: NULL, or it receives code = this call's, n_documents = n_found = K, n_paths = 1, n_no_bits = 0 -- what
 * msj_take_rows_device reads as d_take_select.  capacity: the most input rows the call orders; d_order has room for
 * capacity entries, or for min(capacity, limit) with limit > 0.
 * d_result: a code in d_rows_in_select (it wins) or d_rows_select: a zero result with that code, d_order_select the same,
 * nothing else written.  R > stride, N > capacity or N >= 2^31: MSJ_CAPACITY with n_rows = N (and the flags), nothing else
 * written.  N == 0: a zero result with the flags.
 * Arguments, checked in this order: NULL ctx / d_result / d_rows_select; one of d_rows_in / d_rows_in_select without the
 * other; NULL d_fields with stride > 0, NULL d_order with capacity > 0; an unknown flag: MSJ_ERR_BAD_ARGUMENT.  A stride or
 * capacity of 2^40 or more: MSJ_CAPACITY.  Then d_result == a select result; d_order_select == one of the two input select
 * results; d_order overlapping d_rows_in; alignment -- d_fields 16-byte, d_order / d_rows_in 4-byte, the results 8-byte:
 * MSJ_ERR_BAD_ARGUMENT.  Nothing is launched on any of them.  Asynchronous on `stream`, no host round trip, workspace in
 * the context (about 33 bytes per row of capacity).  Safe on ANY arrays: a record is read only at a row below R <= stride,
 * d_rows_in only below N <= capacity, d_order is written only below K.
 * Two paths, chosen on the device, the same bytes from both.  The full sort: a least-significant-digit radix sort over a
 * 75-bit order-preserving key and the null bit (eleven digits; a pass whose digit is the same in every row is skipped, so a
 * plain int or double column takes at most eight).  The selection, where limit > 0, N >= 16 384 and limit <= N / 8: most-
 * significant-digit histograms find the key of the K-th row, the rows below it and the first rows that equal it are
 * compacted in input order and only they are sorted.  msj_debug_set_sort_mode forces either so that tests compare them on
 * small inputs.
 * Out of scope: string keys here (msj_dictionary_order_device and msj_rank_rows_device give a string column ranks this call
 * orders; or cast); nulls first; sorting msj_aggregate records; top-k per
 * group; merging sorted windows.
 */
#define MSJ_SORT_DESCENDING  1u
#define MSJ_SORT_VALUES_ONLY 2u   /* rows without a number value are left out instead of placed last */
typedef struct msj_sort_rows_result {   /* 48 bytes */
    int32_t  code;            /* 0; MSJ_CAPACITY; or the code of d_rows_in_select (it wins) / d_rows_select */
    uint32_t flags;           /* the call's flags */
    uint64_t n_rows;          /* N, the rows that were ordered */
    uint64_t n_values;        /* of them, rows whose record is a number value */
    uint64_t n_written;       /* K, the entries of d_order */
    uint64_t n_skipped;       /* 'l' / 'd' records without usable bits (MSJ_FIELD_NO_BITS, NaN, infinity) */
    uint64_t n_out_of_range;  /* entries of d_rows_in at or past R */
} msj_sort_rows_result;
int32_t msj_sort_rows_device(msj_ctx *ctx,
        const msj_field *d_fields, uint64_t stride, const msj_select_documents_result *d_rows_select,
        const uint32_t *d_rows_in, const msj_select_documents_result *d_rows_in_select,
        uint32_t flags, uint64_t limit,
        uint32_t *d_order, uint64_t capacity,
        msj_sort_rows_result *d_result, msj_select_documents_result *d_order_select, void *stream);
/* Device workspace of one msj_sort_rows_device call (the context keeps it). */
uint64_t msj_sort_rows_workspace_bytes(uint64_t capacity);
/* TEST AID: 0 the path chosen on the device, 1 always the full sort, 2 always the selection, carried to the key's last digit
 * (more than 2: MSJ_ERR_BAD_ARGUMENT).  Both paths write the same bytes. */
int32_t msj_debug_set_sort_mode(msj_ctx *ctx, uint32_t mode);

/*
 * msj_join_rows_device answers "which row of the users file does this event's /user_id match" on the device: the equi-join
 * of two int32 code columns, as row pairs.  The codes are those of ONE dictionary (msj_dictionary_extend_device over both
 * sides: the right column encoded, the left one encoded or looked up with MSJ_DICTIONARY_FROZEN), so equal values have equal
 * codes in both.  What it writes is a pair of selection vectors, the kind msj_sort_rows_device writes: msj_take_rows_device
 * gathers any columns of either side by them, and no key, no count and no row number reaches the host.
 * Row counts: L = d_n_left ? *d_n_left : left_rows, R and G (the dictionary's entries) the same way, all three read on the
 * device -- &dictionary_result->n_rows, &extend_result->n_distinct -- so a join follows two dictionary calls without a host
 * wait.  left_rows / right_rows are also the rooms of the key arrays.
 * Keys: an int32 is a key iff it lies in [0, G).  Anything else equals nothing, itself included: -1 (null), -2 (a frozen
 * miss), a code from a later window.  match(l): the right rows r < R with d_right_keys[r] == d_left_keys[l], ascending;
 * empty for a left row without a key.  c(l) = |match(l)|; row l emits n(l) pairs:
 *   MSJ_JOIN_INNER  n = c            (l, r) for r in match(l)
 *   MSJ_JOIN_LEFT   n = max(c, 1)    as INNER; (l, MSJ_JOIN_NO_ROW) when c == 0
 *   MSJ_JOIN_SEMI   n = c > 0        (l, match(l)[0])
 *   MSJ_JOIN_ANTI   n = c == 0       (l, MSJ_JOIN_NO_ROW)
 * Outputs: M = the sum of n(l).  d_left_rows[0 .. M) / d_right_rows[0 .. M): the pairs in ascending l and, inside a row, in
 * ascending r.  The answer is unique and every output byte is a pure function of the input, the same from run to run.
 * d_right_rows may be NULL (SEMI / ANTI callers) and is then not written.  d_offsets: NULL, or room for left_rows + 1
 * words: d_offsets[l] = the sum of n(l') for l' < l, d_offsets[L] = M -- with it the result is also a list column over the
 * left rows, a group join.  d_left_select / d_right_select: each NULL, or it receives what msj_sort_rows_device writes to
 * d_order_select: code = this call's, n_documents = n_found = M, n_paths = 1, n_no_bits = 0 -- msj_take_rows_device takes
 * either vector as d_take with no host wait.  MSJ_JOIN_NO_ROW is at or past any R, so the missing side of a LEFT or ANTI
 * pair comes out of msj_take_rows_device as the record of a missing value (code 20).  Nothing at or past M is written.
 * d_result: L > left_rows, R > right_rows, G > keys_capacity, or L or R >= 2^31: MSJ_CAPACITY with the flags and the three
 * counts, both select results the same code with M = 0, nothing else written.  M > pairs_capacity: MSJ_CAPACITY with every
 * counter exact and d_offsets complete; nothing is written to the pair arrays and both select results carry the code, so a
 * take behind it gives a zero result; the caller repeats the call with n_pairs entries of room.  L == 0, R == 0 or G == 0:
 * the same definition (M == 0, or L pairs for LEFT / ANTI).
 * Arguments, checked in this order: NULL ctx / d_result; a NULL key array with rows > 0; NULL d_left_rows with
 * pairs_capacity > 0; an unknown flag; d_offsets overlapping a key array or a count word: MSJ_ERR_BAD_ARGUMENT.  A room or
 * capacity of 2^40 or more: MSJ_CAPACITY.  Then alignment -- the keys and the rows 4-byte; the offsets, the counts and the
 * results 8-byte -- and a select result that is d_result: MSJ_ERR_BAD_ARGUMENT.  Nothing is
 * launched on any of them.  Asynchronous on `stream`, no host round trip, workspace in the context (about 4 bytes per key of
 * keys_capacity, 17 per row of right_rows, 12 per row of left_rows).  Safe on ANY arrays: a key is read only below L / R,
 * nothing at or past M, pairs_capacity or d_offsets[L] is written, and keys_capacity bounds every table.
 * How: the right rows are ordered by key with a stable least-significant-digit radix sort over the eight-bit digits that
 * tell the keys of [0, G) apart (G <= 256: one pass; the first pass also leaves out the rows without a key, so there is
 * always one); a scan of count[key] gives every key's run; the pairs are then written by OUTPUT position, each lane finding
 * its left row by binary search in the offsets, so a key held by millions of rows is spread over the grid like any other.
 * Out of scope: keys that are not dense codes; numeric equality (3 against 3.0: cast first); more than one key column
 * (combine the codes first); right and full outer joins (swap the sides); a shortcut for unique right keys; joins across
 * more than 2^31 - 1 rows a side; a hash table kept between calls.
 */
#define MSJ_JOIN_INNER 0u   /* flags & 3: the kind */
#define MSJ_JOIN_LEFT  1u
#define MSJ_JOIN_SEMI  2u
#define MSJ_JOIN_ANTI  3u
#define MSJ_JOIN_NO_ROW 0xFFFFFFFFu
typedef struct msj_join_rows_result {   /* 64 bytes */
    int32_t  code;            /* 0; MSJ_CAPACITY */
    uint32_t flags;           /* the call's flags */
    uint64_t n_left, n_right, n_keys;   /* L, R, G as read on the device */
    uint64_t n_pairs;         /* M, exact also when the pair arrays were too small */
    uint64_t n_left_matched;  /* left rows with at least one partner */
    uint64_t n_left_null;     /* left rows whose key lies outside [0, G) */
    uint64_t n_right_null;    /* right rows whose key lies outside [0, G) */
} msj_join_rows_result;
int32_t msj_join_rows_device(msj_ctx *ctx,
        const int32_t *d_left_keys,  uint64_t left_rows,  const uint64_t *d_n_left,
        const int32_t *d_right_keys, uint64_t right_rows, const uint64_t *d_n_right,
        uint64_t n_keys, const uint64_t *d_n_keys, uint64_t keys_capacity,
        uint32_t flags,
        uint32_t *d_left_rows, uint32_t *d_right_rows, uint64_t pairs_capacity,
        uint64_t *d_offsets,
        msj_join_rows_result *d_result,
        msj_select_documents_result *d_left_select, msj_select_documents_result *d_right_select,
        void *stream);
/* Device workspace of one msj_join_rows_device call (the context keeps it). */
uint64_t msj_join_rows_workspace_bytes(uint64_t left_rows, uint64_t right_rows, uint64_t keys_capacity);

/*
 * msj_dictionary_order_device answers "these rows by /name" and "the first ten hosts alphabetically" on the device: it
 * orders the V distinct values of a dictionary once, so that every row's value has a rank, a number that
 * msj_sort_rows_device, msj_filter_rows_device and msj_aggregate_device take (msj_rank_rows_device below).
 * Entries: V = d_n_entries ? *d_n_entries : n_entries, read on the device -- &dictionary_result->n_distinct chains without
 * a host wait.  Entry c < V has a value iff d_dict_offsets[c] <= d_dict_offsets[c + 1] <= dict_bytes_capacity (the
 * prior-entry test of msj_dictionary_extend_device: checked, never believed); the value is those bytes, and the empty
 * string is a value.  Arrays with equal values -- any offsets array a caller made -- are legal input.
 * Order: values compare as unsigned bytes, lexicographically, a proper prefix first: memcmp, then length; for UTF-8 that is
 * code-point order.  No collation, no case folding.
 * d_sorted[V]: the entry numbers -- the entries with a value first, ascending by value, equal values by ascending entry
 * number; then the entries without a value in entry order.  The answer is unique.  d_rank[V]: d_rank[c] = the number of
 * entries whose value is smaller than entry c's; equal values share a rank, so for a real dictionary the ranks are a
 * permutation of 0 .. V-1 and d_sorted[d_rank[c]] == c; an entry without a value gets MSJ_ORDER_NO_RANK.
 * The partial order by depth B is the same definition with every value v replaced by its first B bytes, v[:B].  After a
 * call has compared B bytes the two arrays hold exactly that.  An entry is TIED iff it shares its rank with another entry
 * and its length is at least B: such entries agree on B bytes and may still differ behind them.  The order is complete iff
 * no entry is tied.
 * Rounds: a round compares the next eight bytes of the tied entries and runs only while an entry is tied.  A call runs at
 * most max_rounds of them (1 .. 64; 0: the path's default, 64 rounds on the one-workgroup path and 4 on the grid path).
 * Every launch is enqueued up front, sized by `capacity` (the room of d_sorted, d_rank and, plus one, d_dict_offsets); a
 * kernel that finds nothing tied returns at once.
 * d_result: code 0: complete, n_tied == 0.  The budget ended with entries still tied: MSJ_CAPACITY with n_tied > 0, and the
 * arrays hold the order by the first `depth` bytes.  The caller repeats the call with MSJ_ORDER_CONTINUE: the two arrays are
 * the state and `depth` the previous result's depth (8 x the rounds requested so far, so the host knows it without
 * reading).  The chain gives the bytes one call with a large budget gives.  Without MSJ_ORDER_CONTINUE the arrays are
 * written, not read, and depth must be 0.  result.depth: the argument plus 8 x the rounds that ran.  n_equal: the entries
 * whose value an earlier entry also holds, as far as the depth shows (0 for a real dictionary).  V > capacity or V >= 2^31:
 * MSJ_CAPACITY with n_entries = V, depth = 0, n_tied = 0, nothing else written.  V == 0: a zero result with the flags.
 * Arguments, checked in this order: NULL ctx / d_result; NULL d_dict_offsets, d_sorted or d_rank with capacity > 0, NULL
 * d_dict_bytes with dict_bytes_capacity > 0; an unknown flag, max_rounds > 64, a depth that is no multiple of 8, a depth
 * without MSJ_ORDER_CONTINUE: MSJ_ERR_BAD_ARGUMENT.  A capacity of 2^40 or more: MSJ_CAPACITY.  Then alignment -- the
 * offsets, d_n_entries and the result 8-byte, the two arrays 4-byte, the bytes any: MSJ_ERR_BAD_ARGUMENT.  Nothing is
 * launched on any of them.  Asynchronous on `stream`, no host round trip, workspace in the context (about 49 bytes per
 * entry of capacity; the one-workgroup path does not use it).
 * Safe on ANY arrays: no byte outside [0, dict_bytes_capacity) is read, whatever the alignment of d_dict_bytes and of a
 * value's end; an offset is read only at or below V.  With MSJ_ORDER_CONTINUE an entry of d_sorted at or past V is an entry
 * without a value; garbage state gives unspecified but in-bounds output within the budget.  Nothing at or past V is
 * written.  Every output is a pure function of the input, the same bytes from run to run.
 * Two paths, the same bytes from both.  capacity <= 1 024: one workgroup keeps the arrays and the keys in LDS and loops
 * over the rounds inside ONE kernel until nothing is tied or the budget ends.  Above: per round the tied entries are
 * compacted, their words fetched, and ordered by a stable least-significant-digit radix sort over the key (rank, word,
 * nvalid) in eight-bit digits -- a pass whose digit is the same in every tied entry is skipped, so a prefix shared inside a
 * word costs nothing, and of the rank only the digits that tell [0, capacity) apart exist --, written back, and the new
 * groups found by comparing neighbours and a scan.  msj_debug_set_order_mode forces either path.
 * Out of scope: collation and case folding; string range predicates (the rank of an operand); string min / max in one
 * call; skipping a group's common prefix beyond what constant digits give; rewriting a dictionary into sorted order; more
 * than 2^31 - 1 entries; sharing the radix passes with msj_sort_rows_device.
 */
#define MSJ_ORDER_CONTINUE 1u
#define MSJ_ORDER_NO_RANK 0xFFFFFFFFu
typedef struct msj_dictionary_order_result {   /* 48 bytes */
    int32_t  code;       /* 0; MSJ_CAPACITY: entries still tied (n_tied > 0), or V does not fit */
    uint32_t flags;      /* the call's flags */
    uint64_t n_entries;  /* V */
    uint64_t n_values;   /* entries with a value */
    uint64_t n_tied;     /* entries still tied at `depth` */
    uint64_t depth;      /* bytes compared when the call ended */
    uint64_t n_equal;    /* entries whose value an earlier entry also holds */
} msj_dictionary_order_result;
int32_t msj_dictionary_order_device(msj_ctx *ctx,
        const uint64_t *d_dict_offsets, const uint8_t *d_dict_bytes, uint64_t dict_bytes_capacity,
        uint64_t n_entries, const uint64_t *d_n_entries, uint64_t capacity,
        uint64_t depth, uint32_t max_rounds, uint32_t flags,
        uint32_t *d_sorted, uint32_t *d_rank,
        msj_dictionary_order_result *d_result, void *stream);
/* Device workspace of one msj_dictionary_order_device call (the context keeps it). */
uint64_t msj_dictionary_order_workspace_bytes(uint64_t capacity);
/* TEST AID: 0 the path by capacity, 1 always the grid path, 2 the one-workgroup path wherever capacity <= 1 024 (more than
 * 2: MSJ_ERR_BAD_ARGUMENT).  Both paths write the same bytes. */
int32_t msj_debug_set_order_mode(msj_ctx *ctx, uint32_t mode);

/*
 * msj_rank_rows_device turns a column of dictionary codes into records that order like the strings: row k with c =
 * d_codes[k] in [0, V) and d_rank[c] != MSJ_ORDER_NO_RANK gets {bits = d_rank[c], token = 0xFFFFFFFF, type 'l', flags 0,
 * code 0}; every other row -- a null (-1), a frozen miss (-2), a wild code -- gets the record of a missing value that
 * msj_take_rows_device writes (code 20, token 0xFFFFFFFF, the rest 0).  R = d_n_rows ? *d_n_rows : rows and V =
 * d_order_result->n_entries are read on the device.  d_select is written as a select result over the records
 * (n_documents = R, n_paths = 1, n_found = n_ranked), so msj_sort_rows_device, msj_filter_rows_device,
 * msj_aggregate_device and msj_take_rows_device run on them unchanged.
 * A non-zero code in d_order_result -- the tied MSJ_CAPACITY included -- passes through: d_result and d_select carry it and
 * nothing else is written, so the chain stops by itself.  R > rows, R > capacity, V > rank_capacity or R >= 2^31:
 * MSJ_CAPACITY the same way.  Arguments, checked in this order: NULL ctx / d_result / d_select / d_order_result; NULL
 * d_codes with rows > 0, NULL d_fields with capacity > 0, NULL d_rank with rank_capacity > 0: MSJ_ERR_BAD_ARGUMENT.  rows or
 * capacity of 2^40 or more: MSJ_CAPACITY.  Then d_result == d_select, and alignment -- d_fields 16-byte, the codes and
 * ranks 4-byte, d_n_rows and the three results 8-byte: MSJ_ERR_BAD_ARGUMENT.  One kernel, a lane per row; a code is read
 * only below R, a rank only below min(V, rank_capacity), nothing at or past R is written.
 */
typedef struct msj_rank_rows_result {   /* 48 bytes */
    int32_t  code;       /* 0; MSJ_CAPACITY; or the code of d_order_result */
    uint32_t flags;      /* 0 */
    uint64_t n_rows;     /* R */
    uint64_t n_ranked;   /* rows that got a rank */
    uint64_t n_null;     /* rows with code -1 */
    uint64_t n_unknown;  /* every other row without a rank */
    uint64_t reserved;
} msj_rank_rows_result;
int32_t msj_rank_rows_device(msj_ctx *ctx,
        const int32_t *d_codes, uint64_t rows, const uint64_t *d_n_rows,
        const uint32_t *d_rank, uint64_t rank_capacity, const msj_dictionary_order_result *d_order_result,
        msj_field *d_fields, uint64_t capacity,
        msj_rank_rows_result *d_result, msj_select_documents_result *d_select, void *stream);

/*
 * ---- substring patterns over a byte column (DERIVED) -----------------------------------------------------
 * msj_match_strings_device answers "which lines' /message contains timeout" on the device: for every row of a byte column
 * and each of up to 16 patterns, the first place where the pattern matches, as a record that the filter, take, aggregate
 * and sort calls read.  Over a raw column of the documents themselves the same call is grep over the lines of a window.
 * Patterns: msj_patterns_create compiles 1 to 16 patterns into an immutable object, like msj_predicates_create and
 * msj_paths_create: synchronous, the device memory owned by the object, usable on any stream of the context's device;
 * msj_patterns_destroy(NULL) does nothing.  A pattern is 1 to 4 literal PIECES of 1 to 255 bytes each: `bytes` holds them
 * back to back, piece_len[j] their lengths (0 behind n_pieces), and the bytes are read during create only.  There is no
 * text syntax at this level -- no %, *, _ and no escapes: the pieces are explicit, no byte value is special.  Pattern
 * flags: MSJ_MATCH_AT_START, MSJ_MATCH_AT_END, MSJ_MATCH_NOCASE_ASCII.  A NULL array or `out`, a count outside 1..16, a
 * pattern without bytes, with 0 or more than 4 pieces, a piece of 0 or more than 255 bytes, a length behind n_pieces, an
 * unknown pattern flag, a non-zero `flags` of the create call: MSJ_ERR_BAD_ARGUMENT.
 * Match: a value v (bytes) matches the pieces s_0 .. s_(n-1) iff positions p_0 .. p_(n-1) exist with
 *   v[p_j : p_j + len(s_j)] == s_j,   p_(j+1) >= p_j + len(s_j) (pieces do not overlap),
 *   p_0 == 0 under AT_START,   p_(n-1) + len(s_(n-1)) == len(v) under AT_END.
 * The row's number is the smallest p_0 of any such sequence.  With NOCASE_ASCII the bytes A-Z on both sides compare as a-z;
 * every other byte, 0x80-0xFF included, compares as itself.  One piece is "contains", with AT_START "starts with", with
 * AT_END "ends with", with both equality; several pieces are a%b%c of SQL LIKE without _.
 * Inputs: the (d_offsets[rows + 1], d_valid[rows], d_bytes[bytes_len]) layout exactly as msj_dictionary_device takes it: a
 * path's strings, a list's strings, a map's keys, raw JSON text.  R = d_n_rows ? *d_n_rows : rows is read on the device.
 * The row test is checked on the arrays, never believed: a row has a value iff d_valid[k] != 0, and the offsets must ascend
 * over 0 .. R and end inside bytes_len -- d_offsets[k] <= d_offsets[k + 1] <= bytes_len, as both column calls write them.
 * On a violation the code is MSJ_ERR_BAD_ARGUMENT in d_result and d_select and nothing else is written
 * (msj_select_elements_device's rule for rows that do not ascend).  The bytes of a row with d_valid == 0 belong to no row,
 * and a match never spans two rows.
 * Outputs: n_patterns columns of records, d_fields[p * capacity + k] for k < R; nothing at or past R is written.  A row
 * that matches pattern p gets {bits = p_0 as int64, token = 0xFFFFFFFF, type 'l', flags 0, code 0}, the shape
 * msj_rank_rows_device writes; a row that does not, and a null row, gets the record of a missing value that
 * msj_take_rows_device writes (code 20, token 0xFFFFFFFF, the rest 0).  d_select is written as a select result over the
 * records (n_documents = R, n_paths = n_patterns, n_found recounted), so msj_filter_rows_device, msj_take_rows_device,
 * msj_aggregate_device and msj_sort_rows_device run on them unchanged: MSJ_PRED_FOUND on a column is "contains",
 * MSJ_PRED_NUM_EQ 0 is "starts with", MSJ_PRED_NOT also passes a row without a value, and the count of a column per group
 * is the number of matching lines per group.
 * d_result: code; flags 0; n_rows = R; n_values the rows that are not null; n_matched the matching (pattern, row) pairs;
 * max_pieces the most pieces of a pattern.  R > rows, R > capacity or R >= 2^31: MSJ_CAPACITY with n_rows = R and nothing
 * else written.  R == 0 writes zero results (n_paths and max_pieces kept).
 * Arguments, checked in this order: NULL ctx / patterns / d_result / d_select, patterns of another device; NULL d_offsets
 * / d_valid with rows > 0, NULL d_fields with capacity > 0; NULL d_bytes with bytes_len > 0: MSJ_ERR_BAD_ARGUMENT.  rows,
 * capacity or bytes_len of 2^40 or more: MSJ_CAPACITY.  Then d_result == d_select, and alignment -- d_fields 16-byte,
 * d_offsets, d_n_rows and the two results 8-byte, d_bytes and d_valid any: MSJ_ERR_BAD_ARGUMENT.  Nothing is launched on
 * any of them.  Asynchronous on `stream`, no host round trip, workspace in the context.  Safe on ANY arrays: d_bytes is read
 * only inside [0, bytes_len), whatever its alignment; an offset only at or below R; nothing at or past R is touched.  Every
 * output is a pure function of the input, bit for bit from run to run.
 * The search is organised by byte, not by row: a block stages a tile of consecutive bytes and 256 bytes behind it in LDS
 * with aligned 16-byte loads, every lane tests a run of start positions against every pattern, and a hit finds its row by
 * binary search in the offsets and competes there by minimum.  One pass over the bytes per piece level; a pattern of one
 * piece has one pass and no state besides its word per row.
 * Out of scope: _ / ? / character classes / regular expressions; Unicode case folding and normalisation; all occurrences
 * or a count per row (the first one only); replacement.
 */
#define MSJ_MATCH_AT_START 1u       /* msj_pattern.flags: the first piece stands at the value's first byte */
#define MSJ_MATCH_AT_END 2u         /* the last piece ends at the value's last byte */
#define MSJ_MATCH_NOCASE_ASCII 4u   /* A-Z compare as a-z, on both sides */
#define MSJ_MATCH_MAX_PATTERNS 16u
#define MSJ_MATCH_MAX_PIECES 4u
#define MSJ_MATCH_MAX_PIECE_BYTES 255u
typedef struct msj_patterns msj_patterns;
typedef struct msj_pattern {   /* 32 bytes */
    const uint8_t *bytes;      /* the pieces back to back */
    uint32_t n_pieces;         /* 1 .. 4 */
    uint32_t flags;            /* MSJ_MATCH_* */
    uint32_t piece_len[4];     /* 1 .. 255 each; 0 behind n_pieces */
} msj_pattern;
typedef struct msj_match_strings_result {   /* 48 bytes */
    int32_t  code;        /* 0; MSJ_CAPACITY; MSJ_ERR_BAD_ARGUMENT: the offsets do not ascend inside bytes_len */
    uint32_t flags;       /* 0 */
    uint64_t n_rows;      /* R */
    uint64_t n_values;    /* rows that are not null */
    uint64_t n_matched;   /* matching (pattern, row) pairs, summed over the patterns */
    uint64_t max_pieces;  /* the most pieces of a pattern: the passes over the bytes */
    uint64_t reserved;
} msj_match_strings_result;
int32_t msj_patterns_create(msj_ctx *ctx, const msj_pattern *patterns, uint32_t n_patterns, uint32_t flags, msj_patterns **out);
void msj_patterns_destroy(msj_patterns *patterns);
int32_t msj_match_strings_device(msj_ctx *ctx, const msj_patterns *patterns,
        const uint64_t *d_offsets, const uint8_t *d_valid, uint64_t rows, const uint64_t *d_n_rows,
        const uint8_t *d_bytes, uint64_t bytes_len,
        msj_field *d_fields, uint64_t capacity,
        msj_match_strings_result *d_result, msj_select_documents_result *d_select, void *stream);
/* Device workspace of one msj_match_strings_device call (the context keeps it): 16 bytes per (pattern, row) -- the word the
 * places compete on and the chain's cursor -- and the call's state. */
uint64_t msj_match_strings_workspace_bytes(uint64_t rows, uint32_t n_patterns);

/*
 * ---- rows grouped by numbers, time buckets and several keys at once (DERIVED) -------------------------
 * "Errors per minute per status": msj_aggregate_device groups by any int32 codes, and msj_dictionary_device gives dense codes
 * to any (offsets, valid, bytes) column.  The two calls here are the step in front of them: msj_bucket_rows_device floors a
 * column of number records to multiples of a width (/ts cast to milliseconds, width 60 000: the minute), and
 * msj_group_keys_device lays 1 to 8 columns -- number records, int32 codes -- out as ONE canonical, order-preserving,
 * fixed-width byte key per row, in exactly the layout the dictionary calls read.  Codes, first rows, distinct keys, counts,
 * the order of the groups and the aggregate then come from the calls that exist, unchanged.
 *
 * msj_bucket_rows_device.  R = d_rows_select->n_documents is read on the device.  The output record of row k < R:
 *   the input has a code       the input record, unchanged
 *   a number value             msj_aggregate_device's rule: code == 0, type 'l' or 'd', MSJ_FIELD_NO_BITS not set, a 'd' finite.
 *                              Let f be the value of an 'l' and floor(value) of a 'd'.  The result is
 *                              s = origin + floor((f - origin) / width) * width over the integers -- which is the same
 *                              expression over the reals, width and origin being integers: -0.5 with width 1 is -1, 1969-12-31
 *                              T23:59:59.999Z with width 60 000 is -60 000, a floor and not a truncation.  The record is type
 *                              'l', bits = s, token = the input's, flags 0, code 0.  A 'd' whose floor lies outside int64, and
 *                              s < INT64_MIN (s <= f: the other end cannot be left), give code 9 (NUMBER_ERROR), token
 *                              0xFFFFFFFF, everything else 0, counted in n_range
 *   code 0, 'l' / 'd' without usable bits (MSJ_FIELD_NO_BITS, a NaN, an infinity)     code 9 likewise, counted in n_skipped
 *   anything else with code 0  code 17 (INCORRECT_TYPE), token 0xFFFFFFFF, everything else 0, counted in n_other
 * The remainder r = (f - origin) mod width in [0, width) comes from an unsigned 64-bit subtraction and one %, in two cases (f >=
 * origin; f < origin), and s = f - r: no 128-bit word, no multiply that wraps, exact for every int64 f and origin and every
 * width up to 2^63 - 1.
 * d_result: code; flags 0; n_rows = R; n_bucketed the records written as buckets; n_range; n_skipped; n_other.  The codes,
 * the capacity rule (R > capacity or R >= 2^31: MSJ_CAPACITY with n_rows = R, nothing else written), d_rows_select->code != 0,
 * R == 0, d_out_select (n_found = n_bucketed, n_no_bits recounted over what was written) and d_out == d_rows exactly, a bucket
 * in place, are msj_cast_strings_device's.  Every output is a pure function of the input.
 * Arguments, checked in this order: NULL ctx / d_result / d_rows_select; NULL d_rows / d_out with capacity > 0; width < 1 or a
 * non-zero `flags`: MSJ_ERR_BAD_ARGUMENT.  A capacity of 2^40 records or more: MSJ_CAPACITY.  Then d_out overlapping d_rows in
 * any way but d_out == d_rows, d_result == a select result, d_out_select == d_rows_select, and alignment -- d_rows, d_out
 * 16-byte; the result and select results 8-byte: MSJ_ERR_BAD_ARGUMENT.  Nothing is launched on any of them.  Asynchronous on
 * `stream`, no host round trip, workspace in the context.  Safe on ANY records: nothing at or past R or capacity is touched.
 *
 * msj_group_keys_device.  `parts` is a HOST array of n_parts columns, every one with room for `stride` rows:
 *   MSJ_KEY_NUMBER  d_column: msj_field[stride]; 11 key bytes.  The tag byte 0x00, then msj_sort_rows_device's ascending key of
 *                   the value, big-endian: hi in 8 bytes, lo in 2.  So equal reals have equal bytes (3 and 3.0; -0.0 and 0) and
 *                   the bytes' order is the order of the reals, an int64 against a double exactly (9007199254740992.0 <
 *                   9007199254740993 < 9007199254740994.0).  A record that is no number value (the rule above): the tag 0x01
 *                   and ten zero bytes
 *   MSJ_KEY_CODE    d_column: int32_t[stride]; 5 key bytes.  The tag byte 0x00, then the code big-endian in 4 bytes.  A code
 *                   below 0: the tag 0x01 and four zero bytes
 * W, the key's width, is the sum of the parts' widths, at most 88.  R = d_rows_select->n_documents is read on the device.
 * d_offsets[k] = k * W for k <= R; d_bytes[k * W, (k + 1) * W) holds row k's parts in part order; d_valid[k] = 1 iff every
 * null part of row k carries MSJ_KEY_NULL_IS_GROUP.  By default a row with a null part has no key -- code -1 from the
 * dictionary, "ungrouped" in the aggregate; with the flag "no value" is a group of its own, and it sorts last.  Its bytes are
 * written either way.  Nothing at or past R (valid), R + 1 (offsets) or R * W (bytes) is written.  memcmp of two keys is the
 * lexicographic order of their parts, and two keys are equal iff every part is the same real, the same code or null in both.
 * Every output is a pure function of the input.
 * d_result: code; flags 0; n_rows = R; n_keys the rows with d_valid = 1; n_null_rows the rows with any null part; key_width =
 * W (in every case: it is a function of the arguments); bytes_len = R * W.  d_rows_select->code != 0: a zero result with that
 * code, nothing else written.  R > stride, R > capacity, R >= 2^31 or R * W > bytes_capacity: MSJ_CAPACITY with n_rows = R,
 * nothing else written.  R == 0 writes d_offsets[0] = 0 (where d_offsets is given) and a result of zeros and key_width.
 * Arguments, checked in this order: NULL ctx / d_result / d_rows_select / parts; n_parts outside 1..8; an unknown kind or
 * flag; a NULL d_column with stride > 0; NULL d_offsets / d_valid / d_bytes with capacity > 0; d_result == d_rows_select;
 * then alignment -- records and d_bytes 16-byte, codes 4-byte, d_offsets, the result and the select result 8-byte:
 * MSJ_ERR_BAD_ARGUMENT.  Nothing is launched on any of them.  Asynchronous on `stream`, no host round trip, workspace in the
 * context (the counters).  Safe on ANY records and codes: one is read only at k < R <= stride.
 * A block takes 256 consecutive rows: every lane builds its row's W bytes in LDS (at most 22 KiB), then the block writes its
 * 256 * W contiguous bytes -- the first a multiple of 16 -- with aligned 16-byte stores, the last block its tail byte by byte.
 * Out of scope: calendar months and time zones (a bucket is a multiple of a fixed width); a dense path without a hash for
 * small bucket ranges; more than 8 parts; keys on raw JSON text (msj_raw_column_device's column is a dictionary input as it is).
 */
#define MSJ_KEY_NUMBER 1u          /* msj_key_part.kind: d_column is msj_field[stride]; 11 key bytes */
#define MSJ_KEY_CODE   2u          /* d_column is int32_t[stride]; 5 key bytes */
#define MSJ_KEY_NULL_IS_GROUP 1u   /* msj_key_part.flags: a null part does not take the row's key away */
#define MSJ_KEY_MAX_PARTS 8u
typedef struct msj_key_part {   /* 16 bytes; a host array */
    const void *d_column;
    uint32_t kind;    /* MSJ_KEY_NUMBER, MSJ_KEY_CODE */
    uint32_t flags;   /* MSJ_KEY_NULL_IS_GROUP */
} msj_key_part;
typedef struct msj_bucket_rows_result {   /* 48 bytes */
    int32_t  code;        /* 0; MSJ_CAPACITY (R > capacity or R >= 2^31: n_rows = R, nothing else written); or d_rows_select->code */
    uint32_t flags;       /* 0 */
    uint64_t n_rows;      /* R */
    uint64_t n_bucketed;  /* records written as buckets: type 'l', code 0 */
    uint64_t n_range;     /* number values whose floor or bucket lies outside int64 */
    uint64_t n_skipped;   /* 'l' / 'd' records without usable bits (MSJ_FIELD_NO_BITS, NaN, infinity) */
    uint64_t n_other;     /* rows with code 0 that are no number */
} msj_bucket_rows_result;
typedef struct msj_group_keys_result {   /* 48 bytes */
    int32_t  code;         /* 0; MSJ_CAPACITY; or d_rows_select->code */
    uint32_t flags;        /* 0 */
    uint64_t n_rows;       /* R */
    uint64_t n_keys;       /* rows with d_valid = 1 */
    uint64_t n_null_rows;  /* rows with at least one null part */
    uint64_t key_width;    /* W */
    uint64_t bytes_len;    /* R * W */
} msj_group_keys_result;
int32_t msj_bucket_rows_device(msj_ctx *ctx, const msj_field *d_rows, const msj_select_documents_result *d_rows_select,
        int64_t width, int64_t origin, uint32_t flags,
        msj_field *d_out, uint64_t capacity,
        msj_bucket_rows_result *d_result, msj_select_documents_result *d_out_select, void *stream);
int32_t msj_group_keys_device(msj_ctx *ctx, const msj_key_part *parts, uint32_t n_parts, uint64_t stride,
        const msj_select_documents_result *d_rows_select,
        uint64_t *d_offsets, uint8_t *d_valid, uint8_t *d_bytes, uint64_t capacity, uint64_t bytes_capacity,
        msj_group_keys_result *d_result, void *stream);
/* Device workspace of one call of either (the context keeps it): the counters. */
uint64_t msj_bucket_rows_workspace_bytes(uint64_t capacity);
uint64_t msj_group_keys_workspace_bytes(uint64_t capacity);

/*
 * Device memory for hosts that have no HIP binding of their own (a Mojo DLHandle, plain C, the C++ mirrors
 * under include/): allocation on the context's device and blocking copies.  Plumbing, not part of the path.
 */
int32_t msj_device_alloc(msj_ctx *ctx, uint64_t bytes, void **d_out);
int32_t msj_device_free(msj_ctx *ctx, void *d_ptr);
int32_t msj_copy_to_device(msj_ctx *ctx, void *d_dst, const void *src, uint64_t bytes, void *stream);
int32_t msj_copy_to_host(msj_ctx *ctx, void *dst, const void *d_src, uint64_t bytes, void *stream);

/* Tile geometry (for roofline bookkeeping and tests). */
uint32_t msj_tile_bytes(void);

#ifdef __cplusplus
}
#endif
#endif /* MSJ_STAGE1_H */
