// host_pipe_sanitize.cpp -- the host-pointer pipeline of msj_stage1 (csrc/host_pipe.cpp: uploader, downloader, copy pool,
// pinned rings, events, slot-reuse waits) on a fake asynchronous device, under AddressSanitizer + UndefinedBehaviorSanitizer
// and under ThreadSanitizer, in one CPU-only program with its own main (tests/test_host_pipe_sanitizers.py builds and runs
// it).  The real, unmodified host_pipe.cpp is compiled with kilobyte chunks and pieces (-DMSJ_PIPE_CHUNK_BYTES,
// -DMSJ_PIPE_PIECE_BYTES) and linked against tests/cpp/fake_hip_device.h and the fake launch below.
// TEST INFRASTRUCTURE: nothing here is part of the product.
//
// The fake launch (enqueue_shard): ONE operation on the given stream which, when it runs,
//   - reads *d_carry_in (count, bytes, capacity_error);
//   - for every byte i of the chunk that is one of { } [ ] : , -- writes index_bias + i at d_idx[count] if
//     count < idx_capacity, else sets capacity_error; counts it either way;
//   - on is_final: sets capacity_error if count + 3 > idx_capacity, and writes the trailer words (trailer_len,
//     trailer_len, 0) at d_idx[count + 0..2] where they lie below idx_capacity;
//   - writes count, bytes, capacity_error and code into *d_carry_out: code is MSJ_SUCCESS on a chunk that is not final,
//     MSJ_CAPACITY on a final one with capacity_error, else the code the test case chose (g_final_code).
// What the caller must then see is computed by a plain loop over the whole input (run_call).
#include "fake_hip_device.h"

#include <atomic>
#include <string>

#include "../../mojo_simdjson_amd/csrc/ctx.h"

#ifndef MSJ_PIPE_CHUNK_BYTES
#error "build with the same -DMSJ_PIPE_CHUNK_BYTES / -DMSJ_PIPE_PIECE_BYTES as host_pipe.cpp"
#endif

using fakehip::dev;
using fakehip::Fail;
using fakehip::Sched;

#define CHECK FAKE_CHECK

// ---- what host_pipe.cpp links against besides the runtime
std::mutex g_default_mutex;
msj_ctx *default_ctx_locked() { return nullptr; }

namespace {

constexpr uint64_t C = MSJ_PIPE_CHUNK_BYTES, PIECE_WORDS = MSJ_PIPE_PIECE_BYTES / 4;
constexpr int kInSlots = 3, kOutSlots = 2;  // (HostPipe's; the lengths below reuse every input slot and its event)
constexpr uint32_t kPoison = 0xC3C3C3C3u;
constexpr uint64_t kGuard = 64;  // words on either side of the caller's index array

int32_t g_final_code = MSJ_SUCCESS;
bool in_set(uint8_t c) { return c == '{' || c == '}' || c == '[' || c == ']' || c == ':' || c == ','; }

struct ShardCall {
    const uint8_t *d_buf;
    uint64_t len, cap, trailer_len;
    uint32_t *d_idx;
    const msj_carry *cin;
    msj_carry *cout;
    bool has_prefix, is_final, no_emit;
    uint32_t bias;
};
struct CopySeen {
    uint64_t off_words, words;
};
std::mutex g_log_mutex;
std::vector<ShardCall> g_shards;
std::vector<CopySeen> g_downloads;       // device-to-host copies out of d_idx, in the order they were enqueued
const uint32_t *g_d_idx = nullptr;
uint64_t g_d_idx_words = 0;

// ---- the watchdog: a call that does not return is a failure that names its case
std::atomic<int64_t> g_deadline_ms{0};
std::atomic<bool> g_watchdog_stop{false};
char g_what[256] = "";
int64_t now_ms() { return std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
void watchdog() {
    while (!g_watchdog_stop.load()) {
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
        const int64_t d = g_deadline_ms.load();
        if (d && now_ms() > d) {
            std::fprintf(stderr, "FAILED watchdog: the call did not return within its time: %s\n", g_what);
            std::_Exit(3);
        }
    }
}

}  // namespace

int32_t enqueue_shard(msj_ctx *, const uint8_t *d_buf, uint64_t len, uint32_t *d_idx, uint64_t idx_capacity, const msj_carry *d_carry_in,
                      msj_carry *d_carry_out, msj_segment *, uint32_t, uint32_t *, bool has_prefix, bool is_final, bool no_emit,
                      uint64_t trailer_len, hipStream_t stream, uint32_t, uint32_t index_bias, const uint32_t *) {
    {
        std::lock_guard<std::mutex> lk(g_log_mutex);
        g_shards.push_back(ShardCall{d_buf, len, idx_capacity, trailer_len, d_idx, d_carry_in, d_carry_out, has_prefix, is_final, no_emit, index_bias});
    }
    const int32_t final_code = g_final_code;
    const hipError_t e = dev().enqueue(
        "enqueue_shard", stream,
        [=] {
            const msj_carry in = *d_carry_in;
            uint64_t count = in.count;
            uint32_t cap_err = in.capacity_error;
            for (uint64_t i = 0; i < len; i++)
                if (in_set(d_buf[i])) {
                    if (count < idx_capacity)
                        d_idx[count] = index_bias + (uint32_t)i;
                    else
                        cap_err = 1;
                    count++;
                }
            if (is_final) {
                if (count + 3 > idx_capacity) cap_err = 1;
                for (uint64_t j = 0; j < 3; j++)
                    if (count + j < idx_capacity) d_idx[count + j] = j < 2 ? (uint32_t)trailer_len : 0u;
            }
            msj_carry out;
            std::memset(&out, 0, sizeof out);
            out.count = count;
            out.bytes = in.bytes + len;
            out.capacity_error = cap_err;
            out.code = !is_final ? MSJ_SUCCESS : cap_err ? MSJ_CAPACITY : final_code;
            *d_carry_out = out;
        },
        true);
    return e == hipSuccess ? MSJ_SUCCESS : MSJ_ERR_HIP;
}

namespace {

enum CapMode { kFull, kCountPlus3, kCountPlus2, kCount, kCountMinus1, kOne };
struct Case {
    uint64_t len = 1;
    int density = 1;             // 0: no byte of the set, 1: about one in five, 2: every byte
    int64_t first_chunk_set = -1;  // >= 0: exactly that many bytes of the set open chunk 0, every later chunk is dense
    CapMode cap = kFull;
    bool pin_in = false, pin_out = false;
    int32_t code = MSJ_SUCCESS;
};
struct Outcome {
    int32_t rc = 0;
    int64_t entries = 0, enqueued = 0;
    bool injected = false;
    std::string injected_into;
};

struct Ctx {
    msj_ctx c;
    Ctx() { c.device = 0; }
    ~Ctx() {
        if (c.pipe) host_pipe_destroy(c.pipe);
        c.pipe = nullptr;
    }
};

std::mt19937_64 g_rng;
bool g_mis_seen[64];
uint64_t g_calls = 0, g_pieces = 0, g_err_hip = 0, g_unavailable = 0, g_ignored = 0, g_thrown = 0, g_injected = 0;

std::vector<uint8_t> make_input(const Case &k) {
    std::vector<uint8_t> in(k.len);
    static const char set[] = "{}[]:,";
    for (uint64_t i = 0; i < k.len; i++) {
        bool hit;
        if (k.first_chunk_set >= 0)
            hit = i >= C || (int64_t)i < k.first_chunk_set;
        else
            hit = k.density == 2 || (k.density == 1 && g_rng() % 5 == 0);
        in[i] = hit ? (uint8_t)set[g_rng() % 6] : (uint8_t)('a' + g_rng() % 26);
    }
    return in;
}

// One call of host_pipeline as msj_stage1_ctx makes it, on exact-size caller and device memory.  Fail::kNone: the call
// must succeed and every word is compared.  Otherwise entry `fail_at` fails: see the checks at the end.
Outcome run_call(Ctx &ctx, const Case &k, Fail mode, int64_t fail_at, const char *what, bool may_be_unavailable = false) {
    fakehip::Device &d = dev();
    const std::vector<uint8_t> in = make_input(k);
    std::vector<uint32_t> pos;
    for (uint64_t i = 0; i < k.len; i++)
        if (in_set(in[i])) pos.push_back((uint32_t)i);
    const uint64_t count = pos.size();
    uint64_t cap = k.len + 3;
    if (k.cap == kCountPlus3) cap = count + 3;
    if (k.cap == kCountPlus2) cap = count + 2;
    if (k.cap == kCount) cap = count;
    if (k.cap == kCountMinus1) cap = count ? count - 1 : 0;
    if (k.cap == kOne || cap < 1) cap = 1;  // (capacity 0 is no call)
    CHECK(cap >= 1 && cap <= k.len + 3, "%s: a case with capacity %llu", what, (unsigned long long)cap);
    const uint64_t dev_cap = cap < k.len + 3 ? cap : k.len + 3;
    // the caller's memory: exactly the input (a registered input is a view that starts 37 bytes inside its range), and the
    // index array between two guards
    const uint64_t in_off = k.pin_in ? 37 : 0;
    uint8_t *in_block = static_cast<uint8_t *>(std::malloc(in_off + k.len));
    std::memcpy(in_block + in_off, in.data(), k.len);
    uint32_t *idx_block = static_cast<uint32_t *>(std::malloc((cap + 2 * kGuard) * sizeof(uint32_t)));
    for (uint64_t j = 0; j < cap + 2 * kGuard; j++) idx_block[j] = kPoison;
    uint32_t *idx_out = idx_block + kGuard;
    ctx.c.pinned.clear();
    if (k.pin_in) ctx.c.pinned.push_back({in_block, in_off + k.len});
    if (k.pin_out) ctx.c.pinned.push_back({reinterpret_cast<const uint8_t *>(idx_block), (cap + 2 * kGuard) * sizeof(uint32_t)});
    // the context's device staging, sized as msj_stage1_ctx sizes it (released first, so that the bounds are this call's)
    ctx.c.d_in.release();
    ctx.c.d_idx.release();
    CHECK(ctx.c.d_in.reserve((k.len + 63u) & ~63ull, false) && ctx.c.d_idx.reserve(dev_cap * sizeof(uint32_t), false), "device staging");
    d.poison_host_blocks(0xA5);  // the carries and rings of earlier calls
    {
        std::lock_guard<std::mutex> lk(g_log_mutex);
        g_shards.clear();
        g_downloads.clear();
        g_d_idx = ctx.c.d_idx.as<uint32_t>();
        g_d_idx_words = dev_cap;
    }
    g_final_code = k.code;
    std::snprintf(g_what, sizeof g_what, "%s: len %llu density %d cap %llu pinned %d/%d code %d, %s entry %lld", what, (unsigned long long)k.len,
                  k.density, (unsigned long long)cap, (int)k.pin_in, (int)k.pin_out, k.code,
                  mode == Fail::kNone ? "no failure at" : mode == Fail::kSync ? "failing" : mode == Fail::kAsync ? "asynchronously failing" : "throwing",
                  (long long)fail_at);
    msj_carry res;
    std::memset(&res, 0x5A, sizeof res);
    d.begin_call(mode, fail_at);
    g_deadline_ms.store(now_ms() + 60000);
    Outcome o;
    try {
        o.rc = host_pipeline(&ctx.c, in_block + in_off, k.len, idx_out, dev_cap, 0, &res);
    } catch (const std::bad_alloc &) {  // (msj_stage1_ctx catches it the same way)
        o.rc = MSJ_MEMALLOC;
    }
    g_deadline_ms.store(0);
    const size_t pending = d.pending();
    {
        std::lock_guard<std::mutex> lk(d.m);
        o.entries = d.entry;
        o.enqueued = d.enqueued;
        o.injected = d.injected;
        o.injected_into = d.injected_into;
    }
    d.begin_call(Fail::kNone, -1);
    g_calls++;
    if (o.rc != MSJ_SUCCESS) {
        // Behind a return the library owns no pending access to caller memory: the caller frees both arrays at once, and
        // only then does the device run whatever is still queued (AddressSanitizer reports an operation that touches them)
        CHECK(o.injected || (may_be_unavailable && o.rc == kPipeUnavailable), "%s: returned %d though nothing failed", g_what, o.rc);
        std::free(in_block);
        std::free(idx_block);
        ctx.c.pinned.clear();
        d.drain();
        d.clear_errors();
        CHECK(pending == 0, "%s: returned %d with %zu operations still queued (failed in %s)", g_what, o.rc, pending, o.injected_into.c_str());
        if (o.rc == kPipeUnavailable) {
            CHECK(o.enqueued == 0, "%s: kPipeUnavailable after %lld operations were enqueued (failed in %s)", g_what, (long long)o.enqueued,
                  o.injected_into.c_str());
            g_unavailable++;
        } else if (mode == Fail::kThrow) {
            CHECK(o.rc == MSJ_MEMALLOC, "%s: returned %d for an exception", g_what, o.rc);
            g_thrown++;
        } else {
            CHECK(o.rc == MSJ_ERR_HIP, "%s: returned %d (failed in %s)", g_what, o.rc, o.injected_into.c_str());
            g_err_hip++;
        }
        g_injected += o.injected;
        return o;
    }
    // ---- success: every word, the guards, the result, the launches and the downloads
    CHECK(pending == 0, "%s: returned with %zu operations still queued", g_what, pending);
    if (o.injected) {
        CHECK(mode == Fail::kSync, "%s: success though %s failed asynchronously / threw", g_what, o.injected_into.c_str());
        // the failures the code may ignore: the device is selected already, no PCI address means no binding, and the last
        // wait on the kernel stream follows waits that have covered all of its work
        CHECK(o.injected_into == "hipSetDevice" || o.injected_into == "hipDeviceGetPCIBusId" || o.injected_into == "hipStreamSynchronize",
              "%s: success though %s failed", g_what, o.injected_into.c_str());
        g_injected++;
        g_ignored++;
    }
    const bool cap_err = count + 3 > dev_cap;
    const int32_t code = cap_err ? MSJ_CAPACITY : k.code;
    const bool trailer = code == MSJ_SUCCESS || code == MSJ_EMPTY || code == MSJ_UTF8_ERROR;
    uint64_t avail_final = count + (trailer ? 3 : 0);
    if (avail_final > dev_cap) avail_final = dev_cap;
    CHECK(res.count == count && res.bytes == k.len && res.capacity_error == (cap_err ? 1u : 0u) && res.code == code,
          "%s: result (count %llu, bytes %llu, capacity_error %u, code %d), want (%llu, %llu, %d, %d)", g_what, (unsigned long long)res.count,
          (unsigned long long)res.bytes, res.capacity_error, res.code, (unsigned long long)count, (unsigned long long)k.len, (int)cap_err, code);
    for (uint64_t j = 0; j < cap + 2 * kGuard; j++) {
        uint32_t want = kPoison;
        if (j >= kGuard && j - kGuard < avail_final) {
            const uint64_t w = j - kGuard;
            want = w < count ? pos[w] : w - count < 2 ? (uint32_t)k.len : 0u;
        }
        CHECK(idx_block[j] == want, "%s: word %lld of the caller's array (capacity %llu, count %llu) is %#x, want %#x", g_what,
              (long long)j - (long long)kGuard, (unsigned long long)cap, (unsigned long long)count, idx_block[j], want);
    }
    {
        std::lock_guard<std::mutex> lk(g_log_mutex);
        const uint64_t nchunks = (k.len + C - 1) / C;
        CHECK(g_shards.size() == nchunks, "%s: %zu launches for %llu chunks", g_what, g_shards.size(), (unsigned long long)nchunks);
        for (uint64_t c = 0; c < nchunks; c++) {
            const ShardCall &s = g_shards[c];
            CHECK(s.d_buf == ctx.c.d_in.as<uint8_t>() + c * C && s.len == (k.len - c * C < C ? k.len - c * C : C) && s.bias == c * C &&
                      s.d_idx == g_d_idx && s.cap == dev_cap && s.has_prefix == (c > 0) && s.is_final == (c + 1 == nchunks) && !s.no_emit &&
                      s.trailer_len == k.len && (c == 0 || s.cin == g_shards[c - 1].cout),
                  "%s: the arguments of launch %llu", g_what, (unsigned long long)c);
        }
        // the downloads the chunks' counts call for: whole chunks into a registered array, else pieces of at most one slot
        // whose source starts on a 256-byte line of the device array
        std::vector<CopySeen> want;
        uint64_t sent = 0, chunk_end = 0, seen = 0;
        for (uint64_t c = 0; c < nchunks; c++) {
            chunk_end = (c + 1) * C;
            while (seen < count && pos[seen] < chunk_end) seen++;
            uint64_t avail = seen + (c + 1 == nchunks && trailer ? 3 : 0);
            if (avail > dev_cap) avail = dev_cap;
            if (k.pin_out) {
                if (avail > sent) want.push_back({sent, avail - sent});
                if (avail > sent) sent = avail;
                continue;
            }
            while (sent < avail) {
                const uint64_t mis = sent & 63u, n = avail - sent < PIECE_WORDS - mis ? avail - sent : PIECE_WORDS - mis;
                want.push_back({sent - mis, n + mis});
                g_mis_seen[mis] = true;
                g_pieces++;
                sent += n;
            }
        }
        CHECK(g_downloads.size() == want.size(), "%s: %zu downloads, want %zu", g_what, g_downloads.size(), want.size());
        for (size_t p = 0; p < want.size(); p++)
            CHECK(g_downloads[p].off_words == want[p].off_words && g_downloads[p].words == want[p].words,
                  "%s: download %zu reads %llu words at word %llu of the device array, want %llu at %llu", g_what, p,
                  (unsigned long long)g_downloads[p].words, (unsigned long long)g_downloads[p].off_words, (unsigned long long)want[p].words,
                  (unsigned long long)want[p].off_words);
    }
    std::free(in_block);
    std::free(idx_block);
    ctx.c.pinned.clear();
    return o;
}

Outcome ok_call(Ctx &ctx, const Case &k, const char *what) { return run_call(ctx, k, Fail::kNone, -1, what); }

// ---- the success path
void success_cases(int rounds) {
    Ctx ctx;
    std::vector<uint64_t> lens = {1, C - 1, C, C + 1};
    for (uint64_t m = 2; m <= (uint64_t)kInSlots + 2; m++) {  // the input slots and their events are reused from chunk 3 on
        lens.push_back(m * C - 1);
        lens.push_back(m * C);
        lens.push_back(m * C + 1);
    }
    lens.push_back(9 * C + 123);
    for (uint64_t len : lens)
        for (int density = 0; density < 3; density++)
            for (int pins = 0; pins < 4; pins++) {
                Case k;
                k.len = len;
                k.density = density;
                k.pin_in = pins & 1;
                k.pin_out = pins & 2;
                k.code = density ? MSJ_SUCCESS : MSJ_EMPTY;
                (void)ok_call(ctx, k, "lengths");
            }
    // idx_capacity around the count
    for (uint64_t len : {2 * C + 1, 5 * C - 1})
        for (int density = 1; density < 3; density++)
            for (int cap = kFull; cap <= kOne; cap++)
                for (int pin_out = 0; pin_out < 2; pin_out++) {
                    Case k;
                    k.len = len;
                    k.density = density;
                    k.cap = (CapMode)cap;
                    k.pin_out = pin_out;
                    k.pin_in = cap & 1;
                    (void)ok_call(ctx, k, "capacity");
                }
    // every class of final code: the trailer comes down with SUCCESS, EMPTY and UTF8_ERROR only
    for (int32_t code : {MSJ_SUCCESS, MSJ_EMPTY, MSJ_UTF8_ERROR, MSJ_UNCLOSED_STRING, MSJ_UNESCAPED_CHARS, MSJ_UNEXPECTED_ERROR, MSJ_CAPACITY})
        for (int pin_out = 0; pin_out < 2; pin_out++)
            for (uint64_t len : {C - 5, 3 * C + 5}) {
                Case k;
                k.len = len;
                k.code = code;
                k.pin_out = pin_out;
                (void)ok_call(ctx, k, "codes");
            }
    // a piece that starts at every offset inside a 256-byte line: chunk 0 brings 64 + r indices, chunk 1 is dense
    for (int r = 0; r < 64; r++) {
        Case k;
        k.len = 2 * C;
        k.first_chunk_set = 64 + r;
        (void)ok_call(ctx, k, "residues");
    }
    // one context, sizes that grow, shrink and grow again: the carries and events regrow, and a smaller call runs over a
    // larger call's (poisoned) carries
    {
        Ctx seq;
        for (uint64_t len : {2 * C + 5, 9 * C + 1, C - 1, 5 * C, (uint64_t)1, 12 * C + 77, 3 * C, 12 * C + 78, 2 * C}) {
            Case k;
            k.len = len;
            k.density = 1 + (int)(g_rng() % 2);
            k.pin_in = g_rng() & 1;
            k.pin_out = g_rng() & 2;
            (void)ok_call(seq, k, "sequence");
        }
    }
    // seeded cases over everything at once
    static const int32_t codes[] = {MSJ_SUCCESS, MSJ_SUCCESS, MSJ_SUCCESS, MSJ_UTF8_ERROR, MSJ_UNCLOSED_STRING, MSJ_EMPTY};
    for (int i = 0; i < rounds; i++) {
        Case k;
        k.len = 1 + g_rng() % (i % 16 == 0 ? 10 * C : 4 * C);
        k.density = (int)(g_rng() % 3);
        k.pin_in = g_rng() & 1;
        k.pin_out = g_rng() & 2;
        k.code = codes[g_rng() % 6];
        k.cap = (CapMode)(g_rng() % 8 < 3 ? 0 : g_rng() % 6);
        if (i % 32 == 0) {
            Ctx fresh;
            (void)ok_call(fresh, k, "seeded, fresh context");
        } else {
            (void)ok_call(ctx, k, "seeded");
        }
    }
}

// ---- the failure path: entry i of the call fails, for every i
void failure_sweep(bool pin_in, bool pin_out, bool throws) {
    Ctx ctx;
    Case k;
    k.len = 5 * C + 7;  // six chunks: every input slot is reused
    k.density = 2;
    k.pin_in = pin_in;
    k.pin_out = pin_out;
    (void)ok_call(ctx, k, "failure sweep, the call that sets the context up");
    const int64_t entries = ok_call(ctx, k, "failure sweep, clean run").entries;
    CHECK(entries > 30, "the clean call makes %lld entries", (long long)entries);
    for (int m = 0; m < (throws ? 3 : 2); m++) {
        const Fail mode = m == 0 ? Fail::kSync : m == 1 ? Fail::kAsync : Fail::kThrow;
        uint64_t failed = 0;
        const int64_t tries = mode == Fail::kThrow ? (int64_t)((k.len + C - 1) / C) : entries;  // (kThrow counts launches)
        for (int64_t i = 0; i < tries; i++) {
            const Outcome o = run_call(ctx, k, mode, i, "failure sweep");
            failed += o.rc != MSJ_SUCCESS;
            CHECK(mode == Fail::kAsync || o.injected, "entry %lld of %lld was not reached", (long long)i, (long long)entries);
            (void)ok_call(ctx, k, "failure sweep, the same context afterwards");
        }
        CHECK(failed >= (uint64_t)(mode == Fail::kSync ? entries / 2 : mode == Fail::kAsync ? 6 : tries), "only %llu of %lld injected failures failed the call",
              (unsigned long long)failed, (long long)entries);
    }
    std::printf("  failure sweep (input %s, output %s): %lld entry points per call\n", pin_in ? "registered" : "staged",
                pin_out ? "registered" : "staged", (long long)entries);
}

// a fresh context per index: the set-up (rings, streams, events, carries) fails too
void fresh_context_sweep() {
    Case k;
    k.len = 3 * C + 1;
    k.density = 2;
    int64_t entries;
    {
        Ctx ctx;
        entries = ok_call(ctx, k, "fresh context, clean run").entries;
    }
    uint64_t unavailable = 0;
    for (int64_t i = 0; i < entries; i++) {
        Ctx ctx;
        const Outcome o = run_call(ctx, k, Fail::kSync, i, "fresh context");
        unavailable += o.rc == kPipeUnavailable;
        if (o.rc != kPipeUnavailable) {
            (void)ok_call(ctx, k, "fresh context, afterwards");
            continue;
        }
        // the rings or streams could not be had: unavailable for good (msj_stage1_ctx takes plain staging from then on);
        // the carries or a chunk's event could not: the next call reserves them again
        const Outcome again = run_call(ctx, k, Fail::kNone, -1, "fresh context, after kPipeUnavailable", true);
        CHECK(again.rc == MSJ_SUCCESS || again.enqueued == 0, "a pipe that is unavailable enqueues nothing");
    }
    CHECK(unavailable >= 14, "only %llu set-up failures gave kPipeUnavailable", (unsigned long long)unavailable);
    std::printf("  fresh-context sweep: %lld entry points per call, %llu of them in the set-up\n", (long long)entries, (unsigned long long)unavailable);
}

// no PCI address, or one that sysfs does not know: no binding of the copy workers, and a working pipe
void locality_cases() {
    for (int mode = 0; mode < 2; mode++) {
        dev().pci_mode = mode;
        Ctx ctx;
        Case k;
        k.len = 4 * C + 3;
        (void)ok_call(ctx, k, "locality");
        char json[1024];
        CHECK(msj_host_placement(&ctx.c, json, sizeof json) == MSJ_SUCCESS, "msj_host_placement");
        const std::string s(json);
        CHECK(s.find("\"gpu_numa_node\": -1") != std::string::npos && s.find("\"gpu_local_cpus_usable\": 0") != std::string::npos &&
                  s.find("\"copy_threads_bound_to_gpu_node\": 0") != std::string::npos && s.find("\"pipeline_created\": true") != std::string::npos,
              "placement with PCI mode %d: %s", mode, json);
        CHECK((s.find("\"gpu_pci\": \"\"") != std::string::npos) == (mode == 0), "placement with PCI mode %d: %s", mode, json);
    }
    dev().pci_mode = 1;
}

}  // namespace

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    const std::string scheds = argc > 2 ? argv[2] : "lazy,threaded";
    const int rounds = argc > 3 ? std::atoi(argv[3]) : 400;
    std::thread dog(watchdog);
    dev().on_copy = [](void *, const void *src, size_t n, hipMemcpyKind kind) {
        std::lock_guard<std::mutex> lk(g_log_mutex);
        const uint32_t *s = static_cast<const uint32_t *>(src);
        if (kind == hipMemcpyDeviceToHost && g_d_idx && s >= g_d_idx && s < g_d_idx + g_d_idx_words)
            g_downloads.push_back({(uint64_t)(s - g_d_idx), n / 4});
    };
    for (const char *name : {"lazy", "threaded"}) {
        if (scheds.find(name) == std::string::npos) continue;
        const bool lazy = std::strcmp(name, "lazy") == 0;
        dev().sched = lazy ? Sched::kLazy : Sched::kThreaded;
        dev().rng.seed(seed * 2 + lazy);
        g_rng.seed(seed * 977 + lazy);
        std::memset(g_mis_seen, 0, sizeof g_mis_seen);
        std::printf("%s scheduler, chunk %llu bytes, piece %llu bytes\n", name, (unsigned long long)C, (unsigned long long)(PIECE_WORDS * 4));
        success_cases(rounds);
        for (int r = 0; r < 64; r++) CHECK(g_mis_seen[r], "no piece started %d words into a 256-byte line", r);
        for (int pins = 0; pins < 4; pins++) failure_sweep(pins & 1, pins & 2, pins == 0 || pins == 3);
        fresh_context_sweep();
        locality_cases();
        CHECK(dev().live_blocks() == 0 && dev().streams.empty(), "the contexts left %zu blocks and %zu streams behind", dev().live_blocks(),
              dev().streams.size());
    }
    g_watchdog_stop.store(true);
    dog.join();
    std::printf("host_pipe_sanitize ok: seed %llu, %llu calls, %llu staged pieces, %llu injected failures (%llu MSJ_ERR_HIP, %llu unavailable, "
                "%llu exceptions, %llu ignored by design)\n",
                (unsigned long long)seed, (unsigned long long)g_calls, (unsigned long long)g_pieces, (unsigned long long)g_injected,
                (unsigned long long)g_err_hip, (unsigned long long)g_unavailable, (unsigned long long)g_thrown, (unsigned long long)g_ignored);
    return 0;
}
