// host_pipe.cpp -- the host-pointer path of msj_stage1 for large inputs, and where its host side lives (msj_host_placement).
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <new>
#include <thread>

#include <pthread.h>
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#include "ctx.h"

#pragma GCC visibility push(hidden)

// ---- host-pointer path for large inputs: library-owned pinned rings, chunked and overlapped -----------------
// DomParserImplementation.stage1 (include/generic/dom_parser_implementation.mojo:65-69) hands over pageable host
// memory.  Pageable hipMemcpy is synchronous and its two directions do not overlap on this platform (measured:
// 31 GB/s of JSON for 268 MB up + 208 MB down), while pinned memory moves 57 GB/s each way at once
// (scripts/ubench/pcie_probe.cpp).  So: the input goes up in chunks through a ring of pinned buffers, filled by a
// few copy threads (one thread copies 32 GB/s, four 96 GB/s on the box's host); every chunk is one shard launch
// with the carry chained in device memory (msj_stage1_shard_device); a second host thread follows the chunks'
// counts and brings the finished part of the index array down through a second pinned ring while later chunks
// are still on their way up -- both PCIe directions and the kernel run at the same time.
// ---- where the host side of the pipeline lives (round 5: the PCIe-inclusive rate differed by 37 % between two boxes of
// the pool with nothing in the record to say why).  The GPU hangs off ONE NUMA node's root complex: staging copies that
// run on the other socket, or pinned rings whose pages lie there, cross the inter-socket link twice.  The copy workers
// are therefore bound to the CPUs of the GPU's node (those of them the process may use: a cgroup / taskset limit is
// respected; no such CPU -> no binding), the rings are allocated by a thread bound the same way (first touch), and
// msj_host_placement reports all of it.  Linux sysfs / syscalls only, no libnuma; anything unreadable reads as -1.
struct GpuHostLocality {
    char pci[32] = "";
    int node = -1;          // NUMA node of the GPU's PCIe root complex (-1: unknown / single node)
    cpu_set_t cpus;         // CPUs of that node that this process may run on
    int n_cpus = 0;
    char link_speed[32] = "", link_width[16] = "";
};
static bool read_line(const char *path, char *out, size_t cap) {
    FILE *f = std::fopen(path, "r");
    if (!f) return false;
    const bool ok = std::fgets(out, (int)cap, f) != nullptr;
    std::fclose(f);
    if (ok) out[std::strcspn(out, "\n")] = 0;
    return ok;
}
static GpuHostLocality gpu_locality(int device) {
    GpuHostLocality g;
    CPU_ZERO(&g.cpus);
    char bus[32] = "";
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) {
        (void)hipGetLastError();
        return g;
    }
    for (char *c = bus; *c; c++)
        if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');  // sysfs spells the address in lower case
    std::snprintf(g.pci, sizeof g.pci, "%s", bus);
    char path[128], line[4096];
    std::snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    if (read_line(path, line, sizeof line)) g.node = std::atoi(line);
    std::snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/current_link_speed", bus);
    (void)read_line(path, g.link_speed, sizeof g.link_speed);
    std::snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/current_link_width", bus);
    (void)read_line(path, g.link_width, sizeof g.link_width);
    std::snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/local_cpulist", bus);
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    if (read_line(path, line, sizeof line) && sched_getaffinity(0, sizeof allowed, &allowed) == 0) {
        char *save = nullptr;  // (strtok_r: this runs in a library, on whatever thread makes the call)
        for (char *tok = strtok_r(line, ",", &save); tok; tok = strtok_r(nullptr, ",", &save)) {  // "0-31,64-95"
            int lo = 0, hi = 0;
            const int k = std::sscanf(tok, "%d-%d", &lo, &hi);
            if (k == 1) hi = lo;
            for (int c = lo; k >= 1 && c <= hi && c < CPU_SETSIZE; c++)
                if (CPU_ISSET(c, &allowed)) {
                    CPU_SET(c, &g.cpus);
                    g.n_cpus++;
                }
        }
    }
    return g;
}
// NUMA node a mapped page lies on (get_mempolicy(MPOL_F_NODE | MPOL_F_ADDR)); -1 where the kernel will not say
static int numa_node_of(const void *p) {
#ifdef SYS_get_mempolicy
    int node = -1;
    if (p && syscall(SYS_get_mempolicy, &node, nullptr, 0UL, const_cast<void *>(p), 3UL /* MPOL_F_NODE | MPOL_F_ADDR */) == 0) return node;
#endif
    (void)p;
    return -1;
}

struct CopyPool {
    const cpu_set_t *bind = nullptr;  // the GPU's CPUs (HostPipe): every worker runs there
    int bound = 0;                    // workers whose affinity call succeeded
    std::vector<std::thread> threads;
    std::deque<std::function<void()>> tasks;
    std::mutex m;
    std::condition_variable cv;
    bool stop = false;
    explicit CopyPool(int n, const cpu_set_t *cpus = nullptr) : bind(cpus) {
        std::atomic<int> ok{0};
        for (int i = 0; i < n; i++)
            threads.emplace_back([this, &ok] {
                if (bind && pthread_setaffinity_np(pthread_self(), sizeof(cpu_set_t), bind) == 0) ok.fetch_add(1);
                ok.fetch_add(1 << 16);  // this worker has started
                for (;;) {
                    std::function<void()> f;
                    {
                        std::unique_lock<std::mutex> lk(m);
                        cv.wait(lk, [this] { return stop || !tasks.empty(); });
                        if (stop && tasks.empty()) return;
                        f = std::move(tasks.front());
                        tasks.pop_front();
                    }
                    f();
                }
            });
        while ((ok.load() >> 16) < n) std::this_thread::yield();  // (`ok` lives on this frame)
        bound = ok.load() & 0xFFFF;
    }
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> lk(m);
            stop = true;
        }
        cv.notify_all();
        for (auto &t : threads) t.join();
    }
    // memcpy split over `parts` workers, not waited for: *pending counts the slices still to do
    void copy_async(void *dst, const void *src, uint64_t n, int parts, std::atomic<int> *pending) {
        if (parts < 1) parts = 1;
        pending->store(parts, std::memory_order_relaxed);
        const uint64_t step = ((n / parts) + 63) & ~63ull;
        for (int i = 0; i < parts; i++) {
            const uint64_t lo = step * i < n ? step * i : n, hi = (i + 1 == parts || step * (i + 1) > n) ? n : step * (i + 1);
            {
                std::lock_guard<std::mutex> lk(m);
                tasks.emplace_back([=] {
                    if (hi > lo) std::memcpy(static_cast<char *>(dst) + lo, static_cast<const char *>(src) + lo, hi - lo);
                    pending->fetch_sub(1, std::memory_order_release);
                });
            }
            cv.notify_one();
        }
    }
    static void wait(std::atomic<int> *pending) {
        while (pending->load(std::memory_order_acquire) != 0) std::this_thread::yield();
    }
    // memcpy split over `parts` workers; returns when all of it is done
    void copy(void *dst, const void *src, uint64_t n, int parts) {
        if (n < (1u << 20) || parts <= 1) {
            std::memcpy(dst, src, n);
            return;
        }
        std::mutex dm;
        std::condition_variable dcv;
        int left = parts;
        const uint64_t step = ((n / parts) + 63) & ~63ull;
        for (int i = 0; i < parts; i++) {
            const uint64_t lo = step * i < n ? step * i : n, hi = (i + 1 == parts || step * (i + 1) > n) ? n : step * (i + 1);
            {
                std::lock_guard<std::mutex> lk(m);
                tasks.emplace_back([=, &dm, &dcv, &left] {
                    if (hi > lo) std::memcpy(static_cast<char *>(dst) + lo, static_cast<const char *>(src) + lo, hi - lo);
                    std::lock_guard<std::mutex> g(dm);
                    if (--left == 0) dcv.notify_one();
                });
            }
            cv.notify_one();
        }
        std::unique_lock<std::mutex> lk(dm);
        dcv.wait(lk, [&] { return left == 0; });
    }
};

// Tuning knobs of the host pipeline exist in the measurement build only (make -C csrc knobs: -DMSJ_DEBUG_KNOBS,
// scripts/libmsj_stage1_knobs.so); the product library has the measured defaults compiled in and reads no
// environment variable at all.
#ifdef MSJ_DEBUG_KNOBS
static int knob_int(const char *name, int dflt, int lo) {
    const char *v = std::getenv(name);
    const int x = v && *v ? std::atoi(v) : dflt;
    return x < lo ? lo : x;  // a pool without workers would block its callers for ever
}
bool knob_set(const char *name) { return std::getenv(name) != nullptr; }
#else
static int knob_int(const char *, int dflt, int) { return dflt; }
bool knob_set(const char *) { return false; }
#endif

// Chunk and piece sizes: compiled in.  The CPU harness of the pipeline (tests/cpp/host_pipe_sanitize.cpp) builds this file
// with kilobyte sizes, so that every chunk and piece border is reached by thousands of small runs; the product never
// defines either name.
#ifndef MSJ_PIPE_CHUNK_BYTES
#define MSJ_PIPE_CHUNK_BYTES (16ull << 20)
#endif
#ifndef MSJ_PIPE_PIECE_BYTES
#define MSJ_PIPE_PIECE_BYTES (16ull << 20)
#endif

struct HostPipe {
    static constexpr int kInSlots = 3, kOutSlots = 2;
    // copy workers and slices per staging copy (defaults measured on the MI355X box's host)
    const int kCopyThreads = knob_int("MSJ_PIPE_THREADS", 8, 1), kParts = knob_int("MSJ_PIPE_PARTS", 4, 1);
    const bool direct_upload = knob_int("MSJ_PIPE_DIRECT_UPLOAD", 0, 0) != 0;
    static constexpr uint64_t kChunk = MSJ_PIPE_CHUNK_BYTES;  // input bytes per chunk (a multiple of the tile)
    static constexpr uint64_t kPiece = MSJ_PIPE_PIECE_BYTES;  // index bytes per download piece
    static_assert(kChunk > 0 && kChunk % msj::kTileBytes == 0, "a chunk is whole tiles: only the stream's last shard may end inside one");
    static_assert(kPiece % 256 == 0 && kPiece / sizeof(uint32_t) > 64, "a piece keeps its source's offset inside a 256-byte line (up to 63 words) and still moves words");
    uint8_t *pin_in[kInSlots] = {nullptr, nullptr, nullptr};
    uint8_t *pin_out[kOutSlots] = {nullptr, nullptr};
    msj_carry *h_carries = nullptr;  // pinned: the carry after every chunk
    msj_carry *d_carries = nullptr;
    uint64_t n_carries = 0;
    hipStream_t s_up = nullptr, s_k = nullptr, s_down = nullptr;
    hipEvent_t ev_in[kInSlots] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_out[kOutSlots] = {nullptr, nullptr};
    std::vector<hipEvent_t> ev_chunk;
    GpuHostLocality where;            // the GPU's NUMA node and the CPUs of it this process may use
    CopyPool pool;
    bool ok = false;

    explicit HostPipe(int device) : where(gpu_locality(device)), pool(kCopyThreads, where.n_cpus > 0 ? &where.cpus : nullptr) {
        ok = true;
        // the rings: allocated (and touched) by a thread that runs on the GPU's node, so that first-touch placement puts
        // their pages there; the caller's thread keeps its own affinity
        std::thread([&] {
            (void)hipSetDevice(device);
            if (where.n_cpus > 0) (void)pthread_setaffinity_np(pthread_self(), sizeof(cpu_set_t), &where.cpus);
            for (auto &p : pin_in) {
                ok = ok && hip_ok(hipHostMalloc(reinterpret_cast<void **>(&p), kChunk, hipHostMallocDefault));
                if (ok) std::memset(p, 0, kChunk);
            }
            for (auto &p : pin_out) {
                ok = ok && hip_ok(hipHostMalloc(reinterpret_cast<void **>(&p), kPiece, hipHostMallocDefault));
                if (ok) std::memset(p, 0, kPiece);
            }
        }).join();
        ok = ok && hip_ok(hipStreamCreateWithFlags(&s_up, hipStreamNonBlocking)) &&
             hip_ok(hipStreamCreateWithFlags(&s_k, hipStreamNonBlocking)) &&
             hip_ok(hipStreamCreateWithFlags(&s_down, hipStreamNonBlocking));
        for (auto &e : ev_in) ok = ok && hip_ok(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (auto &e : ev_out) ok = ok && hip_ok(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    ~HostPipe() {
        for (auto p : pin_in)
            if (p) (void)hipHostFree(p);
        for (auto p : pin_out)
            if (p) (void)hipHostFree(p);
        if (h_carries) (void)hipHostFree(h_carries);
        if (d_carries) (void)hipFree(d_carries);
        for (auto e : ev_in)
            if (e) (void)hipEventDestroy(e);
        for (auto e : ev_out)
            if (e) (void)hipEventDestroy(e);
        for (auto e : ev_chunk) (void)hipEventDestroy(e);
        if (s_up) (void)hipStreamDestroy(s_up);
        if (s_k) (void)hipStreamDestroy(s_k);
        if (s_down) (void)hipStreamDestroy(s_down);
    }
    bool reserve(uint64_t nchunks) {
        if (nchunks + 1 > n_carries) {
            if (h_carries) (void)hipHostFree(h_carries);
            if (d_carries) (void)hipFree(d_carries);
            h_carries = nullptr;
            d_carries = nullptr;
            n_carries = 0;
            if (!hip_ok(hipHostMalloc(reinterpret_cast<void **>(&h_carries), (nchunks + 1) * sizeof(msj_carry), hipHostMallocDefault)) ||
                !hip_ok(hipMalloc(reinterpret_cast<void **>(&d_carries), (nchunks + 1) * sizeof(msj_carry))))
                return false;
            n_carries = nchunks + 1;
        }
        while (ev_chunk.size() < nchunks) {
            hipEvent_t e;
            if (!hip_ok(hipEventCreateWithFlags(&e, hipEventDisableTiming))) return false;
            ev_chunk.push_back(e);
        }
        return true;
    }
};

void host_pipe_destroy(HostPipe *pipe) { delete pipe; }

// The pipelined form of msj_stage1_ctx's device staging (ctx.h)
int32_t host_pipeline(msj_ctx *ctx, const uint8_t *buf, uint64_t len, uint32_t *idx_out, uint64_t dev_cap, uint32_t flags,
                      msj_carry *res) {
    if (ctx->pipe_fail_setup) return kPipeUnavailable;  // test hook (msj_debug_fail_pipeline_setup)
    if (!ctx->pipe) {
        ctx->pipe = new (std::nothrow) HostPipe(ctx->device);
        if (!ctx->pipe) return kPipeUnavailable;
    }
    HostPipe &P = *ctx->pipe;
    if (!P.ok) return kPipeUnavailable;
    uint8_t *const d_in = ctx->d_in.as<uint8_t>();
    uint32_t *const d_idx = ctx->d_idx.as<uint32_t>();
    const uint64_t chunk = HostPipe::kChunk;
    const uint64_t nchunks = (len + chunk - 1) / chunk;
    if (!P.reserve(nchunks)) return kPipeUnavailable;
    if (!hip_ok(hipMemsetAsync(&P.d_carries[0], 0, sizeof(msj_carry), P.s_k))) return kPipeUnavailable;

    static const bool trace = knob_set("MSJ_PIPE_TRACE");  // measurement build: where the call's time goes
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = now();
    std::vector<double> t_chunk_done(nchunks, 0.0), t_piece;
    // msj_host_register: a side whose caller memory is pinned needs no staging
    const bool in_pinned = P.direct_upload || ctx->is_pinned(buf, len);
    const bool out_pinned = ctx->is_pinned(idx_out, dev_cap * sizeof(uint32_t));
    // ---- the downloader: follows the chunks' cumulative counts, brings finished indices down in pieces
    int32_t down_rc = MSJ_SUCCESS;
    std::atomic<bool> abort{false};
    std::atomic<uint64_t> recorded{0};  // chunks whose event the uploader has recorded (an unrecorded event reads as done)
    std::thread down([&] {
        (void)hipSetDevice(ctx->device);
        uint64_t sent = 0, pieces = 0;
        std::atomic<int> copying[HostPipe::kOutSlots];
        for (auto &c : copying) c.store(0);
        for (uint64_t k = 0; k < nchunks; k++) {
            while (recorded.load(std::memory_order_acquire) <= k && !abort.load()) std::this_thread::yield();
            if (abort.load()) break;
            if (!hip_ok(hipEventSynchronize(P.ev_chunk[k]))) { down_rc = MSJ_ERR_HIP; break; }
            if (abort.load()) break;
            if (trace) t_chunk_done[k] = now() - t_begin;
            const msj_carry &c = P.h_carries[k + 1];
            const bool last = k + 1 == nchunks;
            uint64_t avail = c.count;
            if (last && (c.code == MSJ_SUCCESS || c.code == MSJ_EMPTY || c.code == MSJ_UTF8_ERROR)) avail += 3;  // the trailer
            if (avail > dev_cap) avail = dev_cap;
            if (out_pinned) {  // the caller's array is pinned: one DMA per chunk straight into it, nothing to wait for here
                if (avail > sent &&
                    !hip_ok(hipMemcpyAsync(idx_out + sent, d_idx + sent, (avail - sent) * sizeof(uint32_t), hipMemcpyDeviceToHost, P.s_down))) {
                    down_rc = MSJ_ERR_HIP;
                    break;
                }
                sent = avail;
                if (trace) t_piece.push_back(now() - t_begin);
                continue;
            }
            const uint64_t piece = HostPipe::kPiece / sizeof(uint32_t);
            while (sent < avail) {  // whatever this chunk added, in pieces of at most one slot
                // source and slot keep the same offset inside a 256-byte line: a DMA between differently aligned
                // ends runs at half the rate
                const uint64_t mis = sent & 63u;
                const uint64_t n = avail - sent < piece - mis ? avail - sent : piece - mis;
                const int slot = (int)(pieces % HostPipe::kOutSlots);
                CopyPool::wait(&copying[slot]);  // the piece that used this slot has been copied out
                // the DMA into the pinned slot (this call returns when it is done), then the copy into the
                // caller's memory by the pool while the next piece's DMA runs
                if (!hip_ok(hipMemcpyAsync(P.pin_out[slot], d_idx + (sent - mis), (n + mis) * sizeof(uint32_t), hipMemcpyDeviceToHost, P.s_down)) ||
                    !hip_ok(hipStreamSynchronize(P.s_down))) {
                    down_rc = MSJ_ERR_HIP;
                    break;
                }
                P.pool.copy_async(idx_out + sent, P.pin_out[slot] + mis * sizeof(uint32_t), n * sizeof(uint32_t), P.kParts, &copying[slot]);
                sent += n;
                pieces++;
                if (trace) t_piece.push_back(now() - t_begin);
            }
            if (down_rc != MSJ_SUCCESS) break;
        }
        for (auto &c : copying) CopyPool::wait(&c);
        if (out_pinned && !hip_ok(hipStreamSynchronize(P.s_down))) down_rc = MSJ_ERR_HIP;
    });
    // Whatever leaves this frame from here on (the staging pool's queue or a launch may throw std::bad_alloc, which
    // msj_stage1_ctx catches) leaves it with the downloader joined -- a joinable std::thread that is destroyed is
    // std::terminate -- and with nothing of this call left in the queues that still reads or writes caller memory
    struct JoinDown {
        std::thread &t;
        std::atomic<bool> &abort;
        HostPipe &P;
        ~JoinDown() {
            if (!t.joinable()) return;
            abort.store(true);
            t.join();
            (void)hipStreamSynchronize(P.s_k);
            (void)hipStreamSynchronize(P.s_up);
        }
    } join_down{down, abort, P};

    // ---- the uploader (this thread): pinned staging, H2D, one shard launch per chunk
    double t_copy = 0, t_wait = 0;
    int32_t rc = MSJ_SUCCESS;
    for (uint64_t k = 0; k < nchunks && rc == MSJ_SUCCESS; k++) {
        const uint64_t off = k * chunk, n = len - off < chunk ? len - off : chunk;
        const int slot = (int)(k % HostPipe::kInSlots);
        double t0 = now();
        if (in_pinned) {
            // the caller's pages are pinned (or MSJ_PIPE_DIRECT_UPLOAD: the runtime pins them in flight): no staging copy of ours
            if (!hip_ok(hipMemcpyAsync(d_in + off, buf + off, n, hipMemcpyHostToDevice, P.s_up))) rc = MSJ_ERR_HIP;
            t_copy += now() - t0;
        } else {
            if (k >= (uint64_t)HostPipe::kInSlots && !hip_ok(hipEventSynchronize(P.ev_in[slot]))) rc = MSJ_ERR_HIP;
            double t1 = now();
            if (rc == MSJ_SUCCESS) P.pool.copy(P.pin_in[slot], buf + off, n, P.kParts);
            t_wait += t1 - t0;
            t_copy += now() - t1;
            if (rc == MSJ_SUCCESS && !hip_ok(hipMemcpyAsync(d_in + off, P.pin_in[slot], n, hipMemcpyHostToDevice, P.s_up)))
                rc = MSJ_ERR_HIP;
        }
        if (rc == MSJ_SUCCESS && (!hip_ok(hipEventRecord(P.ev_in[slot], P.s_up)) || !hip_ok(hipStreamWaitEvent(P.s_k, P.ev_in[slot], 0))))
            rc = MSJ_ERR_HIP;
        if (rc == MSJ_SUCCESS)
            rc = enqueue_shard(ctx, d_in + off, n, d_idx, dev_cap, &P.d_carries[k], &P.d_carries[k + 1], nullptr, 0, nullptr,
                               k > 0, k + 1 == nchunks, false, len, P.s_k, flags, (uint32_t)off);
        if (rc == MSJ_SUCCESS &&
            (!hip_ok(hipMemcpyAsync(&P.h_carries[k + 1], &P.d_carries[k + 1], sizeof(msj_carry), hipMemcpyDeviceToHost, P.s_k)) ||
             !hip_ok(hipEventRecord(P.ev_chunk[k], P.s_k))))
            rc = MSJ_ERR_HIP;
        if (rc == MSJ_SUCCESS) recorded.store(k + 1, std::memory_order_release);
        if (rc != MSJ_SUCCESS) {
            // the downloader waits on every chunk's event: record the rest so that it can leave
            abort.store(true);
            for (uint64_t j = k; j < nchunks; j++) (void)hipEventRecord(P.ev_chunk[j], P.s_k);
        }
    }
    const double t_up = now();
    down.join();
    (void)hipStreamSynchronize(P.s_k);
    // a chunk whose upload was enqueued and whose launch then was not: no event ties that copy to s_k, and it reads the
    // caller's registered input (or a staging slot that the next call fills without a wait)
    if (rc != MSJ_SUCCESS) (void)hipStreamSynchronize(P.s_up);
    if (trace)
        std::fprintf(stderr, "msj host pipeline: %llu chunks, upload loop %.2f ms (slot waits %.2f, staging copies %.2f), "
                             "then %.2f ms until the last index was down\n",
                     (unsigned long long)nchunks, t_up - t_begin, t_wait, t_copy, now() - t_up);
    if (trace) {
        std::fprintf(stderr, "  chunk results seen at (ms):");
        for (double t : t_chunk_done) std::fprintf(stderr, " %.2f", t);
        std::fprintf(stderr, "\n  download pieces issued+previous copied out at (ms):");
        for (double t : t_piece) std::fprintf(stderr, " %.2f", t);
        std::fprintf(stderr, "\n");
    }
    ctx->last.valid = false;  // the chunk launches are not one call that msj_carry_fetch could re-issue
    if (rc != MSJ_SUCCESS) return rc;
    if (down_rc != MSJ_SUCCESS) return down_rc;
    *res = P.h_carries[nchunks];
    return MSJ_SUCCESS;
}
#pragma GCC visibility pop

extern "C" {

int32_t msj_host_placement(msj_ctx *ctx, char *out, uint64_t capacity) {
    if (!out || capacity == 0) return MSJ_ERR_BAD_ARGUMENT;
    std::unique_lock<std::mutex> lock(g_default_mutex, std::defer_lock);
    if (!ctx) {
        lock.lock();
        ctx = default_ctx_locked();
        if (!ctx) return MSJ_ERR_NO_DEVICE;
    }
    const GpuHostLocality g = ctx->pipe ? ctx->pipe->where : gpu_locality(ctx->device);
    const int ring_in = ctx->pipe ? numa_node_of(ctx->pipe->pin_in[0]) : -1, ring_out = ctx->pipe ? numa_node_of(ctx->pipe->pin_out[0]) : -1;
    int nodes = 0;
    for (;; nodes++) {
        char path[64];
        std::snprintf(path, sizeof path, "/sys/devices/system/node/node%d", nodes);
        if (access(path, F_OK) != 0) break;
    }
    const int n = std::snprintf(out, (size_t)capacity,
                                "{\"gpu_pci\": \"%s\", \"gpu_numa_node\": %d, \"numa_nodes\": %d, \"gpu_local_cpus_usable\": %d, "
                                "\"pipeline_created\": %s, \"copy_threads\": %d, \"copy_threads_bound_to_gpu_node\": %d, "
                                "\"ring_in_node\": %d, \"ring_out_node\": %d, \"pcie_link_speed\": \"%s\", \"pcie_link_width\": \"%s\"}",
                                g.pci, g.node, nodes, g.n_cpus, ctx->pipe ? "true" : "false", ctx->pipe ? ctx->pipe->kCopyThreads : 0,
                                ctx->pipe ? ctx->pipe->pool.bound : 0, ring_in, ring_out, g.link_speed, g.link_width);
    return (n < 0 || (uint64_t)n >= capacity) ? MSJ_CAPACITY : MSJ_SUCCESS;
}

int32_t msj_debug_numa_node_of(const void *host_ptr) { return numa_node_of(host_ptr); }

}  // extern "C"
