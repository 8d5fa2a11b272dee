// fake_hip_device.h -- an asynchronous fake of the HIP entry points that csrc/host_pipe.cpp calls, for the CPU harness
// tests/cpp/host_pipe_sanitize.cpp.  TEST INFRASTRUCTURE: nothing here is part of the product, no GPU is involved.
//
//   memory    hipMalloc / hipHostMalloc are heap blocks of exactly the requested size (AddressSanitizer sees every bound),
//             filled with a byte that is no input and no index; hipFree / hipHostFree free them.
//   streams   a stream is a FIFO of operations.  hipMemcpyAsync / hipMemsetAsync (and the harness's fake shard launch, through
//             Device::enqueue) move bytes when the operation RUNS, never when it is enqueued.  hipStreamWaitEvent orders the
//             stream behind the event's latest record at the time of the call.
//   events    hipEventSynchronize waits for the latest record; an event that was never recorded reads as complete (HIP's
//             rule, which host_pipe.cpp relies on).
//   schedulers, chosen per run:
//     threaded  one worker thread per stream, seeded random yields and short sleeps between operations; operations run
//               outside the device's lock, so ThreadSanitizer sees the device's accesses as another thread's.
//     lazy      nothing runs until a host thread blocks in hipEventSynchronize / hipStreamSynchronize (/ hipDeviceSynchronize),
//               and then only what that wait requires, on the waiting thread.  Every DMA happens as late as the protocol
//               allows: a missing wait shows as wrong bytes, not as a lost race.
//   failures  every entry point counts (Device::entry); entry number fail_at of a call
//     kSync   returns hipErrorUnknown and does nothing else -- except that a synchronising call has still waited (a HIP wait
//             that reports a fault returns when the queue has stopped, not before), and that frees and destroys always work;
//     kAsync  (enqueueing calls only) returns hipSuccess, the operation moves nothing when it runs and poisons its stream:
//             events recorded behind it carry the error to the streams that wait for them, and every synchronising call
//             that covers it returns hipErrorUnknown until Device::clear_errors();
//     kThrow  launch number fail_at of the call (the harness's fake launch) throws std::bad_alloc, as a std::vector inside a
//             launch may.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

namespace fakehip {

#define FAKE_CHECK(cond, ...)                                                        \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                                       \
            std::fprintf(stderr, "\n");                                              \
            std::_Exit(1);                                                           \
        }                                                                            \
    } while (0)

enum class Sched { kLazy, kThreaded };
enum class Fail { kNone, kSync, kAsync, kThrow };

struct Stream;
struct Event {
    Stream *stream = nullptr;          // of the latest record
    uint64_t recorded = 0, done = 0;   // generation of the latest record; of the latest record that has completed
    bool err = false;                  // the latest completed record found its stream poisoned
};
struct Op {
    enum Kind { kRun, kRecord, kWait } kind = kRun;
    std::function<void()> fn;
    Event *ev = nullptr;
    uint64_t gen = 0;
    bool fail = false;  // kAsync
};
struct Stream {
    std::deque<Op> q;
    bool busy = false, err = false, stop = false;
    std::thread worker;
    std::mt19937_64 rng;
};

struct Device {
    std::mutex m;
    std::condition_variable cv;
    Sched sched = Sched::kLazy;
    std::mt19937_64 rng{1};
    std::vector<Stream *> streams;
    struct Block {
        size_t bytes;
        bool host;
    };
    std::map<void *, Block> blocks;
    int pci_mode = 1;  // hipDeviceGetPCIBusId: 0 fails, 1 names a device that has no sysfs entry
    // the call under test
    Fail fail = Fail::kNone;
    int64_t fail_at = -1;
    int64_t entry = 0;        // entry points called since begin_call
    int64_t enqueued = 0;     // operations enqueued since begin_call
    int64_t launches = 0;     // calls that may throw (the harness's launch) since begin_call
    bool injected = false;    // fail_at was reached by a call that this mode can fail
    const char *injected_into = "";
    // every device-to-host / host-to-device copy at the time it is enqueued (the harness checks sources and sizes)
    std::function<void(void *, const void *, size_t, hipMemcpyKind)> on_copy;

    static constexpr unsigned char kFill = 0xEE;

    void begin_call(Fail mode, int64_t at) {
        std::lock_guard<std::mutex> lk(m);
        fail = mode;
        fail_at = at;
        entry = enqueued = launches = 0;
        injected = false;
        injected_into = "";
    }
    // counts the entry point, decides whether this is the one that fails, and lets other threads run now and then
    bool enter(const char *name, bool sync_can_fail, bool async_can_fail, bool can_throw = false) {
        unsigned jitter;
        bool hit;
        {
            std::lock_guard<std::mutex> lk(m);
            if (fail == Fail::kThrow)
                hit = can_throw && launches++ == fail_at;
            else
                hit = entry == fail_at && ((fail == Fail::kSync && sync_can_fail) || (fail == Fail::kAsync && async_can_fail));
            entry++;
            if (hit) {
                injected = true;
                injected_into = name;
            }
            jitter = (unsigned)(rng() & 127);
        }
        pause(jitter);
        return hit;
    }
    static void pause(unsigned jitter) {
        if (jitter < 24) std::this_thread::yield();
        if (jitter < 8) std::this_thread::yield();
        if (jitter == 0) std::this_thread::sleep_for(std::chrono::microseconds(30));
    }

    // ---- running operations (m held)
    void marker(Stream *s, Op &op) {
        if (op.kind == Op::kRecord) {
            if (op.gen > op.ev->done) {
                op.ev->done = op.gen;
                op.ev->err = s->err;
            }
        } else if (op.ev->err) {
            s->err = true;
        }
    }
    // lazy: run s's operations on this thread until `enough` holds or the queue is empty
    void drive(Stream *s, const std::function<bool()> &enough) {
        while (!enough() && !s->q.empty()) {
            Op op = std::move(s->q.front());
            s->q.pop_front();
            if (op.kind == Op::kRun) {
                if (op.fail)
                    s->err = true;
                else
                    op.fn();
                continue;
            }
            if (op.kind == Op::kWait && op.ev->done < op.gen) {
                Event *e = op.ev;
                const uint64_t gen = op.gen;
                drive(e->stream, [e, gen] { return e->done >= gen; });
                FAKE_CHECK(e->done >= gen, "a stream waits for a record that nothing will complete");
            }
            marker(s, op);
        }
    }
    void worker(Stream *s) {
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
            cv.wait(lk, [&] {
                if (s->q.empty()) return s->stop;
                const Op &f = s->q.front();
                return f.kind != Op::kWait || f.ev->done >= f.gen;
            });
            if (s->q.empty()) return;
            Op op = std::move(s->q.front());
            s->q.pop_front();
            s->busy = true;
            if (op.kind == Op::kRun) {
                const unsigned jitter = (unsigned)(s->rng() & 31);
                lk.unlock();
                pause(jitter);
                if (!op.fail) op.fn();
                lk.lock();
                if (op.fail) s->err = true;
            } else {
                marker(s, op);
            }
            s->busy = false;
            cv.notify_all();
        }
    }
    void wait_until(std::unique_lock<std::mutex> &lk, Stream *s, const std::function<bool()> &enough) {
        if (sched == Sched::kLazy)
            drive(s, enough);
        else
            cv.wait(lk, [&] { return enough() || (s->q.empty() && !s->busy); });
    }
    void push(Stream *s, Op op) {
        enqueued++;
        s->q.push_back(std::move(op));
        if (sched == Sched::kThreaded) cv.notify_all();
    }
    // an operation with a body (a copy, a memset, the harness's launch)
    hipError_t enqueue(const char *name, hipStream_t stream, std::function<void()> fn, bool can_throw = false) {
        const bool hit = enter(name, true, true, can_throw);
        std::lock_guard<std::mutex> lk(m);
        if (hit && fail == Fail::kThrow) throw std::bad_alloc();
        if (hit && fail == Fail::kSync) return hipErrorUnknown;
        Op op;
        op.fn = std::move(fn);
        op.fail = hit;
        push(reinterpret_cast<Stream *>(stream), std::move(op));
        return hipSuccess;
    }
    // ---- the harness's side
    size_t pending() {
        std::lock_guard<std::mutex> lk(m);
        size_t n = 0;
        for (Stream *s : streams) n += s->q.size() + (s->busy ? 1 : 0);
        return n;
    }
    void drain() {
        std::unique_lock<std::mutex> lk(m);
        for (size_t k = 0; k < streams.size(); k++) {  // (a wait drives other streams; none enqueues)
            Stream *s = streams[k];
            wait_until(lk, s, [] { return false; });
        }
    }
    void clear_errors() {
        std::lock_guard<std::mutex> lk(m);
        for (Stream *s : streams) s->err = false;
    }
    // between calls: whatever a call left in pinned host memory (the carries, the rings) must not help the next one
    void poison_host_blocks(unsigned char byte) {
        std::lock_guard<std::mutex> lk(m);
        for (auto &b : blocks)
            if (b.second.host) std::memset(b.first, byte, b.second.bytes);
    }
    size_t live_blocks() {
        std::lock_guard<std::mutex> lk(m);
        return blocks.size();
    }
    hipError_t alloc(const char *name, void **out, size_t bytes, bool host) {
        if (enter(name, true, false)) return hipErrorUnknown;
        void *p = std::malloc(bytes ? bytes : 1);
        FAKE_CHECK(p, "out of memory");
        std::memset(p, kFill, bytes);
        std::lock_guard<std::mutex> lk(m);
        blocks[p] = Block{bytes, host};
        *out = p;
        return hipSuccess;
    }
    hipError_t release(const char *name, void *p, bool host) {
        (void)enter(name, false, false);
        {
            std::lock_guard<std::mutex> lk(m);
            auto it = blocks.find(p);
            FAKE_CHECK(it != blocks.end() && it->second.host == host, "%s of a block that is not live", name);
            blocks.erase(it);
        }
        std::free(p);
        return hipSuccess;
    }
};

inline Device &dev() {
    static Device d;
    return d;
}

}  // namespace fakehip

// ---- the entry points (host_pipe.cpp's undefined hip* symbols, and hipDeviceSynchronize for DeviceBuffer in ctx.h)
extern "C" {
hipError_t hipDeviceGetPCIBusId(char *out, int len, int) {
    fakehip::Device &d = fakehip::dev();
    if (d.enter("hipDeviceGetPCIBusId", true, false) || d.pci_mode == 0) return hipErrorUnknown;
    std::snprintf(out, (size_t)len, "FFFF:FE:1F.7");  // a well-formed address that no machine has
    return hipSuccess;
}
hipError_t hipGetLastError(void) {
    (void)fakehip::dev().enter("hipGetLastError", false, false);
    return hipSuccess;
}
hipError_t hipSetDevice(int) { return fakehip::dev().enter("hipSetDevice", true, false) ? hipErrorUnknown : hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned int) { return fakehip::dev().alloc("hipHostMalloc", p, n, true); }
hipError_t hipMalloc(void **p, size_t n) { return fakehip::dev().alloc("hipMalloc", p, n, false); }
hipError_t hipHostFree(void *p) { return fakehip::dev().release("hipHostFree", p, true); }
hipError_t hipFree(void *p) { return fakehip::dev().release("hipFree", p, false); }
hipError_t hipStreamCreateWithFlags(hipStream_t *out, unsigned int) {
    fakehip::Device &d = fakehip::dev();
    if (d.enter("hipStreamCreateWithFlags", true, false)) return hipErrorUnknown;
    fakehip::Stream *s = new fakehip::Stream();
    std::lock_guard<std::mutex> lk(d.m);
    s->rng.seed(d.rng());
    if (d.sched == fakehip::Sched::kThreaded) s->worker = std::thread([&d, s] { d.worker(s); });
    d.streams.push_back(s);
    *out = reinterpret_cast<hipStream_t>(s);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t stream) {
    fakehip::Device &d = fakehip::dev();
    (void)d.enter("hipStreamDestroy", false, false);
    fakehip::Stream *s = reinterpret_cast<fakehip::Stream *>(stream);
    {
        std::unique_lock<std::mutex> lk(d.m);
        d.wait_until(lk, s, [] { return false; });  // HIP lets the queued work finish
        s->stop = true;
        d.streams.erase(std::find(d.streams.begin(), d.streams.end(), s));
        d.cv.notify_all();
    }
    if (s->worker.joinable()) s->worker.join();
    delete s;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t stream) {
    fakehip::Device &d = fakehip::dev();
    const bool hit = d.enter("hipStreamSynchronize", true, false);
    fakehip::Stream *s = reinterpret_cast<fakehip::Stream *>(stream);
    std::unique_lock<std::mutex> lk(d.m);
    d.wait_until(lk, s, [] { return false; });
    const bool err = s->err;
    s->err = false;  // reported
    return hit || err ? hipErrorUnknown : hipSuccess;
}
hipError_t hipDeviceSynchronize(void) {
    fakehip::Device &d = fakehip::dev();
    const bool hit = d.enter("hipDeviceSynchronize", true, false);
    d.drain();
    return hit ? hipErrorUnknown : hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned int) {
    fakehip::Device &d = fakehip::dev();
    if (d.enter("hipStreamWaitEvent", true, false)) return hipErrorUnknown;
    fakehip::Event *e = reinterpret_cast<fakehip::Event *>(event);
    std::lock_guard<std::mutex> lk(d.m);
    if (e->recorded == 0) return hipSuccess;  // never recorded: nothing to wait for
    fakehip::Op op;
    op.kind = fakehip::Op::kWait;
    op.ev = e;
    op.gen = e->recorded;
    d.push(reinterpret_cast<fakehip::Stream *>(stream), std::move(op));
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *out, unsigned int) {
    if (fakehip::dev().enter("hipEventCreateWithFlags", true, false)) return hipErrorUnknown;
    *out = reinterpret_cast<hipEvent_t>(new fakehip::Event());
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t event) {
    fakehip::Device &d = fakehip::dev();
    (void)d.enter("hipEventDestroy", false, false);
    fakehip::Event *e = reinterpret_cast<fakehip::Event *>(event);
    {
        std::lock_guard<std::mutex> lk(d.m);
        FAKE_CHECK(e->done >= e->recorded, "an event is destroyed while a record of it is still queued");
    }
    delete e;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream) {
    fakehip::Device &d = fakehip::dev();
    if (d.enter("hipEventRecord", true, false)) return hipErrorUnknown;
    fakehip::Event *e = reinterpret_cast<fakehip::Event *>(event);
    std::lock_guard<std::mutex> lk(d.m);
    fakehip::Op op;
    op.kind = fakehip::Op::kRecord;
    op.ev = e;
    op.gen = ++e->recorded;
    e->stream = reinterpret_cast<fakehip::Stream *>(stream);
    d.push(e->stream, std::move(op));
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t event) {
    fakehip::Device &d = fakehip::dev();
    const bool hit = d.enter("hipEventSynchronize", true, false);
    fakehip::Event *e = reinterpret_cast<fakehip::Event *>(event);
    std::unique_lock<std::mutex> lk(d.m);
    const uint64_t gen = e->recorded;
    if (gen == 0) return hit ? hipErrorUnknown : hipSuccess;  // never recorded: complete
    d.wait_until(lk, e->stream, [e, gen] { return e->done >= gen; });
    FAKE_CHECK(e->done >= gen, "a host thread waits for a record that nothing will complete");
    return hit || e->err ? hipErrorUnknown : hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t stream) {
    fakehip::Device &d = fakehip::dev();
    if (d.on_copy) d.on_copy(dst, src, n, kind);
    return d.enqueue("hipMemcpyAsync", stream, [=] { std::memcpy(dst, src, n); });
}
hipError_t hipMemsetAsync(void *dst, int value, size_t n, hipStream_t stream) {
    return fakehip::dev().enqueue("hipMemsetAsync", stream, [=] { std::memset(dst, value, n); });
}
}  // extern "C"
