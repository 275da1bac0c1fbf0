// A stand-in for the few HIP runtime calls deeploopcloser_amd/csrc/host_staging_impl.h makes, for the CPU sanitizer builds
// (ThreadSanitizer / AddressSanitizer + UBSan cannot run on the GPU of this pool).  What matters for a race detector is kept:
// hipMemcpyAsync is ASYNCHRONOUS -- every stream is a FIFO drained by its own "DMA" thread, which copies later, after a
// random pause -- so a pinned piece reused before its copy has run, or read back before its event, is a real data race
// here (and a wrong byte in the driver's comparison); events order through a mutex + condition variable, which the
// sanitizer understands.  "Device" memory is host memory.  Test infrastructure only.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <random>
#include <thread>

typedef int hipError_t;
constexpr hipError_t hipSuccess = 0;
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
constexpr unsigned hipHostMallocDefault = 0, hipEventDisableTiming = 2;
inline const char* hipGetErrorString(hipError_t) { return "stub error"; }

namespace hipstub {
struct Event {
    std::mutex m;
    std::condition_variable cv;
    unsigned long long recorded = 0, completed = 0;
};
struct Stream {
    std::mutex m;
    std::condition_variable cv, idle;
    std::deque<std::function<void()>> q;
    bool busy = false, stop = false;
    std::thread worker;
    Stream() : worker([this] { run(); }) {}
    ~Stream() {
        { std::lock_guard<std::mutex> lk(m); stop = true; }
        cv.notify_all();
        worker.join();
    }
    void run() {
        std::minstd_rand rng(12345);
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return stop || !q.empty(); });
                if (q.empty()) return;
                f = std::move(q.front());
                q.pop_front();
                busy = true;
            }
            if (rng() % 8 == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 40));   // the engine is late, sometimes
            f();
            {
                std::lock_guard<std::mutex> lk(m);
                busy = false;
            }
            idle.notify_all();
        }
    }
    void push(std::function<void()> f) {
        { std::lock_guard<std::mutex> lk(m); q.push_back(std::move(f)); }
        cv.notify_one();
    }
    void drain() {
        std::unique_lock<std::mutex> lk(m);
        idle.wait(lk, [&] { return q.empty() && !busy; });
    }
};
inline std::mutex& reg_lock() { static std::mutex m; return m; }
inline std::map<void*, std::unique_ptr<Stream>>& streams() { static std::map<void*, std::unique_ptr<Stream>> s; return s; }
inline Stream* stream_of(void* handle) {
    std::lock_guard<std::mutex> lk(reg_lock());
    auto& s = streams()[handle];
    if (!s) s.reset(new Stream);
    return s.get();
}
inline void shutdown() {
    std::lock_guard<std::mutex> lk(reg_lock());
    streams().clear();
}
}  // namespace hipstub

typedef void* hipStream_t;
typedef hipstub::Event* hipEvent_t;

inline hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
inline hipError_t hipSetDevice(int) { return hipSuccess; }
inline hipError_t hipHostMalloc(void** p, size_t n, unsigned) { *p = malloc(n); return *p ? hipSuccess : 1; }
inline hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = new hipstub::Event; return hipSuccess; }
inline hipError_t hipEventDestroy(hipEvent_t e) { delete e; return hipSuccess; }
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t st) {
    hipstub::stream_of(st)->push([=] { memcpy(dst, src, n); });
    return hipSuccess;
}
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t st) {
    unsigned long long seq;
    { std::lock_guard<std::mutex> lk(e->m); seq = ++e->recorded; }
    hipstub::stream_of(st)->push([=] {
        { std::lock_guard<std::mutex> lk(e->m); if (e->completed < seq) e->completed = seq; }
        e->cv.notify_all();
    });
    return hipSuccess;
}
inline hipError_t hipEventSynchronize(hipEvent_t e) {
    std::unique_lock<std::mutex> lk(e->m);
    const unsigned long long want = e->recorded;
    e->cv.wait(lk, [&] { return e->completed >= want; });
    return hipSuccess;
}
inline hipError_t hipDeviceSynchronize() {
    std::vector<hipstub::Stream*> all;
    {
        std::lock_guard<std::mutex> lk(hipstub::reg_lock());
        for (auto& kv : hipstub::streams()) all.push_back(kv.second.get());
    }
    for (auto* s : all) s->drain();
    return hipSuccess;
}

// ---- what dlc_internal.h gives the product build -----------------------------------------------------------------------
enum { DLC_OK = 0, DLC_ERR_BAD_ARG = -1, DLC_ERR_BAD_SHAPE = -2, DLC_ERR_UNSUPPORTED = -3, DLC_ERR_HIP = -4, DLC_ERR_WORKSPACE = -5 };
struct dlc_host_staging;
struct dlc_ctx {
    int device;
    char err[512];
    dlc_host_staging* staging;
    int host_threads;
    std::mutex* host_lock;
};
namespace dlc {
void staging_free(dlc_host_staging* s);
inline int fail(dlc_ctx* ctx, int status, const char* fmt, ...) {
    if (ctx) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
        va_end(ap);
    }
    return status;
}
struct DeviceGuard {
    bool ok = true;
    explicit DeviceGuard(int) {}
};
}  // namespace dlc
#define DLC_ON_DEVICE(ctx)                                                                                         \
    dlc::DeviceGuard guard((ctx)->device);                                                                         \
    if (!guard.ok) return dlc::fail((ctx), DLC_ERR_HIP, "hipSetDevice(%d) failed", (ctx)->device)
#define DLC_HIP_CHECK(ctx, expr)                                                                                   \
    do {                                                                                                           \
        hipError_t e__ = (expr);                                                                                   \
        if (e__ != hipSuccess) return dlc::fail((ctx), DLC_ERR_HIP, "%s failed (%s:%d)", #expr, __FILE__, __LINE__); \
    } while (0)
