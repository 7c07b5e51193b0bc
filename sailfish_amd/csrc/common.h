// common.h -- shared host-side plumbing of libsfgpu (error slot, HIP checks, logging).
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/sfgpu.h"

namespace sfgpu {

void set_error(const char* fmt, ...);
void log_msg(int level, const char* fmt, ...);

inline hipStream_t as_stream(sfgpu_stream s) { return reinterpret_cast<hipStream_t>(s); }

// Caching device allocator: hipMalloc / hipFree cost tens of microseconds each and hipFree
// synchronises the whole device; a quantification step creates and drops ~60 scratch buffers.
// Blocks are rounded up to a power of two (>= 256 B) and kept in per-size free lists for reuse;
// sfgpu_pool_trim() returns them to the driver.  Callers free only after the work that used the
// block has been synchronised (handles synchronise their stream before releasing scratch).
hipError_t pool_malloc(void** p, size_t bytes);
void pool_free(void* p);
void pool_free_on(void* p, hipStream_t s);     // back to the cache once the work enqueued on s so far is done (no host wait)
void pool_free_on_many(void* const* ps, int n, hipStream_t s);      // ... several blocks behind ONE event (null entries are skipped)
void pool_trim();
void pool_set_large_limit(long long bytes);     // cached device blocks >= 1 GiB are kept up to this many bytes per device
template <typename T>
inline hipError_t pool_malloc(T** p, size_t bytes) { return pool_malloc(reinterpret_cast<void**>(p), bytes); }
// same recycling for pinned host blocks and for the handles' private non-blocking streams
hipError_t pinned_malloc(void** p, size_t bytes);
void pinned_free(void* p);
template <typename T>
inline hipError_t pinned_malloc(T** p, size_t bytes) { return pinned_malloc(reinterpret_cast<void**>(p), bytes); }
// device memory with the UNCACHED memory type (hipExtMallocWithFlags(.., hipDeviceMallocUncached)): no XCD's L2 ever holds a line of
// it, so what one workgroup stores is what every other workgroup's next load returns -- the exchange buffer of the persistent EM loop
// (em_persist.h).  Recycled like the other kinds (hipFree synchronises the device).
hipError_t uncached_malloc(void** p, size_t bytes);
void uncached_free(void* p);
template <typename T>
inline hipError_t uncached_malloc(T** p, size_t bytes) { return uncached_malloc(reinterpret_cast<void**>(p), bytes); }
hipError_t stream_acquire(hipStream_t* s);
void stream_release(hipStream_t s);

// HIP call -> SFGPU_ERR_HIP with the failing expression recorded.
#define SF_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            ::sfgpu::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return SFGPU_ERR_HIP;                                                            \
        }                                                                                    \
    } while (0)

#define SF_CHECK_LAUNCH() SF_HIP(hipGetLastError())

#define SF_REQUIRE(cond, code, msg)                 \
    do {                                            \
        if (!(cond)) {                              \
            ::sfgpu::set_error("%s", msg);          \
            return code;                            \
        }                                           \
    } while (0)

// grow-only device buffer (hipMalloc/hipFree are synchronising and slow: callers over-reserve)
template <typename T>
struct DevBuf {
    T* p = nullptr;
    uint64_t cap = 0;  // elements
    ~DevBuf() { if (p) pool_free(p); }
    int reserve(uint64_t n, hipStream_t s, bool keep, uint64_t used = 0) {
        if (n <= cap) return SFGPU_OK;
        uint64_t nc = cap ? cap : 1;
        while (nc < n) nc *= 2;
        T* q = nullptr;
        SF_HIP(pool_malloc(&q, nc * sizeof(T)));
        if (keep && p && used) SF_HIP(hipMemcpyAsync(q, p, used * sizeof(T), hipMemcpyDeviceToDevice, s));
        if (p) { SF_HIP(hipStreamSynchronize(s)); pool_free(p); }
        p = q; cap = nc;
        return SFGPU_OK;
    }
};

// waits for the stream when it goes out of scope.  Declare it AFTER the call's DevBufs: an early return then waits for the kernels
// before any scratch block goes back to the pool
struct StreamSyncOnExit { hipStream_t s; ~StreamSyncOnExit() { (void)hipStreamSynchronize(s); } };

// What a file-facing call (eqtext.hip, readtext.hip, textchunks.h, ...) borrows for its duration: streams, events and pinned host
// blocks.  None of them may go back while a copy can still touch a pinned block, so the scope waits for every stream before it
// gives anything back.  The same holds for the call's device scratch, and that cannot be read off the type: declare the scope
// AFTER the call's DevBufs, so that it is destroyed, and drains, BEFORE any scratch block returns to the pool (callers free only
// after the work is synchronised, see pool_malloc).
struct CallScope {
    static constexpr int kMaxStreams = 2, kMaxEvents = 15, kMaxPinned = 4;      // the largest users: readtext.hip, textchunks.h
    CallScope() = default;
    CallScope(const CallScope&) = delete;
    CallScope& operator=(const CallScope&) = delete;
    ~CallScope() {
        drain();
        for (int i = 0; i < n_events; ++i) (void)hipEventDestroy(events[i]);
        for (int i = 0; i < n_pinned; ++i) pinned_free(pinned[i]);
        for (int i = n_streams; i-- > 0;) if (owned[i]) stream_release(streams[i]);
    }
    // a stream of the call's own: drained and released by the scope
    hipError_t acquire(hipStream_t* s) {
        if (n_streams == kMaxStreams) return hipErrorOutOfMemory;
        const hipError_t e = stream_acquire(s);
        if (e == hipSuccess) { streams[n_streams] = *s; owned[n_streams++] = true; }
        return e;
    }
    // the caller's stream: only drained
    hipError_t adopt(hipStream_t s) {
        if (n_streams == kMaxStreams) return hipErrorOutOfMemory;
        streams[n_streams] = s; owned[n_streams++] = false;
        return hipSuccess;
    }
    hipError_t event(hipEvent_t* ev, unsigned flags = hipEventDefault) {
        if (n_events == kMaxEvents) return hipErrorOutOfMemory;
        const hipError_t e = hipEventCreateWithFlags(ev, flags);
        if (e == hipSuccess) events[n_events++] = *ev;
        return e;
    }
    template <typename T>
    hipError_t pinned_block(T** p, size_t bytes) {
        if (n_pinned == kMaxPinned) return hipErrorOutOfMemory;
        const hipError_t e = pinned_malloc(p, bytes);
        if (e == hipSuccess) pinned[n_pinned++] = *p;
        return e;
    }
    // waits for every stream, the last one handed out first: every user takes its compute stream, then its copy stream, and the
    // copy stream is drained before the compute stream
    void drain() {
        for (int i = n_streams; i-- > 0;) (void)hipStreamSynchronize(streams[i]);
    }

private:
    hipStream_t streams[kMaxStreams];
    bool owned[kMaxStreams];
    hipEvent_t events[kMaxEvents];
    void* pinned[kMaxPinned];
    int n_streams = 0, n_events = 0, n_pinned = 0;
};

inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// *ms += the time from event a to event b; false, and *ms as it was, when the query fails
inline bool add_elapsed(double* ms, hipEvent_t a, hipEvent_t b) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, a, b) != hipSuccess) return false;
    *ms += (double)t;
    return true;
}

// Tuning / experiment switches that lost their A/Bs (profiles/r*_notes.md name each) are read only by builds made with
// -DSFGPU_VARIANTS (tools/*_variants.sh -> csrc/variants/libsfgpu_<name>.so): the product library neither reads them nor contains the
// kernels they select.  The switches the product keeps are listed in include/sfgpu.h.
#ifdef SFGPU_VARIANTS
#define SF_DEV_ENV(name) getenv(name)
#else
#define SF_DEV_ENV(name) (static_cast<const char*>(nullptr))
#endif
// SFGPU_TIMING=1: the library says on stderr what its plans look like (dev)
inline bool env_timing() { static const bool on = getenv("SFGPU_TIMING") != nullptr; return on; }

constexpr int kWave = 64;  // gfx950 wavefront

}  // namespace sfgpu
