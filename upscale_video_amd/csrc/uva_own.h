// uva_own.h -- who owns a HIP buffer, stream or event: a move-only handle that destroys what it holds, and a growing buffer
// (the pointer with its capacity).  The core below includes no HIP header -- tests/host/own_check.cpp compiles it with the
// host compiler and a counting policy; the HIP instances follow it (UVA_OWN_CORE_ONLY leaves them out).
//
// A handle converts to the raw pointer it holds, as a view: argument structs, launches and HIP calls take it as they took
// the raw member.  Handles destroy and never wait: whoever drops one that a stream may still use waits for that stream
// first, in a statement of its own.  No object of static storage holds a handle: the runtime is
// not called while the process exits.
#pragma once
#include <atomic>
#include <cstddef>
#include <type_traits>
#include <utility>

namespace uva {

// P, the policy of a kind of resource: static void destroy(T), static std::atomic<long long>& live() -- the handles of the
// kind that hold something -- and, for Buf, static int alloc(void**, size_t bytes) -> 0, or an error code
template <typename T, typename P>
class Owned {
    static_assert(std::is_pointer<T>::value, "a handle holds a pointer, or an opaque handle that is one");
    T p_ = nullptr;

public:
    Owned() = default;
    explicit Owned(T p) { reset(p); }
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    Owned& operator=(Owned&& o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_;
            o.p_ = nullptr;
        }
        return *this;
    }
    ~Owned() { reset(); }

    T get() const { return p_; }
    operator T() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    T operator->() const { return p_; }
    // destroys what it holds and takes over p
    void reset(T p = nullptr)
    {
        if (p_) {
            P::destroy(p_);
            --P::live();
        }
        p_ = p;
        if (p_) ++P::live();
    }
};

// A buffer that only grows: as the code it replaces did, a grow frees first and allocates then, and a failed allocation
// leaves the buffer empty with capacity 0.  Whoever grows a buffer that a stream may still use waits for that stream first.
template <typename T, typename P>
class Buf {
    Owned<T, P> p_;
    size_t cap_ = 0;

public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(std::move(o.p_)), cap_(o.cap_) { o.cap_ = 0; }
    Buf& operator=(Buf&& o) noexcept
    {
        if (this != &o) {
            p_ = std::move(o.p_);
            cap_ = o.cap_;
            o.cap_ = 0;
        }
        return *this;
    }
    T get() const { return p_.get(); }
    operator T() const { return p_.get(); }
    explicit operator bool() const { return (bool)p_; }
    size_t cap() const { return cap_; }
    int grow(size_t bytes)
    {
        if (cap_ >= bytes) return 0;
        reset();
        void* q = nullptr;
        if (const int rc = P::alloc(&q, bytes)) return rc;
        p_.reset((T)q);
        cap_ = bytes;
        return 0;
    }
    void reset()
    {
        p_.reset();
        cap_ = 0;
    }
};

}  // namespace uva

#ifndef UVA_OWN_CORE_ONLY
#include <hip/hip_runtime.h>

namespace uva {

// uva_debug_live_resources: the handles of the library that hold something -- device buffers, host buffers, streams, events
enum { LIVE_DEV, LIVE_HOST, LIVE_STREAM, LIVE_EVENT, LIVE_KINDS };
inline std::atomic<long long> g_live[LIVE_KINDS];

struct DevMem {
    static std::atomic<long long>& live() { return g_live[LIVE_DEV]; }
    static void destroy(void* p) { (void)hipFree(p); }
    static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
};
struct HostMem {                          // page-locked
    static std::atomic<long long>& live() { return g_live[LIVE_HOST]; }
    static void destroy(void* p) { (void)hipHostFree(p); }
    static int alloc(void** p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocDefault); }
};
struct StreamRes {
    static std::atomic<long long>& live() { return g_live[LIVE_STREAM]; }
    static void destroy(hipStream_t s) { (void)hipStreamDestroy(s); }
};
struct EventRes {
    static std::atomic<long long>& live() { return g_live[LIVE_EVENT]; }
    static void destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
};

template <typename T> using DevPtr = Owned<T*, DevMem>;
template <typename T> using HostPtr = Owned<T*, HostMem>;
template <typename T> using DevBuf = Buf<T*, DevMem>;
template <typename T> using HostBuf = Buf<T*, HostMem>;
using Stream = Owned<hipStream_t, StreamRes>;
using Event = Owned<hipEvent_t, EventRes>;

// the makers: into a local first, the handle changes only when the runtime gave something
template <typename T, typename P>
hipError_t alloc_into(Owned<T*, P>& h, size_t bytes)
{
    void* q = nullptr;
    const hipError_t e = (hipError_t)P::alloc(&q, bytes);
    if (e == hipSuccess) h.reset((T*)q);
    return e;
}
inline hipError_t make_stream(Stream& s)                       // (non-blocking, as every stream of the library is)
{
    hipStream_t q = nullptr;
    const hipError_t e = hipStreamCreateWithFlags(&q, hipStreamNonBlocking);
    if (e == hipSuccess) s.reset(q);
    return e;
}
inline hipError_t make_event(Event& ev, unsigned flags)
{
    hipEvent_t q = nullptr;
    const hipError_t e = hipEventCreateWithFlags(&q, flags);
    if (e == hipSuccess) ev.reset(q);
    return e;
}

}  // namespace uva
#endif  // UVA_OWN_CORE_ONLY
