// uva_rt.h -- what every translation unit with C ABI entries shares on the host: the error channel behind uva_last_error, the
// HIP call wrappers, the makers of the handles of csrc/uva_own.h, the per-device tables and the one device check, and the fences that order a
// stateless stage's stream between two nets.  No device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <utility>

#include "uva_own.h"

struct uva_net;

namespace uva {

// records msg for uva_last_error (thread-local, defined in uva_api.hip) and returns 1
int fail(const std::string& msg);

inline int tryhip(hipError_t e, const char* what) { return e == hipSuccess ? 0 : fail(std::string(what) + ": " + hipGetErrorString(e)); }

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(std::string(#expr) + ": " + hipGetErrorString(e_));                    \
    } while (0)

// fills a handle: the buffer is made in a local and moved in once the copy is queued
template <typename T>
int upload(DevPtr<T>& dst, const void* src, size_t bytes, hipStream_t st)
{
    DevPtr<T> d;
    HIP_TRY(alloc_into(d, bytes));
    HIP_TRY(hipMemcpyAsync(d.get(), src, bytes, hipMemcpyHostToDevice, st));
    dst = std::move(d);
    return 0;
}

template <typename T>
int grow_dev(DevBuf<T>& b, size_t bytes) { return tryhip((hipError_t)b.grow(bytes), "hipMalloc"); }
template <typename T>
int grow_host(HostBuf<T>& b, size_t bytes) { return tryhip((hipError_t)b.grow(bytes), "hipHostMalloc"); }

inline bool is_pinned_host(const void* p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();   // an ordinary malloc'ed pointer: not an error
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// entries of the per-device context tables of the stateless stages (pixel formats, PNG, denoise 8 / 16, resize)
constexpr int kMaxDevices = 16;

// makes `device` current for a stateless stage, or says why not: no device at all, or none of that index (in the tables)
int select_device(int device);

// The per-device contexts of a stateless stage.  Ctx holds handles and a `Stream stream`; the table itself lives in storage
// that is never destroyed (`*new DeviceTable<Ctx>`: no HIP call at process exit).  The caller holds `mu` around every call.
template <typename Ctx>
struct DeviceTable {
    std::mutex mu;
    Ctx ctx[kMaxDevices];
    bool used[kMaxDevices] = {};
    Ctx& at(int device) { used[device] = true; return ctx[device]; }
    // makes `device` current and its context's stream exist
    int enter(int device, Ctx** out)
    {
        if (select_device(device)) return 1;
        Ctx& c = at(device);
        if (!c.stream) HIP_TRY(make_stream(c.stream));
        *out = &c;
        return 0;
    }
    // every used context: its device current, stream_of(device) -- where there is one -- waited for, the context reset
    template <typename S>
    void release_all(S stream_of)
    {
        for (int d = 0; d < kMaxDevices; ++d) {
            if (!used[d]) continue;
            (void)hipSetDevice(d);
            if (hipStream_t s = stream_of(d)) (void)hipStreamSynchronize(s);
            ctx[d] = Ctx();
            used[d] = false;
        }
    }
    void release_all() { release_all([this](int d) { return ctx[d].stream.get(); }); }
};

// the stages' teardown, every context of every device: uva_destroy_gpu_instance calls them in this order, after the nets
// and before resize_release_all (csrc/uva_resize.h)
void denoise16_release_all();    // (before denoise_release_all, which destroys the stream both use)
void denoise_release_all();
void png_release_all();
void pix_release_all();

// workgroups of a persistent kernel: one per CU, a multiple of the 8 XCDs
inline int persistent_grid(int ncu) { return std::max(8, (ncu / 8) * 8); }

// a stateless device stage (uva_*_device) between two nets' streams (csrc/uva_api.hip): both nets, where given, live on
// `device`; `stream` waits for what `after` has queued so far; what `before` queues from now on waits for `stream`
int check_fence_nets(int device, uva_net* after, uva_net* before, const char* entry);
int fence_after(uva_net* after, hipStream_t stream);
int fence_before(uva_net* before, hipStream_t stream);

}  // namespace uva
