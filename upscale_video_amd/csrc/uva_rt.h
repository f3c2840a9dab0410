// uva_rt.h -- what every translation unit with C ABI entries shares on the host: the error channel behind uva_last_error, the
// HIP call wrappers, the growing buffers, the per-device tables' size and the one device check, and the fences that order a
// stateless stage's stream between two nets.  No device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>

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

template <typename T>
int upload(T** dst, const void* src, size_t bytes, hipStream_t st)
{
    HIP_TRY(hipMalloc((void**)dst, bytes));
    HIP_TRY(hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, st));
    return 0;
}

template <typename T>
int grow_dev(T** p, size_t* cap, size_t bytes)
{
    if (*cap >= bytes) return 0;
    if (*p) HIP_TRY(hipFree(*p));
    *p = nullptr; *cap = 0;
    HIP_TRY(hipMalloc((void**)p, bytes));
    *cap = bytes;
    return 0;
}

inline int grow_host(uint8_t** p, size_t* cap, size_t bytes)
{
    if (*cap >= bytes) return 0;
    if (*p) HIP_TRY(hipHostFree(*p));
    *p = nullptr; *cap = 0;
    HIP_TRY(hipHostMalloc((void**)p, bytes, hipHostMallocDefault));
    *cap = bytes;
    return 0;
}

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
