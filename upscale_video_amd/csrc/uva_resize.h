// uva_resize.h -- the raw-video route's resampler (include/uva.h uva_resize*): what csrc/uva_resize.hip, a
// translation unit of its own, offers the rest of the library.  A frame of BGR samples (u8 or u16 [h][w][3], channels
// independent, code values as they are) is taken to oh x ow by a separable polyphase filter with integer taps that sum to 2^14.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace uva {

enum { RESIZE_LANCZOS = 0, RESIZE_BICUBIC = 1, RESIZE_BILINEAR = 2, RESIZE_NFILTER = 3 };
constexpr int RESIZE_ONE = 1 << 14;     // every row of a tap table sums to exactly this
constexpr int RESIZE_MAX_TAPS = 24;     // lanczos at the ratio limit 1/4

// null when (n_in -> n_out, filter) is an axis the resampler takes, else what is wrong with it
inline const char* resize_axis_error(int n_in, int n_out, int filter)
{
    if (filter < 0 || filter >= RESIZE_NFILTER) return "resize: unknown filter (0 lanczos, 1 bicubic, 2 bilinear)";
    if (n_in < 1 || n_out < 1) return "resize: sizes must be at least 1";
    if ((long long)n_out * 4 < n_in || (long long)n_out > (long long)n_in * 4) return "resize: the output / input ratio of an axis must lie within [1/4, 4]";
    return nullptr;
}
// taps per output sample, T = 2 ceil(a max(1, n_in / n_out)); 0 for an axis resize_axis_error refuses
int resize_ntaps(int n_in, int n_out, int filter);
// the table of one axis, host only: first[n_out], taps[n_out][T] (dense).  Returns T, 0 for a refused axis.
int resize_build_taps(int n_in, int n_out, int filter, std::vector<int32_t>& first, std::vector<int16_t>& taps);

// d_out (oh x ow, rows out_stride bytes apart) <- d_in (h x w, rows in_stride bytes apart) on `stream` of HIP device `device`
// (the current device); bits 8: u8 samples, 16: u16 samples (strides and addresses even).  The per-axis tables are built on the
// host once per (device, geometry, filter), uploaded and cached.  Returns 0, or non-zero with *err set.
int launch_resize(hipStream_t stream, int device, const void* d_in, int h, int w, size_t in_stride, void* d_out, int oh, int ow,
                  size_t out_stride, int filter, int bits, std::string* err);
// frees every cached table (uva_destroy_gpu_instance)
void resize_release_all();

}  // namespace uva
