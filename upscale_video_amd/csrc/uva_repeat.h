// uva_repeat.h -- the raw-video route's repeated-frame test (include/uva.h uva_frame_diff*, uva_net_set_skip_repeats; DESIGN.md
// section 7.8): what csrc/uva_repeat.hip, a translation unit of its own, offers the rest of the library.  Two packed frames of one
// pixel format are compared sample by sample, in code values as the input conversion reads them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace uva {

// what the kernel leaves in HBM: 32 bytes, zeroed by launch_frame_diff in front of the kernel
struct FrameDiffStats {
    unsigned long long over;      // samples with |a - b| > threshold
    unsigned long long max_abs;   // the largest |a - b|
    unsigned long long sad;       // the sum of |a - b|
    unsigned long long spare;
};

// how a sample of `fmt` is read: bytes per sample (1 or 2; 0 for an unknown format), and for the 16-bit words the shift and the
// mask in front of the difference (p010le: word >> 6; yuv420p10le / yuv422p10le: word & 1023; bgr48le: the whole word)
int frame_diff_sample(int fmt, unsigned* shift, unsigned* mask);

// *d_stats <- the three numbers for the frames d_a and d_b (`bytes` each, 16-byte aligned addresses) on `stream`: a memset of the
// record and one kernel.  threshold is in code values.
hipError_t launch_frame_diff(hipStream_t stream, const void* d_a, const void* d_b, size_t bytes, int fmt, unsigned threshold,
                             FrameDiffStats* d_stats);

}  // namespace uva
