// uva_crop.h -- black-bar detection and cropped input frames on the raw-video route (include/uva.h uva_crop_*, uva_pix_window*,
// uva_net_set_input_window).  Two halves:
//   csrc/uva_crop_host.cpp  plain C++ without HIP: the bright-line scan over a frame's line sums, the running state's rectangle
//                           (ffmpeg cropdetect's rule as tests/cropdetect_ref.py states it), the window validator, the planes
//                           of a window and their staging layout.  Functions of their arguments; built alone by tests/test_crop_sanitized.py.
//   csrc/uva_crop.hip       the kernels: crop_sums_kernel (exact line sums of the luma plane or the packed BGR frame) and
//                           pix_window_kernel (the columns of a window compacted in HBM).
// This header is included by both, so the HIP declarations sit behind __HIPCC__.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace uva {

// ---- host only (uva_crop_host.cpp) ---------------------------------------------------------------------------------------
// The pixel-format codes of uva_pixfmt.h, restated so that the host file needs no HIP header (uva_crop.hip asserts they agree).
enum { CROP_BGR24 = 0, CROP_YUV420P = 1, CROP_NV12 = 2, CROP_P010LE = 3, CROP_YUV420P10LE = 5, CROP_BGR48LE = 6, CROP_YUV422P = 7,
       CROP_YUV422P10LE = 8 };

// how the detector reads a format: bytes per sample (1 / 2; 0: unknown format), the shift and mask in front of a 16-bit word, the
// depth of a code value (8 / 10 / 16) and the samples per pixel of a LINE (1: the luma plane; 3: packed BGR, all components)
struct CropSample {
    int bytes, shift, mask, depth, comps;
};
CropSample crop_sample(int fmt);

// first / last bright row and column of a frame from its line sums: bounds = {first row, last row, first column, last column},
// -1 where no line is bright.  A line of n samples with sum S is bright iff floor(S / n) > limit << (depth - 8).
// Returns nullptr, or what is wrong with the arguments.
const char* crop_bounds(const unsigned long long* rows, const unsigned long long* cols, int fmt, int h, int w, int limit, int bounds[4]);

// state {x1, y1, x2, y2} and `round` -> rect {w, h, x, y}; returns false when there is no rectangle
bool crop_rect(const int state[4], int round, int rect[4]);

// the window h x w at (x, y) of a src_h x src_w frame of fmt: nullptr, or why it is refused
const char* crop_window_error(int fmt, int src_h, int src_w, int x, int y, int h, int w);

// the planes of a window: for plane p the rows [row0, row0 + rows) of the source plane at byte src_off (rows of src_row bytes),
// of each the bytes [xbytes, xbytes + dst_row), go to byte dst_off of the dense h x w frame as rows of dst_row bytes
struct WindowPlane {
    size_t src_off, dst_off;
    size_t src_row, dst_row, xbytes;
    int row0, rows;
};
// fills planes[3], returns how many there are (0: unknown format)
int crop_window_planes(int fmt, int src_h, int src_w, int x, int y, int h, int w, WindowPlane planes[3]);

// bytes of the staging that launch_pix_window reads for these planes: every plane's row range at full width, each starting at a
// multiple of 16 bytes; stage_off[p] receives plane p's offset there
size_t pix_window_staging(const WindowPlane* planes, int n, size_t stage_off[3]);

}  // namespace uva

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace uva {

// row_sums[h], col_sums[w] (unsigned long long, in HBM, zeroed here) <- the line sums of the frame at d_frame (16-byte aligned:
// its luma plane, or all of a packed BGR frame, comes first) on `stream`: two memsets and one kernel.  max_groups > 0 bounds the
// grid below the kernel's own bound (tests: the grid-stride walk on a small frame).
hipError_t launch_crop_sums(hipStream_t stream, const void* d_frame, int fmt, int h, int w, unsigned long long* d_rows,
                            unsigned long long* d_cols, int max_groups = 0);

// d_dst (dense window frame, 16-byte aligned) <- the planes' window rows, of which plane p's first lies at byte stage_off[p] of
// d_stage at full width (pix_window_staging's layout, or a whole source frame: src_off + row0 * src_row), the columns compacted,
// on `stream`: one kernel.  bytes: bytes per sample (1 / 2).
hipError_t launch_pix_window(hipStream_t stream, const void* d_stage, const size_t* stage_off, void* d_dst, const WindowPlane* planes, int n,
                             int bytes);

}  // namespace uva
#endif
