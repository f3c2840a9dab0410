// uva_pixfmt.h -- the raw-video pixel formats (include/uva.h UVA_PIX_*): what csrc/uva_pixfmt.hip, a
// translation unit of its own, offers the rest of the library.  Frames are ffmpeg's rawvideo layouts, dense planes without row
// padding, chroma ceil(w/2) x ceil(h/2):
//   bgr24    [h][w][3] u8
//   yuv420p  Y [h][w] u8, then U [ch][cw], then V [ch][cw]
//   nv12     Y [h][w] u8, then [ch][cw][2] interleaved U, V
//   p010le   nv12's layout in 16-bit little-endian words, the 10-bit value in the high bits (v << 6)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace uva {

enum { PIX_BGR24 = 0, PIX_YUV420P = 1, PIX_NV12 = 2, PIX_P010LE = 3, PIX_NFMT = 4 };
// colour word: matrix in bit 0 (0 BT.601, 1 BT.709), bit 1 set = full ("pc") range, clear = limited ("tv") range
enum { PIX_CSP_BT601 = 0, PIX_CSP_BT709 = 1, PIX_RANGE_FULL = 2, PIX_COLOUR_MASK = 3 };

// bytes of one dense h x w frame of `fmt`; 0 for an unknown format or a size <= 0
size_t pix_frame_bytes(int fmt, int h, int w);

// bgr (dense u8 [h][w][3]) <- src of format fmt (!= PIX_BGR24), on `stream`
hipError_t launch_pix_to_bgr(hipStream_t stream, int fmt, int colour, const void* src, uint8_t* bgr, int h, int w);
// dst of format fmt (!= PIX_BGR24) <- bgr (dense u8 [h][w][3]), on `stream`
hipError_t launch_pix_from_bgr(hipStream_t stream, int fmt, int colour, const uint8_t* bgr, void* dst, int h, int w);

}  // namespace uva
