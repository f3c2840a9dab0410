// uva_pixfmt.h -- the raw-video pixel formats (include/uva.h UVA_PIX_*): what csrc/uva_pixfmt.hip, a
// translation unit of its own, offers the rest of the library.  Frames are ffmpeg's rawvideo layouts, dense planes without row
// padding, chroma ceil(w/2) x ceil(h/2):
//   bgr24    [h][w][3] u8
//   yuv420p  Y [h][w] u8, then U [ch][cw], then V [ch][cw]
//   nv12     Y [h][w] u8, then [ch][cw][2] interleaved U, V
//   p010le   nv12's layout in 16-bit little-endian words, the 10-bit value in the high bits (v << 6)
//   yuv420p10le  yuv420p's layout in 16-bit little-endian words, the 10-bit value in the low bits
//   bgr48le  [h][w][3] u16 (unorm16): the 16-bit route's BGR (section 7.4)
//   yuv422p  Y [h][w] u8, then U [h][cw], then V [h][cw]: one chroma row per luma row (section 7.7)
//   yuv422p10le  yuv422p's layout in 16-bit little-endian words, the 10-bit value in the low bits
// The enums and pix_frame_bytes are plain C++ (csrc/uva_submit.cpp includes this header without HIP); the launchers sit behind
// __HIPCC__.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace uva {

enum { PIX_BGR24 = 0, PIX_YUV420P = 1, PIX_NV12 = 2, PIX_P010LE = 3, PIX_YUV420P10LE = 5, PIX_BGR48LE = 6, PIX_YUV422P = 7,
       PIX_YUV422P10LE = 8, PIX_NFMT = 9 };   // (4: never assigned)
// colour word: matrix in bit 0 (0 BT.601, 1 BT.709), bit 1 set = full ("pc") range, clear = limited ("tv") range; bit 2 set =
// chroma interpolated for its siting instead of replicated / box-averaged, the siting in bits 3 and 4
// (neither: left, as H.264 / HEVC video; bit 3: center; bit 4: topleft)
enum { PIX_CSP_BT601 = 0, PIX_CSP_BT709 = 1, PIX_RANGE_FULL = 2, PIX_CHROMA_BILINEAR = 4, PIX_CHROMA_CENTER = 8, PIX_CHROMA_TOPLEFT = 16,
       PIX_COLOUR_MASK = 31 };
// a siting bit needs the interpolation bit, and there is one siting
inline bool pix_colour_ok(int colour)
{
    if (colour & ~PIX_COLOUR_MASK) return false;
    const int loc = colour & (PIX_CHROMA_CENTER | PIX_CHROMA_TOPLEFT);
    return !loc || ((colour & PIX_CHROMA_BILINEAR) && loc != (PIX_CHROMA_CENTER | PIX_CHROMA_TOPLEFT));
}
// 0: replicate / box (sections 7.3, 7.4); 1: left; 2: center; 3: topleft
inline int pix_chroma_mode(int colour)
{
    if (!(colour & PIX_CHROMA_BILINEAR)) return 0;
    return colour & PIX_CHROMA_CENTER ? 2 : (colour & PIX_CHROMA_TOPLEFT ? 3 : 1);
}

// bytes of one dense h x w frame of `fmt`; 0 for an unknown format or a size <= 0
inline size_t pix_frame_bytes(int fmt, int h, int w)
{
    if (h <= 0 || w <= 0) return 0;
    const size_t wh = (size_t)w * h, c = 2 * ((size_t)(w + 1) / 2) * ((size_t)(h + 1) / 2), c422 = 2 * ((size_t)(w + 1) / 2) * (size_t)h;
    switch (fmt) {
    case PIX_BGR24: return 3 * wh;
    case PIX_YUV420P: case PIX_NV12: return wh + c;
    case PIX_P010LE: case PIX_YUV420P10LE: return 2 * (wh + c);
    case PIX_YUV422P: return wh + c422;
    case PIX_YUV422P10LE: return 2 * (wh + c422);
    case PIX_BGR48LE: return 6 * wh;
    default: return 0;
    }
}

}  // namespace uva

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace uva {

// bgr (dense u8 [h][w][3]) <- src of format fmt (a Y'CbCr format), on `stream`
hipError_t launch_pix_to_bgr(hipStream_t stream, int fmt, int colour, const void* src, uint8_t* bgr, int h, int w);
// dst of format fmt (a Y'CbCr format) <- bgr (dense u8 [h][w][3]), on `stream`
hipError_t launch_pix_from_bgr(hipStream_t stream, int fmt, int colour, const uint8_t* bgr, void* dst, int h, int w);
// the 16-bit route: bgr is dense u16 [h][w][3]; fmt is a Y'CbCr format or PIX_BGR24 (v * 257 in, rint(v / 257) out)
hipError_t launch_pix16_to_bgr(hipStream_t stream, int fmt, int colour, const void* src, uint16_t* bgr, int h, int w);
hipError_t launch_pix16_from_bgr(hipStream_t stream, int fmt, int colour, const uint16_t* bgr, void* dst, int h, int w);

// The four above by the net's sample width, errors through uva_last_error (csrc/uva_frames.hip; the submit stages use them too):
// the packed frame `src` of fmt -> the net's BGR frame `bgr` at `bits` (8: u8 [h][w][3], 16: u16) on `stream`, and back
int pix_to_native(hipStream_t stream, int bits, int fmt, int colour, const void* src, void* bgr, int h, int w);
int pix_from_native(hipStream_t stream, int bits, int fmt, int colour, const void* bgr, void* dst, int h, int w);

}  // namespace uva
#endif
