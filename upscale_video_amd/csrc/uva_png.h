// uva_png.h -- what the PNG encoder's translation unit (csrc/uva_png.hip: the kernels of csrc/uva_png.hip.h, their per-device
// tables and the uva_png_* entries) offers the submit stages and uva_net_collect_u8: the workspace layout and the launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace uva {

constexpr int PNG_TABLES = 4;
constexpr int PNG_FILT_CAP = 48 * 1024;                 // filtered bytes per block
constexpr int PNG_HDR_CAP = 256;                        // bytes reserved for a block's dynamic-Huffman header
constexpr int PNG_STAGE_BYTES = PNG_FILT_CAP * 9 / 8 + PNG_HDR_CAP + 64;   // the flattest table costs <= 9 bits per byte
constexpr int PNG_SLOT_BYTES = (PNG_STAGE_BYTES + 255) / 256 * 256;
constexpr int PNG_META_WORDS = 8;                       // per block: compressed bytes, Adler s1, Adler s2, filtered bytes, CRC-32 of
                                                        // the compressed bytes, the encoder's kind (0: 8-bit, 16: 16-bit), 2 spare

// Rows of one deflate block: its filtered bytes (3w + 1 per row) fit PNG_FILT_CAP, and its RAW rows -- staged in the
// `stage` area at a pitch of (3w + 3) & ~3 bytes before they are filtered -- fit PNG_STAGE_BYTES (for very narrow frames
// the pitch's padding makes that the tighter bound: w = 3, 4 900 rows would overrun the stage area into the tables).
// bits = 16: the 16-bit encoder's frames, 6 bytes per pixel (6w + 1 filtered, pitch (6w + 3) & ~3).
inline int png_rows_per_block(int w, int bits = 8)
{
    const int bpp = 3 * (bits / 8), rawp = (bpp * w + 3) & ~3;
    return std::max(1, std::min(PNG_FILT_CAP / (bpp * w + 1), PNG_STAGE_BYTES / rawp));
}
inline int png_num_blocks(int h, int w, int bits = 8) { const int r = png_rows_per_block(w, bits); return (h + r - 1) / r; }
// bytes of the workspace a frame needs, in HBM ([meta: nblocks x 32 B, padded to 4 KiB][nblocks slots]) and in page-locked
// host memory ([the same meta][the blocks' bytes, concatenated]: the same bound)
inline size_t png_meta_bytes(int h, int w, int bits = 8) { return ((size_t)png_num_blocks(h, w, bits) * PNG_META_WORDS * 4 + 4095) / 4096 * 4096; }
inline size_t png_workspace_bytes(int h, int w, int bits = 8) { return png_meta_bytes(h, w, bits) + (size_t)png_num_blocks(h, w, bits) * PNG_SLOT_BYTES; }
// frames the encoders take: one filtered row must fit a block
inline bool png_takes(int h, int w, int bits = 8) { return h > 0 && w > 0 && 3 * (bits / 8) * (long long)w + 1 <= PNG_FILT_CAP; }

// device layout of a frame's encoder output: [png_workspace_bytes(h, w): meta + slots][the same bound again: the packed bytes]
inline size_t png_device_bytes(int h, int w, int bits = 8) { return 2 * png_workspace_bytes(h, w, bits); }
inline uint8_t* png_packed(uint8_t* d_blocks, int h, int w, int bits = 8) { return d_blocks + png_workspace_bytes(h, w, bits); }

// packed bytes of the frame whose meta is in the workspace
inline size_t png_total_bytes(const void* ws, int h, int w, int bits = 8)
{
    const uint32_t* m = (const uint32_t*)ws;
    size_t t = 0;
    for (int b = 0, nb = png_num_blocks(h, w, bits); b < nb; ++b) t += m[(size_t)b * PNG_META_WORDS];
    return t;
}

// deflate the h x w u8 BGR frame at d_frame (HBM) into blocks at d_blocks (HBM, png_workspace_bytes(h, w)), on `stream`
int png_launch(int device, hipStream_t stream, const uint8_t* d_frame, size_t stride, int h, int w, uint8_t* d_blocks);
// the same for an h x w u16 BGR frame (stride in bytes): png_deflate_kernel16 into png_workspace_bytes(h, w, 16)
int png_launch16(int device, hipStream_t stream, const uint8_t* d_frame, size_t stride, int h, int w, uint8_t* d_blocks);
// the blocks at d_blocks, concatenated behind them (a device-to-device copy: microseconds), on `stream`
int png_pack_launch(hipStream_t stream, uint8_t* d_blocks, int h, int w, int bits = 8);
// meta + the first `bytes` packed bytes -> the page-locked workspace, by the copy engine, on `stream`
int png_download(hipStream_t stream, const uint8_t* d_blocks, int h, int w, void* ws, size_t bytes, int bits = 8);

}  // namespace uva
