// uva_png.hip -- PNG encoding on the device (the kernels of csrc/uva_png.hip.h), their per-device tables, and the uva_png_*
// entries; the decode and zlib hooks forward to csrc/uva_pngread.cpp.
#include "../../include/uva.h"
#include "uva_png.hip.h"
#include "uva_pngread.h"
#include "uva_rt.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>

using namespace uva;

namespace {

// ---- PNG encoding on the device (uva_png.hip.h) ---------------------------------------------------
struct PngCodes {                  // the encoders' tables on one device, complete or absent (d_code says which)
    DevPtr<uint32_t> d_code;
    DevPtr<uint8_t> d_hdr;
    DevPtr<uint32_t> d_crcmul;
    DevPtr<uint32_t> d_code16;     // the 16-bit encoder's tables (png_tables16)
    DevPtr<uint8_t> d_hdr16;
};
struct PngDev : PngCodes {
    // the synchronous utility's own buffers
    DevBuf<uint8_t> d_frame, d_blocks;
    Stream stream;
};
// g_png.mu guards the table uploads, g_png_util_mu uva_png_deflate_u8's stream and frame buffer; one is never taken inside
// the other, except by png_release_all: the utility's first
std::mutex g_png_util_mu;
DeviceTable<PngDev>& g_png = *new DeviceTable<PngDev>;

template <typename T>
int png_table(DevPtr<T>& d, const void* src, size_t bytes)
{
    HIP_TRY(alloc_into(d, bytes));
    HIP_TRY(hipMemcpy(d.get(), src, bytes, hipMemcpyHostToDevice));
    return 0;
}

// the code tables of this device (uploaded on first use); the caller holds no lock
int png_dev(int device, PngDev** out)
{
    if (device < 0 || device >= kMaxDevices) return fail("bad device");
    std::lock_guard<std::mutex> lk(g_png.mu);
    PngDev& c = g_png.at(device);
    if (!c.d_code) {
        const PngTables& T = png_tables();
        const PngTables16& T16 = png_tables16();
        HIP_TRY(hipSetDevice(device));
        PngCodes t;
        if (png_table(t.d_code, T.code, sizeof T.code) || png_table(t.d_hdr, T.hdr, sizeof T.hdr) ||
            png_table(t.d_crcmul, T.crcmul, sizeof T.crcmul) || png_table(t.d_code16, T16.code, sizeof T16.code) ||
            png_table(t.d_hdr16, T16.hdr, sizeof T16.hdr)) return 1;
        HIP_TRY(hipFuncSetAttribute((const void*)png_deflate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, png_lds_bytes()));
        HIP_TRY(hipFuncSetAttribute((const void*)png_deflate_kernel16, hipFuncAttributeMaxDynamicSharedMemorySize, png_lds_bytes()));
        static_cast<PngCodes&>(c) = std::move(t);
    }
    *out = &c;
    return 0;
}

}  // namespace

void uva::png_release_all()
{
    std::lock_guard<std::mutex> lk2(g_png_util_mu);
    std::lock_guard<std::mutex> lk(g_png.mu);
    g_png.release_all();
}

// deflate the h x w u8 BGR frame at d_frame (HBM) into blocks at d_blocks (HBM, png_workspace_bytes(h, w)), on `stream`
int uva::png_launch(int device, hipStream_t stream, const uint8_t* d_frame, size_t stride, int h, int w, uint8_t* d_blocks)
{
    if (h <= 0 || w <= 0 || 3 * (long long)w + 1 > PNG_FILT_CAP) return fail("PNG encoder: frame width out of range");
    PngDev* c = nullptr;
    if (png_dev(device, &c)) return 1;
    PngArgs a;
    std::memset(&a, 0, sizeof a);
    a.src = d_frame; a.stride = stride; a.h = h; a.w = w;
    a.rows_per_block = png_rows_per_block(w);
    a.nblocks = png_num_blocks(h, w);
    a.code = c->d_code; a.hdr = c->d_hdr; a.crcmul = c->d_crcmul;
    for (int t = 0; t < PNG_TABLES; ++t) a.hdr_bits[t] = png_tables().hdr_bits[t];
    a.meta = (uint32_t*)d_blocks;
    a.slots = d_blocks + png_meta_bytes(h, w);
    hipLaunchKernelGGL(png_deflate_kernel, dim3(a.nblocks), dim3(PNG_THREADS), png_lds_bytes(), stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the same for an h x w u16 BGR frame (stride in bytes): png_deflate_kernel16 into png_workspace_bytes(h, w, 16)
int uva::png_launch16(int device, hipStream_t stream, const uint8_t* d_frame, size_t stride, int h, int w, uint8_t* d_blocks)
{
    if (!png_takes(h, w, 16)) return fail("PNG encoder: frame width out of range");
    if ((((uintptr_t)d_frame | stride) & 1) != 0) return fail("PNG encoder: odd address or stride of a 16-bit frame");
    PngDev* c = nullptr;
    if (png_dev(device, &c)) return 1;
    PngArgs16 a;
    std::memset(&a, 0, sizeof a);
    a.src = d_frame; a.stride = stride; a.h = h; a.w = w;
    a.rows_per_block = png_rows_per_block(w, 16);
    a.nblocks = png_num_blocks(h, w, 16);
    a.code = c->d_code16; a.hdr = c->d_hdr16; a.crcmul = c->d_crcmul;
    for (int t = 0; t < PNG_TABLES16; ++t) a.hdr_bits[t] = png_tables16().hdr_bits[t];
    a.meta = (uint32_t*)d_blocks;
    a.slots = d_blocks + png_meta_bytes(h, w, 16);
    hipLaunchKernelGGL(png_deflate_kernel16, dim3(a.nblocks), dim3(PNG_THREADS), png_lds_bytes(), stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the blocks at d_blocks, concatenated behind them (a device-to-device copy: microseconds), on `stream`
int uva::png_pack_launch(hipStream_t stream, uint8_t* d_blocks, int h, int w, int bits)
{
    PngPackArgs a;
    a.meta = (const uint32_t*)d_blocks;
    a.slots = d_blocks + png_meta_bytes(h, w, bits);
    a.nblocks = png_num_blocks(h, w, bits);
    a.out_meta = nullptr;
    a.out_data = png_packed(d_blocks, h, w, bits);
    hipLaunchKernelGGL(png_pack_kernel, dim3(a.nblocks), dim3(PNG_PACK_THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// meta + the first `bytes` packed bytes -> the page-locked workspace, by the copy engine, on `stream`
int uva::png_download(hipStream_t stream, const uint8_t* d_blocks, int h, int w, void* ws, size_t bytes, int bits)
{
    const size_t mb = png_meta_bytes(h, w, bits);
    HIP_TRY(hipMemcpyAsync(ws, d_blocks, mb, hipMemcpyDeviceToHost, stream));
    if (bytes) HIP_TRY(hipMemcpyAsync((uint8_t*)ws + mb, d_blocks + png_workspace_bytes(h, w, bits), bytes, hipMemcpyDeviceToHost, stream));
    return 0;
}

extern "C" {

size_t uva_png_workspace_bytes(int h, int w)
{
    if (h <= 0 || w <= 0 || 3 * (long long)w + 1 > PNG_FILT_CAP) return 0;
    return png_workspace_bytes(h, w);
}

int uva_png_assemble(const void* png_ws, int h, int w, uint8_t* out, size_t cap, size_t* len)
{
    if (!png_ws || uva_png_workspace_bytes(h, w) == 0) return fail("bad argument");
    std::string err;
    if (png_assemble((const uint8_t*)png_ws, h, w, out, cap, len, err)) return fail(err);
    return 0;
}

int uva_png_deflate_u8(int device, const uint8_t* bgr, int h, int w, size_t stride, void* png_ws, size_t png_ws_bytes)
{
    if (!bgr || stride < (size_t)w * 3) return fail("bad frame");
    if (uva_png_workspace_bytes(h, w) == 0) return fail("PNG encoder: frame width out of range");
    if (!is_pinned_host(png_ws)) return fail("PNG workspace must be page-locked host memory (uva_host_alloc)");
    PngDev* c = nullptr;
    if (png_dev(device, &c)) return 1;
    std::lock_guard<std::mutex> lk(g_png_util_mu);
    HIP_TRY(hipSetDevice(device));
    if (!c->stream) HIP_TRY(make_stream(c->stream));
    const size_t row = (size_t)w * 3;
    if (png_ws_bytes < png_workspace_bytes(h, w)) return fail("PNG workspace too small");
    if (grow_dev(c->d_frame, row * h) || grow_dev(c->d_blocks, png_device_bytes(h, w))) return 1;
    HIP_TRY(hipMemcpy2DAsync(c->d_frame, row, bgr, stride, row, h, hipMemcpyHostToDevice, c->stream));
    if (png_launch(device, c->stream, c->d_frame, row, h, w, c->d_blocks) || png_pack_launch(c->stream, c->d_blocks, h, w)) return 1;
    if (png_download(c->stream, c->d_blocks, h, w, png_ws, 0)) return 1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t total = png_total_bytes(png_ws, h, w);
    if (total > png_workspace_bytes(h, w) - png_meta_bytes(h, w)) return fail("PNG encoder: block sizes out of range");
    HIP_TRY(hipMemcpy((uint8_t*)png_ws + png_meta_bytes(h, w), png_packed(c->d_blocks, h, w), total, hipMemcpyDeviceToHost));
    return 0;
}

size_t uva_png_workspace_bytes16(int h, int w)
{
    if (!png_takes(h, w, 16)) return 0;
    return png_workspace_bytes(h, w, 16);
}

int uva_png_assemble16(const void* png_ws, int h, int w, uint8_t* out, size_t cap, size_t* len)
{
    if (!png_ws || uva_png_workspace_bytes16(h, w) == 0) return fail("bad argument");
    std::string err;
    if (png_assemble((const uint8_t*)png_ws, h, w, out, cap, len, err, 16)) return fail(err);
    return 0;
}

int uva_png_deflate_u16(int device, const uint16_t* bgr, int h, int w, size_t stride, void* png_ws, size_t png_ws_bytes)
{
    if (!bgr || stride < (size_t)w * 6 || (((uintptr_t)bgr | stride) & 1) != 0) return fail("bad frame");
    if (uva_png_workspace_bytes16(h, w) == 0) return fail("PNG encoder: frame width out of range");
    if (!is_pinned_host(png_ws)) return fail("PNG workspace must be page-locked host memory (uva_host_alloc)");
    PngDev* c = nullptr;
    if (png_dev(device, &c)) return 1;
    std::lock_guard<std::mutex> lk(g_png_util_mu);
    HIP_TRY(hipSetDevice(device));
    if (!c->stream) HIP_TRY(make_stream(c->stream));
    // (rows a multiple of 4 bytes apart on the device: the kernel then stages every width with dword loads)
    const size_t row = (size_t)w * 6, pitch = (row + 3) & ~(size_t)3;
    if (png_ws_bytes < png_workspace_bytes(h, w, 16)) return fail("PNG workspace too small");
    if (grow_dev(c->d_frame, pitch * h) || grow_dev(c->d_blocks, png_device_bytes(h, w, 16))) return 1;
    HIP_TRY(hipMemcpy2DAsync(c->d_frame, pitch, bgr, stride, row, h, hipMemcpyHostToDevice, c->stream));
    if (png_launch16(device, c->stream, c->d_frame, pitch, h, w, c->d_blocks) || png_pack_launch(c->stream, c->d_blocks, h, w, 16)) return 1;
    if (png_download(c->stream, c->d_blocks, h, w, png_ws, 0, 16)) return 1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t total = png_total_bytes(png_ws, h, w, 16);
    if (total > png_workspace_bytes(h, w, 16) - png_meta_bytes(h, w, 16)) return fail("PNG encoder: block sizes out of range");
    HIP_TRY(hipMemcpy((uint8_t*)png_ws + png_meta_bytes(h, w, 16), png_packed(c->d_blocks, h, w, 16), total, hipMemcpyDeviceToHost));
    return 0;
}

int uva_debug_png_deflate_host16(const uint16_t* bgr, int h, int w, size_t stride, void* png_ws, size_t png_ws_bytes)
{
    if (!bgr || !png_ws || stride < (size_t)w * 6 || uva_png_workspace_bytes16(h, w) == 0 || png_ws_bytes < png_workspace_bytes(h, w, 16))
        return fail("bad argument");
    png_deflate_host16((const uint8_t*)bgr, stride, h, w, (uint8_t*)png_ws);
    return 0;
}

int uva_png_decode_bgr16(const uint8_t* file, size_t len, uint16_t* out, size_t cap, int* h, int* w)
{
    if (!file) return fail("null file image");
    if (((uintptr_t)out & 1) != 0) return fail("odd address of a 16-bit frame");
    std::string err;
    int rc;
    try {
        rc = png_read_bgr16(file, len, out, cap, h, w, err);
    } catch (const std::exception& e) {              // out of memory: an error, not a crash across the C ABI
        return fail(std::string("PNG reader: ") + e.what());
    }
    if (rc == 1) return fail(err);
    if (rc == 2) { fail("PNG of a kind the reader does not take (palette, interlaced or below 8 bits)"); return 2; }
    return 0;
}

int uva_png_decode_bgr(const uint8_t* file, size_t len, uint8_t* out, size_t cap, int* h, int* w)
{
    if (!file) return fail("null file image");
    std::string err;
    int rc;
    try {
        rc = png_read_bgr(file, len, out, cap, h, w, err);
    } catch (const std::exception& e) {              // out of memory: an error, not a crash across the C ABI
        return fail(std::string("PNG reader: ") + e.what());
    }
    if (rc == 1) return fail(err);
    if (rc == 2) { fail("PNG of a kind the fast reader does not take (16-bit, palette or interlaced)"); return 2; }
    return 0;
}

int uva_debug_zlib_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t out_len)
{
    if (!in || (!out && out_len)) return fail("null argument");
    std::string err;
    if (zlib_decompress_exact(in, n, out, out_len, err)) return fail(err);
    return 0;
}

int uva_debug_png_deflate_host(const uint8_t* bgr, int h, int w, size_t stride, void* png_ws, size_t png_ws_bytes)
{
    if (!bgr || !png_ws || stride < (size_t)w * 3 || uva_png_workspace_bytes(h, w) == 0 || png_ws_bytes < png_workspace_bytes(h, w))
        return fail("bad argument");
    png_deflate_host(bgr, stride, h, w, (uint8_t*)png_ws);
    return 0;
}

}  // extern "C"
