// uva_frames.hip -- the stateless frame stages of the raw-video route outside a net: pixel formats, the resampler, repeated
// frames, crop detection, the input window, deinterlacing and inverse telecine.  Host code only: it calls the launchers of csrc/uva_pixfmt.hip,
// csrc/uva_resize.hip, csrc/uva_repeat.hip, csrc/uva_crop.hip, csrc/uva_deint.hip and csrc/uva_ivtc.hip on a per-device stream of its own.
#include "../../include/uva.h"
#include "uva_crop.h"
#include "uva_deint.h"
#include "uva_ivtc.h"
#include "uva_pixfmt.h"
#include "uva_repeat.h"
#include "uva_resize.h"
#include "uva_rt.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

using namespace uva;

// ---- raw-video pixel formats outside a net (uva_pix_convert, uva_pix_convert_device; csrc/uva_pixfmt.hip) -----------
namespace {

struct PixCtx {                          // per device: the conversions' own stream and buffers
    DevBuf<uint8_t> d_in, d_mid, d_out;
    DevPtr<FrameDiffStats> d_stats;      // uva_frame_diff's record
    DevBuf<unsigned long long> d_sums;   // uva_crop_sums' line sums: rows, then columns
    Stream stream;
};
DeviceTable<PixCtx>& g_pix = *new DeviceTable<PixCtx>;

int pix_ctx(int device, PixCtx** out) { return g_pix.enter(device, out); }

// uva_pix_convert_device is asynchronous: frames queued on the stream may still use a buffer about to be replaced
int pix_grow(PixCtx& c, DevBuf<uint8_t>& b, size_t bytes)
{
    if (b.cap() >= bytes) return 0;
    if (b.cap()) HIP_TRY(hipStreamSynchronize(c.stream));
    return grow_dev(b, bytes);
}

int pix_check(const void* in, int in_fmt, const void* out, int out_fmt, int h, int w, int colour, bool u16 = false)
{
    if (!in || !out) return fail("null frame pointer");
    if (h <= 0 || w <= 0 || (long long)h * w > (1ll << 28)) return fail("bad image size");
    if (!pix_frame_bytes(in_fmt, 1, 1) || !pix_frame_bytes(out_fmt, 1, 1)) return fail("unknown pixel format");
    if (!u16 && (in_fmt == PIX_BGR48LE || out_fmt == PIX_BGR48LE)) return fail("bgr48le is a 16-bit format: use the 16-bit entries (uva_pix_convert16)");
    if (!pix_colour_ok(colour)) return fail("bad colour word");
    return 0;
}

// d_in (in_fmt) -> d_out (out_fmt) on the context's stream, through the BGR of `bits` (BGR24 / BGR48LE) in d_mid when neither end
// is that
int pix_convert_launch(PixCtx& c, int bits, const uint8_t* d_in, int in_fmt, uint8_t* d_out, int out_fmt, int h, int w, int colour)
{
    const int native = bits == 16 ? PIX_BGR48LE : PIX_BGR24;
    if (in_fmt == out_fmt) {
        HIP_TRY(hipMemcpyAsync(d_out, d_in, pix_frame_bytes(in_fmt, h, w), hipMemcpyDeviceToDevice, c.stream));
        return 0;
    }
    if (in_fmt == native) return pix_from_native(c.stream, bits, out_fmt, colour, d_in, d_out, h, w);
    if (out_fmt == native) return pix_to_native(c.stream, bits, in_fmt, colour, d_in, d_out, h, w);
    if (pix_grow(c, c.d_mid, pix_frame_bytes(native, h, w))) return 1;
    return pix_to_native(c.stream, bits, in_fmt, colour, d_in, c.d_mid, h, w) ||
           pix_from_native(c.stream, bits, out_fmt, colour, c.d_mid, d_out, h, w);
}

// uva_pix_convert / uva_pix_convert16: one frame, host to host
int pix_convert_host(int device, int bits, const void* in, int in_fmt, void* out, int out_fmt, int h, int w, int colour)
{
    if (pix_check(in, in_fmt, out, out_fmt, h, w, colour, bits == 16)) return 1;
    std::lock_guard<std::mutex> lk(g_pix.mu);
    PixCtx* c = nullptr;
    if (pix_ctx(device, &c)) return 1;
    const size_t nin = pix_frame_bytes(in_fmt, h, w), nout = pix_frame_bytes(out_fmt, h, w);
    if (pix_grow(*c, c->d_in, nin) || pix_grow(*c, c->d_out, nout)) return 1;
    HIP_TRY(hipMemcpyAsync(c->d_in, in, nin, hipMemcpyHostToDevice, c->stream));
    if (pix_convert_launch(*c, bits, c->d_in, in_fmt, c->d_out, out_fmt, h, w, colour)) return 1;
    HIP_TRY(hipMemcpyAsync(out, c->d_out, nout, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace

void uva::pix_release_all()
{
    std::lock_guard<std::mutex> lk(g_pix.mu);
    g_pix.release_all();
}

// the packed frame `src` of fmt -> the net's BGR frame `bgr` at `bits` (8: u8 [h][w][3], 16: u16) on `stream` ...
int uva::pix_to_native(hipStream_t stream, int bits, int fmt, int colour, const void* src, void* bgr, int h, int w)
{
    return bits == 16 ? tryhip(launch_pix16_to_bgr(stream, fmt, colour, src, (uint16_t*)bgr, h, w), "pix16_to_bgr")
                      : tryhip(launch_pix_to_bgr(stream, fmt, colour, src, (uint8_t*)bgr, h, w), "pix_to_bgr");
}

// ... and back
int uva::pix_from_native(hipStream_t stream, int bits, int fmt, int colour, const void* bgr, void* dst, int h, int w)
{
    return bits == 16 ? tryhip(launch_pix16_from_bgr(stream, fmt, colour, (const uint16_t*)bgr, dst, h, w), "pix16_from_bgr")
                      : tryhip(launch_pix_from_bgr(stream, fmt, colour, (const uint8_t*)bgr, dst, h, w), "pix_from_bgr");
}

extern "C" {

size_t uva_pix_frame_bytes(int fmt, int h, int w) { return pix_frame_bytes(fmt, h, w); }

int uva_pix_convert(int device, const void* in, int in_fmt, void* out, int out_fmt, int h, int w, int colour)
{
    return pix_convert_host(device, 8, in, in_fmt, out, out_fmt, h, w, colour);
}

int uva_pix_convert_device(int device, const void* d_in, int in_fmt, void* d_out, int out_fmt, int h, int w, int colour,
                           uva_net* after, uva_net* before)
{
    if (pix_check(d_in, in_fmt, d_out, out_fmt, h, w, colour)) return 1;
    if (check_fence_nets(device, after, before, "uva_pix_convert_device")) return 1;
    std::lock_guard<std::mutex> lk(g_pix.mu);
    PixCtx* c = nullptr;
    if (pix_ctx(device, &c)) return 1;
    if (fence_after(after, c->stream)) return 1;
    if (pix_convert_launch(*c, 8, (const uint8_t*)d_in, in_fmt, (uint8_t*)d_out, out_fmt, h, w, colour)) return 1;
    if (fence_before(before, c->stream)) return 1;
    return 0;
}

int uva_pix_convert16(int device, const void* in, int in_fmt, void* out, int out_fmt, int h, int w, int colour)
{
    return pix_convert_host(device, 16, in, in_fmt, out, out_fmt, h, w, colour);
}

// ---- the resampler (csrc/uva_resize.hip) ----------------------------------------------------------
int uva_resize_taps(int n_in, int n_out, int filter, int32_t* first, int16_t* taps, size_t cap, int* ntaps)
{
    if (const char* e = resize_axis_error(n_in, n_out, filter)) return fail(e);
    const int t = resize_ntaps(n_in, n_out, filter);
    if (ntaps) *ntaps = t;
    if (!first || !taps || cap < (size_t)n_out * t) return fail("uva_resize_taps: the table needs n_out firsts and n_out * ntaps taps");
    std::vector<int32_t> f;
    std::vector<int16_t> tp;
    if (resize_build_taps(n_in, n_out, filter, f, tp) != t) return fail("uva_resize_taps: the taps of a row do not fit");
    std::copy(f.begin(), f.end(), first);
    std::copy(tp.begin(), tp.end(), taps);
    return 0;
}

namespace {
int resize_check(const void* in, int h, int w, size_t in_stride, const void* out, int oh, int ow, size_t out_stride, int filter, int bits)
{
    if (!in || !out) return fail("null frame pointer");
    if (bits != 8 && bits != 16) return fail("resize: bits must be 8 or 16");
    if (const char* e = resize_axis_error(h, oh, filter)) return fail(e);
    if (const char* e = resize_axis_error(w, ow, filter)) return fail(e);
    if ((long long)h * w > (1ll << 28) || (long long)oh * ow > (1ll << 28)) return fail("bad image size");
    const size_t bps = bits / 8;
    if (in_stride < (size_t)w * 3 * bps || out_stride < (size_t)ow * 3 * bps) return fail("row stride too small");
    if (bits == 16 && ((((uintptr_t)in | (uintptr_t)out | in_stride | out_stride) & 1) != 0)) return fail("16-bit frames need 2-byte aligned rows");
    return 0;
}
}  // namespace

int uva_resize_device(int device, const void* d_in, int h, int w, size_t in_stride, void* d_out, int oh, int ow, size_t out_stride,
                      int filter, int bits, uva_net* after, uva_net* before)
{
    if (resize_check(d_in, h, w, in_stride, d_out, oh, ow, out_stride, filter, bits)) return 1;
    if (check_fence_nets(device, after, before, "uva_resize_device")) return 1;
    std::lock_guard<std::mutex> lk(g_pix.mu);
    PixCtx* c = nullptr;
    if (pix_ctx(device, &c)) return 1;
    if (fence_after(after, c->stream)) return 1;
    std::string err;
    if (launch_resize(c->stream, device, d_in, h, w, in_stride, d_out, oh, ow, out_stride, filter, bits, &err)) return fail(err);
    if (fence_before(before, c->stream)) return 1;
    return 0;
}

int uva_resize(int device, const void* in, int h, int w, size_t in_stride, void* out, int oh, int ow, size_t out_stride, int filter,
               int bits)
{
    if (resize_check(in, h, w, in_stride, out, oh, ow, out_stride, filter, bits)) return 1;
    std::lock_guard<std::mutex> lk(g_pix.mu);
    PixCtx* c = nullptr;
    if (pix_ctx(device, &c)) return 1;
    // the frames go up and come down with their row padding, so that the kernel works on the caller's strides; a padded
    // result buffer goes up first (what lies between its rows comes back as it was)
    const size_t in_row = (size_t)w * 3 * (bits / 8), out_row = (size_t)ow * 3 * (bits / 8);
    const size_t nin = in_stride * (size_t)(h - 1) + in_row, nout = out_stride * (size_t)(oh - 1) + out_row;
    if (pix_grow(*c, c->d_in, nin) || pix_grow(*c, c->d_out, nout)) return 1;
    HIP_TRY(hipMemcpyAsync(c->d_in, in, nin, hipMemcpyHostToDevice, c->stream));
    if (out_stride != out_row) HIP_TRY(hipMemcpyAsync(c->d_out, out, nout, hipMemcpyHostToDevice, c->stream));
    std::string err;
    if (launch_resize(c->stream, device, c->d_in, h, w, in_stride, c->d_out, oh, ow, out_stride, filter, bits, &err)) return fail(err);
    HIP_TRY(hipMemcpyAsync(out, c->d_out, nout, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- repeated frames (csrc/uva_repeat.hip) ---------------------------------------------------------
namespace {
int frame_diff_check(const void* a, const void* b, int fmt, int h, int w, int threshold, const unsigned long long* stats)
{
    if (!a || !b || !stats) return fail("null frame pointer");
    if (h <= 0 || w <= 0 || (long long)h * w > (1ll << 28)) return fail("bad image size");
    if (!pix_frame_bytes(fmt, 1, 1) || !frame_diff_sample(fmt, nullptr, nullptr)) return fail("unknown pixel format");
    if (threshold < 0 || threshold > 65535) return fail("uva_frame_diff: the threshold is 0 ... 65535 code values");
    return 0;
}

// the record of the frames d_a, d_b on the conversions' stream, read back and waited for (g_pix.mu held)
int frame_diff_run(PixCtx& c, const void* d_a, const void* d_b, int fmt, int h, int w, int threshold, unsigned long long* stats)
{
    if (!c.d_stats) HIP_TRY(alloc_into(c.d_stats, sizeof(FrameDiffStats)));
    FrameDiffStats st;
    HIP_TRY(launch_frame_diff(c.stream, d_a, d_b, pix_frame_bytes(fmt, h, w), fmt, (unsigned)threshold, c.d_stats));
    HIP_TRY(hipMemcpyAsync(&st, c.d_stats, sizeof st, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    stats[0] = st.over; stats[1] = st.max_abs; stats[2] = st.sad;
    return 0;
}
}  // namespace

int uva_frame_diff(int device, const void* a, const void* b, int fmt, int h, int w, int threshold, unsigned long long* stats)
{
    if (frame_diff_check(a, b, fmt, h, w, threshold, stats)) return 1;
    std::lock_guard<std::mutex> lk(g_pix.mu);
    PixCtx* c = nullptr;
    if (pix_ctx(device, &c)) return 1;
    const size_t bytes = pix_frame_bytes(fmt, h, w);
    if (pix_grow(*c, c->d_in, bytes) || pix_grow(*c, c->d_out, bytes)) return 1;
    HIP_TRY(hipMemcpyAsync(c->d_in, a, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_out, b, bytes, hipMemcpyHostToDevice, c->stream));
    return frame_diff_run(*c, c->d_in, c->d_out, fmt, h, w, threshold, stats);
}

int uva_frame_diff_device(int device, const void* d_a, const void* d_b, int fmt, int h, int w, int threshold, unsigned long long* stats)
{
    if (frame_diff_check(d_a, d_b, fmt, h, w, threshold, stats)) return 1;
    if ((((uintptr_t)d_a | (uintptr_t)d_b) & 15) != 0) return fail("uva_frame_diff_device: the frames must start at 16-byte aligned addresses");
    std::lock_guard<std::mutex> lk(g_pix.mu);
    PixCtx* c = nullptr;
    if (pix_ctx(device, &c)) return 1;
    return frame_diff_run(*c, d_a, d_b, fmt, h, w, threshold, stats);
}

// ---- crop detection and the input window (csrc/uva_crop.hip, csrc/uva_crop_host.cpp) ------------------
namespace {
int crop_sums_check(const void* frame, int fmt, int h, int w, const unsigned long long* rows, const unsigned long long* cols)
{
    if (!frame || !rows || !cols) return fail("null frame pointer");
    if (!crop_sample(fmt).bytes || !pix_frame_bytes(fmt, 1, 1)) return fail("unknown pixel format");
    if (h < 1 || w < 1 || (long long)h * w > (1ll << 28)) return fail("bad image size");
    return 0;
}

// the bytes of a frame that the detector reads: the luma plane, which comes first, or all of a packed BGR frame
size_t crop_read_bytes(int fmt, int h, int w)
{
    const CropSample cs = crop_sample(fmt);
    return (size_t)h * w * cs.comps * cs.bytes;
}

// the line sums of d_frame on the conversions' stream, read back and waited for (g_pix.mu held)
int crop_sums_run(PixCtx& c, const void* d_frame, int fmt, int h, int w, unsigned long long* rows, unsigned long long* cols, int max_groups)
{
    const size_t need = sizeof(unsigned long long) * ((size_t)h + w);
    if (c.d_sums.cap() < need) {
        HIP_TRY(hipStreamSynchronize(c.stream));
        if (grow_dev(c.d_sums, need)) return 1;
    }
    HIP_TRY(launch_crop_sums(c.stream, d_frame, fmt, h, w, c.d_sums, c.d_sums + h, max_groups));
    HIP_TRY(hipMemcpyAsync(rows, c.d_sums, sizeof(unsigned long long) * (size_t)h, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipMemcpyAsync(cols, c.d_sums + h, sizeof(unsigned long long) * (size_t)w, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return 0;
}

int crop_sums_host(int device, const void* frame, int fmt, int h, int w, unsigned long long* rows, unsigned long long* cols, int max_groups)
{
    if (crop_sums_check(frame, fmt, h, w, rows, cols)) return 1;
    std::lock_guard<std::mutex> lk(g_pix.mu);
    PixCtx* c = nullptr;
    if (pix_ctx(device, &c)) return 1;
    const size_t bytes = crop_read_bytes(fmt, h, w);
    if (pix_grow(*c, c->d_in, bytes)) return 1;
    HIP_TRY(hipMemcpyAsync(c->d_in, frame, bytes, hipMemcpyHostToDevice, c->stream));
    return crop_sums_run(*c, c->d_in, fmt, h, w, rows, cols, max_groups);
}

int pix_window_check(const void* in, int fmt, int src_h, int src_w, int x, int y, int h, int w, const void* out)
{
    if (!in || !out) return fail("null frame pointer");
    if (const char* e = crop_window_error(fmt, src_h, src_w, x, y, h, w)) return fail(e);
    return 0;
}
}  // namespace

int uva_crop_sums(int device, const void* frame, int fmt, int h, int w, unsigned long long* rows, unsigned long long* cols)
{
    return crop_sums_host(device, frame, fmt, h, w, rows, cols, 0);
}

int uva_debug_crop_sums(int device, const void* frame, int fmt, int h, int w, unsigned long long* rows, unsigned long long* cols, int max_groups)
{
    if (max_groups < 0) return fail("uva_debug_crop_sums: max_groups is 0 (the kernel's own bound) or a number of workgroups");
    return crop_sums_host(device, frame, fmt, h, w, rows, cols, max_groups);
}

int uva_crop_sums_device(int device, const void* d_frame, int fmt, int h, int w, unsigned long long* rows, unsigned long long* cols)
{
    if (crop_sums_check(d_frame, fmt, h, w, rows, cols)) return 1;
    if (((uintptr_t)d_frame & 15) != 0) return fail("uva_crop_sums_device: the frame must start at a 16-byte aligned address");
    std::lock_guard<std::mutex> lk(g_pix.mu);
    PixCtx* c = nullptr;
    if (pix_ctx(device, &c)) return 1;
    return crop_sums_run(*c, d_frame, fmt, h, w, rows, cols, 0);
}

int uva_crop_bounds(const unsigned long long* rows, const unsigned long long* cols, int fmt, int h, int w, int limit, int* bounds)
{
    if (const char* e = crop_bounds(rows, cols, fmt, h, w, limit, bounds)) return fail(e);
    return 0;
}

int uva_crop_rect(const int* state, int round, int* rect)
{
    if (!state || !rect) return fail("uva_crop_rect: null pointer");
    if (!crop_rect(state, round, rect)) return fail("uva_crop_rect: the state holds no rectangle");
    return 0;
}

int uva_pix_window_check(int fmt, int src_h, int src_w, int x, int y, int h, int w)
{
    if (const char* e = crop_window_error(fmt, src_h, src_w, x, y, h, w)) return fail(e);
    return 0;
}

int uva_pix_window(int device, const void* in, int fmt, int src_h, int src_w, int x, int y, int h, int w, void* out)
{
    if (pix_window_check(in, fmt, src_h, src_w, x, y, h, w, out)) return 1;
    std::lock_guard<std::mutex> lk(g_pix.mu);
    PixCtx* c = nullptr;
    if (pix_ctx(device, &c)) return 1;
    WindowPlane pl[3];
    const int np = crop_window_planes(fmt, src_h, src_w, x, y, h, w, pl);
    size_t at[3] = {0, 0, 0};
    const size_t stage = pix_window_staging(pl, np, at), nout = pix_frame_bytes(fmt, h, w);
    if (pix_grow(*c, c->d_in, stage) || pix_grow(*c, c->d_out, nout)) return 1;
    // the window's rows go up at full width, one copy per plane; the kernel compacts their columns
    for (int p = 0; p < np; ++p)
        HIP_TRY(hipMemcpyAsync(c->d_in + at[p], (const uint8_t*)in + pl[p].src_off + (size_t)pl[p].row0 * pl[p].src_row,
                               pl[p].src_row * (size_t)pl[p].rows, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_pix_window(c->stream, c->d_in, at, c->d_out, pl, np, crop_sample(fmt).bytes));
    HIP_TRY(hipMemcpyAsync(out, c->d_out, nout, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int uva_pix_window_device(int device, const void* d_in, int fmt, int src_h, int src_w, int x, int y, int h, int w, void* d_out)
{
    if (pix_window_check(d_in, fmt, src_h, src_w, x, y, h, w, d_out)) return 1;
    if (((uintptr_t)d_out & 15) != 0) return fail("uva_pix_window_device: the result must start at a 16-byte aligned address");
    if (((uintptr_t)d_in & (uintptr_t)(crop_sample(fmt).bytes - 1)) != 0) return fail("uva_pix_window_device: odd address of a frame of 16-bit words");
    std::lock_guard<std::mutex> lk(g_pix.mu);
    PixCtx* c = nullptr;
    if (pix_ctx(device, &c)) return 1;
    WindowPlane pl[3];
    const int np = crop_window_planes(fmt, src_h, src_w, x, y, h, w, pl);
    size_t at[3] = {0, 0, 0};
    for (int p = 0; p < np; ++p) at[p] = pl[p].src_off + (size_t)pl[p].row0 * pl[p].src_row;
    HIP_TRY(launch_pix_window(c->stream, d_in, at, d_out, pl, np, crop_sample(fmt).bytes));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- deinterlacing (csrc/uva_deint.hip, csrc/uva_deint_host.cpp) ------------------------------------
struct uva_deint {
    int device = 0, fmt = 0, h = 0, w = 0, flags = 0;
    size_t bytes = 0;
    long long pushed = 0;                                  // frames since the last reset
    DevPtr<uint8_t> d_frame[3];                            // frame k of the stream lies in d_frame[k % 3]
    DevPtr<uint8_t> d_out[2];                              // A, and B with UVA_DEINT_FIELD
    Stream stream;
};

namespace {
// everything the stateless entries refuse, before a GPU is looked for
int deint_frames_check(const void* cur, int fmt, int h, int w, int flags, const void* out_a, const void* out_b)
{
    if (const char* e = deint_error(fmt, h, w, flags)) return fail(e);
    if (!cur) return fail("null frame pointer");
    if (!out_a && !out_b) return fail("deinterlace: neither output A nor output B is asked for");
    if (out_b && !(flags & DEINT_FIELD)) return fail("deinterlace: output B exists with UVA_DEINT_FIELD only");
    return 0;
}

int deint_frames_host(int device, const void* prev, const void* cur, const void* next, int fmt, int h, int w, int flags, void* out_a, void* out_b,
                      int max_groups)
{
    if (deint_frames_check(cur, fmt, h, w, flags, out_a, out_b)) return 1;
    std::lock_guard<std::mutex> lk(g_pix.mu);
    PixCtx* c = nullptr;
    if (pix_ctx(device, &c)) return 1;
    const size_t bytes = deint_format(fmt, h, w).frame_bytes, slot = (bytes + 15) & ~(size_t)15;
    // prev, cur, next in d_in; A, B in d_out (every frame at a multiple of 16 bytes)
    if (pix_grow(*c, c->d_in, 3 * slot) || pix_grow(*c, c->d_out, 2 * slot)) return 1;
    const uint8_t *d_cur = c->d_in + slot, *d_prev = d_cur, *d_next = d_cur;
    HIP_TRY(hipMemcpyAsync(c->d_in + slot, cur, bytes, hipMemcpyHostToDevice, c->stream));
    if (prev && prev != cur) {
        HIP_TRY(hipMemcpyAsync(c->d_in, prev, bytes, hipMemcpyHostToDevice, c->stream));
        d_prev = c->d_in;
    }
    if (next && next != cur) {
        HIP_TRY(hipMemcpyAsync(c->d_in + 2 * slot, next, bytes, hipMemcpyHostToDevice, c->stream));
        d_next = c->d_in + 2 * slot;
    }
    HIP_TRY(launch_deint(c->stream, d_prev, d_cur, d_next, fmt, h, w, flags, out_a ? c->d_out : nullptr, out_b ? c->d_out + slot : nullptr,
                         max_groups));
    if (out_a) HIP_TRY(hipMemcpyAsync(out_a, c->d_out, bytes, hipMemcpyDeviceToHost, c->stream));
    if (out_b) HIP_TRY(hipMemcpyAsync(out_b, c->d_out + slot, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// the outputs of frame `k` of the handle's stream (prev / next: k -+ 1, or k itself at an end), downloaded and waited for
int deint_emit(uva_deint* d, long long k, bool has_next, void* out_a, void* out_b, int* produced)
{
    const uint8_t* cur = d->d_frame[k % 3];
    const uint8_t* prev = k > 0 ? d->d_frame[(k - 1) % 3] : cur;
    const uint8_t* next = has_next ? d->d_frame[(k + 1) % 3] : cur;
    const bool field = (d->flags & DEINT_FIELD) != 0;
    HIP_TRY(launch_deint(d->stream, prev, cur, next, d->fmt, d->h, d->w, d->flags, d->d_out[0], field ? d->d_out[1] : nullptr, 0));
    HIP_TRY(hipMemcpyAsync(out_a, d->d_out[0], d->bytes, hipMemcpyDeviceToHost, d->stream));
    if (field) HIP_TRY(hipMemcpyAsync(out_b, d->d_out[1], d->bytes, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    *produced = field ? 2 : 1;
    return 0;
}
}  // namespace

int uva_deint_check(int fmt, int h, int w, int flags)
{
    if (const char* e = deint_error(fmt, h, w, flags)) return fail(e);
    return 0;
}

int uva_deint_frames(int device, const void* prev, const void* cur, const void* next, int fmt, int h, int w, int flags, void* out_a, void* out_b)
{
    return deint_frames_host(device, prev, cur, next, fmt, h, w, flags, out_a, out_b, 0);
}

int uva_debug_deint_frames(int device, const void* prev, const void* cur, const void* next, int fmt, int h, int w, int flags, void* out_a,
                           void* out_b, int max_groups)
{
    if (max_groups < 0) return fail("uva_debug_deint_frames: max_groups is 0 (the kernel's own bound) or a number of workgroups");
    return deint_frames_host(device, prev, cur, next, fmt, h, w, flags, out_a, out_b, max_groups);
}

int uva_deint_frames_device(int device, const void* d_prev, const void* d_cur, const void* d_next, int fmt, int h, int w, int flags,
                            void* d_out_a, void* d_out_b)
{
    if (deint_frames_check(d_cur, fmt, h, w, flags, d_out_a, d_out_b)) return 1;
    if ((((uintptr_t)d_prev | (uintptr_t)d_cur | (uintptr_t)d_next | (uintptr_t)d_out_a | (uintptr_t)d_out_b) & 15) != 0)
        return fail("uva_deint_frames_device: the frames must start at 16-byte aligned addresses");
    std::lock_guard<std::mutex> lk(g_pix.mu);
    PixCtx* c = nullptr;
    if (pix_ctx(device, &c)) return 1;
    HIP_TRY(launch_deint(c->stream, d_prev ? d_prev : d_cur, d_cur, d_next ? d_next : d_cur, fmt, h, w, flags, d_out_a, d_out_b, 0));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int uva_debug_deint_host(const void* prev, const void* cur, const void* next, int fmt, int h, int w, int flags, void* out_a, void* out_b)
{
    if (deint_frames_check(cur, fmt, h, w, flags, out_a, out_b)) return 1;
    deint_host((const uint8_t*)prev, (const uint8_t*)cur, (const uint8_t*)next, fmt, h, w, flags, (uint8_t*)out_a, (uint8_t*)out_b);
    return 0;
}

int uva_deint_create(int device, int fmt, int h, int w, int flags, uva_deint** out)
{
    if (!out) return fail("uva_deint_create: null pointer");
    *out = nullptr;
    if (const char* e = deint_error(fmt, h, w, flags)) return fail(e);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail("no HIP device available: libuva has no CPU path");
    if (device < 0 || device >= count) return fail("HIP device " + std::to_string(device) + " does not exist");
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<uva_deint> d(new uva_deint);
    d->device = device; d->fmt = fmt; d->h = h; d->w = w; d->flags = flags;
    d->bytes = deint_format(fmt, h, w).frame_bytes;
    hipError_t e = make_stream(d->stream);
    for (int k = 0; k < 3 && e == hipSuccess; ++k) e = alloc_into(d->d_frame[k], d->bytes);
    for (int k = 0; k < ((flags & DEINT_FIELD) ? 2 : 1) && e == hipSuccess; ++k) e = alloc_into(d->d_out[k], d->bytes);
    if (e != hipSuccess) return fail(std::string("uva_deint_create: ") + hipGetErrorString(e));     // (nothing is queued yet)
    *out = d.release();
    return 0;
}

int uva_deint_push(uva_deint* d, const void* frame, void* out_a, void* out_b, int* produced)
{
    if (!d || !produced) return fail("uva_deint_push: null pointer");
    *produced = 0;
    if (!out_a || ((d->flags & DEINT_FIELD) && !out_b)) return fail("uva_deint_push: null output frame");
    HIP_TRY(hipSetDevice(d->device));
    if (!frame) {                                   // flush: the last frame has no next
        const long long n = d->pushed;
        d->pushed = 0;
        return n ? deint_emit(d, n - 1, false, out_a, out_b, produced) : 0;
    }
    // (frame k - 2's slot is free: the outputs of frame k - 1, the last to read it, were waited for)
    const long long k = d->pushed;
    HIP_TRY(hipMemcpyAsync(d->d_frame[k % 3], frame, d->bytes, hipMemcpyHostToDevice, d->stream));
    d->pushed = k + 1;
    if (k == 0) {
        HIP_TRY(hipStreamSynchronize(d->stream));   // (`frame` is the caller's again when the call returns)
        return 0;
    }
    return deint_emit(d, k - 1, true, out_a, out_b, produced);
}

int uva_deint_reset(uva_deint* d)
{
    if (!d) return fail("uva_deint_reset: null pointer");
    d->pushed = 0;
    return 0;
}

void uva_deint_destroy(uva_deint* d)
{
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->stream) (void)hipStreamSynchronize(d->stream);
    delete d;
}

// ---- inverse telecine (csrc/uva_ivtc.hip, csrc/uva_ivtc_host.cpp) ------------------------------------
struct uva_ivtc {
    static constexpr int RING = 10;                        // two cycles: a cycle is delivered while the next one is built
    int device = 0, fmt = 0, h = 0, w = 0, flags = 0, T = 0, L = 0;
    size_t bytes = 0;
    long long pushed = 0;                                  // source frames since the last reset
    long long finals = 0;                                  // final frames built since the last reset
    bool ended = false;                                    // a flush has closed the stream
    IvtcDecimator dec;
    unsigned long long counts[7] = {};                     // uva_ivtc_stats
    DevPtr<uint8_t> d_frame[3];                            // source frame k lies in d_frame[k % 3]
    DevPtr<uint8_t> d_final[RING];                         // final frame j lies in d_final[j % RING]
    DevPtr<unsigned long long> d_stats;                    // the six sums, then a FrameDiffStats
    Stream stream;
};

namespace {
constexpr size_t IVTC_STATS_BYTES = 6 * sizeof(unsigned long long) + sizeof(FrameDiffStats);

int ivtc_metrics_check(const void* cur, int fmt, int h, int w, int flags, int T, const unsigned long long* stats)
{
    if (const char* e = ivtc_error(fmt, h, w, flags, T, 0)) return fail(e);
    if (!cur || !stats) return fail("null frame pointer");
    return 0;
}

int ivtc_metrics_up(int device, const void* prev, const void* cur, const void* next, int fmt, int h, int w, int flags, int T,
                    unsigned long long* stats, int max_groups)
{
    if (ivtc_metrics_check(cur, fmt, h, w, flags, T, stats)) return 1;
    std::lock_guard<std::mutex> lk(g_pix.mu);
    PixCtx* c = nullptr;
    if (pix_ctx(device, &c)) return 1;
    const size_t bytes = deint_format(fmt, h, w).frame_bytes, slot = (bytes + 15) & ~(size_t)15;
    // prev, cur, next in d_in (every frame at a multiple of 16 bytes); the sums in d_sums
    if (pix_grow(*c, c->d_in, 3 * slot)) return 1;
    if (c->d_sums.cap() < 6 * sizeof(unsigned long long)) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (grow_dev(c->d_sums, 6 * sizeof(unsigned long long))) return 1;
    }
    const uint8_t *d_cur = c->d_in + slot, *d_prev = d_cur, *d_next = d_cur;
    HIP_TRY(hipMemcpyAsync(c->d_in + slot, cur, bytes, hipMemcpyHostToDevice, c->stream));
    if (prev && prev != cur) {
        HIP_TRY(hipMemcpyAsync(c->d_in, prev, bytes, hipMemcpyHostToDevice, c->stream));
        d_prev = c->d_in;
    }
    if (next && next != cur) {
        HIP_TRY(hipMemcpyAsync(c->d_in + 2 * slot, next, bytes, hipMemcpyHostToDevice, c->stream));
        d_next = c->d_in + 2 * slot;
    }
    HIP_TRY(launch_ivtc_metrics(c->stream, d_prev, d_cur, d_next, fmt, h, w, flags, T, c->d_sums, max_groups));
    HIP_TRY(hipMemcpyAsync(stats, c->d_sums, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

void ivtc_clear(uva_ivtc* d)
{
    d->pushed = d->finals = 0;
    d->ended = false;
    d->dec.reset((d->flags & IVTC_KEEP_ALL) != 0);
}

// final frame k of the handle's stream (prev / next: source frames k -+ 1, or k itself at an end) into its ring slot, its diff
// to the decimator; waited for
int ivtc_finalize(uva_ivtc* d, long long k, bool has_next)
{
    const uint8_t* cur = d->d_frame[k % 3];
    const uint8_t* prev = k > 0 ? d->d_frame[(k - 1) % 3] : cur;
    const uint8_t* next = has_next ? d->d_frame[(k + 1) % 3] : cur;
    unsigned long long st[6];
    HIP_TRY(launch_ivtc_metrics(d->stream, prev, cur, next, d->fmt, d->h, d->w, d->flags, d->T, d->d_stats, 0));
    HIP_TRY(hipMemcpyAsync(st, d->d_stats, sizeof st, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    const DeintFormat f = deint_format(d->fmt, d->h, d->w);
    int rows = 0, match = IVTC_C;
    long long samples = 0;
    ivtc_metric_extent(f, &rows, &samples);
    const bool combed = ivtc_choose(st, rows, samples, d->L, &match);
    uint8_t* dst = d->d_final[k % uva_ivtc::RING];
    if (combed && !(d->flags & IVTC_KEEP_COMBED))
        HIP_TRY(launch_deint(d->stream, prev, cur, next, d->fmt, d->h, d->w, ivtc_deint_flags(d->flags), dst, nullptr, 0));
    else
        HIP_TRY(launch_ivtc_weave(d->stream, cur, match == IVTC_P ? prev : (match == IVTC_N ? next : cur), d->fmt, d->h, d->w, d->flags, dst));
    unsigned long long diff = IVTC_FIRST_DIFF;
    if (k > 0 && !(d->flags & IVTC_KEEP_ALL)) {
        FrameDiffStats fd;
        FrameDiffStats* d_fd = (FrameDiffStats*)(d->d_stats.get() + 6);
        HIP_TRY(launch_frame_diff(d->stream, dst, d->d_final[(k - 1) % uva_ivtc::RING], d->bytes, d->fmt, 0, d_fd));
        HIP_TRY(hipMemcpyAsync(&fd, d_fd, sizeof fd, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        diff = fd.sad;
    }
    d->dec.add(diff);
    d->finals = k + 1;
    ++d->counts[2 + match];
    if (combed) ++d->counts[5];
    return 0;
}
}  // namespace

int uva_ivtc_check(int fmt, int h, int w, int flags, int T, int L)
{
    if (const char* e = ivtc_error(fmt, h, w, flags, T, L)) return fail(e);
    return 0;
}

int uva_ivtc_metrics(int device, const void* prev, const void* cur, const void* next, int fmt, int h, int w, int flags, int T,
                     unsigned long long* stats)
{
    return ivtc_metrics_up(device, prev, cur, next, fmt, h, w, flags, T, stats, 0);
}

int uva_debug_ivtc_metrics(int device, const void* prev, const void* cur, const void* next, int fmt, int h, int w, int flags, int T,
                           unsigned long long* stats, int max_groups)
{
    if (max_groups < 0) return fail("uva_debug_ivtc_metrics: max_groups is 0 (the kernel's own bound) or a number of workgroups");
    return ivtc_metrics_up(device, prev, cur, next, fmt, h, w, flags, T, stats, max_groups);
}

int uva_ivtc_metrics_device(int device, const void* d_prev, const void* d_cur, const void* d_next, int fmt, int h, int w, int flags, int T,
                            unsigned long long* stats)
{
    if (ivtc_metrics_check(d_cur, fmt, h, w, flags, T, stats)) return 1;
    if ((((uintptr_t)d_prev | (uintptr_t)d_cur | (uintptr_t)d_next) & 15) != 0)
        return fail("uva_ivtc_metrics_device: the frames must start at 16-byte aligned addresses");
    std::lock_guard<std::mutex> lk(g_pix.mu);
    PixCtx* c = nullptr;
    if (pix_ctx(device, &c)) return 1;
    if (c->d_sums.cap() < 6 * sizeof(unsigned long long)) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (grow_dev(c->d_sums, 6 * sizeof(unsigned long long))) return 1;
    }
    HIP_TRY(launch_ivtc_metrics(c->stream, d_prev ? d_prev : d_cur, d_cur, d_next ? d_next : d_cur, fmt, h, w, flags, T, c->d_sums, 0));
    HIP_TRY(hipMemcpyAsync(stats, c->d_sums, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int uva_debug_ivtc_host(const void* prev, const void* cur, const void* next, int fmt, int h, int w, int flags, int T, int L,
                        unsigned long long* stats, void* woven, void* chosen, int* decision)
{
    if (const char* e = ivtc_error(fmt, h, w, flags, T, L)) return fail(e);
    if (!cur || !stats) return fail("null frame pointer");
    const uint8_t *c = (const uint8_t*)cur, *x[3] = {c, prev ? (const uint8_t*)prev : c, next ? (const uint8_t*)next : c};
    ivtc_metrics_host(x[1], c, x[2], fmt, h, w, flags, T, stats);
    const DeintFormat f = deint_format(fmt, h, w);
    if (woven)
        for (int k = 0; k < 3; ++k) ivtc_weave_host(c, x[k], fmt, h, w, flags, (uint8_t*)woven + (size_t)k * f.frame_bytes);
    int rows = 0, match = IVTC_C;
    long long samples = 0;
    ivtc_metric_extent(f, &rows, &samples);
    const bool combed = ivtc_choose(stats, rows, samples, L, &match);
    if (decision) {
        decision[0] = match;
        decision[1] = combed ? 1 : 0;
    }
    if (chosen) {
        if (combed && !(flags & IVTC_KEEP_COMBED)) deint_host(x[1], c, x[2], fmt, h, w, ivtc_deint_flags(flags), (uint8_t*)chosen, nullptr);
        else ivtc_weave_host(c, x[match], fmt, h, w, flags, (uint8_t*)chosen);
    }
    return 0;
}

int uva_debug_ivtc_decimate(const unsigned long long* diffs, int n, int flags, long long* delivered, int* n_delivered)
{
    if (!diffs || !delivered || !n_delivered || n < 0) return fail("uva_debug_ivtc_decimate: null pointer");
    if (flags & ~IVTC_FLAGS) return fail(ivtc_error(0, 4, 1, flags, 0, 0));
    // as uva_ivtc_push drives it: one frame in, at most one out, then the flush steps
    IvtcDecimator dec;
    dec.reset((flags & IVTC_KEEP_ALL) != 0);
    int out = 0;
    long long j = 0;
    for (int k = 0; k < n; ++k) {
        dec.add(diffs[k]);
        if (dec.pop(&j)) delivered[out++] = j;
    }
    dec.end();
    while (dec.pop(&j)) delivered[out++] = j;
    *n_delivered = out;
    return 0;
}

int uva_ivtc_create(int device, int fmt, int h, int w, int flags, int T, int L, uva_ivtc** out)
{
    if (!out) return fail("uva_ivtc_create: null pointer");
    *out = nullptr;
    if (const char* e = ivtc_error(fmt, h, w, flags, T, L)) return fail(e);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail("no HIP device available: libuva has no CPU path");
    if (device < 0 || device >= count) return fail("HIP device " + std::to_string(device) + " does not exist");
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<uva_ivtc> d(new uva_ivtc);
    d->device = device; d->fmt = fmt; d->h = h; d->w = w; d->flags = flags; d->T = T; d->L = L;
    d->bytes = deint_format(fmt, h, w).frame_bytes;
    ivtc_clear(d.get());
    hipError_t e = make_stream(d->stream);
    for (int k = 0; k < 3 && e == hipSuccess; ++k) e = alloc_into(d->d_frame[k], d->bytes);
    for (int k = 0; k < uva_ivtc::RING && e == hipSuccess; ++k) e = alloc_into(d->d_final[k], d->bytes);
    if (e == hipSuccess) e = alloc_into(d->d_stats, IVTC_STATS_BYTES);
    if (e != hipSuccess) return fail(std::string("uva_ivtc_create: ") + hipGetErrorString(e));      // (nothing is queued yet)
    *out = d.release();
    return 0;
}

int uva_ivtc_push(uva_ivtc* d, const void* frame, void* out, int* produced)
{
    if (!d || !produced) return fail("uva_ivtc_push: null pointer");
    *produced = 0;
    if (!out) return fail("uva_ivtc_push: null output frame");
    HIP_TRY(hipSetDevice(d->device));
    if (frame) {
        if (d->ended) return fail("uva_ivtc_push: the stream is being flushed: call with frame NULL until it produces 0");
        // (source frame k - 3's slot is free: final frame k - 2, the last to read it, was waited for)
        const long long k = d->pushed;
        HIP_TRY(hipMemcpyAsync(d->d_frame[k % 3], frame, d->bytes, hipMemcpyHostToDevice, d->stream));
        d->pushed = k + 1;
        ++d->counts[0];
        if (k == 0) HIP_TRY(hipStreamSynchronize(d->stream));       // (`frame` is the caller's again when the call returns)
        else if (ivtc_finalize(d, k - 1, true)) return 1;
    } else if (!d->ended) {                         // the first flush step: the last frame has no next
        if (d->finals < d->pushed && ivtc_finalize(d, d->pushed - 1, false)) return 1;
        d->dec.end();
        d->ended = true;
    }
    long long j = 0;
    if (d->dec.pop(&j)) {
        HIP_TRY(hipMemcpyAsync(out, d->d_final[j % uva_ivtc::RING], d->bytes, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        *produced = 1;
        ++d->counts[1];
    } else if (!frame) {                            // flushed empty: as after reset
        d->counts[6] += (unsigned long long)d->dec.dropped;
        ivtc_clear(d);
    }
    return 0;
}

int uva_ivtc_reset(uva_ivtc* d)
{
    if (!d) return fail("uva_ivtc_reset: null pointer");
    d->counts[6] += (unsigned long long)d->dec.dropped;
    ivtc_clear(d);
    return 0;
}

int uva_ivtc_stats(uva_ivtc* d, unsigned long long* stats)
{
    if (!d || !stats) return fail("uva_ivtc_stats: null pointer");
    for (int k = 0; k < 7; ++k) stats[k] = d->counts[k];
    stats[6] += (unsigned long long)d->dec.dropped;         // (the stream in progress)
    return 0;
}

void uva_ivtc_destroy(uva_ivtc* d)
{
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->stream) (void)hipStreamSynchronize(d->stream);
    delete d;
}

}  // extern "C"
