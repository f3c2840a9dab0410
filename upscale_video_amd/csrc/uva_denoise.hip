// uva_denoise.hip -- the non-local-means denoise stage at 8 and at 16 bits (the kernels of csrc/uva_denoise.hip.h and
// csrc/uva_denoise16.hip.h), its per-device buffers and weight tables, and the uva_denoise_* entries.
#include "../../include/uva.h"
#include "uva_denoise.hip.h"
#include "uva_denoise16.hip.h"
#include "uva_rt.h"

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

using namespace uva;

// ---- `-m n=K`: non-local-means denoise (upscale/upscale_processing.py:350-361) -------------------------
namespace {

// the frame buffers of a stage, all sized for cap_px pixels: in / out at 3 samples per pixel, l / l2 at 1, ab / ab2 at 2
template <typename S>
struct NlmFrames {
    DevPtr<S> d_in, d_out, d_l, d_l2, d_ab, d_ab2;
    size_t cap_px = 0;
    hipError_t alloc(size_t px)
    {
        NlmFrames f;
        hipError_t e = hipSuccess;
        const size_t per[6] = {3, 3, 1, 1, 2, 2};
        DevPtr<S>* const to[6] = {&f.d_in, &f.d_out, &f.d_l, &f.d_l2, &f.d_ab, &f.d_ab2};
        for (int k = 0; k < 6 && e == hipSuccess; ++k) e = alloc_into(*to[k], px * per[k] * sizeof(S));
        if (e != hipSuccess) return e;
        f.cap_px = px;
        *this = std::move(f);
        return hipSuccess;
    }
};

struct DenoiseCtx {
    NlmFrames<uint8_t> f;
    DevPtr<int> d_table[2];
    int table_size[2] = {0, 0};
    float table_h[2] = {-1.f, -1.f};
    DevPtr<LabTables> d_lab;             // OpenCV's 8-bit Lab tables (uva_denoise.hip.h)
    Stream stream;
};
DeviceTable<DenoiseCtx>& g_denoise = *new DeviceTable<DenoiseCtx>;

// OpenCV fast_nlmeans_denoising_invoker.hpp: almost_dist2weight_ for 8-bit samples, squared distance
void nlm_weight_table(float h, int cn, std::vector<int>& table)
{
    const int search = 2 * NLM_S + 1, templ = 2 * NLM_T + 1;
    const int fixed_point_mult = INT_MAX / (search * search * 255);
    const double mult = (double)(1 << NLM_SHIFT) / (templ * templ);
    const int max_dist = 255 * 255 * cn;
    const int almost_max = (int)(max_dist / mult + 1);
    table.resize(almost_max);
    for (int ad = 0; ad < almost_max; ++ad) {
        const double dist = ad * mult;
        double w = std::exp(-dist / ((double)h * h * cn));
        if (std::isnan(w)) w = 1.0;
        int weight = (int)std::lrint(fixed_point_mult * w);
        if (weight < 0.001 * fixed_point_mult) weight = 0;
        table[ad] = weight;
    }
}

int denoise_ctx(int device, size_t px, DenoiseCtx** out)
{
    DenoiseCtx* pc = nullptr;
    if (g_denoise.enter(device, &pc)) return 1;
    DenoiseCtx& c = *pc;
    if (!c.d_lab) {
        static const LabTables host_tables = [] { LabTables t; lab_tables_host(t); return t; }();
        DevPtr<LabTables> lab;
        HIP_TRY(alloc_into(lab, sizeof(LabTables)));
        HIP_TRY(hipMemcpy(lab.get(), &host_tables, sizeof(LabTables), hipMemcpyHostToDevice));
        c.d_lab = std::move(lab);
    }
    if (c.f.cap_px < px) {
        // uva_denoise_u8_device is asynchronous: frames queued on the stream may still use the buffers about to go
        // (hipFree happens to synchronise the device; said here instead of relied on)
        if (c.f.cap_px) HIP_TRY(hipStreamSynchronize(c.stream));
        c.f = NlmFrames<uint8_t>();
        HIP_TRY(c.f.alloc(px));
    }
    *out = &c;
    return 0;
}

int denoise_table(DenoiseCtx& c, int which, float h, int cn)
{
    if (c.table_h[which] == h && c.d_table[which]) return 0;
    std::vector<int> t;
    nlm_weight_table(h, cn, t);
    c.d_table[which].reset();
    DevPtr<int> d;
    HIP_TRY(alloc_into(d, t.size() * sizeof(int)));
    HIP_TRY(hipMemcpy(d.get(), t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice));
    c.d_table[which] = std::move(d);
    c.table_size[which] = (int)t.size();
    c.table_h[which] = h;
    return 0;
}


// ---- `-m n=K` at --bit-depth 16 (uva_denoise16.hip.h): its own buffers and tables, the 8-bit stage's
// stream (uva_denoise_synchronize waits for both) and lock
struct Denoise16Ctx {
    NlmFrames<uint16_t> f;
    DevPtr<int> d_table[2];
    int table_size[2] = {0, 0};
    float table_h[2] = {-1.f, -1.f};
    DevPtr<Lab16Tables> d_lab;
};
DeviceTable<Denoise16Ctx>& g_denoise16 = *new DeviceTable<Denoise16Ctx>;       // (its own lock is not used: g_denoise.mu)

int denoise16_ctx(int device, size_t px, Denoise16Ctx** out, hipStream_t* stream)
{
    DenoiseCtx* c8 = nullptr;
    if (g_denoise.enter(device, &c8)) return 1;
    Denoise16Ctx& c = g_denoise16.at(device);
    if (!c.d_lab) {
        static const Lab16Tables* host_tables = [] { Lab16Tables* t = new Lab16Tables; lab16_tables_host(*t); return t; }();
        DevPtr<Lab16Tables> lab;
        HIP_TRY(alloc_into(lab, sizeof(Lab16Tables)));
        HIP_TRY(hipMemcpy(lab.get(), host_tables, sizeof(Lab16Tables), hipMemcpyHostToDevice));
        c.d_lab = std::move(lab);
    }
    if (c.f.cap_px < px) {
        if (c.f.cap_px) HIP_TRY(hipStreamSynchronize(c8->stream));      // queued frames may still use the buffers about to go
        c.f = NlmFrames<uint16_t>();
        HIP_TRY(c.f.alloc(px));
    }
    *out = &c;
    *stream = c8->stream;
    return 0;
}

// one table per channel count, kept until the strength changes (as the 8-bit stage keeps its own)
int denoise16_table(Denoise16Ctx& c, int which, float h, int cn)
{
    if (c.table_h[which] == h && c.d_table[which]) return 0;
    std::vector<int> t;
    if (!nlm16_weight_table(h, cn, t)) return fail("denoise strength too large for the 16-bit weight table");
    c.d_table[which].reset();
    c.table_h[which] = -1.f;
    DevPtr<int> d;
    HIP_TRY(alloc_into(d, t.size() * sizeof(int)));
    HIP_TRY(hipMemcpy(d.get(), t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice));
    c.d_table[which] = std::move(d);
    c.table_size[which] = (int)t.size();
    c.table_h[which] = h;
    return 0;
}

// The four kernels of the stage on `stream`, frame in d_src (strided), result in d_dst (strided)
int denoise16_launch(Denoise16Ctx* c, hipStream_t stream, const uint16_t* d_src, size_t src_stride, uint16_t* d_dst, size_t dst_stride,
                     int h, int w)
{
    const dim3 rows((w + 255) / 256, h), tiles((w + NLM_BLK - 1) / NLM_BLK, (h + NLM_BLK - 1) / NLM_BLK);
    hipLaunchKernelGGL(nlm_bgr2lab16, rows, dim3(256), 0, stream, d_src, src_stride, h, w, c->f.d_l, c->f.d_ab, c->d_lab);
    hipLaunchKernelGGL(nlm_plane16<1>, tiles, dim3(NLM_BLK * NLM_BLK), 0, stream, c->f.d_l, h, w, c->d_table[0], c->table_size[0], c->f.d_l2);
    hipLaunchKernelGGL(nlm_plane16<2>, tiles, dim3(NLM_BLK * NLM_BLK), 0, stream, c->f.d_ab, h, w, c->d_table[1], c->table_size[1], c->f.d_ab2);
    hipLaunchKernelGGL(nlm_lab2bgr16, rows, dim3(256), 0, stream, c->f.d_l2, c->f.d_ab2, h, w, d_dst, dst_stride, c->d_lab);
    HIP_TRY(hipGetLastError());
    return 0;
}

// max strength: K = 1 .. 30 on the command line; the table grows with h^2
constexpr float NLM16_MAX_H = 64.f;

}  // namespace

void uva::denoise_release_all()
{
    std::lock_guard<std::mutex> lk(g_denoise.mu);
    g_denoise.release_all();
}

// (before denoise_release_all destroys the stream that both stages use)
void uva::denoise16_release_all()
{
    std::lock_guard<std::mutex> lk(g_denoise.mu);
    g_denoise16.release_all([](int d) { return g_denoise.ctx[d].stream.get(); });
}

extern "C" {

static int denoise_launch(DenoiseCtx* c, const uint8_t* d_src, size_t src_stride, uint8_t* d_dst, size_t dst_stride, int h, int w);

int uva_denoise_u8(int device, const uint8_t* in, int h, int w, size_t in_stride, uint8_t* out, size_t out_stride,
                   float h_luma, float h_color)
{
    if (!in || !out || h <= 0 || w <= 0 || (long long)h * w > (1ll << 28)) return fail("bad image");
    if (in_stride < (size_t)w * 3 || out_stride < (size_t)w * 3) return fail("row stride too small");
    if (!(h_luma > 0.f) || !(h_color > 0.f)) return fail("denoise strength must be positive");
    std::lock_guard<std::mutex> lk(g_denoise.mu);
    DenoiseCtx* c = nullptr;
    const size_t px = (size_t)h * w;
    if (denoise_ctx(device, px, &c)) return 1;
    if (denoise_table(*c, 0, h_luma, 1) || denoise_table(*c, 1, h_color, 2)) return 1;
    HIP_TRY(hipMemcpy2DAsync(c->f.d_in, (size_t)w * 3, in, in_stride, (size_t)w * 3, h, hipMemcpyHostToDevice, c->stream));
    if (denoise_launch(c, c->f.d_in, (size_t)w * 3, c->f.d_out, (size_t)w * 3, h, w)) return 1;
    HIP_TRY(hipMemcpy2DAsync(out, out_stride, c->f.d_out, (size_t)w * 3, (size_t)w * 3, h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// The four kernels of the stage on the context's stream, frame in d_src (strided), result in d_dst (strided)
static int denoise_launch(DenoiseCtx* c, const uint8_t* d_src, size_t src_stride, uint8_t* d_dst, size_t dst_stride, int h, int w)
{
    const dim3 rows((w + 255) / 256, h), tiles((w + NLM_BLK - 1) / NLM_BLK, (h + NLM_BLK - 1) / NLM_BLK);
    hipLaunchKernelGGL(nlm_bgr2lab, rows, dim3(256), 0, c->stream, d_src, src_stride, h, w, c->f.d_l, c->f.d_ab, c->d_lab);
    hipLaunchKernelGGL(nlm_plane<1>, tiles, dim3(NLM_BLK * NLM_BLK), 0, c->stream, c->f.d_l, h, w, c->d_table[0], c->table_size[0], c->f.d_l2);
    hipLaunchKernelGGL(nlm_plane<2>, tiles, dim3(NLM_BLK * NLM_BLK), 0, c->stream, c->f.d_ab, h, w, c->d_table[1], c->table_size[1], c->f.d_ab2);
    hipLaunchKernelGGL(nlm_lab2bgr, rows, dim3(256), 0, c->stream, c->f.d_l2, c->f.d_ab2, h, w, d_dst, dst_stride, c->d_lab);
    HIP_TRY(hipGetLastError());
    return 0;
}

int uva_denoise_u8_device(int device, const void* d_in, int h, int w, size_t in_stride, void* d_out, size_t out_stride,
                          float h_luma, float h_color, uva_net* after, uva_net* before)
{
    if (!d_in || !d_out || h <= 0 || w <= 0 || (long long)h * w > (1ll << 28)) return fail("bad image");
    if (in_stride < (size_t)w * 3 || out_stride < (size_t)w * 3) return fail("row stride too small");
    if (!(h_luma > 0.f) || !(h_color > 0.f)) return fail("denoise strength must be positive");
    if (check_fence_nets(device, after, before, "uva_denoise_u8_device")) return 1;
    std::lock_guard<std::mutex> lk(g_denoise.mu);
    DenoiseCtx* c = nullptr;
    if (denoise_ctx(device, (size_t)h * w, &c)) return 1;
    // the weight tables are uploaded with a blocking copy: the stream must not be reading the old ones
    if (c->table_h[0] != h_luma || c->table_h[1] != h_color) HIP_TRY(hipStreamSynchronize(c->stream));
    if (denoise_table(*c, 0, h_luma, 1) || denoise_table(*c, 1, h_color, 2)) return 1;
    if (fence_after(after, c->stream)) return 1;
    if (denoise_launch(c, (const uint8_t*)d_in, in_stride, (uint8_t*)d_out, out_stride, h, w)) return 1;
    if (fence_before(before, c->stream)) return 1;
    return 0;
}

int uva_denoise_synchronize(int device)
{
    std::lock_guard<std::mutex> lk(g_denoise.mu);
    if (device < 0 || device >= kMaxDevices) return fail("bad device");
    if (!g_denoise.ctx[device].stream) return 0;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamSynchronize(g_denoise.ctx[device].stream));
    return 0;
}

int uva_debug_denoise_stage(int device, int stage, const uint8_t* in, int h, int w, float strength, uint8_t* out)
{
    if (!in || !out || h <= 0 || w <= 0) return fail("bad argument");
    std::lock_guard<std::mutex> lk(g_denoise.mu);
    DenoiseCtx* c = nullptr;
    const size_t px = (size_t)h * w;
    if (denoise_ctx(device, px, &c)) return 1;
    const dim3 rows((w + 255) / 256, h), tiles((w + NLM_BLK - 1) / NLM_BLK, (h + NLM_BLK - 1) / NLM_BLK);
    if (stage == 0) {          // bgr [h][w][3] -> Lab interleaved [h][w][3]
        HIP_TRY(hipMemcpy(c->f.d_in, in, px * 3, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(nlm_bgr2lab, rows, dim3(256), 0, c->stream, c->f.d_in, (size_t)w * 3, h, w, c->f.d_l, c->f.d_ab, c->d_lab);
        HIP_TRY(hipStreamSynchronize(c->stream));
        std::vector<uint8_t> l(px), ab(px * 2);
        HIP_TRY(hipMemcpy(l.data(), c->f.d_l, px, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(ab.data(), c->f.d_ab, px * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < px; ++i) { out[3 * i] = l[i]; out[3 * i + 1] = ab[2 * i]; out[3 * i + 2] = ab[2 * i + 1]; }
    } else if (stage == 1) {   // Lab interleaved -> bgr
        std::vector<uint8_t> l(px), ab(px * 2);
        for (size_t i = 0; i < px; ++i) { l[i] = in[3 * i]; ab[2 * i] = in[3 * i + 1]; ab[2 * i + 1] = in[3 * i + 2]; }
        HIP_TRY(hipMemcpy(c->f.d_l, l.data(), px, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->f.d_ab, ab.data(), px * 2, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(nlm_lab2bgr, rows, dim3(256), 0, c->stream, c->f.d_l, c->f.d_ab, h, w, c->f.d_out, (size_t)w * 3, c->d_lab);
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(out, c->f.d_out, px * 3, hipMemcpyDeviceToHost));
    } else if (stage == 2 || stage == 3) {   // NLM on a 1-channel (2) / 2-channel (3) u8 image
        const int cn = stage - 1;
        if (!(strength > 0.f)) return fail("denoise strength must be positive");
        if (denoise_table(*c, cn - 1, strength, cn)) return 1;
        uint8_t* src = cn == 1 ? c->f.d_l : c->f.d_ab;
        uint8_t* dst = cn == 1 ? c->f.d_l2 : c->f.d_ab2;
        HIP_TRY(hipMemcpy(src, in, px * cn, hipMemcpyHostToDevice));
        if (cn == 1) hipLaunchKernelGGL(nlm_plane<1>, tiles, dim3(NLM_BLK * NLM_BLK), 0, c->stream, src, h, w, c->d_table[0], c->table_size[0], dst);
        else hipLaunchKernelGGL(nlm_plane<2>, tiles, dim3(NLM_BLK * NLM_BLK), 0, c->stream, src, h, w, c->d_table[1], c->table_size[1], dst);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(out, dst, px * cn, hipMemcpyDeviceToHost));
    } else {
        return fail("bad stage");
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int uva_denoise_u16(int device, const uint16_t* in, int h, int w, size_t in_stride, uint16_t* out, size_t out_stride,
                    float h_luma, float h_color)
{
    if (!in || !out || h <= 0 || w <= 0 || (long long)h * w > (1ll << 28)) return fail("bad image");
    if (in_stride < (size_t)w * 6 || out_stride < (size_t)w * 6) return fail("row stride too small");
    if (!(h_luma > 0.f) || !(h_color > 0.f) || h_luma > NLM16_MAX_H || h_color > NLM16_MAX_H) return fail("denoise strength must be in (0, 64]");
    std::lock_guard<std::mutex> lk(g_denoise.mu);
    Denoise16Ctx* c = nullptr;
    hipStream_t stream = nullptr;
    const size_t px = (size_t)h * w;
    if (denoise16_ctx(device, px, &c, &stream)) return 1;
    if (c->table_h[0] != h_luma || c->table_h[1] != h_color) HIP_TRY(hipStreamSynchronize(stream));
    if (denoise16_table(*c, 0, h_luma, 1) || denoise16_table(*c, 1, h_color, 2)) return 1;
    HIP_TRY(hipMemcpy2DAsync(c->f.d_in, (size_t)w * 6, in, in_stride, (size_t)w * 6, h, hipMemcpyHostToDevice, stream));
    if (denoise16_launch(c, stream, c->f.d_in, (size_t)w * 6, c->f.d_out, (size_t)w * 6, h, w)) return 1;
    HIP_TRY(hipMemcpy2DAsync(out, out_stride, c->f.d_out, (size_t)w * 6, (size_t)w * 6, h, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}

int uva_denoise_u16_device(int device, const void* d_in, int h, int w, size_t in_stride, void* d_out, size_t out_stride,
                           float h_luma, float h_color, uva_net* after, uva_net* before)
{
    if (!d_in || !d_out || h <= 0 || w <= 0 || (long long)h * w > (1ll << 28)) return fail("bad image");
    if (in_stride < (size_t)w * 6 || out_stride < (size_t)w * 6) return fail("row stride too small");
    if ((in_stride | out_stride | (size_t)d_in | (size_t)d_out) & 1) return fail("uva_denoise_u16_device: u16 rows must be 2-byte aligned");
    if (!(h_luma > 0.f) || !(h_color > 0.f) || h_luma > NLM16_MAX_H || h_color > NLM16_MAX_H) return fail("denoise strength must be in (0, 64]");
    if (check_fence_nets(device, after, before, "uva_denoise_u16_device")) return 1;
    std::lock_guard<std::mutex> lk(g_denoise.mu);
    Denoise16Ctx* c = nullptr;
    hipStream_t stream = nullptr;
    if (denoise16_ctx(device, (size_t)h * w, &c, &stream)) return 1;
    // the weight tables are uploaded with a blocking copy: the stream must not be reading the old ones
    if (c->table_h[0] != h_luma || c->table_h[1] != h_color) HIP_TRY(hipStreamSynchronize(stream));
    if (denoise16_table(*c, 0, h_luma, 1) || denoise16_table(*c, 1, h_color, 2)) return 1;
    if (fence_after(after, stream)) return 1;
    if (denoise16_launch(c, stream, (const uint16_t*)d_in, in_stride, (uint16_t*)d_out, out_stride, h, w)) return 1;
    if (fence_before(before, stream)) return 1;
    return 0;
}

int uva_debug_denoise16_stage(int device, int stage, const uint16_t* in, int h, int w, float strength, uint16_t* out)
{
    if (!in || !out || h <= 0 || w <= 0 || (long long)h * w > (1ll << 28)) return fail("bad argument");
    std::lock_guard<std::mutex> lk(g_denoise.mu);
    Denoise16Ctx* c = nullptr;
    hipStream_t stream = nullptr;
    const size_t px = (size_t)h * w;
    if (denoise16_ctx(device, px, &c, &stream)) return 1;
    HIP_TRY(hipStreamSynchronize(stream));           // the blocking copies below write buffers queued frames may still read
    const dim3 rows((w + 255) / 256, h), tiles((w + NLM_BLK - 1) / NLM_BLK, (h + NLM_BLK - 1) / NLM_BLK);
    if (stage == 0) {          // bgr [h][w][3] -> Lab interleaved [h][w][3]
        HIP_TRY(hipMemcpy(c->f.d_in, in, px * 6, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(nlm_bgr2lab16, rows, dim3(256), 0, stream, c->f.d_in, (size_t)w * 6, h, w, c->f.d_l, c->f.d_ab, c->d_lab);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
        std::vector<uint16_t> l(px), ab(px * 2);
        HIP_TRY(hipMemcpy(l.data(), c->f.d_l, px * 2, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(ab.data(), c->f.d_ab, px * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < px; ++i) { out[3 * i] = l[i]; out[3 * i + 1] = ab[2 * i]; out[3 * i + 2] = ab[2 * i + 1]; }
    } else if (stage == 1) {   // Lab interleaved -> bgr
        std::vector<uint16_t> l(px), ab(px * 2);
        for (size_t i = 0; i < px; ++i) { l[i] = in[3 * i]; ab[2 * i] = in[3 * i + 1]; ab[2 * i + 1] = in[3 * i + 2]; }
        HIP_TRY(hipMemcpy(c->f.d_l, l.data(), px * 2, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->f.d_ab, ab.data(), px * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(nlm_lab2bgr16, rows, dim3(256), 0, stream, c->f.d_l, c->f.d_ab, h, w, c->f.d_out, (size_t)w * 6, c->d_lab);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipMemcpy(out, c->f.d_out, px * 6, hipMemcpyDeviceToHost));
    } else if (stage == 2 || stage == 3) {   // NLM on a 1-channel (2) / 2-channel (3) u16 image
        const int cn = stage - 1;
        if (!(strength > 0.f) || strength > NLM16_MAX_H) return fail("denoise strength must be in (0, 64]");
        if (denoise16_table(*c, cn - 1, strength, cn)) return 1;
        uint16_t* src = cn == 1 ? c->f.d_l : c->f.d_ab;
        uint16_t* dst = cn == 1 ? c->f.d_l2 : c->f.d_ab2;
        HIP_TRY(hipMemcpy(src, in, px * cn * 2, hipMemcpyHostToDevice));
        if (cn == 1) hipLaunchKernelGGL(nlm_plane16<1>, tiles, dim3(NLM_BLK * NLM_BLK), 0, stream, src, h, w, c->d_table[0], c->table_size[0], dst);
        else hipLaunchKernelGGL(nlm_plane16<2>, tiles, dim3(NLM_BLK * NLM_BLK), 0, stream, src, h, w, c->d_table[1], c->table_size[1], dst);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipMemcpy(out, dst, px * cn * 2, hipMemcpyDeviceToHost));
    } else {
        return fail("bad stage");
    }
    return 0;
}

}  // extern "C"
