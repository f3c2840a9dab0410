// uva_api.hip -- C ABI (include/uva.h) and device runtime of libuva.so.
//
// Replaces the ncnn_vulkan surface used by the reference worker functions
// (upscale/upscale_processing.py:54-73 init_worker, :258-299 apply_model, :395-477 process_tile,
// :480-542 upscale_image; test_gpus.py:47-67 enumeration).  One uva_net = one ncnn.Net: it owns a
// HIP stream, the packed weights, and a small cache of per-geometry workspaces (zero-bordered
// fp16 NHWC ping-pong planes) sized for 288 GB of HBM: nothing is freed between frames.
#include "../../include/uva.h"
#include "uva_crop.h"
#include "uva_kernels.hip.h"
#include "uva_model.h"
#include "uva_net.h"
#include "uva_pixfmt.h"
#include "uva_plan.h"
#include "uva_png.h"
#include "uva_repeat.h"
#include "uva_resize.h"
#include "uva_rt.h"
#include "uva_submit.h"
#include "uva_wino.h"
#include "uva_sub5.h"
#include "uva_sub10.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <vector>

using namespace uva;

namespace {

thread_local std::string g_err;

std::mutex g_nets_mu;
std::set<uva_net*> g_nets;

}  // namespace

int uva::fail(const std::string& msg)
{
    g_err = msg;
    return 1;
}

int uva::select_device(int device)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail("no HIP device available: libuva has no CPU path");
    if (device < 0 || device >= count || device >= kMaxDevices) return fail("HIP device " + std::to_string(device) + " does not exist");
    HIP_TRY(hipSetDevice(device));
    return 0;
}

namespace {

template <int NF, int MODE, int R>
int launch_conv_t(uva_net* n, const ConvArgs& a)
{
    const size_t lds = conv_lds_bytes<NF>(MODE == 0 ? 0 : R);
    auto kfn = conv3x3_kernel<NF, MODE, R>;
    // a net runs at most one trunk (MODE 0) and the u8 / f32 tails (MODE 1 / 2) of its own graph: slots 0-2
    if (!n->attr_set[MODE]) {
        HIP_TRY(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        n->attr_set[MODE] = true;
    }
    // 24-feature nets: 160 VGPRs and ~52 KB of LDS per workgroup leave room for two persistent
    // workgroups per CU, whose k-loops and epilogues then overlap (the 64-feature tails fill the
    // register file with weights: one workgroup per CU)
    // (measured at 1080p, 1x HurrDeblur: 1 per CU 1 658 fps, 2 per CU 2 145 fps, 3 per CU 1 905 fps)
    const int per_cu = NF == 24 ? 2 : 1;
    const int grid = persistent_grid(n->ncu) * per_cu;
    hipLaunchKernelGGL(kfn, dim3(grid), dim3(256), lds, n->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// trunk layer of the 64-feature nets: split-channel ping-pong kernel, one 8-wave workgroup per CU, 4-row tiles
template <int ABL>
int launch_trunk64_t(uva_net* n, const ConvArgs& a)
{
    const size_t lds = trunk_lds_bytes<64>();
    auto kfn = trunk_kernel<64, ABL>;
    constexpr int SLOT = 3 + (ABL == 0 ? 0 : ABL == 1 ? 1 : ABL == 2 ? 2 : 3);   // slots 3-6
    if (!n->attr_set[SLOT]) {
        HIP_TRY(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        n->attr_set[SLOT] = true;
    }
    const int grid = persistent_grid(n->ncu);
    hipLaunchKernelGGL(kfn, dim3(grid), dim3(512), lds, n->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_trunk64(uva_net* n, const ConvArgs& a, int ablate = 0)
{
#ifdef UVA_INSTRUMENT
    if (ablate == 1) return launch_trunk64_t<1>(n, a);
    if (ablate == 2) return launch_trunk64_t<2>(n, a);
    if (ablate == 4) return launch_trunk64_t<4>(n, a);
#endif
    (void)ablate;
    return launch_trunk64_t<0>(n, a);
}

template <int NF>
int launch_conv_nf(uva_net* n, int mode, int r, const ConvArgs& a)
{
    if (mode == 0) return launch_conv_t<NF, 0, 1>(n, a);
    if (mode == 1) {
        if (r == 1) return launch_conv_t<NF, 1, 1>(n, a);
        if (r == 2) return launch_conv_t<NF, 1, 2>(n, a);
        if (r == 4) return launch_conv_t<NF, 1, 4>(n, a);
    } else {
        if (r == 1) return launch_conv_t<NF, 2, 1>(n, a);
        if (r == 2) return launch_conv_t<NF, 2, 2>(n, a);
        if (r == 4) return launch_conv_t<NF, 2, 4>(n, a);
    }
    return fail("no kernel for this scale");
}

int launch_conv(uva_net* n, int mode, const ConvArgs& a)
{
    if (n->g.nf == 64) return launch_conv_nf<64>(n, mode, n->g.scale, a);
    if (n->g.nf == 24) return launch_conv_nf<24>(n, mode, n->g.scale, a);
    return fail("no kernel for this trunk width");
}

// does the net have the ping-pong tails (the 64-feature 2x and 4x nets), which the 16-bit route needs?
bool has_tail64(const uva_net* n) { return n->g.nf == 64 && (n->g.scale == 2 || n->g.scale == 4) && n->layers.back().wpk16; }

// u8 tails of the 64-feature 2x and 4x nets: ping-pong kernels on 4-row tiles (the other tails: conv3x3_kernel).  u16: the same
// kernels on u16 BGR frames (the 16-bit route; the callers have refused every other net)
int launch_tail_u8(uva_net* n, const Workspace* ws, ConvArgs ca, bool u16 = false)
{
    if (has_tail64(n)) {
        const bool x4 = n->g.scale == 4;
        size_t lds;
        void (*kfn)(ConvArgs);
        if (u16) {
            lds = x4 ? tail4_lds_bytes<64, uint16_t>() : tail_lds_bytes<64, uint16_t>();
            kfn = x4 ? tail4_kernel<64, uint16_t> : tail_kernel<64, 2, uint16_t>;
        } else {
            lds = x4 ? tail4_lds_bytes<64>() : tail_lds_bytes<64>();
            kfn = x4 ? tail4_kernel<64, uint8_t> : tail_kernel<64, 2, uint8_t>;
        }
        const int slot = u16 ? 10 : 7;
        if (!n->attr_set[slot]) {
            HIP_TRY(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            n->attr_set[slot] = true;
        }
        const int grid = persistent_grid(n->ncu);
        const int per_launch = 8 * (2 * (grid / 8)) * ((TAIL_SCHED_MAX - TRUNK_LOOKAHEAD) / 2 - 1);
        ca.sched4 = ws->d_sched4;
        ca.wpk = n->layers.back().wpk16;
        for (int base = 0; base < ws->ntiles4; base += per_launch) {
            ca.tile_base = base;
            ca.ntiles = std::min(per_launch, ws->ntiles4 - base);
            ca.tiles_per_xcd = (ca.ntiles + 7) / 8;
            hipLaunchKernelGGL(kfn, dim3(grid), dim3(512), lds, n->stream, ca);
            HIP_TRY(hipGetLastError());
        }
        return 0;
    }
    if (u16) return fail("the 16-bit route has no tail for this net");
    return launch_conv(n, 1, ca);
}

// one trunk layer: the 64-feature nets use the split-channel kernel on 4-row tiles
int launch_trunk(uva_net* n, const Workspace* ws, ConvArgs ca, int ablate = 0)
{
    if (n->g.nf == 64) {
        // a workgroup's tile schedule must fit its LDS table: split very large frames into launches
        const int grid = persistent_grid(n->ncu);
        const int per_launch = 8 * (2 * (grid / 8)) * ((TRUNK_SCHED_MAX - TRUNK_LOOKAHEAD) / 2 - 1);
        ca.sched4 = ws->d_sched4;
        for (int base = 0; base < ws->ntiles4; base += per_launch) {
            ca.tile_base = base;
            ca.ntiles = std::min(per_launch, ws->ntiles4 - base);
            ca.tiles_per_xcd = (ca.ntiles + 7) / 8;
            if (launch_trunk64(n, ca, ablate)) return 1;
        }
        return 0;
    }
    ca.ntiles = ws->ntiles;
    ca.tiles_per_xcd = (ws->ntiles + 7) / 8;
    return launch_conv(n, 0, ca);
}

int launch_trunk2(uva_net* n, const Workspace* ws, const Trunk2Args& a)
{
    const size_t lds = trunk2_lds_bytes<64>();
    auto kfn = trunk2_kernel<64>;
    if (!n->attr_set[8]) {
        HIP_TRY(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        n->attr_set[8] = true;
    }
    hipLaunchKernelGGL(kfn, dim3(ws->grid2), dim3(512), lds, n->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// layers i, i + 1 of the net in one trunkw_kernel launch.  in_negated: the input's channels with a slope above 1 (layer i - 1's)
// are still negated; carry_out: leave layer i + 1's that way for the next launch (its first layer's weights take the sign back)
int launch_trunkw(uva_net* n, const Workspace* ws, TrunkwArgs& a, int i, bool in_negated = false, bool carry_out = false)
{
    for (int k = 0; k < 2; ++k) {
        a.wpk[k] = n->layers[i + k].wpk_w;
        a.bias[k] = n->act16 ? n->layers[i + k].bias_w : n->layers[i + k].bias;
        a.slope[k] = n->layers[i + k].slope;
    }
    if (in_negated) a.wpk[0] = n->layers[i].wpk_wn;
    const int act = !n->act16 ? TW_ACT_F32 : (n->layers[i + 1].flip_w && !carry_out) ? TW_ACT_F16_FLIP : TW_ACT_F16;
    HIP_TRY(launch_trunkw_kernel(n->stream, ws->grid2, a, act, n->carry));
    return 0;
}

// the 24-feature 1x net as two launches of five layers (u8 route, one plane); returns 2 when the frame is too large for it
int launch_sub5(uva_net* n, Workspace* ws, const void* src, size_t src_stride, void* dst, size_t dst_stride,
                unsigned long long* dbg = nullptr, int dbg_part = -1)
{
    if (ws->sub5_unfit) return 2;
    if (!ws->d_rows5) {
        std::vector<uint4> rows;
        std::vector<int> nrows;
        ws->grid5 = persistent_grid(n->ncu);
        std::string err;
        const int rc = build_sub5_rows(ws->h, ws->w, ws->grid5, rows, nrows, &ws->max_rows5, err);
        if (rc == 1) return fail(err);
        if (rc) {
            ws->sub5_unfit = true;
            return 2;
        }
        DevPtr<char> d_mid;
        DevPtr<uint4> d_rows;
        DevPtr<int> d_nrows;
        hipError_t e = alloc_into(d_mid, (size_t)ws->h * ws->w * S5_MIDB);
        if (e == hipSuccess) e = alloc_into(d_rows, rows.size() * sizeof(uint4));
        if (e == hipSuccess) e = alloc_into(d_nrows, nrows.size() * sizeof(int));
        if (e == hipSuccess) e = hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(uint4), hipMemcpyHostToDevice, n->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_nrows, nrows.data(), nrows.size() * sizeof(int), hipMemcpyHostToDevice, n->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(n->stream);
        if (e != hipSuccess) return fail(std::string("sub5 workspace: ") + hipGetErrorString(e));
        ws->d_mid5 = std::move(d_mid); ws->d_rows5 = std::move(d_rows); ws->d_nrows5 = std::move(d_nrows);
    }
    for (int part = 0; part < 2; ++part) {
        Sub5Args a;
        std::memset(&a, 0, sizeof a);
        a.src = (const uint8_t*)src; a.src_stride = src_stride;
        a.dst = (uint8_t*)dst; a.dst_stride = dst_stride;
        a.mid = ws->d_mid5;
        a.h = ws->h; a.w = ws->w;
        a.rows = ws->d_rows5; a.nrows = ws->d_nrows5; a.max_rows = ws->max_rows5;
        a.dbg = part == dbg_part ? dbg : nullptr;
        for (int i = 0; i < S5_NL; ++i) {
            a.wpk[i] = n->layers[S5_NL * part + i].wpk_s10;
            a.bias[i] = n->layers[S5_NL * part + i].bias_s10;
            a.slope[i] = n->layers[S5_NL * part + i].slope;
        }
        HIP_TRY(launch_sub5_kernel(n->stream, ws->grid5, a, part));
    }
    return 0;
}

// the row lists of `frames` frames per launch (sub10_kernel; one frame: sub10_kernel16 as well), built on first use;
// 0 = there, 1 = error, 2 = that many frames do not fit the kernel's row table (the workspace remembers)
int ensure_sub10_rows(uva_net* n, Workspace* ws, int frames)
{
    if (ws->sub10_unfit || frames < 1 || frames > ws->sub10_max_batch) return 2;
    const int bi = frames - 1;
    if (!ws->d_rows10[bi]) {
        std::vector<uint4> rows;
        std::vector<int> nrows;
        ws->grid10 = persistent_grid(n->ncu);
        std::string err;
        const int rc = build_sub10_rows(ws->h, ws->w, frames, ws->grid10, rows, nrows, &ws->max_rows10[bi], err);
        if (rc == 1) return fail(err);
        if (rc) {
            if (frames == 1) ws->sub10_unfit = true;
            ws->sub10_max_batch = frames - 1;
            return 2;
        }
        DevPtr<uint4> d_rows;
        DevPtr<int> d_nrows;
        hipError_t e = alloc_into(d_rows, rows.size() * sizeof(uint4));
        if (e == hipSuccess) e = alloc_into(d_nrows, nrows.size() * sizeof(int));
        if (e == hipSuccess) e = hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(uint4), hipMemcpyHostToDevice, n->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_nrows, nrows.data(), nrows.size() * sizeof(int), hipMemcpyHostToDevice, n->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(n->stream);
        if (e != hipSuccess) return fail(std::string("sub10 row table: ") + hipGetErrorString(e));
        ws->d_rows10[bi] = std::move(d_rows);
        ws->d_nrows10[bi] = std::move(d_nrows);
    }
    return 0;
}

// the whole 24-feature 1x net in one launch (u8 route, one plane per frame), `frames` frames of the workspace's geometry at once;
// returns 2 when that many frames do not fit the kernel's row table (the caller takes fewer, or for one frame another path)
int launch_sub10(uva_net* n, Workspace* ws, const void* const* srcs, size_t src_stride, void* const* dsts, size_t dst_stride, int frames,
                 unsigned long long* dbg = nullptr)
{
    if (const int rc = ensure_sub10_rows(n, ws, frames)) return rc;
    const int bi = frames - 1;
    Sub10Args a;
    std::memset(&a, 0, sizeof a);
    for (int f = 0; f < S10_MAXB; ++f) {       // (unused slots repeat the last frame: never addressed, never null)
        a.src[f] = (const uint8_t*)srcs[std::min(f, frames - 1)];
        a.dst[f] = (uint8_t*)dsts[std::min(f, frames - 1)];
    }
    a.src_stride = src_stride;
    a.dst_stride = dst_stride;
    a.h = ws->h; a.w = ws->w;
    a.rows = ws->d_rows10[bi]; a.nrows = ws->d_nrows10[bi]; a.max_rows = ws->max_rows10[bi];
    a.dbg = dbg;
    for (int i = 0; i < S10_NL; ++i) {
        a.wpk[i] = n->layers[i].wpk_s10;
        a.bias[i] = n->layers[i].bias_s10;
        a.slope[i] = n->layers[i].slope;
    }
    HIP_TRY(launch_sub10_kernel(n->stream, ws->grid10, a));
    return 0;
}
int launch_sub10(uva_net* n, Workspace* ws, const void* src, size_t src_stride, void* dst, size_t dst_stride, unsigned long long* dbg = nullptr)
{
    return launch_sub10(n, ws, &src, src_stride, &dst, dst_stride, 1, dbg);
}

bool is_sub10_net(const uva_net* n)
{
    return !n->generic && n->g.nf == 24 && n->g.scale == 1 && (int)n->g.convs.size() == S10_NL;
}

// two trunk layers of the 24-feature net per launch (pair24_kernel), two persistent workgroups per CU
int launch_pair24(uva_net* n, const ConvArgs& a)
{
    const size_t lds = pair24_lds_bytes();
    if (!n->attr_set[9]) {
        HIP_TRY(hipFuncSetAttribute((const void*)pair24_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        n->attr_set[9] = true;
    }
    const int grid = persistent_grid(n->ncu) * 2;
    hipLaunchKernelGGL(pair24_kernel, dim3(grid), dim3(256), lds, n->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_head(uva_net* n, bool f32, const HeadArgs& a, bool u16 = false)
{
    if (u16) {                  // the 16-bit route: headp_kernel<64, 2> only (its callers have refused every other net)
        if (n->g.nf != 64 || !a.sink) return fail("the 16-bit route has no head for this net");
        const dim3 grid(std::min(a.ntiles, n->ncu * HEADP_WG_PER_CU)), block(256);
        hipLaunchKernelGGL((headp_kernel<64, 2>), grid, block, headp_lds_bytes<64>(), n->stream, a);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // headp_kernel (persistent, the next tile's pixels requested while this one is computed) unless UVA_HEAD_PERSIST=0
    const char* const hp = uva::debug_env("UVA_HEAD_PERSIST");        // (read per call: the GPU test switches it between two frames)
    const bool persist = !hp || std::atoi(hp) != 0;
    if (persist && a.sink) {
        const dim3 grid(std::min(a.ntiles, n->ncu * HEADP_WG_PER_CU)), block(256);
        if (n->g.nf == 64) {
            const size_t lds = headp_lds_bytes<64>();
            if (f32) hipLaunchKernelGGL((headp_kernel<64, 1>), grid, block, lds, n->stream, a);
            else hipLaunchKernelGGL((headp_kernel<64, 0>), grid, block, lds, n->stream, a);
        } else {
            const size_t lds = headp_lds_bytes<24>();
            if (f32) hipLaunchKernelGGL((headp_kernel<24, 1>), grid, block, lds, n->stream, a);
            else hipLaunchKernelGGL((headp_kernel<24, 0>), grid, block, lds, n->stream, a);
        }
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const dim3 grid(a.ntiles), block(256);
    if (n->g.nf == 64) {
        if (f32) hipLaunchKernelGGL((head_kernel<64, 1>), grid, block, 0, n->stream, a);
        else hipLaunchKernelGGL((head_kernel<64, 0>), grid, block, 0, n->stream, a);
    } else {
        if (f32) hipLaunchKernelGGL((head_kernel<24, 1>), grid, block, 0, n->stream, a);
        else hipLaunchKernelGGL((head_kernel<24, 0>), grid, block, 0, n->stream, a);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// the net's weights on its device, into `d` (all of it, or an error: ensure_device keeps nothing of a `d` that is not ready)
int build_device(const uva_net* n, NetDevice& d)
{
    HIP_TRY(make_stream(d.stream));
    HIP_TRY(alloc_into(d.d_sink, 64 * 128 + 256));
    if (n->generic) {
        // generic graph: every convolution's MFMA image ([tap][cin/32][cout/16][lane][8]) and padded bias
        const GenericGraph& gg = n->gg;
        d.gd.convs.resize(gg.convs.size());
        for (const GLayer& gl : gg.layers) {
            if (gl.kind != GLayer::CONV) continue;
            const ConvWeights& c = gg.convs[gl.conv];
            GenericDevice::ConvDev& cd = d.gd.convs[gl.conv];
            cd.cin_pad = GenericDevice::pad32(c.cin);
            cd.cout_pad = (c.cout + 15) / 16 * 16;
            std::vector<uint16_t> pk;
            pack_generic(c, gl.ksize, cd.cin_pad, cd.cout_pad, pk);
            if (upload(cd.wpk, pk.data(), pk.size() * 2, d.stream)) return 1;
            if (cd.cout_pad <= 64 && cd.cin_pad <= 192 && g_conv3_lds_bytes(cd.cin_pad, cd.cout_pad / 16, gl.ksize) <= 160 * 1024) {
                std::vector<uint16_t> pkl;
                pack_generic(c, gl.ksize, cd.cin_pad, cd.cout_pad, pkl, true);
                if (upload(cd.wpk_lds, pkl.data(), pkl.size() * 2, d.stream)) return 1;
                HIP_TRY(hipStreamSynchronize(d.stream));
            }
            if (gl.ksize == 3 && cd.cin_pad == 192 && cd.cout_pad == 64) {           // a dense block's last convolution: g_conv3_sww
                std::vector<uint16_t> pkw;
                pack_generic_wino(c, cd.cin_pad, cd.cout_pad, pkw);
                if (upload(cd.wpk_w, pkw.data(), pkw.size() * 2, d.stream)) return 1;
                HIP_TRY(hipStreamSynchronize(d.stream));
            }
            std::vector<float> b((size_t)cd.cout_pad, 0.f);
            std::copy(c.bias.begin(), c.bias.end(), b.begin());
            if (upload(cd.bias, b.data(), b.size() * 4, d.stream)) return 1;
            HIP_TRY(hipStreamSynchronize(d.stream));
        }
        d.gd.rdbs = find_rdbs(gg);
        d.gd.prelu.resize(gg.prelu.size());
        for (size_t i = 0; i < gg.prelu.size(); ++i) {
            if (upload(d.gd.prelu[i], gg.prelu[i].data(), gg.prelu[i].size() * 4, d.stream)) return 1;
            HIP_TRY(hipStreamSynchronize(d.stream));
        }
        d.dev_ready = true;
        return 0;
    }
    // weights: head, trunk..., tail
    const Graph& g = n->g;
    d.layers.resize(g.convs.size());
    for (size_t i = 0; i < g.convs.size(); ++i) {
        std::vector<uint16_t> pk;
        int mf = 0;
        if (i == 0) pack_head(g.convs[i], pk, &mf);
        else if (g.nf == 64 && i + 1 < g.convs.size()) { pack_trunk64(g.convs[i], pk); mf = 2; }   // trunk_kernel<64>
        else pack_conv3x3(g.convs[i], g.nf, pk, nullptr, &mf);
        DeviceLayer& dl = d.layers[i];
        if (upload(dl.wpk, pk.data(), pk.size() * 2, d.stream)) return 1;
        std::vector<uint16_t> pkw;
        if (g.nf == 64 && i > 0 && i + 1 < g.convs.size()) {
            // Pairs are (1, 2), (3, 4), ...: an odd layer is the first of its launch.  With the PReLU on packed fp16 a channel
            // whose slope exceeds 1 is computed negated (uva_wino.h): the first layer's stay so on their way through LDS into
            // the second layer (in_sign), the second layer's get their sign back in front of the stores.
            std::vector<float> sin(64, 1.f), sout(64, 1.f), bw(64, 0.f);
            if (n->act16) {
                if (!(i & 1))
                    for (int c = 0; c < 64; ++c) sin[c] = g.slopes[i - 1][c] > 1.f ? -1.f : 1.f;
                for (int c = 0; c < 64; ++c) {
                    sout[c] = g.slopes[i][c] > 1.f ? -1.f : 1.f;
                    dl.flip_w = dl.flip_w || sout[c] < 0.f;
                }
            }
            for (int c = 0; c < 64; ++c) bw[c] = sout[c] * g.convs[i].bias[c];
            pack_trunk64_wino(g.convs[i], pkw, sin.data(), sout.data());
            if (upload(dl.wpk_w, pkw.data(), pkw.size() * 2, d.stream)) return 1;
            if (upload(dl.bias_w, bw.data(), bw.size() * 4, d.stream)) return 1;
            HIP_TRY(hipStreamSynchronize(d.stream));
            if (n->act16 && (i & 1) && i >= 3) {
                // first layer of a launch behind another launch: a second image for an input whose flipped channels arrive negated
                bool any = false;
                for (int c = 0; c < 64; ++c) {
                    sin[c] = g.slopes[i - 1][c] > 1.f ? -1.f : 1.f;
                    any = any || sin[c] < 0.f;
                }
                if (any) {
                    pack_trunk64_wino(g.convs[i], pkw, sin.data(), sout.data());
                    if (upload(dl.wpk_wn, pkw.data(), pkw.size() * 2, d.stream)) return 1;
                    HIP_TRY(hipStreamSynchronize(d.stream));
                }
            }
        }
        std::vector<uint16_t> pk16;
        if (g.nf == 64 && (g.scale == 2 || g.scale == 4) && i + 1 == g.convs.size()) {
            pack_tail64(g.convs[i], pk16);
            if (upload(dl.wpk16, pk16.data(), pk16.size() * 2, d.stream)) return 1;
        }
        if (g.nf == 24 && g.scale == 1 && g.convs.size() == (size_t)S10_NL) {
            // channels whose PReLU slope exceeds 1 travel negated between the layers (uva_model.h pack_sub16)
            std::vector<float> sin(g.convs[i].cin, 1.f), sout(g.convs[i].cout, 1.f), bs(32, 0.f);
            if (i > 0)
                for (int c = 0; c < g.convs[i].cin; ++c) sin[c] = g.slopes[i - 1][c] > 1.f ? -1.f : 1.f;
            if (i + 1 < g.convs.size())
                for (int c = 0; c < g.convs[i].cout; ++c) sout[c] = g.slopes[i][c] > 1.f ? -1.f : 1.f;
            const int brow = g.convs[i].cout == 3 ? 4 : 1;       // (the last layer's channel j sits in MFMA row 4j: pack_sub16)
            for (int c = 0; c < g.convs[i].cout; ++c) bs[brow * c] = sout[c] * g.convs[i].bias[c];
            std::vector<uint16_t> pks;
            pack_sub16(g.convs[i], pks, nullptr, nullptr, sin.data(), sout.data());
            if (upload(dl.wpk_s10, pks.data(), pks.size() * 2, d.stream)) return 1;
            if (upload(dl.bias_s10, bs.data(), bs.size() * 4, d.stream)) return 1;
            HIP_TRY(hipStreamSynchronize(d.stream));
        }
        std::vector<float> b((size_t)mf * 32, 0.f), s((size_t)mf * 32, 0.f);
        std::copy(g.convs[i].bias.begin(), g.convs[i].bias.end(), b.begin());
        if (upload(dl.bias, b.data(), b.size() * 4, d.stream)) return 1;
        if (i + 1 < g.convs.size()) {
            std::copy(g.slopes[i].begin(), g.slopes[i].end(), s.begin());
            if (upload(dl.slope, s.data(), s.size() * 4, d.stream)) return 1;
        }
        HIP_TRY(hipStreamSynchronize(d.stream));   // pk / b / s go out of scope
    }
    d.dev_ready = true;
    return 0;
}

int ensure_device(uva_net* n)
{
    if (n->generic ? !(n->gg.param_loaded && n->gg.model_loaded) : !(n->g.param_loaded && n->g.model_loaded))
        return fail("net has no model: call load_param and load_model first");
    if (n->dev_ready) {
        HIP_TRY(hipSetDevice(n->device));
        return 0;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail("no HIP device available: libuva has no CPU path");
    if (n->device < 0 || n->device >= count)
        return fail("HIP device " + std::to_string(n->device) + " does not exist (" + std::to_string(count) + " visible)");
    HIP_TRY(hipSetDevice(n->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, n->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(std::string("libuva is built for gfx950 (MI355X) only; device is ") + prop.gcnArchName);
    n->ncu = prop.multiProcessorCount;
    if (const char* e = uva::debug_env("UVA_TRUNK_FUSION")) n->fuse_pairs = std::atoi(e) != 0;
    if (const char* e = uva::debug_env("UVA_TRUNK_WINO")) n->wino = std::atoi(e) != 0;
    if (const char* e = uva::debug_env("UVA_TW_ACT16")) n->act16 = std::atoi(e) != 0;
    if (const char* e = uva::debug_env("UVA_TW_CARRY")) n->carry = std::atoi(e) != 0;
    if (const char* e = uva::debug_env("UVA_SUB10")) n->fuse_all = std::atoi(e) != 0;
    if (const char* e = uva::debug_env("UVA_SUB5")) n->split5 = std::atoi(e) != 0;
    if (const char* e = uva::debug_env("UVA_GENERIC_LDS")) n->generic_lds_conv = std::atoi(e) != 0;
    if (const char* e = uva::debug_env("UVA_GENERIC_FUSE_ADD")) n->generic_fuse_add = std::atoi(e) != 0;
    // built in a local and moved in when complete: a failure on the way leaves the net without device state, and a later
    // call starts from scratch
    NetDevice d;
    if (build_device(n, d)) {
        if (d.stream) (void)hipStreamSynchronize(d.stream);      // (uploads may be queued still)
        return 1;
    }
    static_cast<NetDevice&>(*n) = std::move(d);
    return 0;
}

// The planner's A/B switches, read per call (the tests flip them between calls): UVA_TW_SIX (1 / 0: six-row segment starts
// always / never), UVA_TW_FOLD (0: no folded last strips; 14: the known-bad first version), UVA_T2_NARROW (0: every
// trunk2 strip computes both fragment columns).
PlanOpts plan_switches()
{
    PlanOpts o;
    if (const char* e = uva::debug_env("UVA_TW_SIX")) o.tw.six_mode = std::atoi(e) != 0 ? 1 : 0;
    if (const char* e = uva::debug_env("UVA_TW_FOLD")) {
        o.tw.fold = std::atoi(e) != 0;
        if (std::atoi(e) == 14) o.tw.fold_maxw = 14;
    }
    if (const char* e = uva::debug_env("UVA_T2_NARROW")) o.narrow_ok = std::atoi(e) != 0;
    return o;
}

static_assert(Geo<64, 4>::PIXB == PLAN_PIXB, "the planner's byte offsets are those of the 64-feature activations");

int get_workspace(uva_net* n, int h, int w, int tile_size, int border, Workspace** out)
{
    normalize_tiling(tile_size, border);
    for (auto it = n->wss.begin(); it != n->wss.end(); ++it)
        if (it->h == h && it->w == w && it->tile_size == tile_size && it->border == border) {
            n->wss.splice(n->wss.begin(), n->wss, it);
            *out = &n->wss.front();
            return 0;
        }
    Workspace ws;
    ws.h = h; ws.w = w; ws.tile_size = tile_size; ws.border = border;
    // everything that can be refused is checked BEFORE anything is allocated
    FramePlan plan;
    std::string err;
    if (n->g.nf == 64) ws.grid2 = persistent_grid(n->ncu);
    if (plan_frame(h, w, tile_size, border, n->g.nf, ws.grid2, plan_switches(), plan, err)) return fail(err);
    static_cast<PlaneLayout&>(ws) = plan;
    ws.max_steps2 = plan.max_steps2;
    ws.max_stepsw = plan.max_stepsw;
    const size_t bytes = ws.act_pixels * (size_t)n->g.nf * 2 + 2 * ws.guard_bytes;
    // LRU over the cached geometries, by bytes (the fused route keeps one workspace per frame size, the
    // float / Extractor route one per distinct tile shape -- 9 for a 4000x2200 frame): plenty fit 288 GB
    constexpr size_t CACHE_BYTES = (size_t)96 << 30;
    constexpr size_t CACHE_ENTRIES = 32;
    auto cached_bytes = [&]() {
        size_t t = 0;
        for (auto& w2 : n->wss) t += w2.alloc_bytes;
        return t;
    };
    while (!n->wss.empty() && (n->wss.size() >= CACHE_ENTRIES || cached_bytes() + 2 * bytes > CACHE_BYTES)) {
        HIP_TRY(hipStreamSynchronize(n->stream));
        if (n->last.ws == &n->wss.back()) n->last = LastCall();
        n->wss.pop_back();
    }
    // (`ws` is a local until it is complete: a failure from here on releases what it already holds)
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(alloc_into(ws.act_base[i], bytes));
        HIP_TRY(hipMemsetAsync(ws.act_base[i], 0, bytes, n->stream));   // the zero border lives here forever
        ws.act[i] = (_Float16*)(ws.act_base[i] + ws.guard_bytes);
    }
    ws.alloc_bytes = 2 * bytes;
    if (upload(ws.d_planes, ws.planes.data(), ws.planes.size() * sizeof(PlaneDesc), n->stream)) return 1;
    if (n->g.nf == 64) {
        if (upload(ws.d_sched4, plan.sched4.data(), plan.sched4.size() * sizeof(uint4), n->stream)) return 1;
        if (upload(ws.d_steps2, plan.steps2.data(), plan.steps2.size() * sizeof(Trunk2Step), n->stream)) return 1;
        if (upload(ws.d_nsteps2, plan.nsteps2.data(), plan.nsteps2.size() * sizeof(int), n->stream)) return 1;
        if (upload(ws.d_stepsw, plan.stepsw.data(), plan.stepsw.size() * sizeof(Trunk2Step), n->stream)) return 1;
        if (upload(ws.d_nstepsw, plan.nstepsw.data(), plan.nstepsw.size() * sizeof(int), n->stream)) return 1;
    }
    HIP_TRY(hipStreamSynchronize(n->stream));
    n->wss.push_front(std::move(ws));
    *out = &n->wss.front();
    return 0;
}

// an event from `pool`, or a new one with `flags`; an empty handle (with the error recorded) if the runtime cannot create another
Event take_from(std::vector<Event>& pool, unsigned flags)
{
    Event e;
    if (!pool.empty()) {
        e = std::move(pool.back());
        pool.pop_back();
        return e;
    }
    const hipError_t rc = make_event(e, flags);
    if (rc != hipSuccess) fail(std::string("hipEventCreate: ") + hipGetErrorString(rc));
    return e;
}

// An event that orders one stream behind another (default flags: its release makes the producer's writes visible), for the
// length of a scope: it goes back to its net's pool on EVERY path out (HIP_TRY returns from the middle of a function; a wait
// has captured the recorded state by then, or nothing was recorded at all)
struct SyncEventScope {
    uva_net* n;
    Event e;
    explicit SyncEventScope(uva_net* net) : n(net), e(take_from(net->ev_sync_free, hipEventDisableTiming)) {}
    ~SyncEventScope() { if (e) n->ev_sync_free.push_back(std::move(e)); }
    SyncEventScope(const SyncEventScope&) = delete;
    SyncEventScope& operator=(const SyncEventScope&) = delete;
};

// Frames whose last event has completed are added to the statistics and their events recycled; frames still
// in flight (pipelined submits) stay pending for the next call.
void resolve_events(uva_net* n)
{
    std::vector<EvSet> keep;
    for (auto& s : n->ev_pending) {
        if (hipEventQuery(s.e[3]) == hipErrorNotReady) {
            keep.push_back(std::move(s));
            continue;
        }
        float ms[3] = {0, 0, 0};
        bool ok = true;
        for (int k = 0; k < 3; ++k) ok &= hipEventElapsedTime(&ms[k], s.e[k], s.e[k + 1]) == hipSuccess;
        if (ok) {
            n->launches[0] += 1; n->total_ms[0] += ms[0];
            n->launches[1] += s.ntrunk; n->total_ms[1] += ms[1];
            n->launches[2] += 1; n->total_ms[2] += ms[2];
        }
        for (Event& e : s.e) n->ev_free.push_back(std::move(e));
    }
    n->ev_pending.swap(keep);
    std::vector<EvPair> keep2;
    for (auto& q : n->ev_pairs) {
        if (hipEventQuery(q.b) == hipErrorNotReady) { keep2.push_back(std::move(q)); continue; }
        float ms = 0;
        if (hipEventElapsedTime(&ms, q.a, q.b) == hipSuccess) { n->launches[q.kind] += 1; n->total_ms[q.kind] += ms; }
        n->ev_free.push_back(std::move(q.a));
        n->ev_free.push_back(std::move(q.b));
    }
    n->ev_pairs.swap(keep2);
}

// The whole graph for one frame.  stop_after >= 0: run only convolutions 0..stop_after (debug).
// does this call go through sub10_kernel / sub5_kernel (the 24-feature 1x net on a whole-frame plane, u8 in / u8 out)?
bool sub10_route(const uva_net* n, const Workspace* ws, bool f32, int stop_after)
{
    const Graph& g = n->g;
    return n->fuse_all && !f32 && stop_after < 0 && g.nf == 24 && g.scale == 1 && (int)g.convs.size() == S10_NL && ws->planes.size() == 1 &&
           n->layers[0].wpk_s10 && !ws->sub10_unfit;
}

// `frames` frames (1 .. S10_MAXB) of the workspace's geometry through the 1x net in ONE launch, with the profiling events of one
// launch around it; 0 = done, 1 = error, 2 = does not fit (fewer frames, or for one frame the layer-pair path)
int run_sub10(uva_net* n, Workspace* ws, const void* const* srcs, size_t src_stride, void* const* dsts, size_t dst_stride, int frames)
{
    EvScope ev1(n, 4, n->prof);
    if (n->prof && !ev1.taken()) return 1;
    HIP_TRY(ev1.record(0));
    HIP_TRY(ev1.record(1));
    int rc = 2, launches = 2;
    if (frames == 1 && n->split5 && !ws->sub5_unfit) rc = launch_sub5(n, ws, srcs[0], src_stride, dsts[0], dst_stride);
    if (rc == 2) { rc = launch_sub10(n, ws, srcs, src_stride, dsts, dst_stride, frames); launches = 1; }
    if (rc == 0) {
        HIP_TRY(ev1.record(2));
        HIP_TRY(ev1.last(launches));
    }
    return rc;
}

// the 16-bit route of the 1x net (sub10_kernel16): one u16 frame, whole-frame plane, one launch -- or a
// refusal.  Nothing falls back to another kernel: there is no other u16 path for this net.
int run_sub10_u16(uva_net* n, Workspace* ws, const void* src, size_t src_stride, void* dst, size_t dst_stride)
{
    if (ws->planes.size() != 1 || !n->layers[0].wpk_s10) return fail("the 16-bit route runs the 1x net on whole frames only (tile_size 0)");
    // the tail waves read the residual from the input frame while other workgroups store: the frames must not overlap
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + src_stride * (size_t)ws->h, d0 = (uintptr_t)dst, d1 = d0 + dst_stride * (size_t)ws->h;
    if (s0 < d1 && d0 < s1) return fail("the 16-bit route of the 1x net needs input and output frames that do not overlap");
    if (ensure_sub10_rows(n, ws, 1) == 1) return 1;
    if (ws->sub10_unfit)
        return fail("the 16-bit route of the 1x net: a frame of " + std::to_string(ws->w) + " x " + std::to_string(ws->h) +
                    " does not fit the fused kernel's row table (frames up to about 2160p do)");
    Sub10Args16 a;
    std::memset(&a, 0, sizeof a);
    a.src = (const uint16_t*)src; a.dst = (uint16_t*)dst;
    a.src_stride = src_stride; a.dst_stride = dst_stride;
    a.h = ws->h; a.w = ws->w;
    a.rows = ws->d_rows10[0]; a.nrows = ws->d_nrows10[0]; a.max_rows = ws->max_rows10[0];
    for (int i = 0; i < S10_NL; ++i) {
        a.wpk[i] = n->layers[i].wpk_s10;
        a.bias[i] = n->layers[i].bias_s10;
        a.slope[i] = n->layers[i].slope;
    }
    EvScope ev(n, 2, n->prof);
    if (n->prof && !ev.taken()) return 1;
    HIP_TRY(ev.record(0));
    HIP_TRY(launch_sub10_kernel16(n->stream, ws->grid10, a));
    HIP_TRY(ev.last(3));
    return 0;
}

// u16: the 16-bit route (u16 HWC BGR in and out; the 64-feature 2x / 4x nets, and the 1x net where uva_net_enable_u16_1x is on)
int run_graph(uva_net* n, Workspace* ws, bool f32, const void* src, size_t src_stride, void* dst,
              size_t dst_stride, int stop_after, bool u16 = false)
{
    const Graph& g = n->g;
    const int nconv = (int)g.convs.size();
    // the 24-feature 1x net on a whole-frame plane, u8 in / u8 out: one launch for all ten convolutions
    if (u16 && is_sub10_net(n)) return run_sub10_u16(n, ws, src, src_stride, dst, dst_stride);
    if (!u16 && sub10_route(n, ws, f32, stop_after)) {
        const int rc = run_sub10(n, ws, &src, src_stride, &dst, dst_stride, 1);
        if (rc != 2) return rc;
    }
    const bool prof = n->prof && stop_after < 0;
    EvScope ev(n, 4, prof);
    if (prof && !ev.taken()) return 1;
    int ntrunk = 0;  // trunk launches of this frame (a fused pair is one launch)
    HIP_TRY(ev.record(0));
    HeadArgs ha;
    std::memset(&ha, 0, sizeof ha);
    ha.planes = ws->d_planes;
    ha.nplanes = (int)ws->planes.size();
    ha.ntiles = ws->ntiles;
    ha.src_u8 = f32 ? nullptr : (const uint8_t*)src;
    ha.src_stride = src_stride;
    ha.src_f32 = f32 ? (const float*)src : nullptr;
    ha.out_act = ws->act[0];
    ha.wpk = n->layers[0].wpk;
    ha.bias = n->layers[0].bias;
    ha.slope = n->layers[0].slope;
    ha.in_scale = f32 ? 1.0f : (float)(1 / 255.0);      // (u16: the operand is v / 257, see headp_kernel)
    ha.sink = n->d_sink;
    if (launch_head(n, f32, ha, u16)) return 1;
    HIP_TRY(ev.record(1));

    ConvArgs ca;
    std::memset(&ca, 0, sizeof ca);
    ca.planes = ws->d_planes;
    ca.nplanes = (int)ws->planes.size();
    ca.ntiles = ws->ntiles;
    ca.tiles_per_xcd = (ws->ntiles + 7) / 8;
    ca.sink = n->d_sink;
    // ping-pong: every launch (one trunk layer, or a fused pair of them) reads act[cur] and writes act[cur ^ 1]
    int cur = 0;
    n->last_act_buf = 0;
    bool negated = false;         // the current activation image holds the last layer's slope > 1 channels negated (see below)
    for (int i = 1; i < nconv - 1; ++i) {
        if (stop_after >= 0 && i > stop_after) return 0;
        // two trunk layers per launch where a pair is wanted in full (a debug tap on layer i itself runs it alone)
        if (n->fuse_pairs && n->wino && ws->d_stepsw && n->layers[i].wpk_w && i + 1 < nconv - 1 && (stop_after < 0 || i + 1 <= stop_after)) {
            // The packed-fp16 PReLU computes channels with a slope above 1 negated (uva_wino.h).  Where the NEXT launch is a
            // trunkw pair as well, this launch leaves its second layer's that way in HBM (no sign restore: four instructions per
            // block row) and the next launch's first layer reads them through weights packed for it (wpk_wn).  Whole frames only:
            // a debug tap (stop_after) keeps every image in the plain convention.
            const bool next_is_pair = stop_after < 0 && i + 3 < nconv - 1 && n->layers[i + 2].wpk_wn != nullptr;
            const bool carry_out = n->act16 && n->carry && next_is_pair && n->layers[i + 1].flip_w;
            TrunkwArgs wa;
            std::memset(&wa, 0, sizeof wa);
            wa.in_act = ws->act_base[cur];
            wa.out_act = ws->act_base[cur ^ 1];
            wa.steps = ws->d_stepsw;
            wa.nsteps = ws->d_nstepsw;
            wa.max_steps = ws->max_stepsw;
            wa.sink = n->d_sink;
            if (launch_trunkw(n, ws, wa, i, negated, carry_out)) return 1;
            negated = carry_out;
            ++ntrunk;
            ++i;
            cur ^= 1;
            n->last_act_buf = cur;
            continue;
        }
        if (n->fuse_pairs && ws->d_steps2 && i + 1 < nconv - 1 && (stop_after < 0 || i + 1 <= stop_after)) {
            Trunk2Args ta;
            std::memset(&ta, 0, sizeof ta);
            ta.in_act = ws->act_base[cur];
            ta.out_act = ws->act_base[cur ^ 1];
            for (int k = 0; k < 2; ++k) {
                ta.wpk[k] = n->layers[i + k].wpk;
                ta.bias[k] = n->layers[i + k].bias;
                ta.slope[k] = n->layers[i + k].slope;
            }
            ta.steps = ws->d_steps2;
            ta.nsteps = ws->d_nsteps2;
            ta.max_steps = ws->max_steps2;
            ta.sink = n->d_sink;
            if (launch_trunk2(n, ws, ta)) return 1;
            ++ntrunk;
            ++i;
            cur ^= 1;
            n->last_act_buf = cur;
            continue;
        }
        ca.in_act = ws->act[cur];
        ca.out_act = ws->act[cur ^ 1];
        ca.wpk = n->layers[i].wpk;
        ca.bias = n->layers[i].bias;
        ca.slope = n->layers[i].slope;
        ca.reverse = i & 1;   // layer 1 walks backwards over what the head wrote last, layer 2 forwards, ...
        if (n->fuse_pairs && g.nf == 24 && i + 1 < nconv - 1 && (stop_after < 0 || i + 1 <= stop_after)) {
            ca.wpk2 = n->layers[i + 1].wpk;
            ca.bias2 = n->layers[i + 1].bias;
            ca.slope2 = n->layers[i + 1].slope;
            ca.ntiles = ws->ntiles;
            ca.tiles_per_xcd = (ws->ntiles + 7) / 8;
            if (launch_pair24(n, ca)) return 1;
            ++ntrunk;
            ++i;
            cur ^= 1;
            n->last_act_buf = cur;
            continue;
        }
        if (launch_trunk(n, ws, ca)) return 1;
        ++ntrunk;
        cur ^= 1;
        n->last_act_buf = cur;
    }
    if (stop_after >= 0) return 0;
    HIP_TRY(ev.record(2));
    ca.ntiles = ws->ntiles;
    ca.tiles_per_xcd = (ws->ntiles + 7) / 8;
    ca.in_act = ws->act[cur];
    ca.reverse = (nconv - 1) & 1;
    ca.out_act = nullptr;
    ca.wpk = n->layers[nconv - 1].wpk;
    ca.bias = n->layers[nconv - 1].bias;
    ca.slope = nullptr;
    if (f32) {
        ca.src_f32 = (const float*)src;
        ca.dst_f32 = (float*)dst;
    } else {
        ca.src_u8 = (const uint8_t*)src;
        ca.src_stride = src_stride;
        ca.dst_u8 = (uint8_t*)dst;
        ca.dst_stride = dst_stride;
    }
    if (f32 ? launch_conv(n, 2, ca) : launch_tail_u8(n, ws, ca, u16)) return 1;
    HIP_TRY(ev.last(ntrunk));
    return 0;
}

int check_dims(const uva_net* n, int h, int w)
{
    if (!n) return fail("null net");
    if (h <= 0 || w <= 0 || (long long)h * w > (1ll << 28)) return fail("bad image size");
    return 0;
}

}  // namespace

// a timing event
// (hipEventDisableSystemFence -- no L2 write-back at a timing event -- measured: no difference in the frame time or in the
// kernel times the events bracket, profiles/r04_ab_results.txt block 18; default events kept)
Event uva::take_event(uva_net* n) { return take_from(n->ev_free, hipEventDefault); }

// The stateless device stages (uva_*_device: denoise, pixel formats, resize) run on a stream of their own between two nets'
// streams.  Both nets, where given, must live on the stage's device ...
int uva::check_fence_nets(int device, uva_net* after, uva_net* before, const char* entry)
{
    for (uva_net* n : {after, before})
        if (n) {
            if (ensure_device(n)) return 1;
            if (n->device != device) return fail(std::string(entry) + ": the net is on another device");
        }
    return 0;
}

// ... what `after` has been asked to do so far (it wrote the stage's input, or still reads its output) comes first ...
int uva::fence_after(uva_net* after, hipStream_t stream)
{
    if (!after) return 0;
    SyncEventScope ev(after);
    if (!ev.e) return 1;
    HIP_TRY(hipEventRecord(ev.e.get(), after->stream));
    HIP_TRY(hipStreamWaitEvent(stream, ev.e.get(), 0));
    return 0;
}

// ... and whatever `before` is asked to do from now on comes after the stage's frame
int uva::fence_before(uva_net* before, hipStream_t stream)
{
    if (!before) return 0;
    SyncEventScope ev(before);
    if (!ev.e) return 1;
    HIP_TRY(hipEventRecord(ev.e.get(), stream));
    HIP_TRY(hipStreamWaitEvent(before->stream, ev.e, 0));
    return 0;
}

extern "C" {

int uva_abi_version(void) { return UVA_ABI_VERSION; }
const char* uva_last_error(void) { return g_err.c_str(); }

int uva_get_gpu_count(void)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    return count;
}

int uva_get_default_gpu_index(void) { return uva_get_gpu_count() > 0 ? 0 : -1; }

int uva_get_gpu_info(int index, int* type, char* name, size_t name_len)
{
    const int count = uva_get_gpu_count();
    if (index < 0 || index >= count) return fail("no such HIP device");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, index));
    if (type) *type = prop.integrated ? 1 : 0;
    if (name && name_len) std::snprintf(name, name_len, "%s (%s)", prop.name, prop.gcnArchName);
    return 0;
}

int uva_get_gpu_pci_bus_id(int index, char* out, size_t out_len)
{
    if (!out || out_len < 13) return fail("buffer too small for a PCI address");
    const int count = uva_get_gpu_count();
    if (index < 0 || index >= count) return fail("no such HIP device");
    HIP_TRY(hipDeviceGetPCIBusId(out, (int)out_len, index));
    return 0;
}

void uva_destroy_gpu_instance(void)
{
    {
        std::lock_guard<std::mutex> lk(g_nets_mu);
        for (uva_net* n : g_nets) n->free_device();
    }
    denoise16_release_all();
    denoise_release_all();
    png_release_all();
    pix_release_all();
    resize_release_all();
}

uva_net* uva_net_create(void)
{
    uva_net* n = new uva_net();
    std::lock_guard<std::mutex> lk(g_nets_mu);
    g_nets.insert(n);
    return n;
}

void uva_net_destroy(uva_net* n)
{
    if (!n) return;
    {
        std::lock_guard<std::mutex> lk(g_nets_mu);
        g_nets.erase(n);
    }
    n->free_device();
    delete n;
}

int uva_net_set_device(uva_net* n, int device)
{
    if (!n) return fail("null net");
    if (device < 0) return fail("negative device index: libuva has no CPU path");
    if (n->dev_ready && device != n->device) n->free_device();
    n->device = device;
    return 0;
}

int uva_net_load_param(uva_net* n, const char* path)
{
    if (!n || !path) return fail("null argument");
    n->free_device();
    n->generic = false;
    n->u16_1x = false;
    n->gg = GenericGraph();
    std::string err;
    // UVA_GENERIC=1 (tests): run even the SRVGGNetCompact graphs through the generic executor
    const char* force = uva::debug_env("UVA_GENERIC");
    if (!(force && std::atoi(force)) && parse_param(path, n->g, err)) return 0;
    // not the SRVGGNetCompact pattern the fused kernels are written for: the generic executor, if every layer
    // type is one it knows (4x_Valar_v1 is); otherwise the first parser's message stands
    std::string gerr;
    if (!parse_param_generic(path, n->gg, gerr)) return fail(gerr.find("unsupported layer type") != std::string::npos ? gerr : err);
    n->generic = true;
    return 0;
}

int uva_net_load_model(uva_net* n, const char* path)
{
    if (!n || !path) return fail("null argument");
    n->free_device();
    std::string err;
    if (n->generic ? !load_bin_generic(path, n->gg, err) : !load_bin(path, n->g, err)) return fail(err);
    return 0;
}

int uva_net_device(const uva_net* n) { return n ? n->device : -1; }

int uva_net_scale(const uva_net* n)
{
    if (!n) return 0;
    if (n->generic) return n->gg.param_loaded ? n->gg.scale : 0;
    return n->g.param_loaded ? n->g.scale : 0;
}
int uva_net_num_features(const uva_net* n)
{
    if (!n) return 0;
    if (n->generic) return n->gg.param_loaded ? n->gg.max_channels : 0;
    return n->g.param_loaded ? n->g.nf : 0;
}
int uva_net_num_convs(const uva_net* n)
{
    if (!n) return 0;
    if (n->generic) return n->gg.param_loaded ? (int)n->gg.convs.size() : 0;
    return n->g.param_loaded ? (int)n->g.convs.size() : 0;
}

int uva_net_synchronize(uva_net* n)
{
    if (!n) return fail("null net");
    if (!n->dev_ready) return 0;
    HIP_TRY(hipSetDevice(n->device));
    HIP_TRY(hipStreamSynchronize(n->stream));
    if (n->s_d2h) HIP_TRY(hipStreamSynchronize(n->s_d2h));   // in-flight pipelined frames (results stay collectable)
    resolve_events(n);
    return 0;
}

int uva_net_wait_for(uva_net* n, uva_net* producer)
{
    if (!n || !producer) return fail("null net");
    if (n == producer || !producer->dev_ready) return 0;
    if (ensure_device(n)) return 1;
    if (producer->device != n->device) return fail("uva_net_wait_for: nets are on different devices");
    SyncEventScope ev(n);           // (recycled at the end of the scope: the wait has captured the recorded state)
    if (!ev.e) return 1;
    HIP_TRY(hipEventRecord(ev.e.get(), producer->stream));
    HIP_TRY(hipStreamWaitEvent(n->stream, ev.e, 0));
    return 0;
}

int uva_net_process_u8_device(uva_net* n, const void* d_in, int h, int w, size_t in_stride, void* d_out,
                              size_t out_stride, int tile_size, int border)
{
    if (check_dims(n, h, w)) return 1;
    if (!d_in || !d_out) return fail("null frame pointer");
    if (ensure_device(n)) return 1;
    if (in_stride < (size_t)w * 3 || out_stride < (size_t)w * uva_net_scale(n) * 3) return fail("row stride too small");
    // the tail kernels address the residual bytes with 32-bit offsets from the frame's base (the LDS-DMA's lane offset is 32-bit)
    if ((unsigned long long)in_stride * (unsigned long long)h >= (1ull << 32) - 64 ||
        (unsigned long long)out_stride * (unsigned long long)h * (unsigned long long)uva_net_scale(n) >= (1ull << 32) - 64)
        return fail("frame of 4 GB or more");
    if (n->generic) return generic_process_u8_device(n, d_in, h, w, in_stride, d_out, out_stride, tile_size, border);
    Workspace* ws = nullptr;
    if (get_workspace(n, h, w, tile_size, border, &ws)) return 1;
    n->last.valid = true; n->last.ws = ws; n->last.f32 = false; n->last.src = d_in; n->last.src_stride = in_stride;
    n->last.dst = d_out; n->last.dst_stride = out_stride;
    return run_graph(n, ws, false, d_in, in_stride, d_out, out_stride, -1);
}

// the 16-bit route's refusals, shared by every 16-bit entry: 2x / 4x Compact nets only -- and the 1x net where the caller has
// asked for it (uva_net_enable_u16_1x)
static int check_u16_net(uva_net* n)
{
    if (n->u16_1x && is_sub10_net(n)) return 0;
    if (n->generic) return fail("the 16-bit route takes the 2x and 4x Compact nets only (this net runs as a generic graph)");
    if (!has_tail64(n)) return fail("the 16-bit route takes the 2x and 4x Compact nets only (64 features, scale 2 or 4)");
    return 0;
}

int uva_net_process_u16_device(uva_net* n, const void* d_in, int h, int w, size_t in_stride, void* d_out,
                               size_t out_stride, int tile_size, int border)
{
    if (check_dims(n, h, w)) return 1;
    if (!d_in || !d_out) return fail("null frame pointer");
    if (ensure_device(n)) return 1;
    if (check_u16_net(n)) return 1;
    const int s = uva_net_scale(n);
    if (in_stride < (size_t)w * 6 || out_stride < (size_t)w * s * 6) return fail("row stride too small");
    if ((((uintptr_t)d_in | (uintptr_t)d_out | in_stride | out_stride) & 1) != 0) return fail("16-bit frames need 2-byte aligned rows");
    // the tail kernels address the residual and output bytes with 32-bit offsets from the frame's base
    if ((unsigned long long)in_stride * (unsigned long long)h >= (1ull << 32) - 64 ||
        (unsigned long long)out_stride * (unsigned long long)h * (unsigned long long)s >= (1ull << 32) - 64)
        return fail("frame of 4 GB or more");
    if (is_sub10_net(n) && tile_size > 0) return fail("the 16-bit route runs the 1x net on whole frames only (tile_size 0)");
    Workspace* ws = nullptr;
    if (get_workspace(n, h, w, tile_size, border, &ws)) return 1;
    n->last = LastCall();        // the debug replays know u8 and f32 frames only
    return run_graph(n, ws, false, d_in, in_stride, d_out, out_stride, -1, true);
}

// `count` frames of ONE geometry, all resident on the net's device.  The 1x net takes up to S10_MAXB of them per launch
// (sub10_kernel: the segments' warm-up rows and the pipeline's fill and drain are paid once per launch, not once per frame);
// every other net -- and whatever does not fit the kernel's row table -- runs frame by frame, exactly as `count` calls of
// uva_net_process_u8_device would.  The bytes are those of the single-frame calls either way (tests).
int uva_net_process_u8_device_batch(uva_net* n, const void* const* d_in, void* const* d_out, int count, int h, int w,
                                    size_t in_stride, size_t out_stride, int tile_size, int border)
{
    if (check_dims(n, h, w)) return 1;
    if (count < 0 || (count > 0 && (!d_in || !d_out))) return fail("bad frame list");
    for (int i = 0; i < count; ++i)
        if (!d_in[i] || !d_out[i]) return fail("null frame pointer");
    if (count == 0) return 0;
    if (ensure_device(n)) return 1;
    if (in_stride < (size_t)w * 3 || out_stride < (size_t)w * uva_net_scale(n) * 3) return fail("row stride too small");
    Workspace* ws = nullptr;
    if (!n->generic && get_workspace(n, h, w, tile_size, border, &ws)) return 1;
    int i = 0;
    if (ws && sub10_route(n, ws, false, -1) && !n->split5) {
        if ((unsigned long long)in_stride * (unsigned long long)h >= (1ull << 32) - 64 ||
            (unsigned long long)out_stride * (unsigned long long)h >= (1ull << 32) - 64)
            return fail("frame of 4 GB or more");
        while (i < count) {
            const int k = std::min(count - i, std::max(1, ws->sub10_max_batch));
            const int rc = run_sub10(n, ws, d_in + i, in_stride, d_out + i, out_stride, k);
            if (rc == 1) return 1;
            if (rc == 2) {
                if (k == 1) break;              // not even one frame fits: the rest goes frame by frame below
                continue;                       // (launch_sub10 lowered sub10_max_batch)
            }
            i += k;
            n->last.valid = true; n->last.ws = ws; n->last.f32 = false; n->last.src = d_in[i - 1]; n->last.src_stride = in_stride;
            n->last.dst = d_out[i - 1]; n->last.dst_stride = out_stride;
        }
    }
    for (; i < count; ++i)
        if (uva_net_process_u8_device(n, d_in[i], h, w, in_stride, d_out[i], out_stride, tile_size, border)) return 1;
    return 0;
}

// ---- pipelined host route -----------------------------------------------------------------------
void* uva_host_alloc(size_t bytes)
{
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        fail("uva_host_alloc: hipHostMalloc failed");
        return nullptr;
    }
    return p;
}

void uva_host_free(void* p)
{
    if (p) (void)hipHostFree(p);
}

void uva_debug_live_resources(long long counts[4])
{
    for (int k = 0; k < LIVE_KINDS; ++k) counts[k] = g_live[k].load();
}

}  // extern "C"
namespace {
// The pipelined host route.  An entry fills a SubmitSpec, submit_check refuses what the entries refuse,
// submit_plan (csrc/uva_submit.cpp) works out every size and branch from the spec alone, and submit runs three stages over that
// plan: the upload on s_h2d, the compute on the net's stream, the download on s_d2h.

// the refusals of the host entries, in the order every entry has always applied them (a doubly-bad call reports the same one)
int submit_check(uva_net* n, const SubmitSpec& sp, const char* entry)
{
    if (!pix_frame_bytes(sp.in_fmt, 1, 1) || !pix_frame_bytes(sp.out_fmt, 1, 1)) return fail("unknown pixel format");
    if (sp.bits == 8 && (sp.in_fmt == PIX_BGR48LE || sp.out_fmt == PIX_BGR48LE))
        return fail(std::string("bgr48le is a 16-bit format: ") +
                    (std::strcmp(entry, "uva_net_submit_pix_sized") ? "use uva_net_submit_pix16" : "it needs bits = 16"));
    if (!pix_colour_ok(sp.colour)) return fail("bad colour word");
    if (check_dims(n, sp.h, sp.w)) return 1;
    if (sp.bits == 16 && (ensure_device(n) || check_u16_net(n))) return 1;
    if (sp.windowed && uva_net_scale(n) <= 0) return fail("net has no graph");
    return 0;
}

// the net at `bits` on a frame in HBM
int process_device(uva_net* n, int bits, const void* d_in, int h, int w, size_t in_stride, void* d_out, size_t out_stride, int tile_size,
                   int border)
{
    return bits == 16 ? uva_net_process_u16_device(n, d_in, h, w, in_stride, d_out, out_stride, tile_size, border)
                      : uva_net_process_u8_device(n, d_in, h, w, in_stride, d_out, out_stride, tile_size, border);
}

struct SubmitRun {                       // what the stages of one call share
    uva_net* n;
    const SubmitSpec& sp;
    const SubmitPlan& p;
    const uint8_t* in;                   // (a window of a BGR frame: at its offset)
    uint8_t* out;
    PipeSlot* ps = nullptr;
    const uint8_t* d_res = nullptr;      // the BGR frame that leaves: d_out, or d_rs
    const uint8_t* d_src = nullptr;      // what comes down: d_res, the packed frame d_pout, or the kept frame's result
    bool rp_on = false, repeat = false;  // uva_net_set_skip_repeats is in force; this frame repeats the kept one
};

// a free slot, the streams and events, the buffers, and the frame to HBM: into d_in, or (a packed frame) into d_pin
int submit_upload(SubmitRun& r)
{
    uva_net* n = r.n;
    const SubmitSpec& sp = r.sp;
    const SubmitPlan& p = r.p;
    for (auto& c : n->pipe)
        if (!c.busy) { r.ps = &c; break; }
    if (!r.ps) return fail("uva_net_submit_u8: " + std::to_string(uva_net::PIPE_SLOTS) + " frames already in flight, collect one first");
    PipeSlot& ps = *r.ps;
    if (!n->s_d2h) {
        if (tryhip(make_stream(n->s_h2d), "hipStreamCreate") || tryhip(make_stream(n->s_d2h), "hipStreamCreate")) return 1;
    }
    if (!ps.ev_d2h) {
        if (tryhip(make_event(ps.ev_h2d, hipEventDisableTiming), "hipEventCreate") ||
            tryhip(make_event(ps.ev_done, hipEventDisableTiming), "hipEventCreate") ||
            tryhip(make_event(ps.ev_d2h, hipEventDisableTiming), "hipEventCreate")) return 1;
    }
    if (grow_dev(ps.d_in, p.in_bytes) || grow_dev(ps.d_out, p.out_bytes)) return 1;
    if ((p.pin && grow_dev(ps.d_pin, p.pin_bytes)) || (p.pout && grow_dev(ps.d_pout, p.pout_bytes))) return 1;
    if (p.rs && grow_dev(ps.d_rs, p.res_bytes)) return 1;
    if (p.win_cols && grow_dev(ps.d_win, p.wstage_bytes)) return 1;
    r.d_res = p.rs ? ps.d_rs : ps.d_out;
    if (sp.png_ws) {                     // (png_ws: the encoder that matches the net's frames)
        if (!png_takes(p.out_h, p.out_w, sp.bits)) return fail("PNG encoder: frame width out of range");
        if (sp.png_ws_bytes < png_workspace_bytes(p.out_h, p.out_w, sp.bits)) return fail("PNG workspace too small");
        if (grow_dev(ps.d_png, png_device_bytes(p.out_h, p.out_w, sp.bits))) return 1;
    }
    // H2D: straight from the caller's buffer when it is pinned (uva_host_alloc / hipHostMalloc /
    // hipHostRegister), through this slot's pinned staging buffer otherwise
    const bool pinned = is_pinned_host(r.in);
    if (!pinned && grow_host(ps.h_in, p.h_in_bytes)) return 1;
    if (p.win_rows) {
        // one copy per plane of the plane's row range: into the packed frame where the rows are whole, into the staging otherwise
        uint8_t* d_up = p.win_cols ? ps.d_win : ps.d_pin;
        for (int k = 0; k < p.wn; ++k) {
            const WindowPlane& wp = p.wpl[k];
            const size_t at = p.win_cols ? p.wstage[k] : wp.dst_off, nb = wp.src_row * (size_t)wp.rows;
            const uint8_t* from = r.in + wp.src_off + (size_t)wp.row0 * wp.src_row;
            if (!pinned) {
                std::memcpy(ps.h_in + at, from, nb);
                from = ps.h_in + at;
            }
            if (tryhip(hipMemcpyAsync(d_up + at, from, nb, hipMemcpyHostToDevice, n->s_h2d), "H2D")) return 1;
        }
        if (p.win_cols && tryhip(launch_pix_window(n->s_h2d, ps.d_win, p.wstage, ps.d_pin, p.wpl, p.wn, crop_sample(sp.in_fmt).bytes), "pix_window"))
            return 1;
    } else {
        const uint8_t* src = r.in;
        size_t src_stride = p.pin ? p.h2d_row : p.in_stride;
        if (!pinned) {
            if (p.pin) std::memcpy(ps.h_in, r.in, p.pin_bytes);
            else
                for (int y = 0; y < sp.h; ++y) std::memcpy(ps.h_in + y * p.in_row, r.in + y * p.in_stride, p.in_row);
            src = ps.h_in; src_stride = p.h2d_row;
        }
        if (tryhip(hipMemcpy2DAsync(p.pin ? ps.d_pin : ps.d_in, p.h2d_row, src, src_stride, p.h2d_row, p.h2d_rows, hipMemcpyHostToDevice,
                                    n->s_h2d), "H2D")) return 1;
    }
    if (tryhip(hipEventRecord(ps.ev_h2d, n->s_h2d), "hipEventRecord") ||
        tryhip(hipStreamWaitEvent(n->stream, ps.ev_h2d, 0), "hipStreamWaitEvent")) return 1;
    r.d_src = p.pout ? ps.d_pout : r.d_res;
    return 0;
}

// the repeat comparison, then -- unless the frame repeats the kept one -- convert in, the net, the resampler, convert out, the
// PNG deflate, all on the net's stream behind the upload
int submit_compute(SubmitRun& r)
{
    uva_net* n = r.n;
    const SubmitSpec& sp = r.sp;
    const SubmitPlan& p = r.p;
    PipeSlot& ps = *r.ps;
    // --skip-repeats: the frame is compared with the kept frame's input on the upload stream, behind its own upload, and the
    // host waits for the three numbers -- the one blocking point of the route, and only with the option on
    KeptFrame& rp = n->kept;
    r.rp_on = sp.may_skip && !sp.png_ws && n->rep.threshold >= 0;
    if (r.rp_on) {
        const uint8_t* d_packed = p.pin ? ps.d_pin : ps.d_in;
        ++n->rep.submitted;
        if (!rp.ev_read) {
            if (tryhip(alloc_into(rp.d_stats, sizeof(FrameDiffStats)), "hipMalloc") ||
                tryhip(alloc_into(rp.h_stats, sizeof(FrameDiffStats)), "hipHostMalloc") ||
                tryhip(make_event(rp.ev_stats, hipEventDisableTiming), "hipEventCreate") ||
                tryhip(make_event(rp.ev_written, hipEventDisableTiming), "hipEventCreate") ||
                tryhip(make_event(rp.ev_read, hipEventDisableTiming), "hipEventCreate")) return 1;
        }
        if (rp.valid && p.key == rp.key) {
            if (tryhip(launch_frame_diff(n->s_h2d, rp.d_in, d_packed, p.packed_bytes, sp.in_fmt, (unsigned)n->rep.threshold, rp.d_stats), "frame_diff") ||
                tryhip(hipMemcpyAsync(rp.h_stats, rp.d_stats, sizeof(FrameDiffStats), hipMemcpyDeviceToHost, n->s_h2d), "D2H") ||
                tryhip(hipEventRecord(rp.ev_stats, n->s_h2d), "hipEventRecord") ||
                tryhip(hipEventSynchronize(rp.ev_stats), "hipEventSynchronize")) return 1;
            r.repeat = rp.h_stats->over == 0;
        }
        if (!r.repeat) {
            // this frame runs and becomes the kept frame.  Kept input: the comparisons read it and this copy replaces it on one
            // stream, s_h2d, so they are ordered (the slot's own upload buffer is free again once the frame is collected).
            rp.valid = false;
            if (rp.d_in.cap() < p.packed_bytes || rp.d_res.cap() < p.dl_bytes) {      // (a buffer that moves: nothing may still use it)
                if (tryhip(hipStreamSynchronize(n->s_h2d), "hipStreamSynchronize") || tryhip(hipStreamSynchronize(n->s_d2h), "hipStreamSynchronize") ||
                    tryhip(hipStreamSynchronize(n->stream), "hipStreamSynchronize")) return 1;
                if (grow_dev(rp.d_in, p.packed_bytes) || grow_dev(rp.d_res, p.dl_bytes)) return 1;
                rp.reads_pending = false;
            }
            if (tryhip(hipMemcpyAsync(rp.d_in, d_packed, p.packed_bytes, hipMemcpyDeviceToDevice, n->s_h2d), "D2D")) return 1;
            rp.key = p.key;
        }
    }
    if (r.repeat) {
        // the kept result's bytes, by a download alone: behind the copy that wrote them (ev_written, on the net's stream)
        ++n->rep.skipped;
        r.d_src = rp.d_res;
        return tryhip(hipStreamWaitEvent(n->s_d2h, rp.ev_written, 0), "hipStreamWaitEvent");
    }
    std::string rs_err;
    if (p.pin && pix_to_native(n->stream, sp.bits, sp.in_fmt, sp.colour, ps.d_pin, ps.d_in, sp.h, sp.w)) return 1;
    if (process_device(n, sp.bits, ps.d_in, sp.h, sp.w, p.in_row, ps.d_out, p.out_row, sp.tile_size, sp.border)) return 1;
    if (p.rs && launch_resize(n->stream, n->device, ps.d_out, p.out_h, p.out_w, p.out_row, ps.d_rs, p.res_h, p.res_w, p.res_row, sp.rs_filter,
                              sp.bits, &rs_err)) return fail(rs_err);
    if (p.pout && pix_from_native(n->stream, sp.bits, sp.out_fmt, sp.colour, r.d_res, ps.d_pout, p.res_h, p.res_w)) return 1;
    // png: the deflate kernel follows the net on its stream and leaves the blocks in HBM, packed end to end by a second
    // (device-to-device) kernel: 0.15 ms per 4K frame together
    if (sp.png_ws && ((sp.bits == 16 ? png_launch16(n->device, n->stream, ps.d_out, p.out_row, p.out_h, p.out_w, ps.d_png)
                                     : png_launch(n->device, n->stream, ps.d_out, p.out_row, p.out_h, p.out_w, ps.d_png)) ||
                      png_pack_launch(n->stream, ps.d_png, p.out_h, p.out_w, sp.bits))) return 1;
    if (tryhip(hipEventRecord(ps.ev_done, n->stream), "hipEventRecord") ||
        tryhip(hipStreamWaitEvent(n->s_d2h, ps.ev_done, 0), "hipStreamWaitEvent")) return 1;
    if (r.rp_on) {
        // Kept result: skipped frames download it on s_d2h, this copy overwrites it on the net's stream.  s_d2h runs in order,
        // so the event behind the last such download (ev_read) stands for every download of the old contents still pending.
        if (rp.reads_pending && tryhip(hipStreamWaitEvent(n->stream, rp.ev_read, 0), "hipStreamWaitEvent")) return 1;
        if (tryhip(hipMemcpyAsync(rp.d_res, r.d_src, p.dl_bytes, hipMemcpyDeviceToDevice, n->stream), "D2D") ||
            tryhip(hipEventRecord(rp.ev_written, n->stream), "hipEventRecord")) return 1;
        rp.reads_pending = false;
        rp.valid = true;
    }
    return 0;
}

// the result to the caller on s_d2h behind the compute, and the ticket uva_net_collect_u8 takes
int submit_download(SubmitRun& r)
{
    uva_net* n = r.n;
    const SubmitSpec& sp = r.sp;
    const SubmitPlan& p = r.p;
    PipeSlot& ps = *r.ps;
    ps.user_out = nullptr;
    ps.png_ws = nullptr;
    if (sp.png_ws) {
        // ... and the copy engine takes them to the caller's page-locked workspace while the next frame computes.  How
        // many bytes there are is only known on the device: as many as the previous frame had (+ 6 %) go now, collect
        // fetches the rest should this frame be larger.  (A kernel writing to host memory instead keeps CUs busy for
        // the PCIe transfer: 0.24 ms per 4K frame that the next frame's net then waits for.)
        const size_t cap = png_workspace_bytes(p.out_h, p.out_w, sp.bits) - png_meta_bytes(p.out_h, p.out_w, sp.bits);
        const size_t last = sp.bits == 16 ? n->png_guess16 : n->png_guess;
        const size_t guess = last ? std::min(cap, last + last / 16 + 65536) : std::min(cap, p.out_bytes * 5 / 8);
        if (png_download(n->s_d2h, ps.d_png, p.out_h, p.out_w, sp.png_ws, guess, sp.bits)) return 1;
        if (tryhip(hipEventRecord(ps.ev_d2h, n->s_d2h), "hipEventRecord")) return 1;
        ps.png_ws = (uint8_t*)sp.png_ws; ps.png_sent = guess; ps.png_h = p.out_h; ps.png_w = p.out_w; ps.png_bits = sp.bits;
    } else {
        uint8_t* dst = r.out;
        if (!is_pinned_host(r.out)) {
            if (grow_host(ps.h_out, p.dl_bytes)) return 1;
            dst = ps.h_out;
            ps.user_out = r.out; ps.user_out_stride = p.dl_user_stride; ps.out_row = p.dl_row; ps.out_rows = p.dl_rows;
        }
        if (ps.user_out) {
            const int rows = p.dl_rows, per = (rows + PipeSlot::BANDS - 1) / PipeSlot::BANDS;
            const size_t row = p.dl_row;
            for (int k = 0; k < PipeSlot::BANDS; ++k) {
                if (!ps.ev_band[k] && tryhip(make_event(ps.ev_band[k], hipEventDisableTiming), "hipEventCreate")) return 1;
                const int r0 = std::min(rows, k * per), nr = std::min(rows, r0 + per) - r0;
                if (nr > 0 && tryhip(hipMemcpyAsync(dst + (size_t)r0 * row, r.d_src + (size_t)r0 * row, (size_t)nr * row,
                                                    hipMemcpyDeviceToHost, n->s_d2h), "D2H")) return 1;
                if (tryhip(hipEventRecord(ps.ev_band[k], n->s_d2h), "hipEventRecord")) return 1;
            }
        } else if (p.pout) {
            if (tryhip(hipMemcpyAsync(dst, r.d_src, p.dl_bytes, hipMemcpyDeviceToHost, n->s_d2h), "D2H")) return 1;
        } else if (tryhip(hipMemcpy2DAsync(dst, p.out_stride, r.d_src, p.res_row, p.res_row, (size_t)p.res_h, hipMemcpyDeviceToHost, n->s_d2h),
                          "D2H")) {
            return 1;
        }
        if (tryhip(hipEventRecord(ps.ev_d2h, n->s_d2h), "hipEventRecord")) return 1;
        if (r.repeat) {
            if (tryhip(hipEventRecord(n->kept.ev_read, n->s_d2h), "hipEventRecord")) return 1;
            n->kept.reads_pending = true;
        }
    }
    ps.busy = true;
    ps.ticket = n->next_ticket++;
    return 0;
}

// `in` -> `out` (the PNG route: -> sp.png_ws) as `sp` says; returns the ticket, or -1.  The entry has run submit_check.
long long submit(uva_net* n, const void* in, void* out, const SubmitSpec& sp)
{
    SubmitPlan p;
    const char* refusal = submit_plan(sp, uva_net_scale(n), sp.windowed && n->win.src_h > 0 ? &n->win : nullptr, &p);
    // (the plan's refusals keep their places among those that need the pointers and the device: the window's come first)
    if (refusal && p.window_refused) { fail(refusal); return -1; }
    if (!in || (!out && !sp.png_ws)) { fail("null frame pointer"); return -1; }
    if (sp.png_ws && !is_pinned_host(sp.png_ws)) { fail("PNG workspace must be page-locked host memory (uva_host_alloc)"); return -1; }
    if (ensure_device(n)) return -1;
    if (refusal) { fail(refusal); return -1; }
    SubmitRun r = {n, sp, p, (const uint8_t*)in + p.in_offset, (uint8_t*)out};
    if (submit_upload(r) || submit_compute(r) || submit_download(r)) return -1;
    return r.ps->ticket;
}

// a BGR call's spec: the geometry, every other member at its default
SubmitSpec bgr_spec(int h, int w, size_t in_stride, size_t out_stride, int tile_size, int border)
{
    SubmitSpec sp;
    sp.h = h; sp.w = w;
    sp.in_stride = in_stride; sp.out_stride = out_stride;
    sp.tile_size = tile_size; sp.border = border;
    return sp;
}

// a pixel-format call's spec: dense frames, the net's BGR at `bits`, the result at the net's size
SubmitSpec pix_spec(const uva_net* n, int bits, int in_fmt, int out_fmt, int colour, int h, int w, int tile_size, int border)
{
    const size_t bps = bits / 8;
    SubmitSpec sp = bgr_spec(h, w, (size_t)w * 3 * bps, (size_t)w * uva_net_scale(n) * 3 * bps, tile_size, border);
    sp.in_fmt = in_fmt; sp.out_fmt = out_fmt; sp.colour = colour;
    sp.bits = bits;
    sp.may_skip = sp.windowed = true;
    return sp;
}
}  // namespace
extern "C" {

long long uva_net_submit_u8(uva_net* n, const uint8_t* in, int h, int w, size_t in_stride, uint8_t* out,
                            size_t out_stride, int tile_size, int border)
{
    SubmitSpec sp = bgr_spec(h, w, in_stride, out_stride, tile_size, border);
    sp.may_skip = true;
    if (submit_check(n, sp, "uva_net_submit_u8")) return -1;
    return submit(n, in, out, sp);
}

long long uva_net_submit_u8_png(uva_net* n, const uint8_t* in, int h, int w, size_t in_stride, void* png_ws, size_t png_ws_bytes,
                                int tile_size, int border)
{
    if (!png_ws) { fail("null PNG workspace"); return -1; }
    SubmitSpec sp = bgr_spec(h, w, in_stride, 0, tile_size, border);
    sp.png_ws = png_ws; sp.png_ws_bytes = png_ws_bytes;
    if (submit_check(n, sp, "uva_net_submit_u8_png")) return -1;
    return submit(n, in, nullptr, sp);
}

long long uva_net_submit_u16_png(uva_net* n, const uint16_t* in, int h, int w, size_t in_stride, void* png_ws, size_t png_ws_bytes,
                                 int tile_size, int border)
{
    if (!png_ws) { fail("null PNG workspace"); return -1; }
    SubmitSpec sp = bgr_spec(h, w, in_stride, 0, tile_size, border);
    sp.in_fmt = sp.out_fmt = PIX_BGR48LE; sp.bits = 16;
    sp.png_ws = png_ws; sp.png_ws_bytes = png_ws_bytes;
    if (submit_check(n, sp, "uva_net_submit_u16_png")) return -1;
    if (is_sub10_net(n) && tile_size > 0) { fail("the 16-bit route runs the 1x net on whole frames only (tile_size 0)"); return -1; }
    if ((((uintptr_t)in | in_stride) & 1) != 0) { fail("odd address or stride of a 16-bit frame"); return -1; }
    return submit(n, in, nullptr, sp);
}

long long uva_net_submit_pix(uva_net* n, const void* in, int in_fmt, int h, int w, void* out, int out_fmt, int colour,
                             int tile_size, int border)
{
    const SubmitSpec sp = pix_spec(n, 8, in_fmt, out_fmt, colour, h, w, tile_size, border);
    if (submit_check(n, sp, "uva_net_submit_pix")) return -1;
    return submit(n, in, out, sp);
}

long long uva_net_submit_pix16(uva_net* n, const void* in, int in_fmt, int h, int w, void* out, int out_fmt, int colour,
                               int tile_size, int border)
{
    const SubmitSpec sp = pix_spec(n, 16, in_fmt, out_fmt, colour, h, w, tile_size, border);
    if (submit_check(n, sp, "uva_net_submit_pix16")) return -1;
    return submit(n, in, out, sp);
}

int uva_net_enable_u16_1x(uva_net* n, int on)
{
    if (!n) return fail("null net");
    if (!n->g.param_loaded || !is_sub10_net(n))
        return fail("uva_net_enable_u16_1x: not the 1x SubCompact net (24 features, 10 convolutions, scale 1, not a generic graph)");
    n->u16_1x = on != 0;
    return 0;
}

int uva_net_process_u16(uva_net* n, const uint16_t* in, int h, int w, size_t in_stride, uint16_t* out, size_t out_stride,
                        int tile_size, int border)
{
    if (check_dims(n, h, w)) return 1;
    if (!in || !out) return fail("null frame pointer");
    // as uva_net_process_u16_device: the staging copies would take any stride, but a row of u16 samples at an odd address is
    // no uint16_t array
    if ((((uintptr_t)in | (uintptr_t)out | in_stride | out_stride) & 1) != 0) return fail("16-bit frames need 2-byte aligned rows");
    SubmitSpec sp = bgr_spec(h, w, in_stride, out_stride, tile_size, border);
    sp.in_fmt = sp.out_fmt = PIX_BGR48LE; sp.bits = 16;
    if (submit_check(n, sp, "uva_net_process_u16")) return 1;
    const long long t = submit(n, in, out, sp);
    if (t < 0) return 1;
    if (uva_net_collect_u8(n, t)) return 1;
    resolve_events(n);
    return 0;
}

long long uva_net_submit_pix_sized(uva_net* n, const void* in, int in_fmt, int h, int w, void* out, int out_fmt, int colour,
                                   int tile_size, int border, int oh, int ow, int filter, int bits)
{
    if (bits != 8 && bits != 16) { fail("uva_net_submit_pix_sized: bits must be 8 or 16"); return -1; }
    SubmitSpec sp = pix_spec(n, bits, in_fmt, out_fmt, colour, h, w, tile_size, border);
    sp.out_stride = (size_t)ow * 3 * (bits / 8);
    sp.rs_oh = oh; sp.rs_ow = ow; sp.rs_filter = filter;
    if (submit_check(n, sp, "uva_net_submit_pix_sized")) return -1;
    const int s = uva_net_scale(n);
    if (const char* e = resize_axis_error(h * s, oh, filter)) { fail(e); return -1; }
    if (const char* e = resize_axis_error(w * s, ow, filter)) { fail(e); return -1; }
    return submit(n, in, out, sp);
}

int uva_net_set_skip_repeats(uva_net* n, int threshold)
{
    if (!n) return fail("null net");
    if (threshold < -1 || threshold > 65535) return fail("uva_net_set_skip_repeats: the threshold is -1 (off) or 0 ... 65535 code values");
    n->rep.threshold = threshold;
    n->kept.valid = false;
    n->rep.submitted = n->rep.skipped = 0;
    if (threshold < 0 && (n->kept.d_in || n->kept.d_stats)) {     // off again: the kept frame's buffers go (there is a device: they exist)
        HIP_TRY(hipSetDevice(n->device));
        for (hipStream_t st : {n->s_h2d.get(), n->s_d2h.get(), n->stream.get()})
            if (st) HIP_TRY(hipStreamSynchronize(st));
        n->kept = KeptFrame();
    }
    return 0;
}

int uva_net_reset_reference(uva_net* n)
{
    if (!n) return fail("null net");
    n->kept.valid = false;
    return 0;
}

int uva_net_skip_stats(uva_net* n, long long* submitted, long long* skipped)
{
    if (!n) return fail("null net");
    if (submitted) *submitted = n->rep.submitted;
    if (skipped) *skipped = n->rep.skipped;
    return 0;
}

int uva_net_set_input_window(uva_net* n, int src_h, int src_w, int x, int y)
{
    if (!n) return fail("null net");
    const bool off = !src_h && !src_w && !x && !y;
    if (!off && (src_h < 1 || src_w < 1 || (long long)src_h * src_w > (1ll << 28)))
        return fail("uva_net_set_input_window: bad size of the source frame (all zeros switch the window off)");
    if (!off && (x < 0 || y < 0 || x >= src_w || y >= src_h)) return fail("input window: the window leaves the frame");
    n->win.src_h = src_h; n->win.src_w = src_w; n->win.x = x; n->win.y = y;
    // the kept frame of uva_net_set_skip_repeats was compared as another window's bytes: forget it
    n->kept.valid = false;
    n->rep.submitted = n->rep.skipped = 0;
    return 0;
}

int uva_net_collect_u8(uva_net* n, long long ticket)
{
    if (!n || ticket < 0) return fail("bad ticket");
    PipeSlot* slot = nullptr;
    for (auto& c : n->pipe)
        if (c.busy && c.ticket == ticket) slot = &c;
    if (!slot) return fail("uva_net_collect_u8: ticket " + std::to_string(ticket) + " is not in flight");
    PipeSlot& ps = *slot;
    HIP_TRY(hipSetDevice(n->device));
    if (ps.user_out) {
        const int per = (ps.out_rows + PipeSlot::BANDS - 1) / PipeSlot::BANDS;
        for (int k = 0; k < PipeSlot::BANDS; ++k) {
            HIP_TRY(hipEventSynchronize(ps.ev_band[k]));
            const int r0 = std::min(ps.out_rows, k * per), r1 = std::min(ps.out_rows, r0 + per);
            if (ps.user_out_stride == ps.out_row) {
                if (r1 > r0) std::memcpy(ps.user_out + (size_t)r0 * ps.out_row, ps.h_out + (size_t)r0 * ps.out_row, (size_t)(r1 - r0) * ps.out_row);
            } else {
                for (int y = r0; y < r1; ++y)
                    std::memcpy(ps.user_out + (size_t)y * ps.user_out_stride, ps.h_out + (size_t)y * ps.out_row, ps.out_row);
            }
        }
        ps.busy = false;
        return 0;
    }
    HIP_TRY(hipEventSynchronize(ps.ev_d2h));
    if (ps.png_ws) {
        // the meta is here: fetch what the download did not cover (a frame that compressed worse than the one before)
        const int pb = ps.png_bits;
        const size_t mb = png_meta_bytes(ps.png_h, ps.png_w, pb), cap = png_workspace_bytes(ps.png_h, ps.png_w, pb) - mb;
        const size_t total = png_total_bytes(ps.png_ws, ps.png_h, ps.png_w, pb);
        if (total > cap) { ps.busy = false; ps.png_ws = nullptr; return fail("PNG encoder: block sizes out of range"); }
        if (total > ps.png_sent)
            HIP_TRY(hipMemcpy(ps.png_ws + mb + ps.png_sent, png_packed(ps.d_png, ps.png_h, ps.png_w, pb) + ps.png_sent, total - ps.png_sent,
                              hipMemcpyDeviceToHost));
        (pb == 16 ? n->png_guess16 : n->png_guess) = total;
        ps.png_ws = nullptr;
    }
    ps.busy = false;
    return 0;
}

int uva_net_process_u8(uva_net* n, const uint8_t* in, int h, int w, size_t in_stride, uint8_t* out,
                       size_t out_stride, int tile_size, int border)
{
    // (may_skip stays off: the synchronous calls take no part in uva_net_set_skip_repeats)
    const SubmitSpec sp = bgr_spec(h, w, in_stride, out_stride, tile_size, border);
    if (submit_check(n, sp, "uva_net_process_u8")) return 1;
    const long long t = submit(n, in, out, sp);
    if (t < 0) return 1;
    if (uva_net_collect_u8(n, t)) return 1;
    resolve_events(n);
    return 0;
}

int uva_net_extract_f32(uva_net* n, const float* in_chw, int h, int w, float* out_chw)
{
    if (check_dims(n, h, w)) return 1;
    if (!in_chw || !out_chw) return fail("null Mat pointer");
    if (ensure_device(n)) return 1;
    const int s = uva_net_scale(n);
    const size_t in_bytes = (size_t)3 * h * w * 4, out_bytes = (size_t)3 * h * s * w * s * 4;
    if (grow_dev(n->d_fin, in_bytes) || grow_dev(n->d_fout, out_bytes)) return 1;
    if (n->generic) {
        HIP_TRY(hipMemcpyAsync(n->d_fin, in_chw, in_bytes, hipMemcpyHostToDevice, n->stream));
        if (generic_run_plane(n, true, n->d_fin, 0, 0, 0, h, w, n->d_fout, 0, 0, h, 0, w)) return 1;
        HIP_TRY(hipMemcpyAsync(out_chw, n->d_fout, out_bytes, hipMemcpyDeviceToHost, n->stream));
        return uva_net_synchronize(n);
    }
    Workspace* ws = nullptr;
    if (get_workspace(n, h, w, 0, 0, &ws)) return 1;
    HIP_TRY(hipMemcpyAsync(n->d_fin, in_chw, in_bytes, hipMemcpyHostToDevice, n->stream));
    n->last.valid = true; n->last.ws = ws; n->last.f32 = true; n->last.src = n->d_fin; n->last.src_stride = 0;
    if (run_graph(n, ws, true, n->d_fin, 0, n->d_fout, 0, -1)) return 1;
    HIP_TRY(hipMemcpyAsync(out_chw, n->d_fout, out_bytes, hipMemcpyDeviceToHost, n->stream));
    return uva_net_synchronize(n);
}

int uva_net_debug_read_activation(uva_net* n, int conv_idx, float* out_chw, int h, int w)
{
    if (!n || !out_chw) return fail("null argument");
    if (!n->dev_ready || !n->last.valid) return fail("no previous call to replay");
    Workspace* ws = n->last.ws;
    const int nconv = (int)n->g.convs.size();
    if (ws->planes.size() != 1 || ws->h != h || ws->w != w) return fail("debug read needs an untiled call of the same size");
    if (conv_idx < 0 || conv_idx > nconv - 2) return fail("conv_idx out of range");
    HIP_TRY(hipSetDevice(n->device));
    if (run_graph(n, ws, n->last.f32, n->last.src, n->last.src_stride, nullptr, 0, conv_idx)) return 1;
    const PlaneDesc& p = ws->planes[0];
    const int nf = n->g.nf;
    const size_t rows = (size_t)p.nty * TH + 2;
    std::vector<uint16_t> hbuf(rows * p.pitch * nf);
    HIP_TRY(hipMemcpyAsync(hbuf.data(), ws->act[n->last_act_buf], hbuf.size() * 2, hipMemcpyDeviceToHost, n->stream));
    HIP_TRY(hipStreamSynchronize(n->stream));
    for (int c = 0; c < nf; ++c)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                out_chw[((size_t)c * h + y) * w + x] =
                    f16_bits_to_f32(hbuf[((size_t)(y + 1) * p.pitch + (x + 1)) * nf + c]);
    return 0;
}

int uva_net_set_profiling(uva_net* n, int enable)
{
    if (!n) return fail("null net");
    if (uva_net_synchronize(n)) return 1;
    n->prof = enable != 0;
    for (int k = 0; k < 4; ++k) { n->launches[k] = 0; n->total_ms[k] = 0; }
    return 0;
}

int uva_net_kernel_stats(uva_net* n, int kind, long long* launches, double* total_ms)
{
    if (!n || kind < 0 || kind > 3) return fail("bad argument");
    if (launches) *launches = n->launches[kind];
    if (total_ms) *total_ms = n->total_ms[kind];
    return 0;
}

#ifdef UVA_INSTRUMENT
}  // extern "C"
namespace {
// The stamps of one launch and the time of `reps`: a warm-up, `reps` timed launches without stamps, one launch that writes
// its stamps, the stamps copied out.  launch(dbg) runs the kernel with that stamp buffer (null: none) and returns 0, 1 or
// its own refusal, which stamped_run hands on.  The buffer and the events are handles: they go on every path out.
template <typename L>
int stamped_run(uva_net* n, unsigned long long* out, int max_tiles, float* kernel_ms, int reps, L launch)
{
    const size_t bytes = (size_t)max_tiles * 8 * sizeof(unsigned long long);
    DevPtr<unsigned long long> d;
    Event e0, e1;
    HIP_TRY(alloc_into(d, bytes));
    HIP_TRY(make_event(e0, hipEventDefault));
    HIP_TRY(make_event(e1, hipEventDefault));
    int rc = launch(nullptr);
    HIP_TRY(hipEventRecord(e0, n->stream));
    for (int r = 0; r < reps && !rc; ++r) rc = launch(nullptr);
    HIP_TRY(hipEventRecord(e1, n->stream));
    HIP_TRY(hipMemsetAsync(d, 0, bytes, n->stream));
    if (!rc) rc = launch(d.get());
    const hipError_t copied = rc ? hipSuccess : hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, n->stream);
    HIP_TRY(hipStreamSynchronize(n->stream));           // (before `d` goes: the last launch writes to it)
    if (rc) return rc;
    HIP_TRY(copied);
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (kernel_ms) *kernel_ms = ms / reps;
    return 0;
}
}  // namespace
extern "C" {

// debug: one trunk-layer launch on the last call's workspace with in-kernel s_memtime stamps
// (block 0, wave 0): out[8*i + {0,1,2,3,4}] = tile i {start, k-loop done, barrier passed, epilogue done,
// epilogue staging written}
int uva_net_debug_trunk_stamps(uva_net* n, unsigned long long* out, int max_tiles, int* tiles, int ablate,
                               float* kernel_ms)
{
    if (!n || !out || !n->dev_ready || !n->last.valid) return fail("no previous call to replay");
    Workspace* ws = n->last.ws;
    HIP_TRY(hipSetDevice(n->device));
    ConvArgs ca;
    std::memset(&ca, 0, sizeof ca);
    ca.planes = ws->d_planes;
    ca.nplanes = (int)ws->planes.size();
    ca.ntiles = ws->ntiles;
    ca.tiles_per_xcd = (ws->ntiles + 7) / 8;
    ca.in_act = ws->act[0];
    ca.out_act = ws->act[1];
    ca.wpk = n->layers[1].wpk;
    ca.bias = n->layers[1].bias;
    ca.slope = n->layers[1].slope;
    ca.sink = n->d_sink;
    const bool split = n->g.nf == 64;
    const int grid = persistent_grid(n->ncu);
    const int g8 = (split ? 2 : 1) * grid / 8;
    const int txcd = ((split ? ws->ntiles4 : ws->ntiles) + 7) / 8;
    const int per_block = (txcd + g8 - 1) / g8;
    if (per_block > max_tiles) return fail("max_tiles too small");
    const void* const src = n->last.src;
    void* const dst = n->last.dst;
    const size_t src_stride = n->last.src_stride, dst_stride = n->last.dst_stride;
    if (ablate == 3) {
        // the u8 tail kernel of the last host-route call instead of a trunk layer
        if (n->last.f32 || !dst) return fail("tail stamps need a previous uva_net_process_u8 call");
        const int nconv = (int)n->g.convs.size();
        ca.in_act = ws->act[n->last_act_buf];
        ca.out_act = nullptr;
        ca.wpk = n->layers[nconv - 1].wpk;
        ca.bias = n->layers[nconv - 1].bias;
        ca.slope = nullptr;
        ca.src_u8 = (const uint8_t*)src;
        ca.src_stride = src_stride;
        ca.dst_u8 = (uint8_t*)dst;
        ca.dst_stride = dst_stride;
        const int grid3 = persistent_grid(n->ncu);
        const bool pingpong_tail = n->g.nf == 64 && (n->g.scale == 2 || n->g.scale == 4);   // 4-row tiles, 2 groups
        if (tiles) *tiles = pingpong_tail ? per_block : (ca.tiles_per_xcd + grid3 / 8 - 1) / (grid3 / 8);
        return stamped_run(n, out, max_tiles, kernel_ms, 10, [&](unsigned long long* dbg) { ca.dbg = dbg; return launch_tail_u8(n, ws, ca); });
    }
    if (ablate == 7) {
        // sub10_kernel (the whole 1x net): out[(step*12 + wave)*4 + {0 step start, 1 MFMAs done, 2 at the barrier}] of
        // workgroup 0 (max_tiles*8 words must hold 40 per step); *tiles = steps
        if (n->last.f32 || !dst || ws->planes.size() != 1) return fail("sub10 stamps need a previous whole-frame uva_net_process_u8 call");
        int rc7 = launch_sub10(n, ws, src, src_stride, dst, dst_stride);       // (builds the row table: max_rows10)
        if (rc7 == 0 && (size_t)(ws->max_rows10[0] + S10_DRAIN + 2) * 4 * S10_NW > (size_t)max_tiles * 8) return fail("max_tiles too small");
        if (!rc7) rc7 = stamped_run(n, out, max_tiles, kernel_ms, 50, [&](unsigned long long* dbg) { return launch_sub10(n, ws, src, src_stride, dst, dst_stride, dbg); });
        if (tiles) *tiles = ws->max_rows10[0] + S10_DRAIN;
        return rc7 ? (rc7 == 2 ? fail("frame too large for sub10_kernel") : 1) : 0;
    }
    if (ablate == 9 || ablate == 10) {
        // sub5_kernel, part 0 / part 1 (the 1x net as two launches of five layers): out[(step*12 + wave)*4 + {0 step start, 1 MFMAs
        // done (front wave), 2 at the barrier}] of workgroup 0; *tiles = steps; kernel_ms = both launches
        if (n->last.f32 || !dst || ws->planes.size() != 1) return fail("sub5 stamps need a previous whole-frame uva_net_process_u8 call");
        int rc9 = launch_sub5(n, ws, src, src_stride, dst, dst_stride);         // (builds the row table: max_rows5)
        if (rc9 == 0 && (size_t)(ws->max_rows5 + 16) * 4 * 12 > (size_t)max_tiles * 8) return fail("max_tiles too small");
        if (!rc9) rc9 = stamped_run(n, out, max_tiles, kernel_ms, 50, [&](unsigned long long* dbg) { return launch_sub5(n, ws, src, src_stride, dst, dst_stride, dbg, ablate - 9); });
        if (tiles) *tiles = ws->max_rows5 + 14;
        return rc9 ? (rc9 == 2 ? fail("frame too large for sub5_kernel") : 1) : 0;
    }
    if (ablate == 6) {
        // pair24_kernel (two 24-feature trunk layers): out[8*it + {0 top, 1 tile landed, 2 stage A done, 3 intermediate
        // complete, 4 stage B k-loop done, 5 stores issued}] of workgroup 0 / wave 0
        if (n->g.nf != 24) return fail("pair24 stamps need the 24-feature net");
        ca.wpk2 = n->layers[2].wpk; ca.bias2 = n->layers[2].bias; ca.slope2 = n->layers[2].slope;
        ca.ntiles = ws->ntiles; ca.tiles_per_xcd = (ws->ntiles + 7) / 8;
        const int grid6 = persistent_grid(n->ncu) * 2;
        if (tiles) *tiles = (ca.tiles_per_xcd + grid6 / 8 - 1) / (grid6 / 8);
        return stamped_run(n, out, max_tiles, kernel_ms, 50, [&](unsigned long long* dbg) { ca.dbg = dbg; return launch_pair24(n, ca); });
    }
    if (ablate == 8) {
        // trunkw_kernel (the fused pair as Winograd F(2,3)): stamps of workgroup 0, both groups (out[16*it + 8*group + k], entry
        // at out[16*niter]); only an instrumented build (-DUVA_INSTRUMENT) writes them
        if (!ws->d_stepsw || !n->layers[1].wpk_w) return fail("no Winograd fused-pair schedule for this net");
        TrunkwArgs wa;
        std::memset(&wa, 0, sizeof wa);
        wa.in_act = ws->act_base[0];
        wa.out_act = ws->act_base[1];
        wa.steps = ws->d_stepsw; wa.nsteps = ws->d_nstepsw; wa.max_steps = ws->max_stepsw; wa.sink = n->d_sink;
        if (2 * (ws->max_stepsw + 3) + 1 > max_tiles) return fail("max_tiles too small");
        const int rc8 = stamped_run(n, out, max_tiles, kernel_ms, 50, [&](unsigned long long* dbg) { wa.dbg = dbg; return launch_trunkw(n, ws, wa, 1); });
        int ns0 = 0;
        if (!rc8) HIP_TRY(hipMemcpy(&ns0, ws->d_nstepsw, sizeof(int), hipMemcpyDeviceToHost));
        if (tiles) *tiles = ns0 + 2;
        return rc8;
    }
    if (ablate == 5) {
        // the fused pair kernel: stamps of workgroup 0, both groups (out[16*it + 8*group + k], entry at out[16*niter])
        if (!ws->d_steps2) return fail("no fused-pair schedule for this net");
        Trunk2Args ta;
        std::memset(&ta, 0, sizeof ta);
        ta.in_act = ws->act_base[0];
        ta.out_act = ws->act_base[1];
        for (int k = 0; k < 2; ++k) { ta.wpk[k] = n->layers[1 + k].wpk; ta.bias[k] = n->layers[1 + k].bias; ta.slope[k] = n->layers[1 + k].slope; }
        ta.steps = ws->d_steps2; ta.nsteps = ws->d_nsteps2; ta.max_steps = ws->max_steps2; ta.sink = n->d_sink;
        if (2 * (ws->max_steps2 + 3) + 1 > max_tiles) return fail("max_tiles too small");
        const int rc5 = stamped_run(n, out, max_tiles, kernel_ms, 50, [&](unsigned long long* dbg) { ta.dbg = dbg; return launch_trunk2(n, ws, ta); });
        std::vector<int> ns(ws->grid2);
        HIP_TRY(hipMemcpy(ns.data(), ws->d_nsteps2, ns.size() * sizeof(int), hipMemcpyDeviceToHost));
        if (tiles) *tiles = ns[0] + 2;
        return rc5;
    }
    // bits 8.. of `ablate`: hundreds of timed repetitions (sustained, power-limited state) instead of 10
    const int reps = (ablate >> 8) > 0 ? (ablate >> 8) * 100 : 10;
    ablate &= 0xff;
    if (tiles) *tiles = per_block;
    return stamped_run(n, out, max_tiles, kernel_ms, reps, [&](unsigned long long* dbg) { ca.dbg = dbg; return launch_trunk(n, ws, ca, ablate); });
}

#endif  // UVA_INSTRUMENT

// test hook: the packed MFMA weight image of convolution #conv_idx (host side, no device needed)
int uva_net_debug_packed_weights(uva_net* n, int conv_idx, uint16_t* out, size_t out_halfs, size_t* needed)
{
    if (!n || !n->g.model_loaded) return fail("no model");
    if (conv_idx == -1 && n->g.nf != 64) return fail("conv_idx -1 (tail_kernel image) exists for the 64-feature nets only");
    if (conv_idx < -1 || conv_idx >= (int)n->g.convs.size()) return fail("conv_idx out of range");
    std::vector<uint16_t> pk;
    if (conv_idx == -1) pack_tail64(n->g.convs.back(), pk);          // tail_kernel's image of the last convolution
    else if (conv_idx == 0) pack_head(n->g.convs[0], pk, nullptr);
    else if (n->g.nf == 64 && conv_idx + 1 < (int)n->g.convs.size()) pack_trunk64(n->g.convs[conv_idx], pk);
    else pack_conv3x3(n->g.convs[conv_idx], n->g.nf, pk, nullptr, nullptr);
    if (needed) *needed = pk.size();
    if (out && out_halfs >= pk.size()) std::memcpy(out, pk.data(), pk.size() * 2);
    return 0;
}

// the two trunk step-list hooks: the frame's plan as get_workspace gets it, one of its step lists copied out
static int debug_trunk_schedule(bool wino, int h, int w, int tile_size, int border, int grid, uint32_t* steps_words,
                                size_t capacity_words, size_t* needed_words, int* nsteps, int* stride,
                                long long* plane_info, int max_planes, int* nplanes, long long* guard_bytes)
{
    if (h <= 0 || w <= 0 || grid < 8 || grid % 8) return fail("bad argument");
    FramePlan plan;
    std::string err;
    if (plan_frame(h, w, tile_size, border, 64, grid, plan_switches(), plan, err)) return fail(err);
    const std::vector<PlaneDesc>& planes = plan.planes;
    const std::vector<Trunk2Step>& steps = wino ? plan.stepsw : plan.steps2;
    const std::vector<int>& ns = wino ? plan.nstepsw : plan.nsteps2;
    if (needed_words) *needed_words = steps.size() * 8;
    if (stride) *stride = wino ? plan.max_stepsw + TW_PAD_STEPS : plan.max_steps2 + T2_PAD_STEPS;
    if (nplanes) *nplanes = (int)planes.size();
    if (guard_bytes) *guard_bytes = (long long)plan.guard_bytes;
    if (plane_info)
        for (int i = 0; i < (int)planes.size() && i < max_planes; ++i) {
            plane_info[4 * i + 0] = planes[i].h; plane_info[4 * i + 1] = planes[i].w;
            plane_info[4 * i + 2] = planes[i].pitch; plane_info[4 * i + 3] = planes[i].act_off;
        }
    if (!steps_words || capacity_words < steps.size() * 8) return fail("steps buffer too small");
    std::memcpy(steps_words, steps.data(), steps.size() * sizeof(Trunk2Step));
    if (nsteps) std::copy(ns.begin(), ns.end(), nsteps);
    return 0;
}

int uva_debug_trunk2_schedule(int h, int w, int tile_size, int border, int grid, uint32_t* steps_words,
                              size_t capacity_words, size_t* needed_words, int* nsteps, int* stride,
                              long long* plane_info, int max_planes, int* nplanes, long long* guard_bytes)
{
    return debug_trunk_schedule(false, h, w, tile_size, border, grid, steps_words, capacity_words, needed_words, nsteps, stride,
                                plane_info, max_planes, nplanes, guard_bytes);
}

int uva_debug_trunkw_schedule(int h, int w, int tile_size, int border, int grid, uint32_t* steps_words,
                              size_t capacity_words, size_t* needed_words, int* nsteps, int* stride,
                              long long* plane_info, int max_planes, int* nplanes, long long* guard_bytes)
{
    return debug_trunk_schedule(true, h, w, tile_size, border, grid, steps_words, capacity_words, needed_words, nsteps, stride,
                                plane_info, max_planes, nplanes, guard_bytes);
}

// the row-list hooks (frames > 0: sub10_kernel's list for that many frames; 0: sub5_kernel's): the one builder, the copy-out
static int debug_strip_rows(int h, int w, int frames, int grid, uint32_t* rows_words, size_t capacity_words, size_t* needed_words,
                            int* nrows, int* stride)
{
    if (h <= 0 || w <= 0 || grid < 8 || grid % 8) return fail("bad argument");
    std::vector<uint4> rows;
    std::vector<int> nr;
    int max_rows = 0;
    std::string err;
    const int rc = frames ? build_sub10_rows(h, w, frames, grid, rows, nr, &max_rows, err) : build_sub5_rows(h, w, grid, rows, nr, &max_rows, err);
    if (rc == 2) return fail(frames ? "frame too large for the fused 1x kernel's row table" : "frame too large for sub5_kernel's row table");
    if (rc) return fail(err);
    if (needed_words) *needed_words = rows.size() * 4;
    if (stride) *stride = max_rows;
    if (!rows_words || capacity_words < rows.size() * 4) return fail("rows buffer too small");
    std::memcpy(rows_words, rows.data(), rows.size() * sizeof(uint4));
    if (nrows) std::copy(nr.begin(), nr.end(), nrows);
    return 0;
}

int uva_debug_sub10_rows(int h, int w, int grid, uint32_t* rows_words, size_t capacity_words, size_t* needed_words,
                         int* nrows, int* stride)
{
    return debug_strip_rows(h, w, 1, grid, rows_words, capacity_words, needed_words, nrows, stride);
}

int uva_debug_sub10_rows_batch(int h, int w, int frames, int grid, uint32_t* rows_words, size_t capacity_words, size_t* needed_words,
                               int* nrows, int* stride)
{
    if (frames < 1 || frames > S10_MAXB) return fail("bad argument");
    return debug_strip_rows(h, w, frames, grid, rows_words, capacity_words, needed_words, nrows, stride);
}

int uva_debug_sub5_rows(int h, int w, int grid, uint32_t* rows_words, size_t capacity_words, size_t* needed_words, int* nrows, int* stride)
{
    return debug_strip_rows(h, w, 0, grid, rows_words, capacity_words, needed_words, nrows, stride);
}

}  // extern "C"
