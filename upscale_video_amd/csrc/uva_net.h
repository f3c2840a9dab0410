// uva_net.h -- struct uva_net (one net = one ncnn.Net: a HIP stream, the packed weights, the cached workspaces, the pipelined
// route's slots) and what its translation units share.  csrc/uva_api.hip owns the nets; csrc/uva_generic_run.hip runs the
// generic graphs on them.  No device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <list>
#include <vector>

#include "../../include/uva.h"
#include "uva_devutil.hip.h"
#include "uva_generic.h"
#include "uva_generic_dev.h"
#include "uva_model.h"
#include "uva_plan.h"
#include "uva_repeat.h"
#include "uva_rt.h"
#include "uva_sub10.h"
#include "uva_submit.h"

namespace uva {

struct Workspace : PlaneLayout {        // (planes, tile counts, act_pixels, guard_bytes: the planner's, uva_plan.h)
    int h = 0, w = 0, tile_size = 0, border = 0;
    PlaneDesc* d_planes = nullptr;
    uint4* d_sched4 = nullptr;   // per 4-row work tile: trunk_kernel's schedule entry (ConvArgs::sched4)
    // Activation buffers: act_base[i] is the allocation, act[i] = act_base[i] + guard_bytes the planes.
    size_t alloc_bytes = 0;      // device bytes of the two activation buffers (the cache's LRU budget)
    char* act_base[2] = {nullptr, nullptr};
    _Float16* act[2] = {nullptr, nullptr};
    // sub10_kernel (the whole 24-feature 1x net in one launch): per-workgroup row descriptors
    // (one set per number of frames in a launch, built on first use: [k - 1] = k frames; uva_net_process_u8_device_batch)
    uint4* d_rows10[S10_MAXB] = {};
    int* d_nrows10[S10_MAXB] = {};
    int max_rows10[S10_MAXB] = {}, grid10 = 0;
    bool sub10_unfit = false;             // one frame does not fit the kernel's row table: the per-pair path
    int sub10_max_batch = S10_MAXB;       // the largest number of frames whose row table fits (found on demand)
    // sub5_kernel (the 1x net as two launches of five layers, two pipelines per workgroup): row descriptors and the 24-channel
    // image between the launches
    uint4* d_rows5 = nullptr;
    int* d_nrows5 = nullptr;
    int max_rows5 = 0, grid5 = 0;
    char* d_mid5 = nullptr;
    bool sub5_unfit = false;
    // trunk2_kernel (fused layer pair): per-workgroup step lists
    Trunk2Step* d_steps2 = nullptr;
    int* d_nsteps2 = nullptr;
    int max_steps2 = 0, grid2 = 0;
    // trunkw_kernel (fused layer pair, Winograd F(2,3)): its own step lists (segments start without the shared rows)
    Trunk2Step* d_stepsw = nullptr;
    int* d_nstepsw = nullptr;
    int max_stepsw = 0;
    void release()
    {
        auto drop = [](auto*& p) { if (p) (void)hipFree(p); p = nullptr; };
        drop(d_planes); drop(d_sched4); drop(d_steps2); drop(d_nsteps2); drop(d_stepsw); drop(d_nstepsw);
        for (auto& q : d_rows10) drop(q);
        for (auto& q : d_nrows10) drop(q);
        drop(d_rows5); drop(d_nrows5); drop(d_mid5); drop(act_base[0]); drop(act_base[1]);
        act[0] = act[1] = nullptr;
    }
};

struct DeviceLayer {
    half8* wpk = nullptr;
    half8* wpk_w = nullptr;   // 64 -> 64 trunk layers: pack_trunk64_wino image for trunkw_kernel
    half8* wpk_wn = nullptr;  // ... the same for a launch's FIRST layer whose input arrives with the previous layer's slope > 1 channels
                              // still negated (the launch before it did not restore their sign: run_graph, `carry`)
    float* bias_w = nullptr;  // ... and its bias, negated for the channels trunkw_kernel computes negated (uva_wino.h TW_ACT_F16)
    bool flip_w = false;      // ... which this layer has (a PReLU slope above 1)
    half8* wpk16 = nullptr;   // tail layer of the 64-feature 2x / 4x nets: pack_tail64 image for tail_kernel / tail4_kernel
    half8* wpk_s10 = nullptr; // 24-feature 1x net: pack_sub16 image for sub10_kernel, with its own (sign-folded) bias
    float* bias_s10 = nullptr;
    float* bias = nullptr;
    float* slope = nullptr;
};

struct LastCall {
    bool valid = false;
    Workspace* ws = nullptr;
    bool f32 = false;
    const void* src = nullptr;
    size_t src_stride = 0;
    void* dst = nullptr;       // u8 route: device result buffer of the call
    size_t dst_stride = 0;
};

}  // namespace uva

using namespace uva;   // (uva_net is the C ABI's type, so it stands outside the namespace its members come from)

// uva_net::glaunch slots (include/uva.h uva_net_debug_generic_launches): 0..39 are the attr_set slots of the kernels that have
// one (11-23 g_conv3_lds, 24-27 / 29-31 g_conv3_sw, 28 rdb4_kernel, 32-34 g_conv3_sk), the rest have none
enum { GL_CONV1 = 40, GL_CONV3, GL_SWW, GL_SWW_SUM, GL_SWW_SUM2, GL_AXPBY, GL_AXPBY_STRIDED, GL_CONCAT_PART, GL_INTERP, GL_PRELU,
       GL_PIXELSHUFFLE, GL_INPUT_F32, GL_INPUT_U8, GL_OUTPUT_F32, GL_OUTPUT_U8, GL_COUNT };
struct uva_net {
    int device = 0;
    Graph g;
    // graphs outside the SRVGGNetCompact pattern (4x_Valar_v1, `-m r`): generic layer-by-layer executor
    bool generic = false;
    GenericGraph gg;
    GenericDevice gd;
    bool dev_ready = false;
    bool dev_partial = false;     // some device state exists (ensure_device started); free_device() must run
    int ncu = 256;
    hipStream_t stream = nullptr;
    std::vector<DeviceLayer> layers;
    std::list<Workspace> wss;   // most recently used first
    // staging for the f32 (Extractor) entry point
    float *d_fin = nullptr, *d_fout = nullptr;
    size_t d_fin_cap = 0, d_fout_cap = 0;
    _Float16* d_sink = nullptr;   // where out-of-image lanes of the trunk kernel store to
    bool attr_set[40] = {false};  // hipFuncAttributeMaxDynamicSharedMemorySize done for kernel slot k on this net's device
    long long glaunch[GL_COUNT] = {0};   // generic executor: launches per kernel instantiation since the net was created (uva_net_debug_generic_launches)
    int last_act_buf = 0;         // which ping-pong buffer the last run_graph() left its last trunk activation in
    bool generic_fuse_add = true; // generic graphs: sums that follow a convolution are done in its epilogue (UVA_GENERIC_FUSE_ADD=0: own launch)
    bool generic_lds_conv = true; // generic graphs: 3x3 convolutions through g_conv3_lds (UVA_GENERIC_LDS=0: the plain g_conv<3>)
    bool fuse_all = true;         // 24-feature 1x net: all ten convolutions in one launch (sub10_kernel); UVA_SUB10=0 turns it off
    bool split5 = false;          // ... as two launches of five layers instead (sub5_kernel, csrc/uva_sub5.hip.h); UVA_SUB5=1
    bool u16_1x = false;          // ... takes part in the 16-bit route (sub10_kernel16; uva_net_enable_u16_1x)
    bool fuse_pairs = true;       // 64-feature nets: trunk layers run two per launch (trunk2_kernel); UVA_TRUNK_FUSION=0 turns it off
    bool carry = true;            // ... and between two launches the negated channels stay negated in HBM (UVA_TW_CARRY=0: every launch
                                  // restores the signs in front of its stores), and trunkw_kernel's producers carry two rows' partial sums
                                  // from step to step (UVA_TW_CARRY=0: the k-loop that reads all six rows of a step's window)
    bool act16 = true;            // trunkw_kernel: PReLU on packed fp16 (uva_wino.h TW_ACT_F16); UVA_TW_ACT16=0: on the fp32 sums
    bool wino = true;             // ... as 1-D Winograd F(2,3) (trunkw_kernel); UVA_TRUNK_WINO=0: trunk2_kernel (direct convolution)
    LastCall last;
    // pipelined host route (uva_net_submit_u8 / uva_net_collect_u8): H2D, kernels and D2H of
    // consecutive frames overlap on three streams; PIPE_SLOTS frames may be in flight
    static constexpr int PIPE_SLOTS = 3;
    struct PipeSlot {
        bool busy = false;
        long long ticket = -1;
        uint8_t *d_in = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr;   // h_*: pinned staging
        uint8_t* d_png = nullptr;        // the PNG encoder's blocks: [meta][slots], then [the blocks packed end to end]
        uint8_t *d_pin = nullptr, *d_pout = nullptr;   // uva_net_submit_pix: the packed frames (d_in / d_out hold their BGR)
        uint8_t* d_rs = nullptr;         // uva_net_submit_pix_sized: the net's result resampled to the output size (BGR)
        uint8_t* d_win = nullptr;        // uva_net_set_input_window, a window narrower than the frame: its rows at full width
        size_t d_in_cap = 0, d_out_cap = 0, h_in_cap = 0, h_out_cap = 0, d_png_cap = 0, d_pin_cap = 0, d_pout_cap = 0, d_rs_cap = 0;
        size_t d_win_cap = 0;
        uint8_t* png_ws = nullptr;       // PNG submit: the caller's workspace, how many packed bytes went there with the
        size_t png_sent = 0;             // frame's download, and the frame size (collect fetches the rest, if any)
        int png_h = 0, png_w = 0, png_bits = 8;   // (png_bits 16: the 16-bit encoder's workspace layout)
        hipEvent_t ev_h2d = nullptr, ev_done = nullptr, ev_d2h = nullptr;
        static constexpr int BANDS = 4;  // a staged (pageable) result comes down in row bands: collect copies band k to the
        hipEvent_t ev_band[BANDS] = {nullptr, nullptr, nullptr, nullptr};   // caller while band k + 1 is still on PCIe
        uint8_t* user_out = nullptr;     // where collect copies the staged result (null: D2H went there directly)
        size_t user_out_stride = 0, out_row = 0;
        int out_rows = 0;
    };
    PipeSlot pipe[PIPE_SLOTS];
    size_t png_guess = 0;                // packed bytes of the last PNG frame collected: the next download's size
    size_t png_guess16 = 0;              // ... of the last 16-bit PNG frame (about twice the size: a guess of its own)
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    long long next_ticket = 0;
    // uva_net_set_skip_repeats: the kept frame -- the last frame the net ran on -- with its packed input
    // and the bytes that were downloaded for it, both in HBM; nothing here is allocated before a frame is submitted with
    // threshold >= 0
    struct Repeat {
        int threshold = -1;              // -1: off
        bool valid = false;              // there is a kept frame, key says with which arguments it ran
        SubmitKey key = {};
        uint8_t *d_in = nullptr, *d_res = nullptr;
        size_t d_in_cap = 0, d_res_cap = 0;
        FrameDiffStats *d_stats = nullptr, *h_stats = nullptr;    // the kernel's record, and where it is read back (page-locked)
        hipEvent_t ev_stats = nullptr, ev_written = nullptr, ev_read = nullptr;
        bool reads_pending = false;      // ev_read has been recorded since d_res was last written
        long long submitted = 0, skipped = 0;
    };
    Repeat rep;
    // uva_net_set_input_window: the frames the pixel-format submit entries are given are dense
    // src_h x src_w frames of which the call's h x w at (x, y) is uploaded; src_h == 0: off
    SubmitWindow win;
    void release_repeat()                // the device is current, nothing of this net is running
    {
        if (rep.d_in) (void)hipFree(rep.d_in);
        if (rep.d_res) (void)hipFree(rep.d_res);
        if (rep.d_stats) (void)hipFree(rep.d_stats);
        if (rep.h_stats) (void)hipHostFree(rep.h_stats);
        for (hipEvent_t e : {rep.ev_stats, rep.ev_written, rep.ev_read})
            if (e) (void)hipEventDestroy(e);
        Repeat fresh;
        fresh.threshold = rep.threshold; fresh.submitted = rep.submitted; fresh.skipped = rep.skipped;
        rep = fresh;
    }
    // profiling
    bool prof = false;
    std::vector<hipEvent_t> ev_free;        // timing-only events (no system-scope fence: take_event)
    std::vector<hipEvent_t> ev_sync_free;   // ordering events between streams (take_sync_event)
    struct EvSet { hipEvent_t e[4]; int ntrunk; };
    std::vector<EvSet> ev_pending;
    struct EvPair { hipEvent_t a, b; int kind; };       // generic graphs: one launch of rdb4_kernel (kind 1) / the 192 -> 64 convolution (2);
                                                        // the 1x net's sub10_kernel16 (kind 3)
    std::vector<EvPair> ev_pairs;
    long long launches[4] = {0, 0, 0, 0};       // [3]: sub10_kernel16
    double total_ms[4] = {0, 0, 0, 0};

    void free_device()
    {
        if (!dev_ready && !dev_partial) return;
        dev_partial = false;
        std::memset(attr_set, 0, sizeof attr_set);
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (auto& l : layers) {
            if (l.wpk) (void)hipFree(l.wpk);
            if (l.wpk_w) (void)hipFree(l.wpk_w);
            if (l.bias_w) (void)hipFree(l.bias_w);
            if (l.wpk_wn) (void)hipFree(l.wpk_wn);
            if (l.wpk16) (void)hipFree(l.wpk16);
            if (l.wpk_s10) (void)hipFree(l.wpk_s10);
            if (l.bias_s10) (void)hipFree(l.bias_s10);
            if (l.bias) (void)hipFree(l.bias);
            if (l.slope) (void)hipFree(l.slope);
        }
        layers.clear();
        for (auto& w : wss) w.release();
        wss.clear();
        gd.release();
        if (d_fin) (void)hipFree(d_fin);
        if (d_fout) (void)hipFree(d_fout);
        if (d_sink) (void)hipFree(d_sink);
        d_sink = nullptr;
        if (s_h2d) (void)hipStreamSynchronize(s_h2d);
        if (s_d2h) (void)hipStreamSynchronize(s_d2h);
        for (auto& ps : pipe) {
            if (ps.d_in) (void)hipFree(ps.d_in);
            if (ps.d_out) (void)hipFree(ps.d_out);
            if (ps.d_png) (void)hipFree(ps.d_png);
            if (ps.d_pin) (void)hipFree(ps.d_pin);
            if (ps.d_pout) (void)hipFree(ps.d_pout);
            if (ps.d_rs) (void)hipFree(ps.d_rs);
            if (ps.d_win) (void)hipFree(ps.d_win);
            if (ps.h_in) (void)hipHostFree(ps.h_in);
            if (ps.h_out) (void)hipHostFree(ps.h_out);
            if (ps.ev_h2d) (void)hipEventDestroy(ps.ev_h2d);
            if (ps.ev_done) (void)hipEventDestroy(ps.ev_done);
            if (ps.ev_d2h) (void)hipEventDestroy(ps.ev_d2h);
            for (auto& e : ps.ev_band)
                if (e) (void)hipEventDestroy(e);
            ps = PipeSlot();
        }
        release_repeat();
        if (s_h2d) (void)hipStreamDestroy(s_h2d);
        if (s_d2h) (void)hipStreamDestroy(s_d2h);
        s_h2d = s_d2h = nullptr;
        d_fin = d_fout = nullptr;
        d_fin_cap = d_fout_cap = 0;
        for (auto& s : ev_pending)
            for (auto e : s.e) (void)hipEventDestroy(e);
        ev_pending.clear();
        for (auto& q : ev_pairs) { (void)hipEventDestroy(q.a); (void)hipEventDestroy(q.b); }
        ev_pairs.clear();
        for (auto e : ev_free) (void)hipEventDestroy(e);
        ev_free.clear();
        for (auto e : ev_sync_free) (void)hipEventDestroy(e);
        ev_sync_free.clear();
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
        dev_ready = false;
        last = LastCall();
    }
};

namespace uva {

// -> nullptr (with the error recorded) if the runtime cannot create another event
hipEvent_t take_event(uva_net* n);

// A pair of events around one launch (profiling): begin() records the first, end() the second and queues the pair; a pair
// that is not completed -- an event could not be created, a call in between failed -- gives its events back.
struct EvPairScope {
    uva_net* n;
    uva_net::EvPair p;
    bool queued = false;
    EvPairScope(uva_net* net, int kind, bool on) : n(net), p{nullptr, nullptr, kind}
    {
        if (!on) return;
        p.a = take_event(n);
        p.b = p.a ? take_event(n) : nullptr;
        if (p.a && !p.b) { n->ev_free.push_back(p.a); p.a = nullptr; }
    }
    hipError_t begin() { return p.b ? hipEventRecord(p.a, n->stream) : hipSuccess; }
    hipError_t end()
    {
        if (!p.b) return hipSuccess;
        const hipError_t e = hipEventRecord(p.b, n->stream);
        if (e == hipSuccess) { n->ev_pairs.push_back(p); queued = true; }
        return e;
    }
    ~EvPairScope()
    {
        if (queued) return;
        if (p.a) n->ev_free.push_back(p.a);
        if (p.b) n->ev_free.push_back(p.b);
    }
};

// generic graphs (csrc/uva_generic_run.hip): one f32 plane, and the u8 frame call -- every reference tile is one plane
int generic_run_plane(uva_net* n, bool f32, const void* src, size_t src_stride, int sy0, int sx0, int h, int w, void* dst,
                      size_t dst_stride, int cy0, int cy1, int cx0, int cx1);
int generic_process_u8_device(uva_net* n, const void* d_in, int h, int w, size_t in_stride, void* d_out, size_t out_stride,
                              int tile_size, int border);

}  // namespace uva
