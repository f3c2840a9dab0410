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
    DevPtr<PlaneDesc> d_planes;
    DevPtr<uint4> d_sched4;      // per 4-row work tile: trunk_kernel's schedule entry (ConvArgs::sched4)
    // Activation buffers: act_base[i] is the allocation, act[i] = act_base[i] + guard_bytes the planes.
    size_t alloc_bytes = 0;      // device bytes of the two activation buffers (the cache's LRU budget)
    DevPtr<char> act_base[2];
    _Float16* act[2] = {nullptr, nullptr};
    // sub10_kernel (the whole 24-feature 1x net in one launch): per-workgroup row descriptors
    // (one set per number of frames in a launch, built on first use: [k - 1] = k frames; uva_net_process_u8_device_batch)
    DevPtr<uint4> d_rows10[S10_MAXB];
    DevPtr<int> d_nrows10[S10_MAXB];
    int max_rows10[S10_MAXB] = {}, grid10 = 0;
    bool sub10_unfit = false;             // one frame does not fit the kernel's row table: the per-pair path
    int sub10_max_batch = S10_MAXB;       // the largest number of frames whose row table fits (found on demand)
    // sub5_kernel (the 1x net as two launches of five layers, two pipelines per workgroup): row descriptors and the 24-channel
    // image between the launches
    DevPtr<uint4> d_rows5;
    DevPtr<int> d_nrows5;
    int max_rows5 = 0, grid5 = 0;
    DevPtr<char> d_mid5;
    bool sub5_unfit = false;
    // trunk2_kernel (fused layer pair): per-workgroup step lists
    DevPtr<Trunk2Step> d_steps2;
    DevPtr<int> d_nsteps2;
    int max_steps2 = 0, grid2 = 0;
    // trunkw_kernel (fused layer pair, Winograd F(2,3)): its own step lists (segments start without the shared rows)
    DevPtr<Trunk2Step> d_stepsw;
    DevPtr<int> d_nstepsw;
    int max_stepsw = 0;
};

struct DeviceLayer {
    DevPtr<half8> wpk;
    DevPtr<half8> wpk_w;      // 64 -> 64 trunk layers: pack_trunk64_wino image for trunkw_kernel
    DevPtr<half8> wpk_wn;     // ... the same for a launch's FIRST layer whose input arrives with the previous layer's slope > 1 channels
                              // still negated (the launch before it did not restore their sign: run_graph, `carry`)
    DevPtr<float> bias_w;     // ... and its bias, negated for the channels trunkw_kernel computes negated (uva_wino.h TW_ACT_F16)
    bool flip_w = false;      // ... which this layer has (a PReLU slope above 1)
    DevPtr<half8> wpk16;      // tail layer of the 64-feature 2x / 4x nets: pack_tail64 image for tail_kernel / tail4_kernel
    DevPtr<half8> wpk_s10;    // 24-feature 1x net: pack_sub16 image for sub10_kernel, with its own (sign-folded) bias
    DevPtr<float> bias_s10;
    DevPtr<float> bias;
    DevPtr<float> slope;
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

namespace uva {

// pipelined host route (uva_net_submit_u8 / uva_net_collect_u8): H2D, kernels and D2H of consecutive frames overlap on three
// streams; PIPE_SLOTS frames may be in flight
struct PipeSlot {
    bool busy = false;
    long long ticket = -1;
    DevBuf<uint8_t> d_in, d_out;
    HostBuf<uint8_t> h_in, h_out;        // pinned staging
    DevBuf<uint8_t> d_png;               // the PNG encoder's blocks: [meta][slots], then [the blocks packed end to end]
    DevBuf<uint8_t> d_pin, d_pout;       // uva_net_submit_pix: the packed frames (d_in / d_out hold their BGR)
    DevBuf<uint8_t> d_rs;                // uva_net_submit_pix_sized: the net's result resampled to the output size (BGR)
    DevBuf<uint8_t> d_win;               // uva_net_set_input_window, a window narrower than the frame: its rows at full width
    uint8_t* png_ws = nullptr;           // PNG submit: the caller's workspace, how many packed bytes went there with the
    size_t png_sent = 0;                 // frame's download, and the frame size (collect fetches the rest, if any)
    int png_h = 0, png_w = 0, png_bits = 8;   // (png_bits 16: the 16-bit encoder's workspace layout)
    Event ev_h2d, ev_done, ev_d2h;       // (made together: ev_d2h says that all three are there)
    static constexpr int BANDS = 4;      // a staged (pageable) result comes down in row bands: collect copies band k to the
    Event ev_band[BANDS];                // caller while band k + 1 is still on PCIe
    uint8_t* user_out = nullptr;         // where collect copies the staged result (null: D2H went there directly)
    size_t user_out_stride = 0, out_row = 0;
    int out_rows = 0;
};

// uva_net_set_skip_repeats: the kept frame -- the last frame the net ran on -- with its packed input
// and the bytes that were downloaded for it, both in HBM; nothing here is allocated before a frame is submitted with
// threshold >= 0
struct KeptFrame {
    bool valid = false;                  // there is a kept frame, key says with which arguments it ran
    SubmitKey key = {};
    DevBuf<uint8_t> d_in, d_res;
    DevPtr<FrameDiffStats> d_stats;      // the kernel's record,
    HostPtr<FrameDiffStats> h_stats;     // and where it is read back (page-locked)
    Event ev_stats, ev_written, ev_read; // (made after the two records: ev_read says that all five are there)
    bool reads_pending = false;          // ev_read has been recorded since d_res was last written
};

// profiling: the events of one frame (three intervals: head, trunk, tail), or of one launch
struct EvSet { Event e[4]; int ntrunk; };
struct EvPair { Event a, b; int kind; };    // generic graphs: one launch of rdb4_kernel (kind 1) / the 192 -> 64 convolution (2);
                                            // the 1x net's sub10_kernel16 (kind 3)

// What a net holds on its device.  free_device drops it as a whole, ensure_device builds it in a local and moves it in when
// it is complete.  The members are assigned, and so released, in the order they are declared: buffers before streams.
struct NetDevice {
    bool dev_ready = false;
    bool attr_set[40] = {false};  // hipFuncAttributeMaxDynamicSharedMemorySize done for kernel slot k on this net's device
    std::vector<DeviceLayer> layers;
    std::list<Workspace> wss;     // most recently used first
    LastCall last;
    GenericDevice gd;
    DevBuf<float> d_fin, d_fout;  // staging for the f32 (Extractor) entry point
    DevPtr<_Float16> d_sink;      // where out-of-image lanes of the trunk kernel store to
    static constexpr int PIPE_SLOTS = 3;
    PipeSlot pipe[PIPE_SLOTS];
    KeptFrame kept;
    std::vector<Event> ev_free;        // timing-only events (no system-scope fence: take_event)
    std::vector<Event> ev_sync_free;   // ordering events between streams (SyncEventScope)
    std::vector<EvSet> ev_pending;
    std::vector<EvPair> ev_pairs;
    Stream s_h2d, s_d2h;               // (made together: s_d2h says that both are there)
    Stream stream;
};

}  // namespace uva

struct uva_net : NetDevice {
    int device = 0;
    Graph g;
    // graphs outside the SRVGGNetCompact pattern (4x_Valar_v1, `-m r`): generic layer-by-layer executor
    bool generic = false;
    GenericGraph gg;
    int ncu = 256;
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
    size_t png_guess = 0;                // packed bytes of the last PNG frame collected: the next download's size
    size_t png_guess16 = 0;              // ... of the last 16-bit PNG frame (about twice the size: a guess of its own)
    long long next_ticket = 0;
    struct Repeat {                      // uva_net_set_skip_repeats: the option and its counters (the kept frame: NetDevice::kept)
        int threshold = -1;              // -1: off
        long long submitted = 0, skipped = 0;
    };
    Repeat rep;
    // uva_net_set_input_window: the frames the pixel-format submit entries are given are dense
    // src_h x src_w frames of which the call's h x w at (x, y) is uploaded; src_h == 0: off
    SubmitWindow win;
    // profiling
    bool prof = false;
    long long launches[4] = {0, 0, 0, 0};       // [3]: sub10_kernel16
    double total_ms[4] = {0, 0, 0, 0};

    // the ordered teardown: the device current, the three streams waited for, the device state dropped
    void free_device()
    {
        if (!dev_ready) return;
        (void)hipSetDevice(device);
        for (hipStream_t s : {stream.get(), s_h2d.get(), s_d2h.get()})
            if (s) (void)hipStreamSynchronize(s);
        static_cast<NetDevice&>(*this) = NetDevice();
    }
};

namespace uva {

// -> an empty handle (with the error recorded) if the runtime cannot create another event
Event take_event(uva_net* n);

// `count` timing events (4: a frame's set, 2: a pair around one launch) from the net's pool for the length of a scope.
// record(k) records event k on the net's stream, last(tag) records the last one and queues the set for resolve_events
// (tag: the set's trunk launches, the pair's kind); events that were not queued -- one could not be created, a call in
// between failed -- go back to the pool on every path out.  Off, or without its events, every call does nothing.
struct EvScope {
    uva_net* n;
    int count = 0;
    Event e[4];
    EvScope(uva_net* net, int cnt, bool on) : n(net)
    {
        for (int k = 0; on && k < cnt; ++k)
            if (!(e[k] = take_event(n))) return;
        if (on) count = cnt;
    }
    EvScope(const EvScope&) = delete;
    EvScope& operator=(const EvScope&) = delete;
    bool taken() const { return count > 0; }
    hipError_t record(int k) { return count ? hipEventRecord(e[k], n->stream) : hipSuccess; }
    hipError_t last(int tag)
    {
        if (!count) return hipSuccess;
        const hipError_t rc = hipEventRecord(e[count - 1], n->stream);
        if (rc != hipSuccess) return rc;
        if (count == 4) {
            EvSet s;
            for (int k = 0; k < 4; ++k) s.e[k] = std::move(e[k]);
            s.ntrunk = tag;
            n->ev_pending.push_back(std::move(s));
        } else {
            n->ev_pairs.push_back(EvPair{std::move(e[0]), std::move(e[1]), tag});
        }
        return hipSuccess;
    }
    ~EvScope()
    {
        for (Event& q : e)
            if (q) n->ev_free.push_back(std::move(q));
    }
};

// generic graphs (csrc/uva_generic_run.hip): one f32 plane, and the u8 frame call -- every reference tile is one plane
int generic_run_plane(uva_net* n, bool f32, const void* src, size_t src_stride, int sy0, int sx0, int h, int w, void* dst,
                      size_t dst_stride, int cy0, int cy1, int cx0, int cx1);
int generic_process_u8_device(uva_net* n, const void* d_in, int h, int w, size_t in_stride, void* d_out, size_t out_stride,
                              int tile_size, int border);

}  // namespace uva
