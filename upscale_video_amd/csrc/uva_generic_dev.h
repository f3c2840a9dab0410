// uva_generic_dev.h -- the host side of the generic executor's device state (csrc/uva_generic.hip.h, csrc/uva_rdb.hip.h hold the
// kernels): the arrays, the per-net weights and plans, and the work lists of the strip-walking kernels.  No device code, so
// that uva_net (csrc/uva_net.h) can hold a GenericDevice in translation units that compile none of those kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <tuple>
#include <vector>

#include "uva_devutil.hip.h"
#include "uva_generic.h"
#include "uva_own.h"
#include "uva_sw.h"

namespace uva {

// blob b of an h x w plane at scale s: [(h*s + 3)][(w*s + 2)][cpad] fp16; pixel (y, x) at row y+1, col x+1;
// one guard row behind the bottom border row (the convolution reads 16-pixel groups past the right edge)
struct GBuf {
    _Float16* p = nullptr;
    int h = 0, w = 0, c = 0, cpad = 0;
    size_t elems() const { return (size_t)(h + 3) * (w + 2) * cpad; }
    size_t pitch() const { return (size_t)(w + 2) * cpad; }
};

constexpr int GC_TH = 8, GC_TW = 32;
constexpr int GC_CH = 1;          // input channels go through LDS 32 at a time (one k-step): 33 KB and 80-100 registers per
                                  // workgroup, four of them share a CU (64 at a time: two or three, -14 % on Valar)
// (ksize 1: the same kernel without the halo and with a single tap -- the RRDBs' 1x1 residual convolutions)
inline size_t g_conv3_lds_bytes(int cin_pad, int mbn, int ksize = 3, bool wg = false, int nw = 4)
{
    const int th = 2 * nw;                                                                             // tile rows: two per wave
    const size_t npix = (size_t)(th + ksize - 1) * (GC_TW + ksize - 1);
    const int cn = std::min(GC_CH, cin_pad / 32);
    const size_t work = npix * (cn * 64 + 16) + (wg ? 0 : (size_t)ksize * cn * mbn * 1024);            // halo tile chunk + one row of taps
    const size_t stage = (size_t)th * GC_TW * (mbn * 32 + 16);                                         // the epilogue's output staging tile
    return work > stage ? work : stage;
}

// rdb4_kernel (csrc/uva_rdb.hip.h): a strip computes RA_C columns
struct RdbSeg { int c0, yb, ye, own0, own1, plane, pad1, pad2; };   // of plane `plane`: computed columns [c0, c0+48); output rows [yb, ye), columns [own0, own1)
constexpr int RA_C = 48;

// g_conv3_sw's work list: every plane (dims[2k], dims[2k+1] = its height, width) is cut into strips of `cols` columns, a
// strip into blocks of SW_R rows; the blocks -- plane after plane, strip after strip, top to bottom -- are dealt out to
// `grid` workgroups in contiguous runs of equal length (+-1); a run that crosses a strip's end becomes two segments.
// seg_begin has grid + 1 entries.
inline void sw_segments(const std::vector<int>& dims, int cols, int grid, std::vector<GSwSeg>& segs, std::vector<int>& seg_begin)
{
    struct Strip { int plane, c0, nb, h; };
    std::vector<Strip> strips;
    long long total = 0;
    for (size_t pl = 0; 2 * pl + 1 < dims.size(); ++pl) {
        const int h = dims[2 * pl], w = dims[2 * pl + 1], nb = (h + SW_R - 1) / SW_R;
        for (int c0 = 0; c0 < w; c0 += cols) { strips.push_back(Strip{(int)pl, c0, nb, h}); total += nb; }
    }
    segs.clear();
    seg_begin.assign(1, 0);
    // Several planes: like rdb_segments, a segment's start (two barriers and the wait for its first six rows) is counted as
    // SW_FILL blocks and the budget of blocks + starts is what the workgroups share evenly (UVA_RDB_DEAL=0: blocks alone).
    constexpr int SW_FILL = 1;
    static const bool by_steps = [] { const char* e = uva::debug_env("UVA_RDB_DEAL"); return !e || std::atoi(e) != 0; }();
    if (by_steps && dims.size() > 2) {
        auto deal = [&](long long T, bool emit) -> int {
            size_t si = 0;
            int y = 0, g = 0;
            if (emit) { segs.clear(); seg_begin.assign(1, 0); }
            while (si < strips.size()) {
                long long cap = T;
                while (si < strips.size() && cap > SW_FILL) {
                    const Strip& st = strips[si];
                    const int take = (int)std::min<long long>(st.nb - y, cap - SW_FILL);
                    if (emit) segs.push_back(GSwSeg{st.c0, y * SW_R, std::min(st.h, (y + take) * SW_R), st.plane});
                    cap -= take + SW_FILL;
                    y += take;
                    if (y == st.nb) { ++si; y = 0; }
                }
                ++g;
                if (emit) seg_begin.push_back((int)segs.size());
            }
            return g;
        };
        long long lo = total / grid + SW_FILL + 1, hi = total + SW_FILL * (long long)strips.size() + 1;
        while (lo < hi) {
            const long long mid = (lo + hi) / 2;
            if (deal(mid, false) <= grid) hi = mid; else lo = mid + 1;
        }
        deal(lo, true);
        while ((int)seg_begin.size() < grid + 1) seg_begin.push_back((int)segs.size());
        return;
    }
    size_t si = 0;
    long long sbase = 0;                       // blocks before strip si
    for (int g = 0; g < grid; ++g) {
        long long u = total * g / grid;
        const long long u1 = total * (g + 1) / grid;
        while (u < u1) {
            while (u >= sbase + strips[si].nb) { sbase += strips[si].nb; ++si; }
            const Strip& st = strips[si];
            const int b0 = (int)(u - sbase), b1 = (int)std::min<long long>(st.nb, b0 + (u1 - u));
            segs.push_back(GSwSeg{st.c0, b0 * SW_R, std::min(st.h, b1 * SW_R), st.plane});
            u += b1 - b0;
        }
        seg_begin.push_back((int)segs.size());
    }
}
inline void sw_segments(int h, int w, int cols, int grid, std::vector<GSwSeg>& segs, std::vector<int>& seg_begin)
{
    sw_segments(std::vector<int>{h, w}, cols, grid, segs, seg_begin);
}

// rdb4_kernel's work list: strips of 48 computed columns that own 42 of them (45 at the plane's left edge, everything up
// to the right edge in the last one), cut into row segments.
inline void rdb_strips(int h, int w, int plane, std::vector<RdbSeg>& strips)
{
    for (int own0 = 0; own0 < w;) {
        RdbSeg s{};
        s.c0 = own0 == 0 ? 0 : own0 - 3;
        s.own0 = own0;
        s.own1 = s.c0 + RA_C >= w ? w : s.c0 + RA_C - 3;
        s.yb = 0;
        s.ye = h;
        s.plane = plane;
        strips.push_back(s);
        own0 = s.own1;
    }
}
// Several planes in one launch (dims[2k], dims[2k+1] = height, width of plane k): the rows of all strips, plane after
// plane and strip after strip, are dealt out to the workgroups in contiguous runs of equal length; a run that crosses a
// strip's end becomes two segments (each costs RA_LAG steps of pipeline fill: with a whole frame's rows to share, runs are
// a couple of hundred rows long).  One plane: rdb_segments(h, w, ...) below, one segment per workgroup.
inline void rdb_segments(const std::vector<int>& dims, int grid, std::vector<RdbSeg>& segs, std::vector<int>& seg_begin);
inline void rdb_segments(int h, int w, int grid, std::vector<RdbSeg>& segs, std::vector<int>& seg_begin)
{
    std::vector<RdbSeg> strips;
    rdb_strips(h, w, 0, strips);
    // Every segment costs RA_LAG steps of pipeline fill, so a workgroup gets ONE: each strip is cut into k = grid / strips
    // equal row ranges (a few workgroups stay idle; with more strips than workgroups, whole strips are dealt out in turn).
    segs.clear();
    seg_begin.assign(1, 0);
    const int ns = (int)strips.size();
    if (ns >= grid) {
        for (int g = 0; g < grid; ++g) {
            for (int s = g; s < ns; s += grid) {
                RdbSeg sg = strips[s];
                sg.yb = 0;
                sg.ye = h;
                segs.push_back(sg);
            }
            seg_begin.push_back((int)segs.size());
        }
        return;
    }
    const int k = std::max(1, std::min(grid / ns, (h + 7) / 8));     // (ranges of fewer than ~8 rows are all pipeline fill)
    for (int g = 0; g < grid; ++g) {
        const int s = g / k, j = g - s * k;
        if (s < ns) {
            RdbSeg sg = strips[s];
            sg.yb = (int)((long long)h * j / k);
            sg.ye = (int)((long long)h * (j + 1) / k);
            if (sg.ye > sg.yb) segs.push_back(sg);
        }
        seg_begin.push_back((int)segs.size());
    }
}

inline void rdb_segments(const std::vector<int>& dims, int grid, std::vector<RdbSeg>& segs, std::vector<int>& seg_begin)
{
    if (dims.size() == 2) { rdb_segments(dims[0], dims[1], grid, segs, seg_begin); return; }
    std::vector<RdbSeg> strips;
    long long total = 0;
    for (size_t pl = 0; 2 * pl + 1 < dims.size(); ++pl) {
        const size_t n0 = strips.size();
        rdb_strips(dims[2 * pl], dims[2 * pl + 1], (int)pl, strips);
        total += (long long)(strips.size() - n0) * dims[2 * pl];
    }
    // What is dealt out evenly is STEPS, not rows: a segment costs its rows plus RDB_FILL steps of pipeline fill, and a
    // workgroup whose run crosses a strip's end has two segments (dealing rows alone left those 9 steps -- 4 % -- longer than
    // the others: the launch's tail).  A workgroup takes strip rows, in order, until its budget T is used up; T is the
    // smallest budget with which `grid` workgroups are enough.  UVA_RDB_DEAL=0: rows dealt evenly, the A/B switch.
    constexpr int RDB_FILL = 9;                // rdb4_kernel's RA_LAG
    static const bool by_steps = [] { const char* e = uva::debug_env("UVA_RDB_DEAL"); return !e || std::atoi(e) != 0; }();
    auto deal = [&](long long T, bool emit) -> int {
        size_t si = 0;
        int y = 0, g = 0;
        if (emit) { segs.clear(); seg_begin.assign(1, 0); }
        while (si < strips.size()) {
            long long cap = T;
            while (si < strips.size() && cap > RDB_FILL) {
                const int take = (int)std::min<long long>(strips[si].ye - y, cap - RDB_FILL);
                if (emit) { RdbSeg sg = strips[si]; sg.yb = y; sg.ye = y + take; segs.push_back(sg); }
                cap -= take + RDB_FILL;
                y += take;
                if (y == strips[si].ye) { ++si; y = 0; }
            }
            ++g;
            if (emit) seg_begin.push_back((int)segs.size());
        }
        return g;
    };
    if (by_steps) {
        long long lo = total / grid + RDB_FILL + 1, hi = total + RDB_FILL * (long long)strips.size() + 1;     // (a budget <= RDB_FILL buys no row)
        while (lo < hi) {
            const long long mid = (lo + hi) / 2;
            if (deal(mid, false) <= grid) hi = mid; else lo = mid + 1;
        }
        deal(lo, true);
        while ((int)seg_begin.size() < grid + 1) seg_begin.push_back((int)segs.size());
        return;
    }
    segs.clear();
    seg_begin.assign(1, 0);
    size_t si = 0;
    long long sbase = 0;                       // rows before strip si
    for (int g = 0; g < grid; ++g) {
        long long u = total * g / grid;
        const long long u1 = total * (g + 1) / grid;
        while (u < u1) {
            while (u >= sbase + strips[si].ye) { sbase += strips[si].ye; ++si; }
            RdbSeg sg = strips[si];
            const int y0 = (int)(u - sbase), y1 = (int)std::min<long long>(sg.ye, y0 + (u1 - u));
            sg.yb = y0;
            sg.ye = y1;
            segs.push_back(sg);
            u += y1 - y0;
        }
        seg_begin.push_back((int)segs.size());
    }
}

// ---------------------------------------------------------------------------------------------------
struct GenericDevice {
    struct ConvDev {
        DevPtr<half8> wpk;
        DevPtr<half8> wpk_lds;        // g_conv3_lds's image (3x3 convolutions with <= 64 output channels)
        DevPtr<half8> wpk_w;          // g_conv3_sww's image (192 -> 64, 3x3: pack_generic_wino)
        DevPtr<float> bias;
        int cin_pad = 0, cout_pad = 0;
    };
    std::vector<ConvDev> convs;
    std::vector<DevPtr<float>> prelu;
    // the zero-bordered arrays: `arrays` owns every one of them, lent out (a GBuf) or not; pool lists the ones that are free
    std::vector<DevPtr<_Float16>> arrays;
    std::map<std::tuple<int, int, int>, std::vector<_Float16*>> pool;     // (h, w, channels) -> free arrays
    size_t pool_bytes = 0;
    // g_conv3_sw: the strip segments of an h x w plane, dealt out to `grid` workgroups (sw_segments)
    struct SwPlan { DevPtr<GSwSeg> segs; DevPtr<int> seg_begin; int grid = 0; };
    std::map<std::vector<int>, SwPlan> sw_plans;                          // (strip columns, h0, w0, h1, w1, ...)
    struct RdbPlan { DevPtr<RdbSeg> segs; DevPtr<int> seg_begin; int grid = 0; };
    std::map<std::vector<int>, RdbPlan> rdb_plans;                        // (h0, w0, h1, w1, ...)
    std::vector<RdbMatch> rdbs;                                           // find_rdbs() of the loaded graph
    DevPtr<unsigned long long> rdb_dbg;                                   // UVA_INSTRUMENT + UVA_RDB_STAMPS=1: rdb4_kernel's stamps

    static int pad32(int c) { return (c + 31) / 32 * 32; }
};

}  // namespace uva
