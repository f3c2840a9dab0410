// uva_generic_run.hip -- the generic layer-by-layer executor (graphs outside the SRVGGNetCompact pattern: 4x_Valar_v1, `-m r`):
// the kernels of csrc/uva_generic.hip.h and csrc/uva_rdb.hip.h, their launches on a uva_net, and the debug entries that restate
// its planning.
#include "../../include/uva.h"
#include "uva_generic.hip.h"
#include "uva_net.h"
#include "uva_plan.h"
#include "uva_rt.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

using namespace uva;

namespace {

// ---- generic graphs -------------------------------------------------------------------------------
int generic_acquire(uva_net* n, int h, int w, int c, GBuf* out)
{
    out->h = h; out->w = w; out->c = c; out->cpad = GenericDevice::pad32(c);
    auto& free_list = n->gd.pool[std::make_tuple(h, w, c)];
    if (!free_list.empty()) {
        out->p = free_list.back();
        free_list.pop_back();
        return 0;
    }
    const size_t bytes = out->elems() * 2;
    DevPtr<_Float16> d;
    HIP_TRY(alloc_into(d, bytes));
    HIP_TRY(hipMemsetAsync(d.get(), 0, bytes, n->stream));    // border and padding channels stay zero for the array's life
    out->p = d.get();
    n->gd.arrays.push_back(std::move(d));
    n->gd.pool_bytes += bytes;
    return 0;
}

void generic_release(uva_net* n, const GBuf& b)
{
    if (b.p) n->gd.pool[std::make_tuple(b.h, b.w, b.c)].push_back(b.p);
}

// One BATCH of planes (reference tiles, or the whole frame) through the graph in lockstep: layer by layer, every plane's
// launch of that layer -- and for the residual-dense-block kernels (csrc/uva_rdb.hip.h) ONE launch for all planes, their
// arrays in a table: a frame's small planes then share the workgroups with the large ones instead of under-filling the
// chip in launches of their own.  Arrays are recycled as soon as their last reader has been queued (stream order makes
// that safe) and only ever for a blob of the same shape, so borders and padding channels -- never written -- stay zero.
// All planes of a batch take the same kernels (generic_plane_class: the same side of every width threshold).
struct PlaneJob {
    const void* src; size_t src_stride; int sy0, sx0, h, w;
    void* dst; size_t dst_stride; int cy0, cy1, cx0, cx1;
};
// workgroups of the persistent kernels: one per CU (UVA_GENERIC_GRID=K: a test hook -- few workgroups give long segments
// and several of them per workgroup on frames small enough for the numpy restatement)
inline int generic_grid(const uva_net* n)
{
    static const int forced = [] { const char* e = uva::debug_env("UVA_GENERIC_GRID"); return e ? std::atoi(e) : 0; }();
    return forced > 0 ? forced : persistent_grid(n->ncu);
}
// (the strip kernels want 32 / 64 output columns at 1x, 2x or 4x the plane's width; a batch is planned with its narrowest
// plane, so mixing classes would only cost speed, never change a result)
inline int generic_plane_class(int w) { return (w >= 8) + (w >= 16) + (w >= 32) + (w >= 64); }

int generic_run_planes(uva_net* n, bool f32, const std::vector<PlaneJob>& jobs)
{
    const GenericGraph& g = n->gg;
    const int np = (int)jobs.size();
    if (np <= 0 || np > GEN_MAX_PLANES) return fail("generic executor: bad plane batch");
    auto root = [&](int b) { while (g.blobs[b].alias_of >= 0) b = g.blobs[b].alias_of; return b; };
    // dense chains (uva_generic.h plan_concat_groups): the blobs of a chain are channel ranges of one shared array, which
    // goes back to the pool when the last of them has been read.  Needs g_conv3_lds (prefix reads, strided writes).
    const bool use_groups = n->generic_lds_conv;
    auto group_of = [&](int b) { return use_groups ? g.blobs[b].group : -1; };
    struct PlaneState {
        PlaneJob j;
        std::vector<GBuf> buf, garr;
        std::vector<int> left, glive;
    };
    std::vector<PlaneState> P(np);
    int wmin = jobs[0].w;
    for (int pi = 0; pi < np; ++pi) {
        PlaneState& ps = P[pi];
        ps.j = jobs[pi];
        ps.buf.assign(g.blobs.size(), GBuf());
        ps.left.assign(g.blobs.size(), 0);
        for (size_t b = 0; b < g.blobs.size(); ++b) ps.left[b] = g.blobs[b].consumers;
        ps.garr.assign(g.group_channels.size(), GBuf());
        ps.glive.assign(g.group_blobs.begin(), g.group_blobs.end());
        wmin = std::min(wmin, jobs[pi].w);
    }
    auto done_with = [&](PlaneState& ps, int b) {
        b = root(b);
        if (--ps.left[b] != 0) return;
        const int gi = group_of(b);
        if (gi >= 0) {
            ps.buf[b].p = nullptr;
            if (--ps.glive[gi] == 0) { generic_release(n, ps.garr[gi]); ps.garr[gi].p = nullptr; }
        } else {
            generic_release(n, ps.buf[b]);
            ps.buf[b].p = nullptr;
        }
    };
    struct Cleanup {
        uva_net* n; std::vector<PlaneState>* P; const GenericGraph* g; bool use_groups;
        ~Cleanup()
        {
            for (PlaneState& ps : *P) {
                for (size_t b = 0; b < ps.buf.size(); ++b)
                    if (ps.buf[b].p && !(use_groups && g->blobs[b].group >= 0)) generic_release(n, ps.buf[b]);
                for (auto& a : ps.garr) if (a.p) generic_release(n, a);
            }
        }
    } cleanup{n, &P, &g, use_groups};
    const int T = 256;
    // Element-wise sums that directly follow a convolution of g_conv3_lds are done in its epilogue (GConvArgs::res): the
    // convolution's own result never goes to memory, the sum layer is skipped.  Conditions: the convolution's result has
    // no other reader, the other operand exists when the convolution runs, whole 16-byte channel units.
    std::vector<int> fuse_add(g.layers.size(), -1), fuse_pos(g.layers.size(), 0);
    std::vector<char> skip(g.layers.size(), 0);
    if (n->generic_lds_conv && n->generic_fuse_add) {
        std::vector<int> producer(g.blobs.size(), -1);
        for (size_t li = 0; li < g.layers.size(); ++li)
            if (g.layers[li].kind != GLayer::SPLIT && !g.layers[li].out.empty()) producer[g.layers[li].out[0]] = (int)li;
        for (size_t ri = 0; ri < g.layers.size(); ++ri) {
            const GLayer& r = g.layers[ri];
            if ((r.kind != GLayer::ADD && r.kind != GLayer::ELTWISE_SUM) || r.in.size() != 2 || r.coeffs.size() != 2) continue;
            for (int k = 0; k < 2 && !skip[ri]; ++k) {
                const int cb = root(r.in[k]), ob2 = root(r.in[1 - k]);
                const int li = producer[cb];
                if (li < 0 || cb == ob2 || g.layers[li].kind != GLayer::CONV || fuse_add[li] >= 0) continue;
                if (g.blobs[cb].consumers != 1 || g.blobs[cb].channels % 8 || group_of(cb) >= 0) continue;
                if (!n->gd.convs[g.layers[li].conv].wpk_lds || producer[ob2] < 0 || producer[ob2] >= li) continue;
                fuse_add[li] = (int)ri;
                fuse_pos[li] = k;
                skip[ri] = 1;
            }
        }
    }
    // g_conv3_sw (the 192 -> 64 and 64 -> 64 convolutions on planes wide enough for its strips) also takes a SECOND sum
    // behind the first -- the `rrdb_in*1.0 + rdb_out*0.2` that closes every third dense block of 4x_Valar_v1
    // (models/4x_Valar_v1.param:55-56): the first sum's result then never goes to memory either.
    static const bool sw_on = [] { const char* e = uva::debug_env("UVA_GENERIC_SW"); return !e || std::atoi(e) != 0; }();
    auto sw_cols_of = [&](size_t li) -> int {      // strip width g_conv3_sw would use for layer li on this plane, 0: not its case
        const GLayer& l = g.layers[li];
        if (!sw_on || !n->generic_lds_conv || l.kind != GLayer::CONV || l.ksize != 3) return 0;
        const GenericDevice::ConvDev& cd = n->gd.convs[l.conv];
        if (cd.cout_pad != 64 || g.blobs[l.out[0]].channels != 64 || (cd.cin_pad != 64 && cd.cin_pad != 192)) return 0;
        const int cols = cd.cin_pad == 192 ? sw_cols<1>() : sw_cols<2>();
        return wmin * g.blobs[l.out[0]].scale >= cols ? cols : 0;
    };
    // the instantiations of g_conv3_sw that exist (what 4x_Valar_v1 needs): -1 = none, the layer-by-layer kernel takes it
    auto sw_variant = [](int cin_pad, bool act, int rm, int rm2) -> int {
        if (cin_pad == 192 && !act && rm == 2 && rm2 == 0) return 0;
        if (cin_pad == 192 && !act && rm == 2 && rm2 == 2) return 1;
        if (cin_pad == 64 && !act && rm == 1 && rm2 == 0) return 2;
        if (cin_pad == 64 && act && rm == 0 && rm2 == 0) return 3;
        if (cin_pad == 192 && !act && rm == 0 && rm2 == 0) return 4;     // (UVA_GENERIC_FUSE_ADD=0: the sums as launches of their own)
        if (cin_pad == 64 && !act && rm == 0 && rm2 == 0) return 5;
        return -1;
    };
    std::vector<int> fuse_add2(g.layers.size(), -1), fuse_pos2(g.layers.size(), 0);
    static const bool add2_on = [] { const char* e = uva::debug_env("UVA_GENERIC_FUSE_ADD2"); return !e || std::atoi(e) != 0; }();
    if (n->generic_lds_conv && n->generic_fuse_add && add2_on) {
        std::vector<int> producer(g.blobs.size(), -1);
        std::vector<std::vector<int>> readers(g.blobs.size());
        for (size_t li = 0; li < g.layers.size(); ++li) {
            if (g.layers[li].kind == GLayer::SPLIT) continue;
            if (!g.layers[li].out.empty()) producer[g.layers[li].out[0]] = (int)li;
            for (int b : g.layers[li].in) readers[root(b)].push_back((int)li);
        }
        for (size_t li = 0; li < g.layers.size(); ++li) {
            if (fuse_add[li] < 0 || !sw_cols_of(li)) continue;
            const int o1 = root(g.layers[fuse_add[li]].out[0]);
            if (g.blobs[o1].consumers != 1 || readers[o1].size() != 1 || group_of(o1) >= 0 || o1 == root(g.out_blob)) continue;
            const int ri = readers[o1][0];
            const GLayer& r = g.layers[ri];
            if ((r.kind != GLayer::ADD && r.kind != GLayer::ELTWISE_SUM) || r.in.size() != 2 || r.coeffs.size() != 2 || skip[ri]) continue;
            const int k = root(r.in[0]) == o1 ? 0 : 1, ob3 = root(r.in[1 - k]);
            if (ob3 == o1 || producer[ob3] < 0 || producer[ob3] >= (int)li) continue;
            const GLayer& cl = g.layers[li];
            if (sw_variant(n->gd.convs[cl.conv].cin_pad, cl.has_act, fuse_pos[li] == 1 ? 1 : 2, k == 1 ? 1 : 2) < 0) continue;
            fuse_add2[li] = ri;
            fuse_pos2[li] = k;
            skip[ri] = 1;
        }
    }
    // A nearest-neighbour 2x Interp whose only reader is a 64 -> 64 convolution of g_conv3_sw is folded into that
    // convolution's row DMA (g_conv3_sw<..., UP>): the enlarged array is never written (models/4x_Valar_v1.param:1000-1003:
    // at 4x it is 16x the 1x plane).  UVA_GENERIC_FUSE_INTERP=0: the Interp as a launch of its own, the A/B switch.
    static const bool up_on = [] { const char* e = uva::debug_env("UVA_GENERIC_FUSE_INTERP"); return !e || std::atoi(e) != 0; }();
    std::vector<int> up_of(g.layers.size(), -1);
    if (up_on) {
        std::vector<int> producer(g.blobs.size(), -1);
        for (size_t li = 0; li < g.layers.size(); ++li)
            if (g.layers[li].kind != GLayer::SPLIT && !g.layers[li].out.empty()) producer[g.layers[li].out[0]] = (int)li;
        for (size_t li = 0; li < g.layers.size(); ++li) {
            const GLayer& cl = g.layers[li];
            if (!sw_cols_of(li) || fuse_add[li] >= 0 || cl.in.size() != 1) continue;
            if (sw_variant(n->gd.convs[cl.conv].cin_pad, cl.has_act, 0, 0) != 3) continue;
            const int ib = root(cl.in[0]), pi = producer[ib];
            if (pi < 0 || g.layers[pi].kind != GLayer::INTERP_NEAREST || g.layers[pi].factor != 2 || g.blobs[ib].consumers != 1) continue;
            if (group_of(ib) >= 0 || group_of(root(g.layers[pi].in[0])) >= 0 || ib == root(g.out_blob)) continue;
            up_of[li] = pi;
            skip[pi] = 1;
        }
    }
    // On the u8 route the graph's last convolution (3 output channels, no activation, no sum, g_conv3_lds) writes the frame's
    // bytes itself (GConvArgs::u8dst): no fp16 result array, no g_output_u8 launch.  UVA_GENERIC_FUSE_OUT=0: the A/B switch.
    static const bool out_on = [] { const char* e = uva::debug_env("UVA_GENERIC_FUSE_OUT"); return !e || std::atoi(e) != 0; }();
    int out_conv = -1;
    if (out_on && !f32 && n->generic_lds_conv) {
        for (size_t li = 0; li < g.layers.size(); ++li) {
            const GLayer& l = g.layers[li];
            if (l.kind != GLayer::CONV || l.out.empty() || root(l.out[0]) != root(g.out_blob)) continue;
            const GenericDevice::ConvDev& cd = n->gd.convs[l.conv];
            const GBlob& ob = g.blobs[l.out[0]];
            if (cd.wpk_lds && l.ksize == 3 && !l.has_act && fuse_add[li] < 0 && ob.channels == 3 && group_of(l.out[0]) < 0 && ob.scale == g.scale)
                out_conv = (int)li;
        }
    }
    // residual dense blocks whose first four convolutions run as one rdb4_kernel launch at the first one (UVA_GENERIC_RDB=0:
    // layer by layer, the A/B switch): the other six layers are bookkeeping only, and none of their sums is fused elsewhere
    static const bool rdb_on = [] { const char* e = uva::debug_env("UVA_GENERIC_RDB"); return !e || std::atoi(e) != 0; }();
    std::vector<int> rdb_at(g.layers.size(), -1);
    std::vector<char> rdb_skip(g.layers.size(), 0);
    if (rdb_on && use_groups && wmin >= 16) {
        for (size_t k = 0; k < n->gd.rdbs.size(); ++k) {
            const RdbMatch& m = n->gd.rdbs[k];
            rdb_at[m.c1] = (int)k;
            for (int li : {m.c2, m.c2s, m.add2, m.c3, m.c4, m.add4}) {
                rdb_skip[li] = 1;
                skip[li] = 0;
                fuse_add[li] = -1;
            }
        }
    }
    auto acquire_out = [&](PlaneState& ps, const GLayer& ly, GBuf* out) -> int {
        const GBlob& ob = g.blobs[ly.out[0]];
        GBuf o;
        if (group_of(ly.out[0]) >= 0) {
            GBuf& ga = ps.garr[ob.group];
            if (!ga.p && generic_acquire(n, ps.j.h * ob.scale, ps.j.w * ob.scale, g.group_channels[ob.group], &ga)) return 1;
            o = ga;                                   // same geometry and pixel stride (cpad) ...
            o.p = ga.p + ob.group_off;                // ... starting at the blob's first channel
            o.c = ob.channels;
        } else if (generic_acquire(n, ps.j.h * ob.scale, ps.j.w * ob.scale, ob.channels, &o)) return 1;
        ps.buf[ly.out[0]] = o;
        *out = o;
        return 0;
    };
    for (size_t layer_i = 0; layer_i < g.layers.size(); ++layer_i) {
        const GLayer& gl = g.layers[layer_i];
        if (gl.kind == GLayer::SPLIT || skip[layer_i]) continue;
        if (rdb_skip[layer_i]) {          // done by the rdb4 launch at the block's first convolution: buffers and counts only
            for (PlaneState& ps : P) {
                GBuf o;
                if (group_of(gl.out[0]) >= 0 && acquire_out(ps, gl, &o)) return 1;
                for (int b : gl.in) done_with(ps, b);
            }
            continue;
        }
        const GLayer* const sum = fuse_add[layer_i] >= 0 ? &g.layers[fuse_add[layer_i]] : nullptr;
        const GLayer* const sum2 = fuse_add2[layer_i] >= 0 ? &g.layers[fuse_add2[layer_i]] : nullptr;
        const GLayer* const up = gl.kind == GLayer::CONV && up_of[layer_i] >= 0 ? &g.layers[up_of[layer_i]] : nullptr;
        auto finish_layer = [&](PlaneState& ps) {
            if (up) done_with(ps, up->in[0]);          // (the Interp's own result was never made)
            else for (int b : gl.in) done_with(ps, b);
            if (sum) done_with(ps, sum->in[1 - fuse_pos[layer_i]]);
            if (sum2) done_with(ps, sum2->in[1 - fuse_pos2[layer_i]]);
        };
        // ---- the kernels that take all planes in one launch ----------------------------------------------------------
        if (gl.kind == GLayer::CONV && rdb_at[layer_i] >= 0) {
            const RdbMatch& m = n->gd.rdbs[rdb_at[layer_i]];
            auto cdev = [&](int li) -> const GenericDevice::ConvDev& { return n->gd.convs[g.layers[li].conv]; };
            RdbArgs ra;
            std::memset(&ra, 0, sizeof ra);
            std::vector<int> dims;
            for (int pi = 0; pi < np; ++pi) {
                GBuf o;
                if (acquire_out(P[pi], gl, &o)) return 1;
                const GBuf& arr = P[pi].garr[m.group];
                ra.arr[pi] = arr.p; ra.ph[pi] = arr.h; ra.pw[pi] = arr.w; ra.stride = arr.cpad;
                dims.push_back(arr.h); dims.push_back(arr.w);
            }
            GenericDevice::RdbPlan& plan = n->gd.rdb_plans[dims];
            if (!plan.segs) {
                std::vector<RdbSeg> segs;
                std::vector<int> sbeg;
                GenericDevice::RdbPlan fresh;
                fresh.grid = generic_grid(n);
                rdb_segments(dims, fresh.grid, segs, sbeg);
                if (upload(fresh.segs, segs.data(), segs.size() * sizeof(RdbSeg), n->stream)) return 1;
                if (upload(fresh.seg_begin, sbeg.data(), sbeg.size() * sizeof(int), n->stream)) return 1;
                HIP_TRY(hipStreamSynchronize(n->stream));
                plan = std::move(fresh);
            }
            ra.w1 = cdev(m.c1).wpk; ra.w2 = cdev(m.c2).wpk; ra.w2s = cdev(m.c2s).wpk; ra.w3 = cdev(m.c3).wpk; ra.w4 = cdev(m.c4).wpk;
            ra.b1 = cdev(m.c1).bias; ra.b2 = cdev(m.c2).bias; ra.b3 = cdev(m.c3).bias; ra.b4 = cdev(m.c4).bias;
            ra.slope = m.slope;
            ra.segs = plan.segs; ra.seg_begin = plan.seg_begin; ra.sink = n->d_sink;
#ifdef UVA_INSTRUMENT
            if (uva::debug_env("UVA_RDB_STAMPS")) {
                if (!n->gd.rdb_dbg) HIP_TRY(alloc_into(n->gd.rdb_dbg, 1024 * 16 * 8));
                HIP_TRY(hipMemsetAsync(n->gd.rdb_dbg, 0, 1024 * 16 * 8, n->stream));
                ra.dbg = n->gd.rdb_dbg;
            }
#endif
            if (!n->attr_set[28]) {
                HIP_TRY(hipFuncSetAttribute((const void*)rdb4_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
                n->attr_set[28] = true;
            }
            EvScope evp(n, 2, n->prof);
            HIP_TRY(evp.record(0));
            hipLaunchKernelGGL(rdb4_kernel, dim3(plan.grid), dim3(256), rdb4_lds_bytes(), n->stream, ra);
            ++n->glaunch[28];
            HIP_TRY(hipGetLastError());
            HIP_TRY(evp.last(1));
            for (PlaneState& ps : P) finish_layer(ps);
            continue;
        }
        if (gl.kind == GLayer::CONV && sw_cols_of(layer_i)) {
            const GenericDevice::ConvDev& cd = n->gd.convs[gl.conv];
            const int rm = !sum ? 0 : fuse_pos[layer_i] == 1 ? 1 : 2, rm2 = !sum2 ? 0 : fuse_pos2[layer_i] == 1 ? 1 : 2;
            const int variant = sw_variant(cd.cin_pad, gl.has_act, rm, rm2);
            if (variant >= 0) {
                const int cols = sw_cols_of(layer_i);
                GSwArgs sa;
                std::memset(&sa, 0, sizeof sa);
                std::vector<int> dims{cols};
                for (int pi = 0; pi < np; ++pi) {
                    PlaneState& ps = P[pi];
                    GBuf o;
                    if (acquire_out(ps, sum2 ? *sum2 : sum ? *sum : gl, &o)) return 1;
                    const GBuf& a = ps.buf[root(up ? up->in[0] : gl.in[0])];
                    sa.in[pi] = a.p; sa.out[pi] = o.p; sa.ph[pi] = o.h; sa.pw[pi] = o.w;
                    sa.in_stride = a.cpad; sa.out_stride = o.cpad;
                    if (sum) {
                        const GBuf& other = ps.buf[root(sum->in[1 - fuse_pos[layer_i]])];
                        sa.res[pi] = other.p; sa.res_stride = other.cpad;
                    }
                    if (sum2) {
                        const GBuf& other = ps.buf[root(sum2->in[1 - fuse_pos2[layer_i]])];
                        sa.res2[pi] = other.p; sa.res2_stride = other.cpad;
                    }
                    dims.push_back(o.h); dims.push_back(o.w);
                }
                GenericDevice::SwPlan& plan = n->gd.sw_plans[dims];
                if (!plan.segs) {
                    std::vector<GSwSeg> segs;
                    std::vector<int> sbeg;
                    GenericDevice::SwPlan fresh;
                    fresh.grid = generic_grid(n);
                    sw_segments(std::vector<int>(dims.begin() + 1, dims.end()), cols, fresh.grid, segs, sbeg);
                    if (upload(fresh.segs, segs.data(), segs.size() * sizeof(GSwSeg), n->stream)) return 1;
                    if (upload(fresh.seg_begin, sbeg.data(), sbeg.size() * sizeof(int), n->stream)) return 1;
                    HIP_TRY(hipStreamSynchronize(n->stream));       // (the vectors go away)
                    plan = std::move(fresh);
                }
                sa.wpk = cd.wpk; sa.bias = cd.bias; sa.out_coff = 0; sa.slope = gl.act_slope;
                if (sum) { sa.ca = sum->coeffs[0]; sa.cb = sum->coeffs[1]; }
                if (sum2) { sa.ca2 = sum2->coeffs[0]; sa.cb2 = sum2->coeffs[1]; }
                sa.segs = plan.segs; sa.seg_begin = plan.seg_begin; sa.sink = n->d_sink;
                auto launch_sw = [&](auto kern, int slot, size_t lds) -> int {
                    if (!n->attr_set[slot]) {
                        HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
                        n->attr_set[slot] = true;
                    }
                    EvScope evp(n, 2, n->prof && cd.cin_pad == 192);
                    HIP_TRY(evp.record(0));
                    hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(256), lds, n->stream, sa);
                    ++n->glaunch[slot];
                    HIP_TRY(evp.last(2));
                    return 0;
                };
                // 192 inputs: UVA_GENERIC_SK=1 takes g_conv3_sk (32x32x16 MFMAs, the k-loop split between wave pairs) instead of
                // g_conv3_sw<6, 1>.  Measured equal within 1 % (profiles/r03_ab_results.txt, block 10: both sit at the package's
                // power limit), so the simpler kernel stays the default; the other is kept runnable for the next round's work.
                static const bool sk_on = [] { const char* e = uva::debug_env("UVA_GENERIC_SK"); return e && std::atoi(e) != 0; }();
                // 192 inputs, round 6: g_conv3_sww -- the same convolution as 1-D Winograd F(2,3), two thirds of the MFMAs
                // (csrc/uva_sww.hip.h).  UVA_GENERIC_WINO=0: the direct kernels below, the A/B switch.
                static const bool wino_on = [] { const char* e = uva::debug_env("UVA_GENERIC_WINO"); return !e || std::atoi(e) != 0; }();
                if ((variant == 0 || variant == 1 || variant == 4) && wino_on && !sk_on && cd.wpk_w) {
                    sa.wpk = cd.wpk_w;
                    EvScope evp(n, 2, n->prof);
                    HIP_TRY(evp.record(0));
                    HIP_TRY(launch_conv3_sww(n->stream, plan.grid, sa, variant == 4 ? 0 : 2, variant == 1 ? 2 : 0));
                    ++n->glaunch[variant == 4 ? GL_SWW : variant == 0 ? GL_SWW_SUM : GL_SWW_SUM2];
                    HIP_TRY(evp.last(2));
                }
                else if (variant == 0 && sk_on) { if (launch_sw(g_conv3_sk<2, 0>, 32, sk_lds_bytes())) return 1; }
                else if (variant == 1 && sk_on) { if (launch_sw(g_conv3_sk<2, 2>, 33, sk_lds_bytes())) return 1; }
                else if (variant == 4 && sk_on) { if (launch_sw(g_conv3_sk<0, 0>, 34, sk_lds_bytes())) return 1; }
                else if (variant == 0) { if (launch_sw(g_conv3_sw<6, 1, false, 2, 0>, 24, sw_lds_bytes<6, 1>())) return 1; }
                else if (variant == 1) { if (launch_sw(g_conv3_sw<6, 1, false, 2, 2>, 25, sw_lds_bytes<6, 1>())) return 1; }
                else if (variant == 2) { if (launch_sw(g_conv3_sw<2, 2, false, 1, 0>, 26, sw_lds_bytes<2, 2>())) return 1; }
                else if (variant == 3 && up) { if (launch_sw(g_conv3_sw<2, 2, true, 0, 0, true>, 31, sw_lds_bytes<2, 2>())) return 1; }
                else if (variant == 3) { if (launch_sw(g_conv3_sw<2, 2, true, 0, 0>, 27, sw_lds_bytes<2, 2>())) return 1; }
                else if (variant == 4) { if (launch_sw(g_conv3_sw<6, 1, false, 0, 0>, 29, sw_lds_bytes<6, 1>())) return 1; }
                else { if (launch_sw(g_conv3_sw<2, 2, false, 0, 0>, 30, sw_lds_bytes<2, 2>())) return 1; }
                HIP_TRY(hipGetLastError());
                for (PlaneState& ps : P) finish_layer(ps);
                continue;
            }
        }
        // ---- everything else: one launch per plane ------------------------------------------------------------------------
        for (PlaneState& ps : P) {
        std::vector<GBuf>& buf = ps.buf;
        const int h = ps.j.h, w = ps.j.w;
        GBuf o;
        if (acquire_out(ps, sum2 ? *sum2 : sum ? *sum : gl, &o)) return 1;       // (a fused convolution writes the last sum's array, it has none of its own)
        auto in = [&](int k) -> const GBuf& { return buf[root(gl.in[k])]; };
        switch (gl.kind) {
        case GLayer::INPUT:
            ++n->glaunch[f32 ? GL_INPUT_F32 : GL_INPUT_U8];
            if (f32) hipLaunchKernelGGL(g_input_f32, dim3((w + T - 1) / T, h), dim3(T), 0, n->stream, (const float*)ps.j.src, h, w, o.p, o.cpad);
            else hipLaunchKernelGGL(g_input_u8, dim3((w + T - 1) / T, h), dim3(T), 0, n->stream, (const uint8_t*)ps.j.src, ps.j.src_stride, ps.j.sy0, ps.j.sx0, h, w, o.p, o.cpad);
            break;
        case GLayer::CONV: {
            const GenericDevice::ConvDev& cd = n->gd.convs[gl.conv];
            const GBuf& a = in(0);
            if ((group_of(gl.out[0]) >= 0 || group_of(root(gl.in[0])) >= 0) && !cd.wpk_lds)
                return fail("generic executor: a dense-chain convolution without the LDS kernel (plan_concat_groups and ensure_device disagree)");
            if (cd.wpk_lds && n->generic_lds_conv) {
                GConvArgs ga;
                std::memset(&ga, 0, sizeof ga);
                ga.in = a.p; ga.in_stride = a.cpad; ga.cin_pad = cd.cin_pad;
                ga.wpk = cd.wpk_lds; ga.bias = cd.bias;
                ga.out = o.p; ga.out_stride = o.cpad; ga.out_coff = 0; ga.cout = o.c;
                ga.h = a.h; ga.w = a.w;
                ga.has_act = gl.has_act ? 1 : 0; ga.slope = gl.act_slope;
                if (sum) {
                    const GBuf& other = buf[root(sum->in[1 - fuse_pos[layer_i]])];
                    ga.res = other.p; ga.res_stride = other.cpad; ga.res_first = fuse_pos[layer_i] == 1;
                    ga.ca = sum->coeffs[0]; ga.cb = sum->coeffs[1];
                }
                if ((int)layer_i == out_conv) {       // the frame's bytes leave from this convolution's epilogue (no g_output_u8)
                    const int s = g.scale;
                    ga.u8dst = (uint8_t*)ps.j.dst; ga.u8stride = ps.j.dst_stride;
                    ga.dy0 = ps.j.sy0 * s; ga.dx0 = ps.j.sx0 * s;
                    ga.cy0 = ps.j.cy0 * s; ga.cy1 = ps.j.cy1 * s; ga.cx0 = ps.j.cx0 * s; ga.cx1 = ps.j.cx1 * s;
                }
                const int mbn = cd.cout_pad / 16;
                // (UVA_GENERIC_WG=0: the 3x3 convolutions stage their weights through LDS again -- the A/B switch)
                static const int wg_max = [] { const char* e = uva::debug_env("UVA_GENERIC_WG"); return e ? std::atoi(e) : 4; }();
                const bool wg = gl.ksize == 3 && mbn <= wg_max && (mbn == 2 || mbn == 4);
                // 16-row tiles (8 waves) where the plane is tall enough to keep every CU busy with them
                static const int nw_max = [] { const char* e = uva::debug_env("UVA_GENERIC_NW"); return e ? std::atoi(e) : 4; }();
                const int nw = (wg && nw_max >= 8 && (long long)((a.w + GC_TW - 1) / GC_TW) * ((a.h + 15) / 16) >= 4LL * n->ncu) ? 8 : 4;
                const size_t lds = g_conv3_lds_bytes(cd.cin_pad, mbn, gl.ksize, wg, nw);
                const dim3 g3((a.w + GC_TW - 1) / GC_TW, (a.h + 2 * nw - 1) / (2 * nw));
                auto launch = [&](auto kern, int slot) -> int {
                    if (!n->attr_set[slot]) {
                        HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
                        n->attr_set[slot] = true;
                    }
                    hipLaunchKernelGGL(kern, g3, dim3(64 * nw), lds, n->stream, ga);
                    ++n->glaunch[slot];
                    return 0;
                };
                if (gl.ksize == 1) {
                    if (mbn == 1) { if (launch(g_conv3_lds<1, 1>, 16)) return 1; }
                    else if (mbn == 2) { if (launch(g_conv3_lds<2, 1>, 17)) return 1; }
                    else if (mbn == 3) { if (launch(g_conv3_lds<3, 1>, 18)) return 1; }
                    else { if (launch(g_conv3_lds<4, 1>, 19)) return 1; }
                }
                else if (wg && mbn == 2 && nw == 8) { if (launch(g_conv3_lds<2, 3, true, 8>, 23)) return 1; }
                else if (wg && mbn == 4 && nw == 8) { if (launch(g_conv3_lds<4, 3, true, 8>, 15)) return 1; }
                else if (wg && mbn == 2) { if (launch(g_conv3_lds<2, 3, true>, 21)) return 1; }
                else if (wg && mbn == 4) { if (launch(g_conv3_lds<4, 3, true>, 22)) return 1; }
                else if (mbn == 1) { if (launch(g_conv3_lds<1>, 11)) return 1; }
                else if (mbn == 2) { if (launch(g_conv3_lds<2>, 12)) return 1; }
                else if (mbn == 3) { if (launch(g_conv3_lds<3>, 13)) return 1; }
                else { if (launch(g_conv3_lds<4>, 14)) return 1; }
                break;
            }
            const dim3 grid((a.w + 63) / 64, (a.h + 3) / 4, (cd.cout_pad + 63) / 64);
            ++n->glaunch[gl.ksize == 3 ? GL_CONV3 : GL_CONV1];
            if (gl.ksize == 3)
                hipLaunchKernelGGL(g_conv<3>, grid, dim3(256), 0, n->stream, a.p, a.cpad, cd.wpk, cd.bias, o.p, o.c, cd.cout_pad, o.cpad, a.h, a.w, gl.has_act ? 1 : 0, gl.act_slope);
            else
                hipLaunchKernelGGL(g_conv<1>, grid, dim3(256), 0, n->stream, a.p, a.cpad, cd.wpk, cd.bias, o.p, o.c, cd.cout_pad, o.cpad, a.h, a.w, gl.has_act ? 1 : 0, gl.act_slope);
            break;
        }
        case GLayer::ADD:
        case GLayer::ELTWISE_SUM: {
            if (group_of(root(gl.in[0])) >= 0 || group_of(root(gl.in[1])) >= 0 || group_of(gl.out[0]) >= 0) {
                // an operand or the result is a channel range of a wider array (dense chain): per-pixel strides
                if (o.c % 8) return fail("generic executor: strided add needs a multiple of 8 channels");
                const size_t npix = (size_t)(o.h + 3) * (o.w + 2), work = npix * (o.c / 8);
                ++n->glaunch[GL_AXPBY_STRIDED];
                hipLaunchKernelGGL(g_axpby_strided, dim3((unsigned)((work + T - 1) / T)), dim3(T), 0, n->stream, in(0).p, in(0).cpad,
                                   gl.coeffs[0], in(1).p, in(1).cpad, gl.coeffs[1], o.p, o.cpad, o.c / 8, npix);
                break;
            }
            const size_t n8 = o.elems() / 8;
            ++n->glaunch[GL_AXPBY];
            hipLaunchKernelGGL(g_axpby, dim3((unsigned)((n8 + T - 1) / T)), dim3(T), 0, n->stream, (const half8*)in(0).p, gl.coeffs[0],
                               (const half8*)in(1).p, gl.coeffs[1], (half8*)o.p, n8);
            break;
        }
        case GLayer::CONCAT: {
            const size_t npix = (size_t)(o.h + 3) * (o.w + 2);
            int c_off = 0;
            const int mode = use_groups ? gl.concat_mode : 0;
            if (mode == 2) break;                     // every input already sits in its channel range of the shared array
            for (size_t k = 0; k < (mode == 1 ? 1 : gl.in.size()); ++k) {
                const GBuf& a = in((int)k);
                const size_t work = npix * (a.c / 8);
                ++n->glaunch[GL_CONCAT_PART];
                hipLaunchKernelGGL(g_concat_part, dim3((unsigned)((work + T - 1) / T)), dim3(T), 0, n->stream, a.p, a.cpad, a.c, o.p, o.cpad, c_off, npix);
                c_off += a.c;
            }
            break;
        }
        case GLayer::INTERP_NEAREST: {
            const GBuf& a = in(0);
            const size_t work = (size_t)o.h * o.w * (o.cpad / 8);
            ++n->glaunch[GL_INTERP];
            hipLaunchKernelGGL(g_interp_nearest, dim3((unsigned)((work + T - 1) / T)), dim3(T), 0, n->stream, a.p, a.h, a.w, a.cpad, o.p, gl.factor);
            break;
        }
        case GLayer::PRELU: {
            const size_t npix = (size_t)(o.h + 3) * (o.w + 2), work = npix * o.c;
            ++n->glaunch[GL_PRELU];
            hipLaunchKernelGGL(g_prelu, dim3((unsigned)((work + T - 1) / T)), dim3(T), 0, n->stream, in(0).p, n->gd.prelu[gl.slopes], o.p, o.c, o.cpad, npix);
            break;
        }
        case GLayer::PIXELSHUFFLE: {
            const GBuf& a = in(0);
            const size_t work = (size_t)o.h * o.w * o.c;
            ++n->glaunch[GL_PIXELSHUFFLE];
            hipLaunchKernelGGL(g_pixelshuffle, dim3((unsigned)((work + T - 1) / T)), dim3(T), 0, n->stream, a.p, a.h, a.w, a.cpad, o.p, o.c, o.cpad, gl.factor);
            break;
        }
        default: return fail("generic executor: unhandled layer kind");
        }
        HIP_TRY(hipGetLastError());
        finish_layer(ps);
        }
    }
    const int T2 = 256;
    for (PlaneState& ps : P) {
        const PlaneJob& j = ps.j;
        const GBuf& res = ps.buf[root(g.out_blob)];
        const int s = g.scale;
        if (f32) ++n->glaunch[GL_OUTPUT_F32];
        if (f32) hipLaunchKernelGGL(g_output_f32, dim3((j.w * s + T2 - 1) / T2, j.h * s), dim3(T2), 0, n->stream, res.p, j.h * s, j.w * s, res.cpad, (float*)j.dst);
        else if (out_conv >= 0) { /* written by the last convolution */ }
        else if (j.cx1 > j.cx0 && j.cy1 > j.cy0) {
            ++n->glaunch[GL_OUTPUT_U8];
            hipLaunchKernelGGL(g_output_u8, dim3(((j.cx1 - j.cx0) * s + T2 - 1) / T2, (j.cy1 - j.cy0) * s), dim3(T2), 0, n->stream, res.p, j.h * s, j.w * s, res.cpad,
                               (uint8_t*)j.dst, j.dst_stride, j.sy0 * s, j.sx0 * s, j.cy0 * s, j.cy1 * s, j.cx0 * s, j.cx1 * s);
        }
        HIP_TRY(hipGetLastError());
        done_with(ps, g.out_blob);
    }
    return 0;
}

// which planes of a frame go through the graph together: batch_of[i] = the batch of plane i, batches numbered in the order
// they run.  Planes of a batch are of one class (generic_plane_class), at most GEN_MAX_PLANES and `batch_pixels` input
// pixels (a single plane may exceed the bound: it is then a batch of its own).
void generic_plan_batches(const std::vector<PlaneDesc>& planes, bool batch_on, long long batch_pixels, std::vector<int>& batch_of)
{
    std::vector<int> cls, count;
    std::vector<long long> px;
    batch_of.clear();
    for (const PlaneDesc& p : planes) {
        const int c = generic_plane_class(p.w);
        const long long ppx = (long long)p.h * p.w;
        size_t k = 0;
        for (; batch_on && k < cls.size(); ++k)
            if (cls[k] == c && count[k] < GEN_MAX_PLANES && px[k] + ppx <= batch_pixels) break;
        if (!batch_on || k == cls.size()) { cls.push_back(c); count.push_back(0); px.push_back(0); k = cls.size() - 1; }
        ++count[k];
        px[k] += ppx;
        batch_of.push_back((int)k);
    }
}
// UVA_GENERIC_BATCH=0: one plane after the other (the A/B switch).  UVA_GENERIC_BATCH_PIXELS: a batch holds every array of
// its planes at once (at 4x, 16x the plane's pixels x 64 channels), so it is bounded to the planes of one 1080p frame
// (2.13 Mpixel) -- measured with 4x_Valar_v1 at 3840x2160 (12 planes), same bytes every way: this bound 0.343 s per frame
// and 33 GB in use, 4.2 Mpixel 0.345 s and 61 GB, all planes in one batch 0.338 s and 64 GB, one plane after the other
// 0.361 s and 33 GB
bool generic_batch_on() { static const bool on = [] { const char* e = uva::debug_env("UVA_GENERIC_BATCH"); return !e || std::atoi(e) != 0; }(); return on; }
long long generic_batch_pixels() { static const long long v = [] { const char* e = uva::debug_env("UVA_GENERIC_BATCH_PIXELS"); return e ? std::atoll(e) : 2200000ll; }(); return v; }

}  // namespace

int uva::generic_run_plane(uva_net* n, bool f32, const void* src, size_t src_stride, int sy0, int sx0, int h, int w, void* dst,
                           size_t dst_stride, int cy0, int cy1, int cx0, int cx1)
{
    return generic_run_planes(n, f32, std::vector<PlaneJob>{PlaneJob{src, src_stride, sy0, sx0, h, w, dst, dst_stride, cy0, cy1, cx0, cx1}});
}

// the u8 frame call for a generic graph: every reference tile (upscale_processing.py:499-516) is one plane; planes that
// take the same kernels go through the graph together
int uva::generic_process_u8_device(uva_net* n, const void* d_in, int h, int w, size_t in_stride, void* d_out, size_t out_stride,
                                   int tile_size, int border)
{
    std::vector<PlaneDesc> planes;
    normalize_tiling(tile_size, border);
    std::string err;
    if (build_planes(h, w, tile_size, border, planes, err)) return fail(err);
    std::vector<int> batch_of;
    generic_plan_batches(planes, generic_batch_on(), generic_batch_pixels(), batch_of);
    std::vector<std::vector<PlaneJob>> batches;
    for (size_t i = 0; i < planes.size(); ++i) {
        const PlaneDesc& p = planes[i];
        if ((size_t)batch_of[i] >= batches.size()) batches.resize(batch_of[i] + 1);
        batches[batch_of[i]].push_back(PlaneJob{d_in, in_stride, p.src_y0, p.src_x0, p.h, p.w, d_out, out_stride, p.core_y0,
                                                std::min(p.core_y1, p.h), p.core_x0, std::min(p.core_x1, p.w)});
    }
    for (const auto& b : batches)
        if (generic_run_planes(n, false, b)) return 1;
    return 0;
}

extern "C" {

int uva_net_debug_generic_plan(const uva_net* n, int* info)
{
    if (!n || !info) return fail("null argument");
    if (!n->generic || !n->gg.param_loaded) return fail("not a generic graph");
    const GenericGraph& g = n->gg;
    info[0] = (int)g.group_channels.size();
    info[1] = info[2] = info[3] = 0;
    for (const GLayer& l : g.layers)
        if (l.kind == GLayer::CONCAT) { info[1]++; info[2] += l.concat_mode == 2; info[3] += l.concat_mode == 1; }
    int lds = 0;
    for (const GLayer& l : g.layers)
        if (l.kind == GLayer::CONV && l.ksize == 3) {
            const ConvWeights& c = g.convs[l.conv];
            const int cin_pad = (c.cin + 31) / 32 * 32, cout_pad = (c.cout + 15) / 16 * 16;
            lds += cout_pad <= 64 && cin_pad <= 192 && g_conv3_lds_bytes(cin_pad, cout_pad / 16) <= 160 * 1024;
        }
    info[4] = lds;
    info[5] = 0;
    for (int c : g.group_channels) info[5] = std::max(info[5], c);
    info[6] = (int)find_rdbs(g).size();
    return 0;
}

int uva_net_debug_generic_launches(const uva_net* n, long long* counts, int capacity, int* count)
{
    if (!n || !count) return fail("null argument");
    if (!n->generic) return fail("not a generic graph");
    *count = GL_COUNT;
    if (!counts || capacity < GL_COUNT) return counts ? fail("uva_net_debug_generic_launches: capacity too small") : 0;
    std::memcpy(counts, n->glaunch, sizeof n->glaunch);
    return 0;
}

#ifdef UVA_INSTRUMENT
// debug: rdb4_kernel's in-kernel stamps of the last launch (UVA_RDB_STAMPS=1): out[(step * 4 + wave) * 4 + k]
int uva_net_debug_rdb_stamps(uva_net* n, unsigned long long* out, int max_steps)
{
    if (!n || !out || !n->gd.rdb_dbg) return fail("no rdb4 stamps (UVA_RDB_STAMPS=1, a generic graph, one call)");
    HIP_TRY(hipSetDevice(n->device));
    HIP_TRY(hipStreamSynchronize(n->stream));
    HIP_TRY(hipMemcpy(out, n->gd.rdb_dbg, (size_t)std::min(max_steps, 1024) * 16 * 8, hipMemcpyDeviceToHost));
    return 0;
}
#endif  // UVA_INSTRUMENT

int uva_debug_generic_segments_planes(int kind, const int* dims, int nplanes, int grid, int32_t* out, size_t capacity_words,
                                      size_t* needed_words, int* seg_begin)
{
    if (!dims || nplanes <= 0 || nplanes > GEN_MAX_PLANES || grid <= 0) return fail("bad argument");
    for (int i = 0; i < 2 * nplanes; ++i)
        if (dims[i] <= 0) return fail("bad argument");
    const std::vector<int> d(dims, dims + 2 * nplanes);
    std::vector<int32_t> words;
    std::vector<int> sbeg;
    if (kind == 0) {
        std::vector<RdbSeg> segs;
        rdb_segments(d, grid, segs, sbeg);
        for (const RdbSeg& sg : segs) words.insert(words.end(), {sg.c0, sg.yb, sg.ye, sg.own0, sg.own1, sg.plane, 0, 0});
    } else if (kind == 1 || kind == 2) {
        std::vector<GSwSeg> segs;
        const int cols = kind == 1 ? sw_cols<1>() : sw_cols<2>();
        sw_segments(d, cols, grid, segs, sbeg);
        for (const GSwSeg& sg : segs) words.insert(words.end(), {sg.c0, sg.y0, sg.y1, sg.c0, sg.c0 + cols, sg.plane, 0, 0});
    } else {
        return fail("bad kind");
    }
    if (needed_words) *needed_words = words.size();
    if (!out || capacity_words < words.size()) return fail("segment buffer too small");
    std::memcpy(out, words.data(), words.size() * sizeof(int32_t));
    if (seg_begin) std::copy(sbeg.begin(), sbeg.end(), seg_begin);
    return 0;
}

int uva_debug_generic_batches(int h, int w, int tile_size, int border, long long batch_pixels, int32_t* out, size_t capacity_words,
                              size_t* needed_words)
{
    if (h <= 0 || w <= 0) return fail("bad argument");
    std::vector<PlaneDesc> planes;
    normalize_tiling(tile_size, border);
    std::string err;
    if (build_planes(h, w, tile_size, border, planes, err)) return fail(err);
    std::vector<int> batch_of;
    generic_plan_batches(planes, true, batch_pixels > 0 ? batch_pixels : generic_batch_pixels(), batch_of);
    if (needed_words) *needed_words = planes.size() * 4;
    if (!out || capacity_words < planes.size() * 4) return fail("batch buffer too small");
    for (size_t i = 0; i < planes.size(); ++i) {
        out[4 * i] = planes[i].h; out[4 * i + 1] = planes[i].w; out[4 * i + 2] = batch_of[i]; out[4 * i + 3] = generic_plane_class(planes[i].w);
    }
    return 0;
}

int uva_debug_generic_segments(int kind, int h, int w, int grid, int32_t* out, size_t capacity_words, size_t* needed_words, int* seg_begin)
{
    const int dims[2] = {h, w};
    return uva_debug_generic_segments_planes(kind, dims, 1, grid, out, capacity_words, needed_words, seg_begin);
}

}  // extern "C"
