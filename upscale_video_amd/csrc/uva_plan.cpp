// uva_plan.cpp -- the host-side frame planner (uva_plan.h): pure arithmetic, no HIP calls.
#include "uva_plan.h"

#include <algorithm>
#include <cstring>

namespace uva {

static int refuse(std::string& err, const char* msg)
{
    err = msg;
    return 1;
}

static bool grid_ok(int grid, std::string& err)
{
    return (grid >= 8 && grid % 8 == 0) || !refuse(err, "schedule grid must be a multiple of 8, at least 8");
}

// Deals a sequence out into contiguous chunks of capacity `cap`, raising cap from cap0 until at most `grid` chunks come
// out; deal(cap, chunks) appends to chunks.back() and opens new chunks as it goes.  Returns the capacity that fit.
template <class Seg, class Deal>
static int deal_into_chunks(int grid, int cap0, std::vector<std::vector<Seg>>& chunks, Deal deal)
{
    for (int cap = cap0;; ++cap) {
        chunks.assign(1, {});
        deal(cap, chunks);
        while (!chunks.empty() && chunks.back().empty()) chunks.pop_back();
        if ((int)chunks.size() <= grid) return cap;
    }
}

// steps of the longest chunk
template <class Seg>
static int most_steps(const std::vector<std::vector<Seg>>& chunks)
{
    int most = 0;
    for (const auto& v : chunks) {
        int k = 0;
        for (const Seg& sg : v) k += sg.k;
        most = std::max(most, k);
    }
    return most;
}

// Plane list of one frame: the reference's tile grid (upscale_processing.py:398-434, :499-516)
// or a single whole-frame plane (apply_model, :263-288).
int build_planes(int h, int w, int tile_size, int border, std::vector<PlaneDesc>& out, std::string& err)
{
    out.clear();
    auto add = [&](int sy0, int sx0, int ph, int pw, int cy0, int cy1, int cx0, int cx1) {
        PlaneDesc p;
        std::memset(&p, 0, sizeof p);
        p.h = ph; p.w = pw;
        p.src_y0 = sy0; p.src_x0 = sx0;
        p.core_y0 = cy0; p.core_y1 = cy1; p.core_x0 = cx0; p.core_x1 = cx1;
        out.push_back(p);
    };
    if (tile_size <= 0) {
        add(0, 0, h, w, 0, h, 0, w);
    } else {
        const int tiles_x = (w + tile_size - 1) / tile_size, tiles_y = (h + tile_size - 1) / tile_size;
        if ((long long)tiles_x * tiles_y > MAX_PLANES) return refuse(err, "frame needs more than 64 tiles");
        for (int ty = 0; ty < tiles_y; ++ty)
            for (int tx = 0; tx < tiles_x; ++tx) {
                const int y0 = ty * tile_size, x0 = tx * tile_size;
                const int y1 = std::min(y0 + tile_size, h), x1 = std::min(x0 + tile_size, w);
                const int by0 = y0 >= border ? border : 0, by1 = y1 <= h - border ? border : 0;
                const int bx0 = x0 >= border ? border : 0, bx1 = x1 <= w - border ? border : 0;
                add(y0 - by0, x0 - bx0, (y1 + by1) - (y0 - by0), (x1 + bx1) - (x0 - bx0), by0, by0 + (y1 - y0),
                    bx0, bx0 + (x1 - x0));
            }
    }
    return 0;
}

// Work-tile counts, activation pitch and array offset of every plane (see PlaneDesc).
void layout_planes(PlaneLayout& l)
{
    l.act_pixels = 0;
    l.ntiles = l.ntiles4 = 0;
    for (auto& p : l.planes) {
        p.nty = (p.h + TH - 1) / TH;
        p.ntx = (p.w + TW - 1) / TW;
        p.pitch = p.ntx * TW + 2;
        p.tile_begin = l.ntiles;
        p.nty4 = (p.h + 3) / 4;
        p.tile_begin4 = l.ntiles4;
        p.act_off = (long long)l.act_pixels;
        l.ntiles += p.nty * p.ntx;
        l.ntiles4 += p.nty4 * p.ntx;
        l.act_pixels += (size_t)(p.nty * TH + 2) * p.pitch;
    }
}

size_t plan_guard_bytes(const std::vector<PlaneDesc>& planes, int nf)
{
    int max_pitch = 0;
    for (const auto& p : planes) max_pitch = std::max(max_pitch, p.pitch);
    return (size_t)8 * max_pitch * nf * 2;
}

// trunk_kernel's schedule: one entry per 4-row work tile, plane after plane, row-major
int build_sched4(const std::vector<PlaneDesc>& planes, std::vector<uint4>& sched4, std::string& err)
{
    sched4.clear();
    for (size_t pi = 0; pi < planes.size(); ++pi) {
        const PlaneDesc& p = planes[pi];
        if (p.nty4 >= 4096 || p.ntx >= 256) return refuse(err, "frame too large for the tile schedule encoding");
        for (int ty = 0; ty < p.nty4; ++ty)
            for (int tx = 0; tx < p.ntx; ++tx) {
                const unsigned long long off =
                    ((unsigned long long)p.act_off + (unsigned long long)(ty * 4) * p.pitch + (unsigned long long)tx * TW) * PLAN_PIXB;
                if (off >> 40) return refuse(err, "activation buffer too large for the tile schedule encoding");
                const int vy = std::min(4, p.h - ty * 4), vx = std::min(TW, p.w - tx * TW);
                sched4.push_back(make_uint4((unsigned)off, (unsigned)(off >> 32) | ((unsigned)pi << 8), (unsigned)(p.pitch * PLAN_PIXB),
                                            (unsigned)(vx | (vy << 6) | (tx << 9) | (ty << 17))));
            }
    }
    return 0;
}

// Step lists of trunk2_kernel for one frame geometry: every plane is cut into 30-column strips, a strip
// is a column of 4-row steps walked top to bottom, and the sequence (plane, strip, step) is dealt out to
// the workgroups in contiguous ranges of (nearly) equal length.  A range that ends inside a strip ends a
// SEGMENT there: k producer steps yield 4k - 2 output rows (the consumer needs one intermediate row below
// its last output row), the next segment starts on the following row and recomputes two intermediate rows.
int build_trunk2_schedule(const std::vector<PlaneDesc>& planes, int grid, size_t guard_bytes, std::vector<Trunk2Step>& steps,
                          std::vector<int>& nsteps, int* max_steps, bool narrow_ok, std::string& err)
{
    if (!grid_ok(grid, err)) return 1;
    constexpr int PIXB = PLAN_PIXB;
    struct Seg { int plane, x0, ya, rows, k; };
    // ranges of equal COST: a step of a narrow strip (<= 14 columns: one fragment column instead of two) runs its k-loops
    // with half the MFMAs and is counted as 8 tenths of a step (measured: its phases are then bounded by the other group's epilogue)
    constexpr int COST = 10, COST_NARROW = 8;
    auto step_cost = [&](const PlaneDesc& p, int x0) { return (narrow_ok && p.w - x0 <= 14) ? COST_NARROW : COST; };
    long long total = 0;
    for (const auto& p : planes)
        for (int x0 = 0; x0 < p.w; x0 += T2_SW) total += (long long)((p.h + 2 + 3) / 4) * step_cost(p, x0);
    std::vector<std::vector<Seg>> per_wg;
    deal_into_chunks(grid, (int)std::max<long long>(4 * COST, (total + grid - 1) / grid), per_wg, [&](int L, std::vector<std::vector<Seg>>& out) {
        int cap = L;
        auto next_wg = [&]() { out.emplace_back(); cap = L; };
        for (size_t pi = 0; pi < planes.size(); ++pi) {
            const PlaneDesc& p = planes[pi];
            for (int x0 = 0; x0 < p.w; x0 += T2_SW) {
                const int c = step_cost(p, x0);
                int y = 0;
                while (y < p.h) {
                    const int need = (p.h - y + 2 + 3) / 4, fit = cap / c;
                    if (need <= fit) {
                        out.back().push_back({(int)pi, x0, y, p.h - y, need});
                        cap -= need * c;
                        y = p.h;
                    } else if (fit < 2) {
                        next_wg();
                        continue;
                    } else {
                        out.back().push_back({(int)pi, x0, y, 4 * fit - 2, fit});
                        y += 4 * fit - 2;
                        cap = 0;
                    }
                    if (cap < COST_NARROW) next_wg();
                }
            }
        }
    });
    const int most = most_steps(per_wg);
    *max_steps = most;
    const int stride = most + T2_PAD_STEPS;
    steps.assign((size_t)grid * stride, Trunk2Step{make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)});
    nsteps.assign(grid, 0);
    for (size_t c = 0; c < per_wg.size(); ++c) {
        const int b = workgroup_of_chunk(c, grid);
        Trunk2Step* out = steps.data() + (size_t)b * stride;
        int g = 0;
        for (const Seg& sg : per_wg[c]) {
            const PlaneDesc& p = planes[sg.plane];
            const int nb = (sg.rows + 3) / 4;
            for (int j = 0; j < sg.k; ++j, ++g) {
                const int yA = sg.ya - 1 + 4 * j;                        // first intermediate row of the block
                // halo origin = input pixel (yA - 1, x0 - 2) = array position (yA, x0 - 1)
                const long long ao = (long long)guard_bytes +
                                     ((long long)p.act_off + (long long)yA * p.pitch + (sg.x0 - 1)) * PIXB;
                if (ao < 0 || (ao >> 40)) return refuse(err, "activation buffer too large for the step encoding");
                unsigned rmask = 0;
                for (int r = 0; r < 4; ++r)
                    if (yA + r >= 0 && yA + r < p.h) rmask |= 1u << r;
                const unsigned c_lo = sg.x0 == 0 ? 1 : 0, c_hi = (unsigned)std::min(32, p.w - sg.x0 + 1);
                // strips of at most 14 columns need only the first of the two 16-column fragment columns (bit 25, both halves)
                const unsigned narrow = (p.w - sg.x0 <= 14 && narrow_ok) ? 1u << 25 : 0u;
                out[g].a = make_uint4((unsigned)ao, (unsigned)(ao >> 32) | (rmask << 8) | (c_lo << 12) | (c_hi << 18) | (1u << 24) | narrow,
                                      (unsigned)(p.pitch * PIXB), (unsigned)sg.plane);
                if (j < nb) {
                    const int yo = sg.ya + 4 * j;
                    const long long bo = (long long)guard_bytes +
                                         ((long long)p.act_off + (long long)(yo + 1) * p.pitch + (sg.x0 + 1)) * PIXB;
                    const unsigned vy = (unsigned)std::min(4, sg.ya + sg.rows - yo), vx = (unsigned)std::min(T2_SW, p.w - sg.x0);
                    out[g].b = make_uint4((unsigned)bo, (unsigned)(bo >> 32) | (vy << 8) | (vx << 11) | (1u << 24) | narrow,
                                          (unsigned)(p.pitch * PIXB), (unsigned)sg.plane);
                }
            }
        }
        nsteps[b] = g;
        for (int k = 0; k < T2_PAD_STEPS; ++k) {      // harmless re-fetches of the last tile, nothing active
            out[g + k].a = out[g - 1].a;
            out[g + k].a.y &= 0xffu;
        }
    }
    return 0;
}

// Step lists of trunkw_kernel: the same 30-column strips and 4-row steps as trunk2_kernel's, but a segment that is not its
// workgroup's first starts WITHOUT the two input rows a step shares with the one above it: its first producer step yields
// two valid intermediate rows and its first consumer step nothing, so k steps yield 4 (k - 1) output rows and a segment
// of `rows` output rows beginning at row r0 has its first intermediate block at row r0 - 3 (a workgroup's first segment:
// r0 - 1, 4k - 2 rows -- the kernel's prologue fetches all six rows).  Step g of a segment:
//   producer: intermediate rows yA .. yA+3, yA = r0 - 3 (- 1) + 4g, from the new input rows yA+1 .. yA+4 (+ the two above);
//   consumer: output rows yA-1 .. yA+2, of which those inside the segment are stored, from the last two rows of block g-1
//             and block g.
int build_trunkw_schedule(const std::vector<PlaneDesc>& planes, int grid, size_t guard_bytes, std::vector<Trunk2Step>& steps,
                          std::vector<int>& nsteps, int* max_steps, const TrunkwOpts& opts, std::string& err)
{
    if (!grid_ok(grid, err)) return 1;
    constexpr int PIXB = PLAN_PIXB;
    // A workgroup's FIRST segment can start with the two input rows a step shares with the one above it (the kernel's prologue
    // fetches and transforms them: entry bit 25) and then yields 4k - 2 rows in k steps instead of 4 (k - 1).  The prologue is
    // 0.3 % of a launch (measured), so this is done only where it shortens the LONGEST list (opts.six_mode: 1 always, 0 never):
    // a whole 1080p frame 69 -> 68 steps (+0.5 %), the reference tiling 73 -> 73 (left alone).  Also measured and not kept
    // (profiles/r04_ab_results.txt block 20): segments at the TOP of a plane starting on two zero rows written by the consumers
    // -- with the six-row starts 73 -> 72 steps at the reference tiling, and the same launch time: a segment's fill step, in
    // which the consumers idle, costs about half a step.
    //
    // FOLDED last strips (round 5).  A strip costs its 16 MFMA pair columns whatever its width, and 970 columns (the reference
    // tiling's planes at 1080p) are 32 strips and a THIRD of one: 2 % of a launch's steps compute nothing.  Where two planes have
    // the same size and a last strip of at most TW_FOLD_MAXW = 12 columns, ONE strip walk does both: lanes with pair index 0..7
    // work on the first plane, 8..15 on the second.  Why 12 and not 14: v output columns need the intermediate columns -1..v,
    // i.e. the producers' pairs 0..(v + 1) / 2, and producer pair p reads raw columns 2p..2p+3 -- for v = 13, 14 that is pair 7
    // and raw columns 16, 17, which in a folded step hold the SECOND plane's first pixels (the first version allowed 14: one
    // wrong column per 74-wide plane, 1.4 dB on the 128x96 probe, inside every parity bar -- found by the probe's PSNR moving,
    // now pinned by a byte-for-byte fold on / off test).  Everything in between (rings,
    // transforms, k-loops) is pair-wise and does not care; what differs is where the raw rows come from and where the results
    // go: the second plane's addresses = the first's + a constant (entry .w = that constant - 2048, flags a.y bit 27 / b.y
    // bit 25; csrc/uva_wino.hip.h).  opts.fold = false: off.
    // opts.fold_maxw = 14 (debug opt-in only) is that first version, kept as the known-bad schedule the tests' structured-error
    // detector must catch (tests/test_gpu_parity.py::test_structure_detector_catches_the_fold14_schedule).
    std::vector<int> fold_partner(planes.size(), -1);
    std::vector<char> folded_away(planes.size(), 0);
    auto last_x0 = [](const PlaneDesc& p) { return ((p.w + TW_SW - 1) / TW_SW - 1) * TW_SW; };
    if (opts.fold)
        for (size_t i = 0; i < planes.size(); ++i) {
            if (fold_partner[i] >= 0 || folded_away[i] || planes[i].w - last_x0(planes[i]) > opts.fold_maxw) continue;
            for (size_t j = i + 1; j < planes.size(); ++j) {
                if (fold_partner[j] >= 0 || folded_away[j]) continue;
                const long long delta = ((long long)planes[j].act_off - (long long)planes[i].act_off) * PIXB;
                if (planes[j].h == planes[i].h && planes[j].w == planes[i].w && planes[j].pitch == planes[i].pitch && delta > 2048 && delta < (1ll << 31)) {
                    fold_partner[i] = (int)j;
                    folded_away[j] = 1;
                    break;
                }
            }
        }
    struct Seg { int plane, x0, r0, rows, k; bool full; int fold; };
    long long total = 0;
    for (const auto& p : planes) total += (long long)((p.w + TW_SW - 1) / TW_SW) * ((p.h + 3) / 4 + 1);     // (an upper bound: full segments need less)
    auto pack = [&](bool six_ok, std::vector<std::vector<Seg>>& per_wg) {
        deal_into_chunks(grid, (int)std::max<long long>(4, (total + grid - 1) / grid - 2), per_wg, [&](int L, std::vector<std::vector<Seg>>& out) {
            int cap = L;
            auto next_wg = [&]() { out.emplace_back(); cap = L; };
            for (size_t pi = 0; pi < planes.size(); ++pi) {
                const PlaneDesc& p = planes[pi];
                for (int x0 = 0; x0 < p.w; x0 += TW_SW) {
                    const bool last = x0 + TW_SW >= p.w;
                    if (last && folded_away[pi]) continue;          // done by its partner's last strip
                    const int fold = last ? fold_partner[pi] : -1;
                    int y = 0;
                    while (y < p.h) {
                        const bool full = six_ok && out.back().empty() && fold < 0;     // (the prologue's six-row fetch knows one plane)
                        const int need = full ? (p.h - y + 2 + 3) / 4 : (p.h - y + 3) / 4 + 1;
                        if (need <= cap) {
                            out.back().push_back({(int)pi, x0, y, p.h - y, need, full, fold});
                            cap -= need;
                            y = p.h;
                        } else if (cap < 3) {             // a segment of fewer than 3 steps is mostly pipeline fill
                            next_wg();
                            continue;
                        } else {
                            const int rows = full ? 4 * cap - 2 : 4 * (cap - 1);
                            out.back().push_back({(int)pi, x0, y, rows, cap, full, fold});
                            y += rows;
                            cap = 0;
                        }
                        if (cap < 1) next_wg();
                    }
                }
            }
        });
        return most_steps(per_wg);
    };
    std::vector<std::vector<Seg>> per_wg;
    int most;
    if (opts.six_mode >= 0) most = pack(opts.six_mode != 0, per_wg);
    else {
        std::vector<std::vector<Seg>> with_six;
        most = pack(false, per_wg);
        const int m1 = pack(true, with_six);
        if (m1 < most) { per_wg.swap(with_six); most = m1; }
    }
    *max_steps = most;
    const int stride = most + TW_PAD_STEPS;
    steps.assign((size_t)grid * stride, Trunk2Step{make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)});
    nsteps.assign(grid, 0);
    for (size_t c = 0; c < per_wg.size(); ++c) {
        const int b = workgroup_of_chunk(c, grid);
        Trunk2Step* out = steps.data() + (size_t)b * stride;
        int g = 0;
        for (const Seg& sg : per_wg[c]) {
            const PlaneDesc& p = planes[sg.plane];
            for (int j = 0; j < sg.k; ++j, ++g) {
                const int yA = sg.r0 - (sg.full ? 1 : 3) + 4 * j;        // first intermediate row of the block
                // first new input row = pixel (yA + 1, x0 - 2) = array position (yA + 2, x0 - 1)
                const long long ao = (long long)guard_bytes +
                                     ((long long)p.act_off + (long long)(yA + 2) * p.pitch + (sg.x0 - 1)) * PIXB;
                if (ao < 0 || (ao >> 40)) return refuse(err, "activation buffer too large for the step encoding");
                unsigned rmask = 0;
                for (int r = 0; r < 4; ++r)
                    if (yA + r >= 0 && yA + r < p.h) rmask |= 1u << r;
                const unsigned c_lo = sg.x0 == 0 ? 1 : 0, c_hi = (unsigned)std::min(32, p.w - sg.x0 + 1);
                // (a folded step carries its first plane's index in .z's top byte: the debug view's, the kernel masks it off)
                if (sg.fold >= 0 && sg.plane > 255) return refuse(err, "trunkw schedule: more than 256 planes with folded strips");
                // a folded step: the second plane's pixels lie fold_add + 2048 bytes behind the first's
                const unsigned fold_add = sg.fold >= 0 ? (unsigned)(((long long)planes[sg.fold].act_off - (long long)p.act_off) * PIXB - 2048) : 0u;
                // (folded: .w is taken, the plane index rides in .z's top byte)
                const unsigned z = (unsigned)(p.pitch * PIXB) | (sg.fold >= 0 ? (unsigned)sg.plane << 24 : 0u), w = sg.fold >= 0 ? fold_add : (unsigned)sg.plane;
                out[g].a = make_uint4((unsigned)ao, (unsigned)(ao >> 32) | (rmask << 8) | (c_lo << 12) | (c_hi << 18) | (1u << 24) |
                                                    ((sg.full && j == 0) ? 1u << 25 : 0u) | (sg.fold >= 0 ? 1u << 27 : 0u), z, w);
                if ((unsigned)(p.pitch * PIXB) >> 24) return refuse(err, "plane too wide for the step encoding");
                // the consumer step stores rows yo + [v0, v1) of its four (yo = yA - 1): those inside the segment
                const int yo = yA - 1;
                const int v0 = std::max(0, sg.r0 - yo), v1 = std::min(4, sg.r0 + sg.rows - yo);
                if (v1 > v0) {
                    const long long bo = (long long)guard_bytes +
                                         ((long long)p.act_off + (long long)(yo + 1) * p.pitch + (sg.x0 + 1)) * PIXB;
                    if (bo < 0 || (bo >> 40)) return refuse(err, "activation buffer too large for the step encoding");
                    const unsigned vx = (unsigned)std::min(TW_SW, p.w - sg.x0);
                    out[g].b = make_uint4((unsigned)bo, (unsigned)(bo >> 32) | ((unsigned)v1 << 8) | (vx << 11) | ((unsigned)v0 << 17) | (1u << 24) |
                                                        (sg.fold >= 0 ? 1u << 25 : 0u), z, w);
                }
            }
        }
        nsteps[b] = g;
        for (int k = 0; k < TW_PAD_STEPS && g > 0; ++k) {     // harmless re-fetches of the last rows, nothing active
            out[g + k].a = out[g - 1].a;
            out[g + k].a.y &= 0xffu;
        }
    }
    return 0;
}

// The sequence (frame, strip unit, row) is dealt out to the workgroups in contiguous ranges; every range (segment) starts
// nl rows early and ends nl rows late (the rows the layers in between need), only its own rows are written out.
int build_strip_rows(const StripRowsSpec& s, int h, int grid, std::vector<uint4>& rows, std::vector<int>& nrows, int* max_rows,
                     std::string& err)
{
    if (!grid_ok(grid, err)) return 1;
    const int ns = s.units_per_frame * s.frames;             // k = frame * units_per_frame + unit
    const long long total = (long long)ns * h;
    struct Seg { int k, y0, n; };
    std::vector<std::vector<Seg>> per_wg;
    const int D = deal_into_chunks(grid, (int)std::max<long long>(2 * s.nl + 4, (total + grid - 1) / grid + 2 * s.nl), per_wg,
                                   [&](int cap0, std::vector<std::vector<Seg>>& out) {
        int cap = cap0;
        for (int k = 0; k < ns; ++k) {
            int y = 0;
            while (y < h) {
                if (cap < 2 * s.nl + 1) { out.emplace_back(); cap = cap0; }
                const int n = std::min(h - y, cap - 2 * s.nl);
                out.back().push_back({k, y, n});
                cap -= n + 2 * s.nl;
                y += n;
            }
        }
    });
    if (D > s.max_rows) return 2;        // the row table does not fit the kernel's LDS copy: the caller takes another path
    *max_rows = D;
    rows.assign((size_t)grid * D, make_uint4(0, 0, 0, 0));
    nrows.assign(grid, 0);
    for (size_t c = 0; c < per_wg.size(); ++c) {
        const int b = workgroup_of_chunk(c, grid);
        uint4* out = rows.data() + (size_t)b * D;
        int g = 0;
        for (const Seg& sg : per_wg[c])
            for (int y = sg.y0 - s.nl; y < sg.y0 + sg.n + s.nl; ++y, ++g) {
                // dist = how many rows y lies outside the segment's own rows (0 inside, 1..nl): sub10's layer i (0 = the first) is
                // needed on rows with dist <= 9 - i only, and the kernel's wave of that layer skips the others
                const int dist = y < sg.y0 ? sg.y0 - y : y >= sg.y0 + sg.n ? y - (sg.y0 + sg.n - 1) : 0;
                out[g] = make_uint4((unsigned)y, (unsigned)((sg.k % s.units_per_frame) * s.unit_w - s.nl),
                                    (dist == 0 ? 1u : 0u) | ((unsigned)(sg.k / s.units_per_frame) << 8), s.dist_in_w ? (unsigned)dist : 0u);
            }
        nrows[b] = g;
    }
    return 0;
}

// Row descriptors of sub10_kernel for `frames` h x w frames in one launch: 60-column strips, 10 warm-up rows either side.
int build_sub10_rows(int h, int w, int frames, int grid, std::vector<uint4>& rows, std::vector<int>& nrows, int* max_rows, std::string& err)
{
    if (!grid_ok(grid, err)) return 1;
    if (frames < 1 || frames > S10_MAXB || h > S10_MAX_H) return 2;
    return build_strip_rows({S10_VALID, (w + S10_VALID - 1) / S10_VALID, frames, S10_NL, S10_MAX_ROWS, true}, h, grid, rows, nrows, max_rows, err);
}

// Row descriptors of sub5_kernel (both launches use the same lists): PAIRS of 54-column strips, 5 warm-up rows either side;
// a word's column is that of the pair's FIRST strip (the second one's is S5_VALID further right).
int build_sub5_rows(int h, int w, int grid, std::vector<uint4>& rows, std::vector<int>& nrows, int* max_rows, std::string& err)
{
    return build_strip_rows({S5_PAIRW, (w + S5_PAIRW - 1) / S5_PAIRW, 1, S5_NL, S5_MAX_ROWS, false}, h, grid, rows, nrows, max_rows, err);
}

int plan_frame(int h, int w, int tile_size, int border, int nf, int grid, const PlanOpts& opts, FramePlan& plan, std::string& err)
{
    normalize_tiling(tile_size, border);
    if (build_planes(h, w, tile_size, border, plan.planes, err)) return 1;
    layout_planes(plan);
    plan.guard_bytes = plan_guard_bytes(plan.planes, nf);
    if (nf != 64) return 0;
    if (build_sched4(plan.planes, plan.sched4, err)) return 1;
    if (build_trunk2_schedule(plan.planes, grid, plan.guard_bytes, plan.steps2, plan.nsteps2, &plan.max_steps2, opts.narrow_ok, err)) return 1;
    return build_trunkw_schedule(plan.planes, grid, plan.guard_bytes, plan.stepsw, plan.nstepsw, &plan.max_stepsw, opts.tw, err);
}

}  // namespace uva
