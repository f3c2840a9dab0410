// plan_check.cpp -- the frame planner (csrc/uva_plan.cpp) run alone, without HIP and without a GPU, so that it can be built
// with -fsanitize=address,undefined (tests/test_plan_sanitized.py).  Every builder runs over the cases of
// tools/plan_digests.py and over a seeded sweep of geometries; of each table only what the planner's own code states for
// certain is checked (the Python schedule tests check the meaning).  Prints one line of counts; the first violation ends
// the run with exit status 1.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../upscale_video_amd/csrc/uva_plan.h"

using namespace uva;

namespace {

struct Counts { long plans = 0, steps = 0, rows = 0, tiles = 0, unfit = 0, refused = 0; } counts;

[[noreturn]] void violation(const std::string& what, const std::string& where)
{
    std::fprintf(stderr, "plan_check: %s (%s)\n", what.c_str(), where.c_str());
    std::exit(1);
}

#define CHECK(cond, where) do { if (!(cond)) violation(#cond, where); } while (0)

unsigned long long offset40(const uint4& e) { return (unsigned long long)e.x | ((unsigned long long)(e.y & 0xffu) << 32); }

void check_steps(const char* kind, const std::string& where0, const FramePlan& plan, int grid, const std::vector<Trunk2Step>& steps,
                 const std::vector<int>& nsteps, int max_steps, int pad, bool wino)
{
    const std::string where = std::string(kind) + " " + where0;
    const int stride = max_steps + pad;
    const unsigned long long end = 2ull * plan.guard_bytes + (unsigned long long)plan.act_pixels * PLAN_PIXB;
    CHECK((int)nsteps.size() == grid && steps.size() == (size_t)grid * stride, where);
    for (int b = 0; b < grid; ++b) {
        CHECK(nsteps[b] >= 0 && nsteps[b] + pad <= stride, where);
        for (int g = 0; g < stride; ++g) {
            const Trunk2Step& s = steps[(size_t)b * stride + g];
            if ((s.a.y >> 24) & 1) {
                CHECK(offset40(s.a) < end, where);
                ++counts.steps;
            }
            if ((s.b.y >> 24) & 1) {
                CHECK(offset40(s.b) < end, where);
                const bool folded = wino && ((s.b.y >> 25) & 1);
                CHECK((folded ? s.b.z >> 24 : s.b.w) < plan.planes.size(), where);
            }
        }
    }
}

void check_rows(const char* kind, const std::string& where0, int rc, int h, int grid, int limit, const std::vector<uint4>& rows,
                const std::vector<int>& nrows, int max_rows)
{
    const std::string where = std::string(kind) + " " + where0;
    CHECK(rc == 0 || rc == 2, where);
    if (rc == 2) { ++counts.unfit; return; }
    CHECK(max_rows > 0 && max_rows <= limit, where);
    CHECK((int)nrows.size() == grid && rows.size() == (size_t)grid * max_rows, where);
    for (int b = 0; b < grid; ++b) {
        CHECK(nrows[b] >= 0 && nrows[b] <= max_rows, where);
        for (int g = 0; g < nrows[b]; ++g) {
            const uint4& r = rows[(size_t)b * max_rows + g];
            if (r.z & 1) CHECK((int)r.x >= 0 && (int)r.x < h, where);
            ++counts.rows;
        }
    }
}

// every builder refuses these grids with a message
void check_bad_grids(const FramePlan& plan, int h, int w)
{
    for (int grid : {4, 12, 0}) {
        const std::string where = "grid " + std::to_string(grid);
        std::vector<Trunk2Step> steps;
        std::vector<int> n;
        std::vector<uint4> rows;
        int m = 0;
        std::string err;
        CHECK(build_trunk2_schedule(plan.planes, grid, plan.guard_bytes, steps, n, &m, true, err) == 1 && !err.empty(), where);
        err.clear();
        CHECK(build_trunkw_schedule(plan.planes, grid, plan.guard_bytes, steps, n, &m, TrunkwOpts(), err) == 1 && !err.empty(), where);
        err.clear();
        CHECK(build_sub10_rows(h, w, 1, grid, rows, n, &m, err) == 1 && !err.empty(), where);
        err.clear();
        CHECK(build_sub5_rows(h, w, grid, rows, n, &m, err) == 1 && !err.empty(), where);
        err.clear();
        FramePlan whole;
        CHECK(plan_frame(h, w, 0, 0, 64, grid, PlanOpts(), whole, err) == 1 && !err.empty(), where);
        counts.refused += 5;
    }
}

void check_frame(int h, int w, int tile, int border, int grid, const PlanOpts& opts)
{
    const std::string where = std::to_string(h) + "x" + std::to_string(w) + " tile " + std::to_string(tile) + " border " + std::to_string(border) +
                              " grid " + std::to_string(grid) + " six " + std::to_string(opts.tw.six_mode) + " fold " +
                              std::to_string(opts.tw.fold ? opts.tw.fold_maxw : 0) + " narrow " + std::to_string((int)opts.narrow_ok);
    FramePlan plan;
    std::string err;
    if (plan_frame(h, w, tile, border, 64, grid, opts, plan, err)) violation("plan_frame refused: " + err, where);
    ++counts.plans;
    CHECK(!plan.planes.empty() && (int)plan.planes.size() <= MAX_PLANES && (int)plan.sched4.size() == plan.ntiles4, where);
    for (const uint4& e : plan.sched4) {
        CHECK(offset40(e) < (unsigned long long)plan.act_pixels * PLAN_PIXB && ((e.y >> 8) & 0xffu) < plan.planes.size(), where);
        ++counts.tiles;
    }
    check_steps("trunk2", where, plan, grid, plan.steps2, plan.nsteps2, plan.max_steps2, T2_PAD_STEPS, false);
    check_steps("trunkw", where, plan, grid, plan.stepsw, plan.nstepsw, plan.max_stepsw, TW_PAD_STEPS, true);
}

// frames > 0: sub10_kernel's list for that many frames; 0: sub5_kernel's
void check_sub(int h, int w, int frames, int grid)
{
    const std::string where = std::to_string(h) + "x" + std::to_string(w) + " frames " + std::to_string(frames) + " grid " + std::to_string(grid);
    std::vector<uint4> rows;
    std::vector<int> nrows;
    int max_rows = 0;
    std::string err;
    const int rc = frames ? build_sub10_rows(h, w, frames, grid, rows, nrows, &max_rows, err) : build_sub5_rows(h, w, grid, rows, nrows, &max_rows, err);
    check_rows(frames ? "sub10" : "sub5", where, rc, h, grid, frames ? S10_MAX_ROWS : S5_MAX_ROWS, rows, nrows, max_rows);
}

PlanOpts options(int six_mode, int fold)        // fold: 0 off, else the widest folded strip
{
    PlanOpts o;
    o.tw.six_mode = six_mode;
    o.tw.fold = fold != 0;
    if (fold) o.tw.fold_maxw = fold;
    return o;
}

}  // namespace

int main(int argc, char** argv)
{
    const int sweep = argc > 1 ? std::atoi(argv[1]) : 300;
    // the cases of tools/plan_digests.py
    const int trunk[][4] = {{1080, 1920, 960, 10}, {2160, 3840, 960, 10}, {1080, 1920, 0, 0}, {256, 256, 960, 10}, {24, 40, 0, 0},
                            {70, 75, 32, 10}, {5, 3, 0, 0}, {131, 61, 64, 10}, {1, 1, 0, 0}, {960, 960, 0, 0}, {96, 128, 64, 10},
                            {540, 960, 240, 10}, {33, 1000, 0, 0}, {1000, 9, 0, 0}};
    const int sub[][2] = {{1080, 1920}, {720, 1280}, {61, 59}, {1, 1}, {9, 1000}, {1000, 9}, {2160, 3840}};
    for (const auto& t : trunk)
        for (int grid : {8, 256})
            for (int six : {-1, 0, 1})
                for (int fold : {TW_FOLD_MAXW, 0, 14}) check_frame(t[0], t[1], t[2], t[3], grid, options(six, fold));
    for (const auto& s : sub)
        for (int grid : {8, 256}) {
            for (int frames : {1, 2, 4, 8, 0}) check_sub(s[0], s[1], frames, grid);
        }
    {
        FramePlan plan;
        std::string err;
        if (plan_frame(1080, 1920, 960, 10, 64, 256, PlanOpts(), plan, err)) violation("plan_frame refused: " + err, "1080x1920");
        check_bad_grids(plan, 1080, 1920);
        CHECK(plan_frame(4000, 4000, 32, 10, 64, 256, PlanOpts(), plan, err) == 1 && err == "frame needs more than 64 tiles", "4000x4000 tile 32");
    }
    // the sweep (raw engine output: the same geometries with every standard library)
    std::mt19937 rng(2029);
    auto below = [&](unsigned n) { return (int)(rng() % n); };
    const int tiles[] = {0, 32, 48, 64, 100, 240, 960}, grids[] = {8, 64, 256, 304};
    for (int i = 0; i < sweep; ++i) {
        const int h = 1 + below(1200), w = 1 + below(2000), grid = grids[below(4)];
        int tile = tiles[below(7)];
        if (tile && (long long)((h + tile - 1) / tile) * ((w + tile - 1) / tile) > MAX_PLANES) tile = 240;
        PlanOpts o = options(below(3) - 1, below(2) ? TW_FOLD_MAXW : 0);
        o.narrow_ok = below(4) != 0;
        check_frame(h, w, tile, tile ? 10 : 0, grid, o);
        check_sub(h, w, 1 + below(S10_MAXB), grid);
        check_sub(h, w, 0, grid);
    }
    std::printf("plan_check: %ld frame plans, %ld tile entries, %ld active steps, %ld rows, %ld unfit row lists, %ld refusals: ok\n",
                counts.plans, counts.tiles, counts.steps, counts.rows, counts.unfit, counts.refused);
    return 0;
}
