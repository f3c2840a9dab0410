// submit_check.cpp -- the pipelined host route's plan (csrc/uva_submit.cpp, with csrc/uva_crop_host.cpp for the window's planes)
// run alone, without HIP and without a GPU (tests/test_submit_plan.py), so that it can also be built with
// -fsanitize=address,undefined (tests/test_submit_sanitized.py).  Known answers worked out by hand from the frame layouts of
// csrc/uva_pixfmt.h, then a seeded sweep that holds every plan to the relations between its members.  Prints one line of
// counts; the first violation ends the run with exit status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

#include "../../upscale_video_amd/csrc/uva_submit.h"

using namespace uva;

namespace {

struct Counts { long plans = 0, windows = 0, sized = 0, refused = 0; } counts;

[[noreturn]] void violation(const std::string& what, const std::string& where)
{
    std::fprintf(stderr, "submit_check: %s (%s)\n", what.c_str(), where.c_str());
    std::exit(1);
}

#define CHECK(cond, where) do { if (!(cond)) violation(#cond, where); } while (0)

const char* const REFUSALS[] = {
    "row stride too small",
    "result frame of 2 GB or more",
    "unknown pixel format",
    "input window: bad size of the source frame",
    "input window: bad image size",
    "input window: the window leaves the frame",
    "input window: x and the width must be even for a Y'CbCr format (chroma pairs are not split)",
    "input window: y and the height must be even for a 4:2:0 format (chroma rows are not split)",
};

bool known_refusal(const char* e)
{
    for (const char* r : REFUSALS)
        if (!std::strcmp(e, r)) return true;
    return false;
}

// a pixel-format call as the entries fill it: dense BGR rows on both sides (sized: the result oh x ow)
SubmitSpec spec(int bits, int in_fmt, int out_fmt, int h, int w, int scale, int oh = 0, int ow = 0)
{
    const size_t bps = bits / 8;
    SubmitSpec sp;
    sp.h = h; sp.w = w;
    sp.in_stride = (size_t)w * 3 * bps;
    sp.out_stride = (size_t)(ow ? ow : w * scale) * 3 * bps;
    sp.in_fmt = in_fmt; sp.out_fmt = out_fmt;
    sp.bits = bits;
    sp.rs_oh = oh; sp.rs_ow = ow;
    sp.may_skip = sp.windowed = true;
    return sp;
}

void known_answers()
{
    SubmitPlan p;
    {   // 5 rows of 7 BGR pixels, twice the size out
        const char* where = "bgr24 -> bgr24 5x7 x2";
        CHECK(submit_plan(spec(8, PIX_BGR24, PIX_BGR24, 5, 7, 2), 2, nullptr, &p) == nullptr, where);
        CHECK(p.in_row == 21 && p.out_row == 42 && p.in_bytes == 105 && p.out_bytes == 420, where);
        CHECK(!p.pin && !p.pout && !p.rs && !p.win && p.dl_bytes == 420, where);
        CHECK(p.h2d_rows == 5 && p.h2d_row == 21 && p.h_in_bytes == 105, where);
        CHECK(p.dl_rows == 10 && p.dl_row == 42 && p.dl_user_stride == 42, where);
    }
    {   // yuv420p: 35 luma + 2 planes of 3 x 4 chroma; nv12 at 10 x 14: 140 luma + 5 rows of 7 pairs
        const char* where = "yuv420p -> nv12 5x7 x2";
        CHECK(submit_plan(spec(8, PIX_YUV420P, PIX_NV12, 5, 7, 2), 2, nullptr, &p) == nullptr, where);
        CHECK(p.pin && p.pout && p.pin_bytes == 59 && p.pout_bytes == 210 && p.dl_bytes == 210, where);
        CHECK(p.h2d_rows == 1 && p.h2d_row == 59 && p.h_in_bytes == 59 && p.packed_bytes == 59, where);
        CHECK(p.dl_rows == 210 && p.dl_row == 1 && p.dl_user_stride == 1, where);
        CHECK(p.in_bytes == 105 && p.out_bytes == 420, where);        // (the net still works on BGR)
    }
    {   // 16 bits: 4 rows of 6 pixels, four times the size, resampled to 10 x 20; p010le: (24 luma + 2 rows of 3 pairs) words
        const char* where = "p010le -> bgr48le 4x6 x4 sized 10x20";
        CHECK(submit_plan(spec(16, PIX_P010LE, PIX_BGR48LE, 4, 6, 4, 10, 20), 4, nullptr, &p) == nullptr, where);
        CHECK(p.bps == 2 && p.in_row == 36 && p.out_row == 144 && p.out_bytes == 2304, where);
        CHECK(p.rs && p.res_h == 10 && p.res_w == 20 && p.res_row == 120 && p.res_bytes == 1200, where);
        CHECK(p.pin && p.pin_bytes == 72 && !p.pout && p.dl_bytes == 1200, where);
        CHECK(p.key.res_h == 10 && p.key.res_w == 20 && p.key.u16 == 1, where);
        where = "p010le -> bgr48le 4x6 x4 sized 16x24";               // the net's own size: nothing to resample
        CHECK(submit_plan(spec(16, PIX_P010LE, PIX_BGR48LE, 4, 6, 4, 16, 24), 4, nullptr, &p) == nullptr, where);
        CHECK(!p.rs && p.res_h == 16 && p.res_w == 24 && p.dl_bytes == 2304, where);
    }
    {   // strides: a padded pair is taken, a short one is not; the PNG route has no output rows at the caller's
        const char* where = "strides";
        SubmitSpec sp = spec(8, PIX_BGR24, PIX_BGR24, 5, 7, 2);
        sp.in_stride = 32; sp.out_stride = 64;
        CHECK(submit_plan(sp, 2, nullptr, &p) == nullptr && p.in_stride == 32 && p.out_stride == 64 && p.dl_user_stride == 64, where);
        CHECK(p.in_bytes == 105 && p.dl_bytes == 420, where);
        sp.in_stride = 20;
        CHECK(!std::strcmp(submit_plan(sp, 2, nullptr, &p), "row stride too small") && !p.window_refused, where);
        sp.in_stride = 21; sp.out_stride = 41;
        CHECK(!std::strcmp(submit_plan(sp, 2, nullptr, &p), "row stride too small"), where);
        int ws = 0;
        sp.png_ws = &ws; sp.out_stride = 0;
        CHECK(submit_plan(sp, 2, nullptr, &p) == nullptr && p.out_stride == 42, where);
        counts.refused += 2;
    }
    {   // 65536 x 65536 nv12 is 6 GB; the same frame in BGR is not the packed frame's business
        const char* where = "2 GB";
        CHECK(!std::strcmp(submit_plan(spec(8, PIX_BGR24, PIX_NV12, 16384, 16384, 4), 4, nullptr, &p), "result frame of 2 GB or more"), where);
        CHECK(submit_plan(spec(8, PIX_BGR24, PIX_NV12, 16384, 16384, 1), 1, nullptr, &p) == nullptr && p.pout_bytes == 402653184u, where);
        ++counts.refused;
    }
    {   // a window of a BGR frame is the frame at an offset: 4 x 6 at (x 3, y 2) of 9 x 11
        const char* where = "bgr24 window";
        const SubmitWindow win = {9, 11, 3, 2};
        CHECK(submit_plan(spec(8, PIX_BGR24, PIX_BGR24, 4, 6, 2), 2, &win, &p) == nullptr, where);
        CHECK(p.win && !p.win_rows && !p.win_cols && p.in_offset == 2 * 33 + 9 && p.in_stride == 33 && p.in_bytes == 72, where);
        // ... of a yuv420p frame 8 x 12, rows 2 .. 5 at full width: row ranges; columns 4 .. 9: through the staging
        const SubmitWindow rows = {8, 12, 0, 2}, cols = {8, 12, 4, 2};
        CHECK(submit_plan(spec(8, PIX_YUV420P, PIX_YUV420P, 4, 12, 2), 2, &rows, &p) == nullptr, where);
        CHECK(p.win_rows && !p.win_cols && p.wn == 3 && p.in_offset == 0 && p.h_in_bytes == 72 && p.pin_bytes == 72, where);
        CHECK(p.wpl[1].src_off == 96 && p.wpl[1].row0 == 1 && p.wpl[1].rows == 2 && p.wpl[1].dst_off == 48 && p.wpl[2].dst_off == 60, where);
        CHECK(submit_plan(spec(8, PIX_YUV420P, PIX_YUV420P, 4, 6, 2), 2, &cols, &p) == nullptr, where);
        // (staging: 4 rows of 12, then 2 rows of 6 twice, each plane from a multiple of 16)
        CHECK(p.win_cols && p.wstage[0] == 0 && p.wstage[1] == 48 && p.wstage[2] == 64 && p.wstage_bytes == 80 && p.h_in_bytes == 80, where);
        const SubmitWindow odd = {8, 12, 3, 2};
        CHECK(known_refusal(submit_plan(spec(8, PIX_YUV420P, PIX_YUV420P, 4, 6, 2), 2, &odd, &p)) && p.window_refused, where);
        ++counts.refused;
    }
}

bool same_sizes(const SubmitPlan& a, const SubmitPlan& b)
{
    return a.bps == b.bps && a.in_row == b.in_row && a.out_row == b.out_row && a.in_bytes == b.in_bytes && a.out_bytes == b.out_bytes &&
           a.out_h == b.out_h && a.out_w == b.out_w && a.native == b.native && a.rs == b.rs && a.res_h == b.res_h && a.res_w == b.res_w &&
           a.res_row == b.res_row && a.res_bytes == b.res_bytes && a.pin == b.pin && a.pout == b.pout && a.pin_bytes == b.pin_bytes &&
           a.pout_bytes == b.pout_bytes && !a.win_cols && !b.win_cols && a.wstage_bytes == 0 && b.wstage_bytes == 0 &&
           a.in_offset == b.in_offset && a.in_stride == b.in_stride && a.out_stride == b.out_stride && a.h2d_row == b.h2d_row &&
           a.h2d_rows == b.h2d_rows && a.packed_bytes == b.packed_bytes && a.h_in_bytes == b.h_in_bytes && a.dl_bytes == b.dl_bytes &&
           a.dl_row == b.dl_row && a.dl_rows == b.dl_rows && a.dl_user_stride == b.dl_user_stride && a.key == b.key;
}

void check_plan(const SubmitSpec& sp, int scale, const SubmitWindow* win, const std::string& where)
{
    SubmitPlan p;
    const char* e = submit_plan(sp, scale, win, &p);
    if (e) {
        CHECK(known_refusal(e), where + ": " + e);
        CHECK(!p.window_refused || win, where);
        ++counts.refused;
        return;
    }
    ++counts.plans;
    const size_t bps = sp.bits / 8;
    const int native = sp.bits == 16 ? PIX_BGR48LE : PIX_BGR24;
    CHECK(p.bps == bps && p.native == native, where);
    CHECK(p.pin == (sp.in_fmt != native) && p.pout == (sp.out_fmt != native), where);
    CHECK(p.in_row == (size_t)sp.w * 3 * bps && p.in_bytes == p.in_row * sp.h, where);
    CHECK(p.out_h == sp.h * scale && p.out_w == sp.w * scale && p.out_row == (size_t)p.out_w * 3 * bps && p.out_bytes == p.out_row * p.out_h, where);
    const bool sized = sp.rs_oh > 0 && !(sp.rs_oh == p.out_h && sp.rs_ow == p.out_w);
    CHECK(p.rs == sized && p.res_h == (sized ? sp.rs_oh : p.out_h) && p.res_w == (sized ? sp.rs_ow : p.out_w), where);
    CHECK(p.res_row == (size_t)p.res_w * 3 * bps && p.res_bytes == p.res_row * p.res_h, where);
    CHECK(p.pin_bytes == pix_frame_bytes(sp.in_fmt, sp.h, sp.w) && p.pout_bytes == pix_frame_bytes(sp.out_fmt, p.res_h, p.res_w), where);
    CHECK(p.dl_bytes == (p.pout ? p.pout_bytes : p.res_bytes), where);
    CHECK(p.dl_row * (size_t)p.dl_rows == p.dl_bytes && p.dl_user_stride >= p.dl_row, where);
    CHECK(p.h2d_row * (size_t)p.h2d_rows == p.packed_bytes && p.packed_bytes == (p.pin ? p.pin_bytes : p.in_bytes), where);
    CHECK(p.key.h == sp.h && p.key.w == sp.w && p.key.res_h == p.res_h && p.key.res_w == p.res_w && p.key.filter == (p.rs ? sp.rs_filter : 0), where);
    CHECK(p.win == (win != nullptr), where);
    if (!win) {
        CHECK(!p.win_rows && !p.win_cols && p.wn == 0 && p.wstage_bytes == 0 && p.in_offset == 0 && p.in_stride == sp.in_stride, where);
        CHECK(p.h_in_bytes == p.packed_bytes, where);
        return;
    }
    ++counts.windows;
    CHECK(p.wn >= 1 && p.wn <= 3 && p.win_rows == p.pin, where);
    CHECK(p.win_cols == (p.win_rows && p.wpl[0].dst_row != p.wpl[0].src_row), where);
    size_t at[3] = {0, 0, 0}, dense = 0;
    const size_t staging = pix_window_staging(p.wpl, p.wn, at);
    CHECK(p.wstage_bytes == (p.win_cols ? staging : 0), where);
    for (int k = 0; k < p.wn; ++k) {
        const WindowPlane& q = p.wpl[k];
        CHECK(q.xbytes + q.dst_row <= q.src_row && q.rows >= 1 && q.row0 >= 0, where);
        CHECK(!p.win_cols || (p.wstage[k] == at[k] && at[k] % 16 == 0 && at[k] + q.src_row * q.rows <= staging), where);
        CHECK(q.dst_off == dense, where);           // the planes of the dense window frame lie end to end
        dense += q.dst_row * q.rows;
    }
    CHECK(dense == p.pin_bytes || !p.pin, where);
    CHECK(p.h_in_bytes == (p.win_cols ? p.wstage_bytes : p.packed_bytes), where);
    if (!p.pin) CHECK(p.in_stride == p.wpl[0].src_row && p.in_offset == (size_t)win->y * p.in_stride + (size_t)win->x * 3 * bps, where);
    // a window that is the whole frame: the plan of no window, apart from the window's own members (a BGR window takes the
    // source's dense rows, so there the caller's stride has to be the dense one)
    if (win->src_h == sp.h && win->src_w == sp.w && (p.pin || sp.in_stride == p.in_row)) {
        SubmitPlan whole;
        CHECK(submit_plan(sp, scale, nullptr, &whole) == nullptr && same_sizes(p, whole), where);
        for (int k = 0; k < p.wn; ++k) CHECK(p.wpl[k].row0 == 0 && p.wpl[k].xbytes == 0 && p.wpl[k].src_row == p.wpl[k].dst_row, where);
    }
}

}  // namespace

int main(int argc, char** argv)
{
    const int sweep = argc > 1 ? std::atoi(argv[1]) : 20000;
    known_answers();
    const int fmts[] = {PIX_BGR24, PIX_YUV420P, PIX_NV12, PIX_P010LE, PIX_YUV420P10LE, PIX_BGR48LE, PIX_YUV422P, PIX_YUV422P10LE};
    const int scales[] = {1, 2, 4};
    // (raw engine output: the same cases with every standard library)
    std::mt19937 rng(2031);
    auto below = [&](unsigned n) { return (int)(rng() % n); };
    auto fmt_for = [&](int bits) {
        int f = fmts[below(8)];
        return bits == 8 && f == PIX_BGR48LE ? PIX_BGR24 : f;       // (the entries refuse bgr48le in an 8-bit call)
    };
    for (int i = 0; i < sweep; ++i) {
        const int bits = below(2) ? 16 : 8, scale = scales[below(3)];
        int h = 1 + below(37), w = 1 + below(53);
        if (below(2)) { h = (h + 1) & ~1; w = (w + 1) & ~1; }
        const int in_fmt = fmt_for(bits), out_fmt = fmt_for(bits);
        int oh = 0, ow = 0;
        if (below(2)) {
            oh = below(4) ? 1 + below(4 * h * scale) : h * scale;
            ow = below(4) ? 1 + below(4 * w * scale) : w * scale;
            ++counts.sized;
        }
        SubmitSpec sp = spec(bits, in_fmt, out_fmt, h, w, scale, oh, ow);
        sp.rs_filter = below(3);
        sp.colour = below(32);
        if (!below(8)) sp.in_stride += 1 + below(64);
        if (!below(8)) sp.out_stride += 1 + below(64);
        if (!below(16)) sp.in_stride -= 1;
        const std::string where = "case " + std::to_string(i) + ": bits " + std::to_string(bits) + " fmt " + std::to_string(in_fmt) + " -> " +
                                  std::to_string(out_fmt) + " " + std::to_string(h) + "x" + std::to_string(w) + " x" + std::to_string(scale) +
                                  " sized " + std::to_string(oh) + "x" + std::to_string(ow);
        check_plan(sp, scale, nullptr, where);
        SubmitWindow win;
        if (below(4)) {
            win.src_h = h + 2 * below(6) + below(2) * below(2); win.src_w = w + 2 * below(6) + below(2) * below(2);
            win.y = below(win.src_h - h + 1 + below(2)); win.x = below(win.src_w - w + 1 + below(2));
            if (below(2)) { win.y &= ~1; win.x &= ~1; }
        } else {
            win.src_h = h; win.src_w = w;
        }
        check_plan(sp, scale, &win, where + " window " + std::to_string(win.src_h) + "x" + std::to_string(win.src_w) + " at " +
                                        std::to_string(win.x) + "," + std::to_string(win.y));
    }
    std::printf("submit_check: %ld plans, %ld with a window, %ld sized calls, %ld refusals: ok\n", counts.plans, counts.windows, counts.sized,
                counts.refused);
    return 0;
}
