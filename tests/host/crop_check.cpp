// crop_check.cpp -- the host half of the crop detector and of the input window (csrc/uva_crop_host.cpp) run alone, without HIP and
// without a GPU, so that it can be built with -fsanitize=address,undefined (tests/test_crop_sanitized.py).  The bright-line scan
// runs over line sums in heap arrays of exactly h and w entries (a read past either end is the sanitizer's to find), the
// rectangle arithmetic over a seeded sweep of states -- extreme ints among them -- and the window's planes over a sweep of
// windows, each checked against what the functions' own contract states.  Prints one line of counts; the first violation ends the
// run with exit status 1.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../upscale_video_amd/csrc/uva_crop.h"

using namespace uva;

namespace {

struct Counts { long bounds = 0, rects = 0, none = 0, windows = 0, refused = 0; } counts;

[[noreturn]] void violation(const std::string& what, const std::string& where)
{
    std::fprintf(stderr, "crop_check: %s (%s)\n", what.c_str(), where.c_str());
    std::exit(1);
}

#define CHECK(cond, where) do { if (!(cond)) violation(#cond, where); } while (0)

const int FMTS[] = {CROP_BGR24, CROP_YUV420P, CROP_NV12, CROP_P010LE, CROP_YUV420P10LE, CROP_BGR48LE, CROP_YUV422P, CROP_YUV422P10LE};

std::mt19937 rng(20260102);
int below(int n) { return (int)(rng() % (unsigned)n); }

size_t frame_bytes(int fmt, int h, int w)
{
    const CropSample cs = crop_sample(fmt);
    const size_t b = (size_t)cs.bytes, cw = ((size_t)w + 1) / 2, ch = ((size_t)h + 1) / 2;
    if (cs.comps == 3) return (size_t)h * w * 3 * b;
    const bool v422 = fmt == CROP_YUV422P || fmt == CROP_YUV422P10LE;
    return ((size_t)h * w + 2 * cw * (v422 ? (size_t)h : ch)) * b;
}

void check_bounds(int fmt, int h, int w, int limit)
{
    const std::string where = "bounds fmt " + std::to_string(fmt) + " " + std::to_string(h) + "x" + std::to_string(w);
    const CropSample cs = crop_sample(fmt);
    const unsigned long long top = (1ull << cs.depth) - 1, L = (unsigned long long)limit << (cs.depth - 8);
    std::vector<unsigned long long> rows((size_t)h), cols((size_t)w);
    int fr = -1, lr = -1, fc = -1, lc = -1;
    for (int r = 0; r < h; ++r) {
        const unsigned long long mean = below(3) ? (unsigned long long)below((int)(L + 2 > top ? top + 1 : L + 2)) : top;
        rows[(size_t)r] = mean * (unsigned long long)w * cs.comps + (unsigned long long)below(w * cs.comps);
        if (mean > L) { if (fr < 0) fr = r; lr = r; }
    }
    for (int c = 0; c < w; ++c) {
        const unsigned long long mean = below(3) ? (unsigned long long)below((int)(L + 2 > top ? top + 1 : L + 2)) : top;
        cols[(size_t)c] = mean * (unsigned long long)h * cs.comps + (unsigned long long)below(h * cs.comps);
        if (mean > L) { if (fc < 0) fc = c; lc = c; }
    }
    int b[4] = {7, 7, 7, 7};
    CHECK(crop_bounds(rows.data(), cols.data(), fmt, h, w, limit, b) == nullptr, where);
    CHECK(b[0] == fr && b[1] == lr && b[2] == fc && b[3] == lc, where);
    ++counts.bounds;
}

void check_rect(const int state[4], int round, int h, int w, bool inside)
{
    const std::string where = "rect {" + std::to_string(state[0]) + "," + std::to_string(state[1]) + "," + std::to_string(state[2]) + "," +
                              std::to_string(state[3]) + "} round " + std::to_string(round);
    int r[4] = {-1, -1, -1, -1};
    if (!crop_rect(state, round, r)) { ++counts.none; return; }
    ++counts.rects;
    CHECK(r[0] > 0 && r[1] > 0 && r[2] >= 0 && r[3] >= 0, where);
    CHECK(((r[0] | r[1] | r[2] | r[3]) & 1) == 0, where);
    if (!inside) return;
    CHECK((long long)r[2] + r[0] <= w && (long long)r[3] + r[1] <= h, where);
    for (int fmt : FMTS) CHECK(crop_window_error(fmt, h, w, r[2], r[3], r[1], r[0]) == nullptr, where);
}

void check_window(int fmt, int sh, int sw, int x, int y, int h, int w)
{
    const std::string where = "window fmt " + std::to_string(fmt) + " " + std::to_string(sh) + "x" + std::to_string(sw) + " " +
                              std::to_string(w) + ":" + std::to_string(h) + ":" + std::to_string(x) + ":" + std::to_string(y);
    if (crop_window_error(fmt, sh, sw, x, y, h, w)) { ++counts.refused; return; }
    ++counts.windows;
    WindowPlane p[3];
    const int n = crop_window_planes(fmt, sh, sw, x, y, h, w, p);
    CHECK(n >= 1 && n <= 3, where);
    const size_t src_bytes = frame_bytes(fmt, sh, sw), dst_bytes = frame_bytes(fmt, h, w);
    size_t at = 0;
    for (int k = 0; k < n; ++k) {
        CHECK(p[k].rows >= 1 && p[k].row0 >= 0 && p[k].dst_row >= 1, where);
        CHECK(p[k].xbytes + p[k].dst_row <= p[k].src_row, where);                                        // inside a source row
        CHECK(p[k].src_off + ((size_t)p[k].row0 + p[k].rows) * p[k].src_row <= src_bytes, where);     // inside the source frame
        CHECK(p[k].dst_off == at, where);                                                                // planes follow each other
        at += p[k].dst_row * (size_t)p[k].rows;
    }
    CHECK(at == dst_bytes, where);                                                                       // and fill the window frame
}

}  // namespace

int main()
{
    for (int fmt : FMTS)
        for (int i = 0; i < 40; ++i) check_bounds(fmt, 1 + below(300), 1 + below(400), below(256));
    int b[4];
    unsigned long long one = 0;
    CHECK(crop_bounds(nullptr, &one, CROP_NV12, 1, 1, 24, b) != nullptr, "null rows");
    CHECK(crop_bounds(&one, &one, 4, 1, 1, 24, b) != nullptr, "format 4");
    CHECK(crop_bounds(&one, &one, CROP_NV12, 1, 1, 256, b) != nullptr, "limit 256");
    CHECK(crop_bounds(&one, &one, CROP_NV12, 0, 1, 24, b) != nullptr, "h 0");

    const int all[4] = {0, 0, 299, 69};
    int r[4];
    CHECK(crop_rect(all, 16, r) && r[0] == 288 && r[1] == 64 && r[2] == 6 && r[3] == 4, "288:64:6:4");
    const int rounds[] = {INT_MIN, -1, 0, 1, 2, 3, 15, 16, 32, 33, INT_MAX};
    for (int i = 0; i < 20000; ++i) {
        const int h = 1 + below(2200), w = 1 + below(4100);
        const int st[4] = {below(w), below(h), below(w), below(h)};
        check_rect(st, rounds[2 + below(8)], h, w, true);
    }
    const int extremes[] = {INT_MIN, INT_MIN + 1, -2, -1, 0, 1, INT_MAX - 1, INT_MAX};
    for (int a : extremes)
        for (int c : extremes)
            for (int rd : rounds) {
                const int st[4] = {a, c, c, a};
                check_rect(st, rd, 0, 0, false);
                const int ts[4] = {c, a, a, c};
                check_rect(ts, rd, 0, 0, false);
            }

    for (int fmt : FMTS)
        for (int i = 0; i < 400; ++i) {
            const int sh = 1 + below(200), sw = 1 + below(300);
            check_window(fmt, sh, sw, below(sw + 2) - 1, below(sh + 2) - 1, below(sh + 2), below(sw + 2));
            check_window(fmt, sh, sw, 0, 0, sh, sw);
        }
    CHECK(crop_window_error(CROP_YUV420P, 96, 160, 0, 16, 64, 160) == nullptr, "letterbox");
    CHECK(crop_window_error(CROP_YUV420P, 96, 160, 0, 15, 64, 160) != nullptr, "odd y");
    CHECK(crop_window_error(CROP_YUV422P, 96, 160, 1, 0, 96, 158) != nullptr, "odd x");
    CHECK(crop_window_error(CROP_BGR24, 96, 160, 1, 1, 95, 159) == nullptr, "bgr any");
    CHECK(crop_window_error(CROP_BGR24, 96, 160, INT_MAX, 0, 1, INT_MAX) != nullptr, "overflow");
    std::printf("crop_check: %ld bright-line scans, %ld rectangles, %ld states without one, %ld windows, %ld refusals: ok\n", counts.bounds,
                counts.rects, counts.none, counts.windows, counts.refused);
    return 0;
}
