// ivtc_check.cpp -- the host half of the inverse telecine (csrc/uva_ivtc_host.cpp, with csrc/uva_deint_host.cpp for the plane
// table) run alone, without HIP and without a GPU, so that it can be built with -fsanitize=address,undefined
// (tests/test_ivtc_sanitized.py).  For every format and every size h = 4 ... 40, w = 1 ... 40 the metric, the three weaves and
// the decision run over three frames in heap buffers of exactly a frame's bytes -- a read or write past either end of any of
// them is the sanitizer's to find.  Checked on the way: a woven frame's rows are cur's or the candidate's byte for byte, the
// candidate c of a frame is the frame, identical neighbours give identical sums, and the decimator delivers n - n / 5 frames in
// order whatever the diffs.  Prints one line of counts; the first violation ends the run with status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../upscale_video_amd/csrc/uva_ivtc.h"

using namespace uva;

namespace {

struct Counts { long frames = 0, rows = 0, streams = 0, refused = 0; } counts;

[[noreturn]] void violation(const std::string& what, const std::string& where)
{
    std::fprintf(stderr, "ivtc_check: %s (%s)\n", what.c_str(), where.c_str());
    std::exit(1);
}

#define CHECK(cond, where) do { if (!(cond)) violation(#cond, where); } while (0)

const int FMTS[] = {DEINT_BGR24, DEINT_YUV420P, DEINT_NV12, DEINT_P010LE, DEINT_YUV420P10LE, DEINT_BGR48LE, DEINT_YUV422P, DEINT_YUV422P10LE};

unsigned long long state = 20261021ull;
unsigned next_random()
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(state >> 33);
}

void check_size(int fmt, int h, int w, int flags)
{
    const std::string where = "fmt " + std::to_string(fmt) + " " + std::to_string(h) + "x" + std::to_string(w) + " flags " + std::to_string(flags);
    const int T = (int)(next_random() % 256), L = (int)(next_random() % 1000001);
    CHECK(ivtc_error(fmt, h, w, flags, T, L) == nullptr, where);
    const DeintFormat f = deint_format(fmt, h, w);
    const size_t n = f.frame_bytes;
    // three frames of random words (ignored bits included) and a woven frame, each a heap block of exactly n bytes
    std::vector<uint8_t*> buf;
    for (int k = 0; k < 4; ++k) buf.push_back((uint8_t*)std::malloc(n));
    for (int k = 0; k < 3; ++k)
        for (size_t i = 0; i < n; ++i) buf[k][i] = (uint8_t)next_random();
    const uint8_t* prev = (h + w) % 5 == 0 ? nullptr : buf[0];
    const uint8_t* next = (h + w) % 7 == 0 ? nullptr : buf[2];
    unsigned long long st[6], again[6];
    ivtc_metrics_host(prev, buf[1], next, fmt, h, w, flags, T, st);
    if (!prev) CHECK(st[2] == st[0] && st[3] == st[1], where + " null prev");
    if (!next) CHECK(st[4] == st[0] && st[5] == st[1], where + " null next");
    const unsigned long long all = (unsigned long long)(f.plane[0].ph - 2) * f.plane[0].pw * f.plane[0].stride;
    for (int k = 0; k < 3; ++k) CHECK(st[2 * k] <= all && st[2 * k + 1] <= st[2 * k] * (unsigned long long)f.mask, where);
    int rows = 0, match = -1;
    long long samples = 0;
    ivtc_metric_extent(f, &rows, &samples);
    (void)ivtc_choose(st, rows, samples, L, &match);
    CHECK(match >= 0 && match <= 2, where);
    for (int k = 0; k < 3; ++k) CHECK(st[2 * match + 1] <= st[2 * k + 1], where + " the match has the smallest M");
    const uint8_t* x[3] = {buf[1], prev ? prev : buf[1], next ? next : buf[1]};
    const int first = ivtc_first(flags);
    for (int k = 0; k < 3; ++k) {
        std::memset(buf[3], 0xa5, n);
        ivtc_weave_host(buf[1], x[k], fmt, h, w, flags, buf[3]);
        for (int p = 0; p < f.nplanes; ++p) {
            const DeintPlane& pl = f.plane[p];
            for (int y = 0; y < pl.ph; ++y) {
                const size_t o = pl.off + (size_t)y * pl.row_bytes;
                CHECK(std::memcmp(buf[3] + o, ((y & 1) == first ? buf[1] : x[k]) + o, pl.row_bytes) == 0, where + " woven row " + std::to_string(y));
                ++counts.rows;
            }
        }
        if (k == 0) CHECK(std::memcmp(buf[3], buf[1], n) == 0, where + " candidate c is cur");
        // the metric of the woven frame as its own candidate c is the candidate's
        ivtc_metrics_host(nullptr, buf[3], nullptr, fmt, h, w, flags, T, again);
        CHECK(again[0] == st[2 * k] && again[1] == st[2 * k + 1], where + " metric of the woven frame");
    }
    for (uint8_t* b : buf) std::free(b);
    ++counts.frames;
}

void check_decimator()
{
    for (int n = 0; n <= 23; ++n) {
        for (int keep_all = 0; keep_all < 2; ++keep_all) {
            IvtcDecimator dec;
            dec.reset(keep_all != 0);
            std::vector<long long> got;
            long long j = 0;
            for (int k = 0; k < n; ++k) {
                dec.add(k == 0 ? IVTC_FIRST_DIFF : (unsigned long long)(next_random() % 4));       // (many ties)
                if (dec.pop(&j)) got.push_back(j);
            }
            dec.end();
            while (dec.pop(&j)) got.push_back(j);
            const std::string where = "decimator n " + std::to_string(n) + " keep_all " + std::to_string(keep_all);
            CHECK((int)got.size() == (keep_all ? n : n - n / 5), where);
            CHECK(dec.dropped == (keep_all ? 0 : n / 5), where);
            for (size_t i = 0; i < got.size(); ++i) {
                CHECK(got[i] >= 0 && got[i] < n && (i == 0 || got[i] > got[i - 1]), where);
                if (!keep_all) CHECK(got[i] / 5 == (long long)(i / 4) || got[i] >= (n / 5) * 5, where + " four of every five");
            }
            ++counts.streams;
        }
    }
    // equal diffs drop the earliest; the first frame of a stream is never the smallest
    IvtcDecimator dec;
    dec.reset(false);
    long long j = -1;
    const unsigned long long d[5] = {IVTC_FIRST_DIFF, 7, 3, 3, 9};
    std::vector<long long> got;
    for (unsigned long long v : d) dec.add(v);
    while (dec.pop(&j)) got.push_back(j);
    CHECK(got.size() == 4 && got[0] == 0 && got[1] == 1 && got[2] == 3 && got[3] == 4, "ties drop the earliest");
}

void check_refusals()
{
    const struct { int fmt, h, w, flags, T, L; } bad[] = {
        {4, 8, 8, 0, 9, 1000}, {9, 8, 8, 0, 9, 1000}, {-1, 8, 8, 0, 9, 1000}, {DEINT_YUV420P, 3, 8, 0, 9, 1000}, {DEINT_BGR24, 0, 8, 0, 9, 1000},
        {DEINT_BGR24, 8, 0, 0, 9, 1000}, {DEINT_NV12, 8, 8, 8, 9, 1000}, {DEINT_NV12, 8, 8, -1, 9, 1000}, {DEINT_NV12, 8, 8, 0, -1, 1000},
        {DEINT_NV12, 8, 8, 0, 256, 1000}, {DEINT_NV12, 8, 8, 0, 9, -1}, {DEINT_NV12, 8, 8, 0, 9, 1000001},
        {DEINT_BGR48LE, 1 << 15, (1 << 13) + 1, 0, 9, 1000},
    };
    for (const auto& b : bad) {
        CHECK(ivtc_error(b.fmt, b.h, b.w, b.flags, b.T, b.L) != nullptr, "refusal of fmt " + std::to_string(b.fmt) + " " + std::to_string(b.h) + "x" +
                                                                          std::to_string(b.w) + " flags " + std::to_string(b.flags));
        ++counts.refused;
    }
    CHECK(ivtc_error(DEINT_BGR48LE, 1 << 15, 1 << 13, IVTC_FLAGS, 255, 1000000) == nullptr, "2^28 pixels are taken");
    CHECK(ivtc_error(DEINT_BGR24, 4, 1, 0, 0, 0) == nullptr, "4 x 1 is taken");
}

}  // namespace

int main()
{
    check_refusals();
    check_decimator();
    for (int fmt : FMTS)
        for (int h = 4; h <= 40; ++h)
            for (int w = 1; w <= 40; ++w) check_size(fmt, h, w, (h * 3 + w) & IVTC_FLAGS);
    std::printf("ivtc_check: %ld frames, %ld woven rows, %ld decimated streams, %ld refusals: ok\n", counts.frames, counts.rows,
                counts.streams, counts.refused);
    return 0;
}
