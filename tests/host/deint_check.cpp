// deint_check.cpp -- the host half of the deinterlacer (csrc/uva_deint_host.cpp) run alone, without HIP and without a GPU, so
// that it can be built with -fsanitize=address,undefined (tests/test_deint_sanitized.py).  For every format and every size
// h = 4 ... 40, w = 1 ... 40 the table of planes is checked against the frame's size as this file computes it, and the scalar
// rule runs over three frames in heap buffers of exactly that many bytes -- a read or write past either end of any of the five
// is the sanitizer's to find.  Checked on the way: the kept rows of output A and of output B together are `cur`, byte for byte,
// and interpolated samples are clean code values.  Prints one line of counts; the first violation ends the run with status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../upscale_video_amd/csrc/uva_deint.h"

using namespace uva;

namespace {

struct Counts { long frames = 0, planes = 0, kept = 0, samples = 0, refused = 0; } counts;

[[noreturn]] void violation(const std::string& what, const std::string& where)
{
    std::fprintf(stderr, "deint_check: %s (%s)\n", what.c_str(), where.c_str());
    std::exit(1);
}

#define CHECK(cond, where) do { if (!(cond)) violation(#cond, where); } while (0)

const int FMTS[] = {DEINT_BGR24, DEINT_YUV420P, DEINT_NV12, DEINT_P010LE, DEINT_YUV420P10LE, DEINT_BGR48LE, DEINT_YUV422P, DEINT_YUV422P10LE};

unsigned long long state = 20261020ull;
unsigned next_random()
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(state >> 33);
}

// bytes of a dense frame, by the formats' definition (csrc/uva_pixfmt.h), not by the table under test
size_t frame_bytes(int fmt, int h, int w)
{
    const size_t cw = ((size_t)w + 1) / 2, ch = ((size_t)h + 1) / 2, y = (size_t)h * w;
    switch (fmt) {
    case DEINT_BGR24: return 3 * y;
    case DEINT_BGR48LE: return 6 * y;
    case DEINT_YUV420P: case DEINT_NV12: return y + 2 * cw * ch;
    case DEINT_P010LE: case DEINT_YUV420P10LE: return 2 * (y + 2 * cw * ch);
    case DEINT_YUV422P: return y + 2 * cw * (size_t)h;
    default: return 2 * (y + 2 * cw * (size_t)h);
    }
}

void check_size(int fmt, int h, int w, int flags)
{
    const std::string where = "fmt " + std::to_string(fmt) + " " + std::to_string(h) + "x" + std::to_string(w) + " flags " + std::to_string(flags);
    CHECK(deint_error(fmt, h, w, flags) == nullptr, where);
    const DeintFormat f = deint_format(fmt, h, w);
    const size_t n = frame_bytes(fmt, h, w);
    CHECK(f.bytes == 1 || f.bytes == 2, where);
    CHECK(f.frame_bytes == n, where);
    // the planes tile the frame: each begins where the one before ends, the last ends with the frame
    size_t at = 0;
    for (int p = 0; p < f.nplanes; ++p) {
        const DeintPlane& pl = f.plane[p];
        CHECK(pl.off == at && pl.ph >= 2 && pl.pw >= 1 && pl.stride >= 1 && pl.stride <= 3, where);
        CHECK(pl.row_bytes == (size_t)pl.pw * pl.stride * f.bytes, where);
        at += pl.row_bytes * (size_t)pl.ph;
        ++counts.planes;
    }
    CHECK(at == n, where);
    // three frames of random words (ignored bits included) and two outputs, each a heap block of exactly n bytes
    std::vector<uint8_t*> buf;
    for (int k = 0; k < 5; ++k) buf.push_back((uint8_t*)std::malloc(n));
    for (int k = 0; k < 3; ++k)
        for (size_t i = 0; i < n; ++i) buf[k][i] = (uint8_t)next_random();
    std::memset(buf[3], 0xa5, n);
    std::memset(buf[4], 0x5a, n);
    const bool field = (flags & DEINT_FIELD) != 0;
    // (the ends of a stream too: a null neighbour is the frame itself)
    const uint8_t* prev = (h + w) % 5 == 0 ? nullptr : buf[0];
    const uint8_t* next = (h + w) % 7 == 0 ? nullptr : buf[2];
    deint_host(prev, buf[1], next, fmt, h, w, flags, buf[3], field ? buf[4] : nullptr);
    const int par_a = deint_parity_a(flags);
    for (int p = 0; p < f.nplanes; ++p) {
        const DeintPlane& pl = f.plane[p];
        for (int y = 0; y < pl.ph; ++y) {
            const size_t o = pl.off + (size_t)y * pl.row_bytes;
            const bool in_a = (y & 1) == par_a;          // A interpolates the row, B keeps it
            const uint8_t* keeper = in_a ? (field ? buf[4] : nullptr) : buf[3];
            const uint8_t* other = in_a ? buf[3] : (field ? buf[4] : nullptr);
            if (keeper) {
                CHECK(std::memcmp(keeper + o, buf[1] + o, pl.row_bytes) == 0, where + " kept row " + std::to_string(y));
                ++counts.kept;
            }
            if (other && f.bytes == 2) {
                for (size_t j = 0; j < pl.row_bytes; j += 2) {
                    const unsigned word = other[o + j] | ((unsigned)other[o + j + 1] << 8);
                    CHECK((word & ~((unsigned)f.mask << f.shift)) == 0, where + " unclean sample in row " + std::to_string(y));
                    ++counts.samples;
                }
            } else if (other) {
                counts.samples += (long)pl.row_bytes;
            }
        }
    }
    for (uint8_t* b : buf) std::free(b);
    ++counts.frames;
}

void check_refusals()
{
    const struct { int fmt, h, w, flags; } bad[] = {
        {4, 8, 8, 0}, {9, 8, 8, 0}, {-1, 8, 8, 0}, {DEINT_YUV420P, 3, 8, 0}, {DEINT_BGR24, 0, 8, 0}, {DEINT_BGR24, 8, 0, 0},
        {DEINT_BGR24, -4, 8, 0}, {DEINT_NV12, 8, 8, 4}, {DEINT_NV12, 8, 8, -1}, {DEINT_BGR48LE, 1 << 15, (1 << 13) + 1, 0},
    };
    for (const auto& b : bad) {
        CHECK(deint_error(b.fmt, b.h, b.w, b.flags) != nullptr, "refusal of fmt " + std::to_string(b.fmt) + " " + std::to_string(b.h) + "x" +
                                                                 std::to_string(b.w) + " flags " + std::to_string(b.flags));
        ++counts.refused;
    }
    CHECK(deint_error(DEINT_BGR48LE, 1 << 15, 1 << 13, DEINT_FIELD | DEINT_BFF) == nullptr, "2^28 pixels are taken");
}

}  // namespace

int main()
{
    check_refusals();
    for (int fmt : FMTS)
        for (int h = 4; h <= 40; ++h)
            for (int w = 1; w <= 40; ++w) check_size(fmt, h, w, (h * 3 + w) & 3);
    std::printf("deint_check: %ld frames, %ld planes, %ld kept rows, %ld interpolated samples, %ld refusals: ok\n", counts.frames,
                counts.planes, counts.kept, counts.samples, counts.refused);
    return 0;
}
