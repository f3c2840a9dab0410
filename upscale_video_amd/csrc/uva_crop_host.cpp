// uva_crop_host.cpp -- the host half of the crop detector and of the input window (uva_crop.h): plain
// C++, no HIP, every function a function of its arguments.  The arithmetic restates ffmpeg cropdetect's rule (the filter the
// reference runs, upscale/upscale_processing.py:137-181) as tests/cropdetect_ref.py defines it for this project.
#include "uva_crop.h"

namespace uva {

CropSample crop_sample(int fmt)
{
    switch (fmt) {
    case CROP_BGR24: return {1, 0, 0xff, 8, 3};
    case CROP_YUV420P: case CROP_NV12: case CROP_YUV422P: return {1, 0, 0xff, 8, 1};
    case CROP_P010LE: return {2, 6, 0xffff, 10, 1};
    case CROP_YUV420P10LE: case CROP_YUV422P10LE: return {2, 0, 1023, 10, 1};
    case CROP_BGR48LE: return {2, 0, 0xffff, 16, 3};
    default: return {0, 0, 0, 0, 0};
    }
}

const char* crop_bounds(const unsigned long long* rows, const unsigned long long* cols, int fmt, int h, int w, int limit, int bounds[4])
{
    if (!rows || !cols || !bounds) return "uva_crop_bounds: null pointer";
    const CropSample cs = crop_sample(fmt);
    if (!cs.bytes) return "unknown pixel format";
    if (h < 1 || w < 1 || (long long)h * w > (1ll << 28)) return "bad image size";
    if (limit < 0 || limit > 255) return "uva_crop_bounds: the limit is 0 ... 255 on the 8-bit scale";
    const unsigned long long L = (unsigned long long)limit << (cs.depth - 8);
    const unsigned long long n_row = (unsigned long long)w * cs.comps, n_col = (unsigned long long)h * cs.comps;
    int first_r = -1, last_r = -1, first_c = -1, last_c = -1;
    for (int r = 0; r < h; ++r)
        if (rows[r] / n_row > L) {
            if (first_r < 0) first_r = r;
            last_r = r;
        }
    for (int c = 0; c < w; ++c)
        if (cols[c] / n_col > L) {
            if (first_c < 0) first_c = c;
            last_c = c;
        }
    bounds[0] = first_r; bounds[1] = last_r; bounds[2] = first_c; bounds[3] = last_c;
    return nullptr;
}

bool crop_rect(const int state[4], int round, int rect[4])
{
    long long R = round <= 1 ? 16 : round;
    if (R & 1) R *= 2;
    // (64-bit throughout: a caller may hand any four ints)
    const long long x1 = state[0], y1 = state[1], x2 = state[2], y2 = state[3];
    long long x = (x1 + 1) & ~1ll, y = (y1 + 1) & ~1ll;
    long long cw = x2 - x + 1, ch = y2 - y + 1;
    if (cw <= 0 || ch <= 0) return false;
    long long k = cw % R;
    cw -= k; x += (k / 2 + 1) & ~1ll;
    k = ch % R;
    ch -= k; y += (k / 2 + 1) & ~1ll;
    if (cw <= 0 || ch <= 0) return false;
    if (cw > 0x7fffffffll || ch > 0x7fffffffll || x > 0x7fffffffll || y > 0x7fffffffll || x < 0 || y < 0) return false;
    rect[0] = (int)cw; rect[1] = (int)ch; rect[2] = (int)x; rect[3] = (int)y;
    return true;
}

namespace {
bool is_ycbcr(int fmt) { return fmt != CROP_BGR24 && fmt != CROP_BGR48LE; }
bool is_420(int fmt) { return fmt == CROP_YUV420P || fmt == CROP_NV12 || fmt == CROP_P010LE || fmt == CROP_YUV420P10LE; }
}  // namespace

const char* crop_window_error(int fmt, int src_h, int src_w, int x, int y, int h, int w)
{
    if (!crop_sample(fmt).bytes) return "unknown pixel format";
    if (src_h < 1 || src_w < 1 || (long long)src_h * src_w > (1ll << 28)) return "input window: bad size of the source frame";
    if (h < 1 || w < 1) return "input window: bad image size";
    if (x < 0 || y < 0 || (long long)x + w > src_w || (long long)y + h > src_h) return "input window: the window leaves the frame";
    if (is_ycbcr(fmt) && ((x | w) & 1)) return "input window: x and the width must be even for a Y'CbCr format (chroma pairs are not split)";
    if (is_420(fmt) && ((y | h) & 1)) return "input window: y and the height must be even for a 4:2:0 format (chroma rows are not split)";
    return nullptr;
}

int crop_window_planes(int fmt, int src_h, int src_w, int x, int y, int h, int w, WindowPlane planes[3])
{
    const CropSample cs = crop_sample(fmt);
    if (!cs.bytes) return 0;
    const size_t b = (size_t)cs.bytes;
    auto plane = [&](size_t src_off, size_t dst_off, size_t src_row, size_t dst_row, size_t xbytes, int row0, int rows) {
        WindowPlane p;
        p.src_off = src_off; p.dst_off = dst_off; p.src_row = src_row; p.dst_row = dst_row; p.xbytes = xbytes; p.row0 = row0; p.rows = rows;
        return p;
    };
    if (!is_ycbcr(fmt)) {
        planes[0] = plane(0, 0, (size_t)src_w * 3 * b, (size_t)w * 3 * b, (size_t)x * 3 * b, y, h);
        return 1;
    }
    const size_t scw = ((size_t)src_w + 1) / 2, cw = ((size_t)w + 1) / 2;          // chroma samples of a row
    const bool v420 = is_420(fmt);
    const size_t sch = v420 ? ((size_t)src_h + 1) / 2 : (size_t)src_h;            // chroma rows of the source
    const int crow0 = v420 ? y / 2 : y, crows = v420 ? (h + 1) / 2 : h;
    const size_t ysrc = (size_t)src_w * src_h * b, ydst = (size_t)w * h * b;
    planes[0] = plane(0, 0, (size_t)src_w * b, (size_t)w * b, (size_t)x * b, y, h);
    if (fmt == CROP_NV12 || fmt == CROP_P010LE) {
        planes[1] = plane(ysrc, ydst, scw * 2 * b, cw * 2 * b, (size_t)(x / 2) * 2 * b, crow0, crows);
        return 2;
    }
    planes[1] = plane(ysrc, ydst, scw * b, cw * b, (size_t)(x / 2) * b, crow0, crows);
    planes[2] = plane(ysrc + scw * sch * b, ydst + cw * (size_t)crows * b, scw * b, cw * b, (size_t)(x / 2) * b, crow0, crows);
    return 3;
}

size_t pix_window_staging(const WindowPlane* planes, int n, size_t stage_off[3])
{
    size_t at = 0;
    for (int p = 0; p < n; ++p) {
        stage_off[p] = at;
        at += (planes[p].src_row * (size_t)planes[p].rows + 15) & ~(size_t)15;
    }
    return at;
}

}  // namespace uva
