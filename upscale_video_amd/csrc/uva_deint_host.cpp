// uva_deint_host.cpp -- the host half of the deinterlacer (uva_deint.h): plain C++, no HIP, every
// function a function of its arguments.  The table of a format's planes, the refusals, and the rule of tests/yadif_ref.py
// sample by sample (deint_sample_mem, the function the kernel's ragged ends use too) behind uva_debug_deint_host.
#include "uva_deint.h"

#include <string.h>

namespace uva {

DeintFormat deint_format(int fmt, int h, int w)
{
    DeintFormat f;
    memset(&f, 0, sizeof f);
    int b = 0, shift = 0, mask = 0;
    switch (fmt) {
    case DEINT_BGR24: case DEINT_YUV420P: case DEINT_NV12: case DEINT_YUV422P: b = 1; mask = 0xff; break;
    case DEINT_P010LE: b = 2; shift = 6; mask = 1023; break;
    case DEINT_YUV420P10LE: case DEINT_YUV422P10LE: b = 2; mask = 1023; break;
    case DEINT_BGR48LE: b = 2; mask = 0xffff; break;
    default: return f;
    }
    f.bytes = b; f.shift = shift; f.mask = mask;
    if (h < 1 || w < 1) return f;
    auto plane = [&](size_t off, int pw, int ph, int stride) {
        DeintPlane p;
        p.off = off; p.pw = pw; p.ph = ph; p.stride = stride; p.row_bytes = (size_t)pw * stride * b;
        return p;
    };
    if (fmt == DEINT_BGR24 || fmt == DEINT_BGR48LE) {
        f.nplanes = 1;
        f.plane[0] = plane(0, w, h, 3);
        f.frame_bytes = (size_t)h * f.plane[0].row_bytes;
        return f;
    }
    const bool v422 = fmt == DEINT_YUV422P || fmt == DEINT_YUV422P10LE;
    const int cw = (w + 1) / 2, ch = v422 ? h : (h + 1) / 2;
    const size_t ysz = (size_t)w * h * b;
    f.plane[0] = plane(0, w, h, 1);
    if (fmt == DEINT_NV12 || fmt == DEINT_P010LE) {
        f.nplanes = 2;
        f.plane[1] = plane(ysz, cw, ch, 2);
        f.frame_bytes = ysz + (size_t)ch * f.plane[1].row_bytes;
        return f;
    }
    f.nplanes = 3;
    f.plane[1] = plane(ysz, cw, ch, 1);
    f.plane[2] = plane(ysz + (size_t)cw * ch * b, cw, ch, 1);
    f.frame_bytes = ysz + 2 * (size_t)cw * ch * b;
    return f;
}

const char* deint_error(int fmt, int h, int w, int flags)
{
    if (!deint_format(fmt, 1, 1).bytes) return "unknown pixel format";
    if (flags & ~DEINT_FLAGS) return "deinterlace: unknown flag bits (UVA_DEINT_FIELD | UVA_DEINT_BFF)";
    if (h <= 0 || w <= 0 || (long long)h * w > (1ll << 28)) return "bad image size";
    if (h < 4) return "deinterlace: a frame of fewer than 4 rows has no two rows of either field in its chroma planes";
    return nullptr;
}

namespace {

// rows of parity `par` of the plane: interpolated into out; the others copied from cur
template <int BYTES>
void deint_plane_host(const uint8_t* prev, const uint8_t* cur, const uint8_t* next, const uint8_t* p2, const uint8_t* n2, const DeintPlane& pl,
                      int shift, int mask, int par, uint8_t* out)
{
    const int n = pl.pw * pl.stride;
    for (int y = 0; y < pl.ph; ++y) {
        uint8_t* dst = out + (size_t)y * pl.row_bytes;
        if ((y & 1) != par) {
            memcpy(dst, cur + (size_t)y * pl.row_bytes, pl.row_bytes);
            continue;
        }
        for (int j = 0; j < n; ++j) {
            const int sp = deint_sample_mem<BYTES>(prev, cur, next, p2, n2, pl.row_bytes, pl.pw, pl.ph, pl.stride, shift, mask, y, j);
            if (BYTES == 1) {
                dst[j] = (uint8_t)sp;
            } else {
                const uint32_t word = (uint32_t)sp << shift;
                dst[2 * j] = (uint8_t)(word & 255u);
                dst[2 * j + 1] = (uint8_t)(word >> 8);
            }
        }
    }
}

}  // namespace

void deint_host(const uint8_t* prev, const uint8_t* cur, const uint8_t* next, int fmt, int h, int w, int flags, uint8_t* out_a, uint8_t* out_b)
{
    const DeintFormat f = deint_format(fmt, h, w);
    if (!prev) prev = cur;
    if (!next) next = cur;
    const int par_a = deint_parity_a(flags);
    for (int p = 0; p < f.nplanes; ++p) {
        const DeintPlane& pl = f.plane[p];
        const uint8_t *pv = prev + pl.off, *cu = cur + pl.off, *nx = next + pl.off;
        for (int o = 0; o < 2; ++o) {
            uint8_t* out = o ? out_b : out_a;
            if (!out) continue;
            const uint8_t *p2 = o ? cu : pv, *n2 = o ? nx : cu;
            if (f.bytes == 1) deint_plane_host<1>(pv, cu, nx, p2, n2, pl, f.shift, f.mask, o ? 1 - par_a : par_a, out + pl.off);
            else deint_plane_host<2>(pv, cu, nx, p2, n2, pl, f.shift, f.mask, o ? 1 - par_a : par_a, out + pl.off);
        }
    }
}

}  // namespace uva
