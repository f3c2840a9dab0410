// uva_pixfmt.hip -- the raw-video route's colour conversions (csrc/uva_pixfmt.h; the arithmetic: DESIGN.md section 7.3), a
// translation unit of its own like uva_sww.hip.  Two kernel families, each instantiated per format:
//   pix_from_bgr  u8 BGR -> yuv420p / nv12 / p010le   (behind the net: its u8 result is what gets converted)
//   pix_to_bgr    yuv420p / nv12 / p010le -> u8 BGR   (in front of the net)
// One thread covers 8 pixels of two rows -- a 2x2 block per chroma sample, so every chroma sample is read or written once.  Both
// are memory-bound: with w % 8 == 0 (and 16-byte aligned bases) a thread's bytes move as 8- and 16-byte accesses, lanes side by
// side along the row; elsewhere (odd sizes, the frame's right / bottom edge) byte by byte with bounds checks.
#include <cmath>

#include "uva_pixfmt.h"

namespace uva {

namespace {

constexpr int PX = 8;               // pixels of a row per thread (rows 2*gy and 2*gy + 1; 4 chroma samples per plane)
constexpr int BX = 64, BY = 4;      // threads of a workgroup along x (groups of PX pixels) and y (row pairs)

// Fixed point: every coefficient is round(c * 2^16) (floor(c * 2^16 + 0.5)), sums in int32, + half, >> 16 (chroma of an n-pixel
// block from the block's sums: >> 16 + log2 n), clamped to the format's codes.
struct FwdCoef { int yr, yg, yb, ur, ug, ub, vr, vg, vb, yoff, coff, maxv; };
struct InvCoef { int ky, rv, gu, gv, bu, yoff, coff; };

int fix16(double c) { return (int)std::floor(c * 65536.0 + 0.5); }

void matrix(int colour, double& kr, double& kb)
{
    if (colour & PIX_CSP_BT709) { kr = 0.2126; kb = 0.0722; }
    else { kr = 0.299; kb = 0.114; }
}

// code ranges at `depth` bits: luma 16..235 / chroma 16..240 scaled by 2^(depth-8) (limited), 0..2^depth-1 (full)
void ranges(int colour, int depth, int& ys, int& cs, int& yoff)
{
    const bool full = colour & PIX_RANGE_FULL;
    ys = full ? (1 << depth) - 1 : 219 << (depth - 8);
    cs = full ? (1 << depth) - 1 : 224 << (depth - 8);
    yoff = full ? 0 : 16 << (depth - 8);
}

FwdCoef fwd_coef(int colour, int depth)
{
    double kr, kb;
    matrix(colour, kr, kb);
    const double kg = 1.0 - kr - kb;
    int ys, cs, yoff;
    ranges(colour, depth, ys, cs, yoff);
    const double sy = ys / 255.0, sc = cs / 255.0;
    FwdCoef c;
    c.yr = fix16(kr * sy); c.yg = fix16(kg * sy); c.yb = fix16(kb * sy);
    c.ur = fix16(-kr / (2 * (1 - kb)) * sc); c.ug = fix16(-kg / (2 * (1 - kb)) * sc); c.ub = fix16(0.5 * sc);
    c.vr = fix16(0.5 * sc); c.vg = fix16(-kg / (2 * (1 - kr)) * sc); c.vb = fix16(-kb / (2 * (1 - kr)) * sc);
    c.yoff = yoff; c.coff = 1 << (depth - 1); c.maxv = (1 << depth) - 1;
    return c;
}

InvCoef inv_coef(int colour, int depth)
{
    double kr, kb;
    matrix(colour, kr, kb);
    const double kg = 1.0 - kr - kb;
    int ys, cs, yoff;
    ranges(colour, depth, ys, cs, yoff);
    const double ky = 255.0 / ys, kc = 255.0 / cs;
    InvCoef c;
    c.ky = fix16(ky);
    c.rv = fix16(2 * (1 - kr) * kc);
    c.bu = fix16(2 * (1 - kb) * kc);
    c.gu = fix16(-2 * kb * (1 - kb) / kg * kc);
    c.gv = fix16(-2 * kr * (1 - kr) / kg * kc);
    c.yoff = yoff; c.coff = 1 << (depth - 1);
    return c;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ uint32_t pack4(int a, int b, int c, int d)
{
    return (uint32_t)a | ((uint32_t)b << 8) | ((uint32_t)c << 16) | ((uint32_t)d << 24);
}
__device__ __forceinline__ uint32_t pack2(int a, int b) { return (uint32_t)a | ((uint32_t)b << 16); }
__device__ __forceinline__ int byte_of(const uint32_t* d, int k) { return (d[k >> 2] >> (8 * (k & 3))) & 255; }
__device__ __forceinline__ int half_of(const uint32_t* d, int k) { return (d[k >> 1] >> (16 * (k & 1))) & 0xffff; }

// u8 BGR [h][w][3] -> planes.  yp: the Y plane; up / vp: U and V (yuv420p) or the interleaved plane and null (nv12, p010le).
template <int FMT, bool VEC>
__global__ __launch_bounds__(BX * BY) void pix_from_bgr(const uint8_t* __restrict__ bgr, uint8_t* __restrict__ yp, uint8_t* __restrict__ up,
                                                         uint8_t* __restrict__ vp, int h, int w, FwdCoef c)
{
    constexpr bool W16 = FMT == PIX_P010LE;
    const int x0 = (blockIdx.x * BX + threadIdx.x) * PX, gy = blockIdx.y * BY + threadIdx.y, y0 = 2 * gy;
    if (x0 >= w || y0 >= h) return;
    const int cw = (w + 1) >> 1;
    const bool whole = VEC && x0 + PX <= w && y0 + 2 <= h;
    int r[2][PX], g[2][PX], b[2][PX];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint8_t* row = bgr + ((size_t)(y0 + k) * w + x0) * 3;
        if (whole) {
            uint32_t d[6];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint2 v = reinterpret_cast<const uint2*>(row)[q];
                d[2 * q] = v.x; d[2 * q + 1] = v.y;
            }
#pragma unroll
            for (int i = 0; i < PX; ++i) { b[k][i] = byte_of(d, 3 * i); g[k][i] = byte_of(d, 3 * i + 1); r[k][i] = byte_of(d, 3 * i + 2); }
        } else {
#pragma unroll
            for (int i = 0; i < PX; ++i) {
                const bool in = y0 + k < h && x0 + i < w;
                b[k][i] = in ? row[3 * i] : 0; g[k][i] = in ? row[3 * i + 1] : 0; r[k][i] = in ? row[3 * i + 2] : 0;
            }
        }
    }
    // luma
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (y0 + k >= h) break;
        int yv[PX];
#pragma unroll
        for (int i = 0; i < PX; ++i)
            yv[i] = clampi((c.yr * r[k][i] + c.yg * g[k][i] + c.yb * b[k][i] + (c.yoff << 16) + 32768) >> 16, c.maxv);
        const size_t o = (size_t)(y0 + k) * w + x0;
        if (W16) {
            uint16_t* dst = reinterpret_cast<uint16_t*>(yp) + o;
            if (whole) {
                reinterpret_cast<uint4*>(dst)[0] = make_uint4(pack2(yv[0] << 6, yv[1] << 6), pack2(yv[2] << 6, yv[3] << 6),
                                                              pack2(yv[4] << 6, yv[5] << 6), pack2(yv[6] << 6, yv[7] << 6));
            } else {
#pragma unroll
                for (int i = 0; i < PX; ++i)
                    if (x0 + i < w) dst[i] = (uint16_t)(yv[i] << 6);
            }
        } else {
            uint8_t* dst = yp + o;
            if (whole) {
                reinterpret_cast<uint2*>(dst)[0] = make_uint2(pack4(yv[0], yv[1], yv[2], yv[3]), pack4(yv[4], yv[5], yv[6], yv[7]));
            } else {
#pragma unroll
                for (int i = 0; i < PX; ++i)
                    if (x0 + i < w) dst[i] = (uint8_t)yv[i];
            }
        }
    }
    // chroma: one sample per 2x2 block (2 or 1 pixels at an odd edge), from the block's sums; the division is in the shift
    const int rows = h - y0 < 2 ? 1 : 2;
    int cu[PX / 2], cv[PX / 2];
#pragma unroll
    for (int j = 0; j < PX / 2; ++j) {
        const int cols = w - (x0 + 2 * j) < 2 ? 1 : 2;
        int sr = 0, sg = 0, sb = 0;
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int i = 0; i < 2; ++i)
                if (k < rows && i < cols) { sr += r[k][2 * j + i]; sg += g[k][2 * j + i]; sb += b[k][2 * j + i]; }
        const int s = 16 + (rows - 1) + (cols - 1);
        cu[j] = clampi((c.ur * sr + c.ug * sg + c.ub * sb + (c.coff << s) + (1 << (s - 1))) >> s, c.maxv);
        cv[j] = clampi((c.vr * sr + c.vg * sg + c.vb * sb + (c.coff << s) + (1 << (s - 1))) >> s, c.maxv);
    }
    const int cx0 = x0 >> 1;
    if (FMT == PIX_YUV420P) {
        uint8_t* du = up + (size_t)gy * cw + cx0;
        uint8_t* dv = vp + (size_t)gy * cw + cx0;
        if (whole) {
            reinterpret_cast<uint32_t*>(du)[0] = pack4(cu[0], cu[1], cu[2], cu[3]);
            reinterpret_cast<uint32_t*>(dv)[0] = pack4(cv[0], cv[1], cv[2], cv[3]);
        } else {
#pragma unroll
            for (int j = 0; j < PX / 2; ++j)
                if (cx0 + j < cw) { du[j] = (uint8_t)cu[j]; dv[j] = (uint8_t)cv[j]; }
        }
    } else if (FMT == PIX_NV12) {
        uint8_t* d = up + (size_t)gy * 2 * cw + 2 * cx0;
        if (whole) {
            reinterpret_cast<uint2*>(d)[0] = make_uint2(pack4(cu[0], cv[0], cu[1], cv[1]), pack4(cu[2], cv[2], cu[3], cv[3]));
        } else {
#pragma unroll
            for (int j = 0; j < PX / 2; ++j)
                if (cx0 + j < cw) { d[2 * j] = (uint8_t)cu[j]; d[2 * j + 1] = (uint8_t)cv[j]; }
        }
    } else {
        uint16_t* d = reinterpret_cast<uint16_t*>(up) + (size_t)gy * 2 * cw + 2 * cx0;
        if (whole) {
            reinterpret_cast<uint4*>(d)[0] = make_uint4(pack2(cu[0] << 6, cv[0] << 6), pack2(cu[1] << 6, cv[1] << 6),
                                                        pack2(cu[2] << 6, cv[2] << 6), pack2(cu[3] << 6, cv[3] << 6));
        } else {
#pragma unroll
            for (int j = 0; j < PX / 2; ++j)
                if (cx0 + j < cw) { d[2 * j] = (uint16_t)(cu[j] << 6); d[2 * j + 1] = (uint16_t)(cv[j] << 6); }
        }
    }
}

// planes -> u8 BGR [h][w][3]; chroma replicated over its 2x2 block; p010le converts from the 10-bit values (word >> 6)
template <int FMT, bool VEC>
__global__ __launch_bounds__(BX * BY) void pix_to_bgr(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ up,
                                                       const uint8_t* __restrict__ vp, uint8_t* __restrict__ bgr, int h, int w, InvCoef c)
{
    constexpr bool W16 = FMT == PIX_P010LE;
    const int x0 = (blockIdx.x * BX + threadIdx.x) * PX, gy = blockIdx.y * BY + threadIdx.y, y0 = 2 * gy;
    if (x0 >= w || y0 >= h) return;
    const int cw = (w + 1) >> 1, cx0 = x0 >> 1;
    const bool whole = VEC && x0 + PX <= w && y0 + 2 <= h;
    int cu[PX / 2], cv[PX / 2];
    if (FMT == PIX_YUV420P) {
        const uint8_t* su = up + (size_t)gy * cw + cx0;
        const uint8_t* sv = vp + (size_t)gy * cw + cx0;
        if (whole) {
            const uint32_t du = reinterpret_cast<const uint32_t*>(su)[0], dv = reinterpret_cast<const uint32_t*>(sv)[0];
#pragma unroll
            for (int j = 0; j < PX / 2; ++j) { cu[j] = byte_of(&du, j); cv[j] = byte_of(&dv, j); }
        } else {
#pragma unroll
            for (int j = 0; j < PX / 2; ++j) {
                const bool in = cx0 + j < cw;
                cu[j] = in ? su[j] : 0; cv[j] = in ? sv[j] : 0;
            }
        }
    } else if (FMT == PIX_NV12) {
        const uint8_t* s = up + (size_t)gy * 2 * cw + 2 * cx0;
        if (whole) {
            const uint2 v = reinterpret_cast<const uint2*>(s)[0];
            const uint32_t d[2] = {v.x, v.y};
#pragma unroll
            for (int j = 0; j < PX / 2; ++j) { cu[j] = byte_of(d, 2 * j); cv[j] = byte_of(d, 2 * j + 1); }
        } else {
#pragma unroll
            for (int j = 0; j < PX / 2; ++j) {
                const bool in = cx0 + j < cw;
                cu[j] = in ? s[2 * j] : 0; cv[j] = in ? s[2 * j + 1] : 0;
            }
        }
    } else {
        const uint16_t* s = reinterpret_cast<const uint16_t*>(up) + (size_t)gy * 2 * cw + 2 * cx0;
        if (whole) {
            const uint4 v = reinterpret_cast<const uint4*>(s)[0];
            const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < PX / 2; ++j) { cu[j] = half_of(d, 2 * j) >> 6; cv[j] = half_of(d, 2 * j + 1) >> 6; }
        } else {
#pragma unroll
            for (int j = 0; j < PX / 2; ++j) {
                const bool in = cx0 + j < cw;
                cu[j] = in ? s[2 * j] >> 6 : 0; cv[j] = in ? s[2 * j + 1] >> 6 : 0;
            }
        }
    }
    // the chroma terms of a sample are shared by its block's pixels
    int tr[PX / 2], tg[PX / 2], tb[PX / 2];
#pragma unroll
    for (int j = 0; j < PX / 2; ++j) {
        const int u = cu[j] - c.coff, v = cv[j] - c.coff;
        tr[j] = c.rv * v + 32768;
        tg[j] = c.gu * u + c.gv * v + 32768;
        tb[j] = c.bu * u + 32768;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (y0 + k >= h) break;
        const size_t o = (size_t)(y0 + k) * w + x0;
        int yv[PX];
        if (W16) {
            const uint16_t* s = reinterpret_cast<const uint16_t*>(yp) + o;
            if (whole) {
                const uint4 v = reinterpret_cast<const uint4*>(s)[0];
                const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int i = 0; i < PX; ++i) yv[i] = half_of(d, i) >> 6;
            } else {
#pragma unroll
                for (int i = 0; i < PX; ++i) yv[i] = x0 + i < w ? s[i] >> 6 : 0;
            }
        } else {
            const uint8_t* s = yp + o;
            if (whole) {
                const uint2 v = reinterpret_cast<const uint2*>(s)[0];
                const uint32_t d[2] = {v.x, v.y};
#pragma unroll
                for (int i = 0; i < PX; ++i) yv[i] = byte_of(d, i);
            } else {
#pragma unroll
                for (int i = 0; i < PX; ++i) yv[i] = x0 + i < w ? s[i] : 0;
            }
        }
        int px[3 * PX];
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            const int yy = c.ky * (yv[i] - c.yoff);
            px[3 * i] = clampi((yy + tb[i >> 1]) >> 16, 255);
            px[3 * i + 1] = clampi((yy + tg[i >> 1]) >> 16, 255);
            px[3 * i + 2] = clampi((yy + tr[i >> 1]) >> 16, 255);
        }
        uint8_t* dst = bgr + o * 3;
        if (whole) {
#pragma unroll
            for (int q = 0; q < 3; ++q)
                reinterpret_cast<uint2*>(dst)[q] = make_uint2(pack4(px[8 * q], px[8 * q + 1], px[8 * q + 2], px[8 * q + 3]),
                                                              pack4(px[8 * q + 4], px[8 * q + 5], px[8 * q + 6], px[8 * q + 7]));
        } else {
#pragma unroll
            for (int i = 0; i < 3 * PX; ++i)
                if (x0 + i / 3 < w) dst[i] = (uint8_t)px[i];
        }
    }
}

// the planes of a frame of `fmt` at `base`
void planes(int fmt, const uint8_t* base, int h, int w, const uint8_t** yp, const uint8_t** up, const uint8_t** vp)
{
    const size_t cw = (size_t)(w + 1) / 2, ch = (size_t)(h + 1) / 2, wh = (size_t)w * h;
    *yp = base;
    if (fmt == PIX_YUV420P) { *up = base + wh; *vp = base + wh + cw * ch; }
    else if (fmt == PIX_NV12) { *up = base + wh; *vp = nullptr; }
    else { *up = base + 2 * wh; *vp = nullptr; }
}

// the wide accesses need w % 8 == 0 (every row, plane and chroma row then starts on a multiple of 8 pixels) and aligned bases
bool vec_ok(const void* a, const void* b, int w) { return w % PX == 0 && ((uintptr_t)a | (uintptr_t)b) % 16 == 0; }

dim3 grid_of(int h, int w) { return dim3((unsigned)((w + PX * BX - 1) / (PX * BX)), (unsigned)((h + 2 * BY - 1) / (2 * BY))); }

}  // namespace

size_t pix_frame_bytes(int fmt, int h, int w)
{
    if (h <= 0 || w <= 0) return 0;
    const size_t wh = (size_t)w * h, c = 2 * ((size_t)(w + 1) / 2) * ((size_t)(h + 1) / 2);
    switch (fmt) {
    case PIX_BGR24: return 3 * wh;
    case PIX_YUV420P: case PIX_NV12: return wh + c;
    case PIX_P010LE: return 2 * (wh + c);
    default: return 0;
    }
}

hipError_t launch_pix_from_bgr(hipStream_t stream, int fmt, int colour, const uint8_t* bgr, void* dst, int h, int w)
{
    if (h <= 0 || w <= 0 || (colour & ~PIX_COLOUR_MASK) || grid_of(h, w).y > 65535) return hipErrorInvalidValue;
    const uint8_t *yp, *up, *vp;
    planes(fmt, (const uint8_t*)dst, h, w, &yp, &up, &vp);
    const FwdCoef c = fwd_coef(colour, fmt == PIX_P010LE ? 10 : 8);
    const bool vec = vec_ok(bgr, dst, w);
    const dim3 grid = grid_of(h, w), block(BX, BY);
    uint8_t *y = const_cast<uint8_t*>(yp), *u = const_cast<uint8_t*>(up), *v = const_cast<uint8_t*>(vp);
#define UVA_PIX_LAUNCH(F)                                                                                                   \
    do {                                                                                                                    \
        if (vec) hipLaunchKernelGGL((pix_from_bgr<F, true>), grid, block, 0, stream, bgr, y, u, v, h, w, c);               \
        else hipLaunchKernelGGL((pix_from_bgr<F, false>), grid, block, 0, stream, bgr, y, u, v, h, w, c);                  \
    } while (0)
    switch (fmt) {
    case PIX_YUV420P: UVA_PIX_LAUNCH(PIX_YUV420P); break;
    case PIX_NV12: UVA_PIX_LAUNCH(PIX_NV12); break;
    case PIX_P010LE: UVA_PIX_LAUNCH(PIX_P010LE); break;
    default: return hipErrorInvalidValue;
    }
#undef UVA_PIX_LAUNCH
    return hipGetLastError();
}

hipError_t launch_pix_to_bgr(hipStream_t stream, int fmt, int colour, const void* src, uint8_t* bgr, int h, int w)
{
    if (h <= 0 || w <= 0 || (colour & ~PIX_COLOUR_MASK) || grid_of(h, w).y > 65535) return hipErrorInvalidValue;
    const uint8_t *y, *u, *v;
    planes(fmt, (const uint8_t*)src, h, w, &y, &u, &v);
    const InvCoef c = inv_coef(colour, fmt == PIX_P010LE ? 10 : 8);
    const bool vec = vec_ok(bgr, src, w);
    const dim3 grid = grid_of(h, w), block(BX, BY);
#define UVA_PIX_LAUNCH(F)                                                                                                   \
    do {                                                                                                                    \
        if (vec) hipLaunchKernelGGL((pix_to_bgr<F, true>), grid, block, 0, stream, y, u, v, bgr, h, w, c);                 \
        else hipLaunchKernelGGL((pix_to_bgr<F, false>), grid, block, 0, stream, y, u, v, bgr, h, w, c);                    \
    } while (0)
    switch (fmt) {
    case PIX_YUV420P: UVA_PIX_LAUNCH(PIX_YUV420P); break;
    case PIX_NV12: UVA_PIX_LAUNCH(PIX_NV12); break;
    case PIX_P010LE: UVA_PIX_LAUNCH(PIX_P010LE); break;
    default: return hipErrorInvalidValue;
    }
#undef UVA_PIX_LAUNCH
    return hipGetLastError();
}

}  // namespace uva
