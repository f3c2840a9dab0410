// uva_pixfmt.hip -- the raw-video route's colour conversions (csrc/uva_pixfmt.h; the arithmetic: DESIGN.md section 7.3), a
// translation unit of its own like uva_sww.hip.  Two kernel families, each instantiated per format:
//   pix_from_bgr  u8 BGR -> yuv420p / nv12 / p010le   (behind the net: its u8 result is what gets converted)
//   pix_to_bgr    yuv420p / nv12 / p010le -> u8 BGR   (in front of the net)
// (yuv420p10le: p010le's arithmetic in planar words, the value in the low 10 bits), and the 16-bit route's twins (section 7.4).
// Template parameter MODE picks the chroma resampling: 0 replicates / box-averages (sections 7.3, 7.4), 1..3 interpolate for
// chroma sited left, center or topleft (section 7.5).
// Both families are templated on the BGR sample type S: u8, or u16 (unorm16) for the 16-bit route (section 7.4).  Beside them
//   pix_widen / pix_narrow  u8 BGR <-> u16 BGR (v * 257, rint(v / 257))
// yuv422p / yuv422p10le (section 7.7) have twin kernels of their own, pix422_from_bgr / pix422_to_bgr, further down.
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

int fixs(double c, int sh) { return (int)std::floor(std::ldexp(c, sh) + 0.5); }

// The 16-bit route's shifts: u16 samples times round(c * 2^16) would overflow int32, so the forward
// coefficients are c * (code range / 65535) * 2^19 (a 2x2 chroma sum of 10-bit full range stays below 2^31) and the inverse
// ones c * (65535 / code range) * 2^13 (the largest |sum|, ~1.41e5 * 2^13, likewise)
constexpr int FWD16_SH = 19, INV16_SH = 13;

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

FwdCoef fwd_coef(int colour, int depth, bool u16 = false)
{
    double kr, kb;
    matrix(colour, kr, kb);
    const double kg = 1.0 - kr - kb;
    int ys, cs, yoff;
    ranges(colour, depth, ys, cs, yoff);
    const double vmax = u16 ? 65535.0 : 255.0;
    const int sh = u16 ? FWD16_SH : 16;
    const double sy = ys / vmax, sc = cs / vmax;
    FwdCoef c;
    c.yr = fixs(kr * sy, sh); c.yg = fixs(kg * sy, sh); c.yb = fixs(kb * sy, sh);
    c.ur = fixs(-kr / (2 * (1 - kb)) * sc, sh); c.ug = fixs(-kg / (2 * (1 - kb)) * sc, sh); c.ub = fixs(0.5 * sc, sh);
    c.vr = fixs(0.5 * sc, sh); c.vg = fixs(-kg / (2 * (1 - kr)) * sc, sh); c.vb = fixs(-kb / (2 * (1 - kr)) * sc, sh);
    c.yoff = yoff; c.coff = 1 << (depth - 1); c.maxv = (1 << depth) - 1;
    return c;
}

InvCoef inv_coef(int colour, int depth, bool u16 = false)
{
    double kr, kb;
    matrix(colour, kr, kb);
    const double kg = 1.0 - kr - kb;
    int ys, cs, yoff;
    ranges(colour, depth, ys, cs, yoff);
    const double vmax = u16 ? 65535.0 : 255.0;
    const int sh = u16 ? INV16_SH : 16;
    const double ky = vmax / ys, kc = vmax / cs;
    InvCoef c;
    c.ky = fixs(ky, sh);
    c.rv = fixs(2 * (1 - kr) * kc, sh);
    c.bu = fixs(2 * (1 - kb) * kc, sh);
    c.gu = fixs(-2 * kb * (1 - kb) / kg * kc, sh);
    c.gv = fixs(-2 * kr * (1 - kr) / kg * kc, sh);
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

// ---- the interpolating chroma modes ----------------------------------------------------------
// MODE 0: chroma replicated coming in, the 2x2 box going out (sections 7.3, 7.4).  MODE 1..3: bilinear for chroma sited
// `left` (horizontally on luma 2k, vertically midway), `center` (midway on both axes) or `topleft` (on luma 2k, 2k on both).
// A tap outside the plane takes the nearest sample inside.  The weights are integers over 2^DL; the division is in the
// final shift.  u8 sums stay in int32; u16 sums (section 7.4's scales times up to 16) are added in int64.
template <int MODE> struct Siting {
    static constexpr bool HCO = MODE == 1 || MODE == 3;      // horizontally co-sited
    static constexpr bool VCO = MODE == 3;                   // vertically co-sited
    static constexpr int DL = 4 - (HCO ? 1 : 0) - (VCO ? 1 : 0);       // coming in: 2 x 2, 2 x 4 or 4 x 4
    static constexpr int DLF = 2 + (HCO ? 1 : 0) + (VCO ? 1 : 0);      // going out: [1 1] or [1 2 1] per axis
};
template <typename S, int MODE> struct AccOf { typedef long long type; };
template <int MODE> struct AccOf<uint8_t, MODE> { typedef int type; };
template <typename S> struct AccOf<S, 0> { typedef int type; };

// one chroma sample pair at (cy, cx), both inside the plane
template <int FMT>
__device__ __forceinline__ void chroma_at(const uint8_t* __restrict__ up, const uint8_t* __restrict__ vp, int cy, int cx, int cw, int& u, int& v)
{
    const size_t o = (size_t)cy * cw + cx;
    if (FMT == PIX_YUV420P) { u = up[o]; v = vp[o]; }
    else if (FMT == PIX_YUV420P10LE) { u = reinterpret_cast<const uint16_t*>(up)[o] & 1023; v = reinterpret_cast<const uint16_t*>(vp)[o] & 1023; }
    else if (FMT == PIX_NV12) { u = up[2 * o]; v = up[2 * o + 1]; }
    else { u = reinterpret_cast<const uint16_t*>(up)[2 * o] >> 6; v = reinterpret_cast<const uint16_t*>(up)[2 * o + 1] >> 6; }
}

// chroma row cy, samples cx0 - 1 .. cx0 + 4 (clamped into the row) -> u[0..5], v[0..5]; `whole`: the middle four lie inside
// and aligned, and move as one access per plane
template <int FMT>
__device__ __forceinline__ void chroma_row6(const uint8_t* __restrict__ up, const uint8_t* __restrict__ vp, int cy, int cx0, int cw, bool whole,
                                            int* u, int* v)
{
    if (whole) {
        const size_t o = (size_t)cy * cw + cx0;
        if (FMT == PIX_YUV420P) {
            const uint32_t du = *reinterpret_cast<const uint32_t*>(up + o), dv = *reinterpret_cast<const uint32_t*>(vp + o);
#pragma unroll
            for (int j = 0; j < 4; ++j) { u[j + 1] = byte_of(&du, j); v[j + 1] = byte_of(&dv, j); }
        } else if (FMT == PIX_YUV420P10LE) {
            const uint2 vu = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(up) + o);
            const uint2 vv = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(vp) + o);
            const uint32_t du[2] = {vu.x, vu.y}, dv[2] = {vv.x, vv.y};
#pragma unroll
            for (int j = 0; j < 4; ++j) { u[j + 1] = half_of(du, j) & 1023; v[j + 1] = half_of(dv, j) & 1023; }
        } else if (FMT == PIX_NV12) {
            const uint2 q = *reinterpret_cast<const uint2*>(up + 2 * o);
            const uint32_t d[2] = {q.x, q.y};
#pragma unroll
            for (int j = 0; j < 4; ++j) { u[j + 1] = byte_of(d, 2 * j); v[j + 1] = byte_of(d, 2 * j + 1); }
        } else {
            const uint4 q = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(up) + 2 * o);
            const uint32_t d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) { u[j + 1] = half_of(d, 2 * j) >> 6; v[j + 1] = half_of(d, 2 * j + 1) >> 6; }
        }
        chroma_at<FMT>(up, vp, cy, max(cx0 - 1, 0), cw, u[0], v[0]);
        chroma_at<FMT>(up, vp, cy, min(cx0 + 4, cw - 1), cw, u[5], v[5]);
    } else {
#pragma unroll
        for (int j = 0; j < 6; ++j) chroma_at<FMT>(up, vp, cy, min(max(cx0 - 1 + j, 0), cw - 1), cw, u[j], v[j]);
    }
}

// BGR row `line`, pixels x0 - 1 .. x0 + 7 (clamped into the row) -> b[0..8], g[0..8], r[0..8]; `whole`: the last eight lie
// inside and aligned
template <typename S>
__device__ __forceinline__ void bgr_row9(const S* __restrict__ line, int x0, int w, bool whole, int* b, int* g, int* r)
{
    const S* l = line + 3 * (size_t)max(x0 - 1, 0);
    b[0] = l[0]; g[0] = l[1]; r[0] = l[2];
    if (whole) {
        const S* row = line + 3 * (size_t)x0;
        if constexpr (sizeof(S) == 1) {
            uint32_t d[6];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint2 v = reinterpret_cast<const uint2*>(row)[q];
                d[2 * q] = v.x; d[2 * q + 1] = v.y;
            }
#pragma unroll
            for (int i = 0; i < PX; ++i) { b[i + 1] = byte_of(d, 3 * i); g[i + 1] = byte_of(d, 3 * i + 1); r[i + 1] = byte_of(d, 3 * i + 2); }
        } else {
            uint32_t d[12];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint4 v = reinterpret_cast<const uint4*>(row)[q];
                d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int i = 0; i < PX; ++i) { b[i + 1] = half_of(d, 3 * i); g[i + 1] = half_of(d, 3 * i + 1); r[i + 1] = half_of(d, 3 * i + 2); }
        }
    } else {
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            const S* p = line + 3 * (size_t)min(x0 + i, w - 1);
            b[i + 1] = p[0]; g[i + 1] = p[1]; r[i + 1] = p[2];
        }
    }
}

// the horizontal filter going out, around chroma sample j of a thread: [1 2 1] on luma 2j (co-sited) or [1 1] on 2j, 2j + 1;
// p[0] is the pixel left of the thread's eight
template <bool HCO> __device__ __forceinline__ int hsum(const int* p, int j) { return HCO ? p[2 * j] + 2 * p[2 * j + 1] + p[2 * j + 2] : p[2 * j + 1] + p[2 * j + 2]; }

// BGR [h][w][3] of S (u8, or u16 for the 16-bit route) -> planes.  yp: the Y plane; up / vp: U and V (yuv420p, yuv420p10le) or
// the interleaved plane and null (nv12, p010le).
template <int FMT, bool VEC, typename S, int MODE = 0>
__global__ __launch_bounds__(BX * BY) void pix_from_bgr(const S* __restrict__ bgr, uint8_t* __restrict__ yp, uint8_t* __restrict__ up,
                                                         uint8_t* __restrict__ vp, int h, int w, FwdCoef c)
{
    constexpr bool W16 = FMT == PIX_P010LE || FMT == PIX_YUV420P10LE;
    constexpr int LS = FMT == PIX_P010LE ? 6 : 0;                 // where a 10-bit value sits in its word
    constexpr int SH = sizeof(S) == 1 ? 16 : FWD16_SH;
    const int x0 = (blockIdx.x * BX + threadIdx.x) * PX, gy = blockIdx.y * BY + threadIdx.y, y0 = 2 * gy;
    if (x0 >= w || y0 >= h) return;
    const int cw = (w + 1) >> 1;
    const bool whole = VEC && x0 + PX <= w && y0 + 2 <= h;
    int r[2][PX], g[2][PX], b[2][PX];
    int er[3][PX + 1], eg[3][PX + 1], eb[3][PX + 1];    // MODE != 0: rows y0 - 1, y0, y0 + 1, the pixel left of the eight in front
    if constexpr (MODE == 0) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const S* row = bgr + ((size_t)(y0 + k) * w + x0) * 3;
            if (whole) {
                if constexpr (sizeof(S) == 1) {
                    uint32_t d[6];
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const uint2 v = reinterpret_cast<const uint2*>(row)[q];
                        d[2 * q] = v.x; d[2 * q + 1] = v.y;
                    }
#pragma unroll
                    for (int i = 0; i < PX; ++i) { b[k][i] = byte_of(d, 3 * i); g[k][i] = byte_of(d, 3 * i + 1); r[k][i] = byte_of(d, 3 * i + 2); }
                } else {
                    uint32_t d[12];
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const uint4 v = reinterpret_cast<const uint4*>(row)[q];
                        d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
                    }
#pragma unroll
                    for (int i = 0; i < PX; ++i) { b[k][i] = half_of(d, 3 * i); g[k][i] = half_of(d, 3 * i + 1); r[k][i] = half_of(d, 3 * i + 2); }
                }
            } else {
#pragma unroll
                for (int i = 0; i < PX; ++i) {
                    const bool in = y0 + k < h && x0 + i < w;
                    b[k][i] = in ? row[3 * i] : 0; g[k][i] = in ? row[3 * i + 1] : 0; r[k][i] = in ? row[3 * i + 2] : 0;
                }
            }
        }
    } else {
#pragma unroll
        for (int k = Siting<MODE>::VCO ? 0 : 1; k < 3; ++k)
            bgr_row9<S>(bgr + (size_t)min(max(y0 - 1 + k, 0), h - 1) * w * 3, x0, w, whole, eb[k], eg[k], er[k]);
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int i = 0; i < PX; ++i) { b[k][i] = eb[k + 1][i + 1]; g[k][i] = eg[k + 1][i + 1]; r[k][i] = er[k + 1][i + 1]; }
    }
    // luma
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (y0 + k >= h) break;
        int yv[PX];
#pragma unroll
        for (int i = 0; i < PX; ++i)
            yv[i] = clampi((c.yr * r[k][i] + c.yg * g[k][i] + c.yb * b[k][i] + (c.yoff << SH) + (1 << (SH - 1))) >> SH, c.maxv);
        const size_t o = (size_t)(y0 + k) * w + x0;
        if (W16) {
            uint16_t* dst = reinterpret_cast<uint16_t*>(yp) + o;
            if (whole) {
                reinterpret_cast<uint4*>(dst)[0] = make_uint4(pack2(yv[0] << LS, yv[1] << LS), pack2(yv[2] << LS, yv[3] << LS),
                                                              pack2(yv[4] << LS, yv[5] << LS), pack2(yv[6] << LS, yv[7] << LS));
            } else {
#pragma unroll
                for (int i = 0; i < PX; ++i)
                    if (x0 + i < w) dst[i] = (uint16_t)(yv[i] << LS);
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
    int cu[PX / 2], cv[PX / 2];
    if constexpr (MODE == 0) {
        const int rows = h - y0 < 2 ? 1 : 2;
#pragma unroll
        for (int j = 0; j < PX / 2; ++j) {
            const int cols = w - (x0 + 2 * j) < 2 ? 1 : 2;
            int sr = 0, sg = 0, sb = 0;
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    if (k < rows && i < cols) { sr += r[k][2 * j + i]; sg += g[k][2 * j + i]; sb += b[k][2 * j + i]; }
            const int s = SH + (rows - 1) + (cols - 1);
            cu[j] = clampi((c.ur * sr + c.ug * sg + c.ub * sb + (c.coff << s) + (1 << (s - 1))) >> s, c.maxv);
            cv[j] = clampi((c.vr * sr + c.vg * sg + c.vb * sb + (c.coff << s) + (1 << (s - 1))) >> s, c.maxv);
        }
    } else {
        // section 7.5: the weighted sums of R, G, B over the siting's window (3x2, 2x2 or 3x3), the weights' 2^DLF in the shift
        typedef typename AccOf<S, MODE>::type Acc;
        constexpr bool HCO = Siting<MODE>::HCO, VCO = Siting<MODE>::VCO;
        constexpr int s = SH + Siting<MODE>::DLF;
#pragma unroll
        for (int j = 0; j < PX / 2; ++j) {
            int sr = hsum<HCO>(er[1], j) + hsum<HCO>(er[2], j), sg = hsum<HCO>(eg[1], j) + hsum<HCO>(eg[2], j),
                sb = hsum<HCO>(eb[1], j) + hsum<HCO>(eb[2], j);
            if (VCO) {
                sr += hsum<HCO>(er[0], j) + hsum<HCO>(er[1], j); sg += hsum<HCO>(eg[0], j) + hsum<HCO>(eg[1], j);
                sb += hsum<HCO>(eb[0], j) + hsum<HCO>(eb[1], j);
            }
            cu[j] = clampi((int)(((Acc)c.ur * sr + (Acc)c.ug * sg + (Acc)c.ub * sb + ((Acc)c.coff << s) + ((Acc)1 << (s - 1))) >> s), c.maxv);
            cv[j] = clampi((int)(((Acc)c.vr * sr + (Acc)c.vg * sg + (Acc)c.vb * sb + ((Acc)c.coff << s) + ((Acc)1 << (s - 1))) >> s), c.maxv);
        }
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
    } else if (FMT == PIX_YUV420P10LE) {
        uint16_t* du = reinterpret_cast<uint16_t*>(up) + (size_t)gy * cw + cx0;
        uint16_t* dv = reinterpret_cast<uint16_t*>(vp) + (size_t)gy * cw + cx0;
        if (whole) {
            reinterpret_cast<uint2*>(du)[0] = make_uint2(pack2(cu[0], cu[1]), pack2(cu[2], cu[3]));
            reinterpret_cast<uint2*>(dv)[0] = make_uint2(pack2(cv[0], cv[1]), pack2(cv[2], cv[3]));
        } else {
#pragma unroll
            for (int j = 0; j < PX / 2; ++j)
                if (cx0 + j < cw) { du[j] = (uint16_t)cu[j]; dv[j] = (uint16_t)cv[j]; }
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

// planes -> BGR [h][w][3] of S; chroma replicated over its 2x2 block (MODE 0) or interpolated (MODE 1..3); p010le converts from the 10-bit values (word >> 6),
// yuv420p10le from the low 10 bits of its words
template <int FMT, bool VEC, typename S, int MODE = 0>
__global__ __launch_bounds__(BX * BY) void pix_to_bgr(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ up,
                                                       const uint8_t* __restrict__ vp, S* __restrict__ bgr, int h, int w, InvCoef c)
{
    constexpr bool W16 = FMT == PIX_P010LE || FMT == PIX_YUV420P10LE;
    constexpr int SH = sizeof(S) == 1 ? 16 : INV16_SH;
    constexpr int VMAX = sizeof(S) == 1 ? 255 : 65535;
    const int x0 = (blockIdx.x * BX + threadIdx.x) * PX, gy = blockIdx.y * BY + threadIdx.y, y0 = 2 * gy;
    if (x0 >= w || y0 >= h) return;
    const int cw = (w + 1) >> 1, cx0 = x0 >> 1;
    const bool whole = VEC && x0 + PX <= w && y0 + 2 <= h;
    int cu[PX / 2], cv[PX / 2];
    int tr[PX / 2], tg[PX / 2], tb[PX / 2];
    int nu[3][PX / 2 + 2], nv[3][PX / 2 + 2];      // MODE != 0: chroma rows gy - 1, gy, gy + 1, samples cx0 - 1 .. cx0 + 4
    if constexpr (MODE == 0) {
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
        } else if (FMT == PIX_YUV420P10LE) {
            const uint16_t* su = reinterpret_cast<const uint16_t*>(up) + (size_t)gy * cw + cx0;
            const uint16_t* sv = reinterpret_cast<const uint16_t*>(vp) + (size_t)gy * cw + cx0;
            if (whole) {
                const uint2 vu = reinterpret_cast<const uint2*>(su)[0], vv = reinterpret_cast<const uint2*>(sv)[0];
                const uint32_t du[2] = {vu.x, vu.y}, dv[2] = {vv.x, vv.y};
#pragma unroll
                for (int j = 0; j < PX / 2; ++j) { cu[j] = half_of(du, j) & 1023; cv[j] = half_of(dv, j) & 1023; }
            } else {
#pragma unroll
                for (int j = 0; j < PX / 2; ++j) {
                    const bool in = cx0 + j < cw;
                    cu[j] = in ? su[j] & 1023 : 0; cv[j] = in ? sv[j] & 1023 : 0;
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
#pragma unroll
        for (int j = 0; j < PX / 2; ++j) {
            const int u = cu[j] - c.coff, v = cv[j] - c.coff;
            tr[j] = c.rv * v + (1 << (SH - 1));
            tg[j] = c.gu * u + c.gv * v + (1 << (SH - 1));
            tb[j] = c.bu * u + (1 << (SH - 1));
        }
    } else {
        const int ch = (h + 1) >> 1;
#pragma unroll
        for (int k = Siting<MODE>::VCO ? 1 : 0; k < 3; ++k)
            chroma_row6<FMT>(up, vp, min(max(gy - 1 + k, 0), ch - 1), cx0, cw, whole, nu[k], nv[k]);
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
                for (int i = 0; i < PX; ++i) yv[i] = FMT == PIX_P010LE ? half_of(d, i) >> 6 : half_of(d, i) & 1023;
            } else {
#pragma unroll
                for (int i = 0; i < PX; ++i) {
                    if (FMT == PIX_P010LE) yv[i] = x0 + i < w ? s[i] >> 6 : 0;
                    else yv[i] = x0 + i < w ? s[i] & 1023 : 0;
                }
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
        if constexpr (MODE == 0) {
#pragma unroll
            for (int i = 0; i < PX; ++i) {
                const int yy = c.ky * (yv[i] - c.yoff);
                px[3 * i] = clampi((yy + tb[i >> 1]) >> SH, VMAX);
                px[3 * i + 1] = clampi((yy + tg[i >> 1]) >> SH, VMAX);
                px[3 * i + 2] = clampi((yy + tr[i >> 1]) >> SH, VMAX);
            }
        } else {
            // section 7.5: the two axes' integer weights multiplied out, over 2^DL; the sum goes into the matrix unrounded
            typedef typename AccOf<S, MODE>::type Acc;
            constexpr bool HCO = Siting<MODE>::HCO, VCO = Siting<MODE>::VCO;
            constexpr int DL = Siting<MODE>::DL, s = SH + DL;
            int vu[PX / 2 + 2], vv[PX / 2 + 2];     // this luma row's vertical sums
#pragma unroll
            for (int j = 0; j < PX / 2 + 2; ++j) {
                if (VCO) {
                    vu[j] = k == 0 ? 2 * nu[1][j] : nu[1][j] + nu[2][j];
                    vv[j] = k == 0 ? 2 * nv[1][j] : nv[1][j] + nv[2][j];
                } else {
                    vu[j] = k == 0 ? nu[0][j] + 3 * nu[1][j] : 3 * nu[1][j] + nu[2][j];
                    vv[j] = k == 0 ? nv[0][j] + 3 * nv[1][j] : 3 * nv[1][j] + nv[2][j];
                }
            }
#pragma unroll
            for (int i = 0; i < PX; ++i) {
                const int j = (i >> 1) + 1;
                int u, v;
                if (HCO) {
                    u = i & 1 ? vu[j] + vu[j + 1] : 2 * vu[j];
                    v = i & 1 ? vv[j] + vv[j + 1] : 2 * vv[j];
                } else {
                    u = i & 1 ? 3 * vu[j] + vu[j + 1] : vu[j - 1] + 3 * vu[j];
                    v = i & 1 ? 3 * vv[j] + vv[j + 1] : vv[j - 1] + 3 * vv[j];
                }
                u -= c.coff << DL; v -= c.coff << DL;
                const Acc yy = (Acc)(c.ky * (yv[i] - c.yoff)) * (1 << DL) + ((Acc)1 << (s - 1));
                px[3 * i] = clampi((int)((yy + (Acc)c.bu * u) >> s), VMAX);
                px[3 * i + 1] = clampi((int)((yy + (Acc)c.gu * u + (Acc)c.gv * v) >> s), VMAX);
                px[3 * i + 2] = clampi((int)((yy + (Acc)c.rv * v) >> s), VMAX);
            }
        }
        S* dst = bgr + o * 3;
        if (whole) {
            if constexpr (sizeof(S) == 1) {
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    reinterpret_cast<uint2*>(dst)[q] = make_uint2(pack4(px[8 * q], px[8 * q + 1], px[8 * q + 2], px[8 * q + 3]),
                                                                  pack4(px[8 * q + 4], px[8 * q + 5], px[8 * q + 6], px[8 * q + 7]));
            } else {
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    reinterpret_cast<uint4*>(dst)[q] = make_uint4(pack2(px[8 * q], px[8 * q + 1]), pack2(px[8 * q + 2], px[8 * q + 3]),
                                                                  pack2(px[8 * q + 4], px[8 * q + 5]), pack2(px[8 * q + 6], px[8 * q + 7]));
            }
        } else {
#pragma unroll
            for (int i = 0; i < 3 * PX; ++i)
                if (x0 + i / 3 < w) dst[i] = (S)px[i];
        }
    }
}

// ---- 4:2:2: yuv422p, yuv422p10le ---------------------------------------------------------------
// One chroma row per luma row, so the vertical axis is the identity and a thread covers 8 pixels of ONE row: 8 luma and 4
// chroma samples per plane, every one read or written once.  HM is the horizontal chroma mode: 0 replicates / averages the
// pair, 1 is co-sited (`left` and `topleft`: the same bytes), 2 centred.  W16: the planes hold 16-bit words, the 10-bit value
// in the low bits.  Fixed point and coefficients are sections 7.3 / 7.4's; the interpolating modes' sums go unrounded into
// the matrix (section 7.5).  int32 everywhere but the u16 inverse of HM 1 / 2, whose sums (section 7.4's 2^13 scale times 2
// or 4) need int64; the u16 forward sums are at most section 7.4's 2x2 sum, which its 2^19 scale was sized for.
template <typename S, int HM> struct Acc422 { typedef int type; };
template <> struct Acc422<uint16_t, 1> { typedef long long type; };
template <> struct Acc422<uint16_t, 2> { typedef long long type; };

// BGR row `line`, pixels x0 .. x0 + 7 (clamped into the row) -> b[1..8], g[1..8], r[1..8]; LEFT: pixel x0 - 1 (clamped) -> [0]
template <typename S, bool LEFT>
__device__ __forceinline__ void bgr422_row(const S* __restrict__ line, int x0, int w, bool whole, int* b, int* g, int* r)
{
    if (LEFT) {
        const S* l = line + 3 * (size_t)max(x0 - 1, 0);
        b[0] = l[0]; g[0] = l[1]; r[0] = l[2];
    }
    if (whole) {
        const S* row = line + 3 * (size_t)x0;
        if constexpr (sizeof(S) == 1) {
            uint32_t d[6];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint2 v = reinterpret_cast<const uint2*>(row)[q];
                d[2 * q] = v.x; d[2 * q + 1] = v.y;
            }
#pragma unroll
            for (int i = 0; i < PX; ++i) { b[i + 1] = byte_of(d, 3 * i); g[i + 1] = byte_of(d, 3 * i + 1); r[i + 1] = byte_of(d, 3 * i + 2); }
        } else {
            uint32_t d[12];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint4 v = reinterpret_cast<const uint4*>(row)[q];
                d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int i = 0; i < PX; ++i) { b[i + 1] = half_of(d, 3 * i); g[i + 1] = half_of(d, 3 * i + 1); r[i + 1] = half_of(d, 3 * i + 2); }
        }
    } else {
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            const S* p = line + 3 * (size_t)min(x0 + i, w - 1);
            b[i + 1] = p[0]; g[i + 1] = p[1]; r[i + 1] = p[2];
        }
    }
}

// BGR [h][w][3] of S -> Y [h][w], U [h][cw], V [h][cw]
template <bool W16, bool VEC, typename S, int HM>
__global__ __launch_bounds__(BX * BY) void pix422_from_bgr(const S* __restrict__ bgr, uint8_t* __restrict__ yp, uint8_t* __restrict__ up,
                                                            uint8_t* __restrict__ vp, int h, int w, FwdCoef c)
{
    constexpr int SH = sizeof(S) == 1 ? 16 : FWD16_SH;
    const int x0 = (blockIdx.x * BX + threadIdx.x) * PX, y = blockIdx.y * BY + threadIdx.y;
    if (x0 >= w || y >= h) return;
    const int cw = (w + 1) >> 1, cx0 = x0 >> 1;
    const bool whole = VEC && x0 + PX <= w;
    int r[PX + 1], g[PX + 1], b[PX + 1];        // [0]: the pixel left of the eight (HM 1 alone)
    bgr422_row<S, HM == 1>(bgr + (size_t)y * w * 3, x0, w, whole, b, g, r);
    int yv[PX];
#pragma unroll
    for (int i = 0; i < PX; ++i)
        yv[i] = clampi((c.yr * r[i + 1] + c.yg * g[i + 1] + c.yb * b[i + 1] + (c.yoff << SH) + (1 << (SH - 1))) >> SH, c.maxv);
    const size_t o = (size_t)y * w + x0;
    if (W16) {
        uint16_t* dst = reinterpret_cast<uint16_t*>(yp) + o;
        if (whole) {
            reinterpret_cast<uint4*>(dst)[0] = make_uint4(pack2(yv[0], yv[1]), pack2(yv[2], yv[3]), pack2(yv[4], yv[5]), pack2(yv[6], yv[7]));
        } else {
#pragma unroll
            for (int i = 0; i < PX; ++i)
                if (x0 + i < w) dst[i] = (uint16_t)yv[i];
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
    // chroma sample j from pixels 2j, 2j + 1 (HM 0: one pixel at an odd right edge; HM 2: [1 1]) or 2j - 1, 2j, 2j + 1 ([1 2 1])
    int cu[PX / 2], cv[PX / 2];
#pragma unroll
    for (int j = 0; j < PX / 2; ++j) {
        int sr, sg, sb, s;
        if (HM == 1) {
            sr = r[2 * j] + 2 * r[2 * j + 1] + r[2 * j + 2]; sg = g[2 * j] + 2 * g[2 * j + 1] + g[2 * j + 2];
            sb = b[2 * j] + 2 * b[2 * j + 1] + b[2 * j + 2];
            s = SH + 2;
        } else if (HM == 2) {
            sr = r[2 * j + 1] + r[2 * j + 2]; sg = g[2 * j + 1] + g[2 * j + 2]; sb = b[2 * j + 1] + b[2 * j + 2];
            s = SH + 1;
        } else {
            const bool two = x0 + 2 * j + 1 < w;
            sr = r[2 * j + 1] + (two ? r[2 * j + 2] : 0); sg = g[2 * j + 1] + (two ? g[2 * j + 2] : 0);
            sb = b[2 * j + 1] + (two ? b[2 * j + 2] : 0);
            s = SH + (two ? 1 : 0);
        }
        cu[j] = clampi((c.ur * sr + c.ug * sg + c.ub * sb + (c.coff << s) + (1 << (s - 1))) >> s, c.maxv);
        cv[j] = clampi((c.vr * sr + c.vg * sg + c.vb * sb + (c.coff << s) + (1 << (s - 1))) >> s, c.maxv);
    }
    const size_t co = (size_t)y * cw + cx0;
    if (W16) {
        uint16_t* du = reinterpret_cast<uint16_t*>(up) + co;
        uint16_t* dv = reinterpret_cast<uint16_t*>(vp) + co;
        if (whole) {
            reinterpret_cast<uint2*>(du)[0] = make_uint2(pack2(cu[0], cu[1]), pack2(cu[2], cu[3]));
            reinterpret_cast<uint2*>(dv)[0] = make_uint2(pack2(cv[0], cv[1]), pack2(cv[2], cv[3]));
        } else {
#pragma unroll
            for (int j = 0; j < PX / 2; ++j)
                if (cx0 + j < cw) { du[j] = (uint16_t)cu[j]; dv[j] = (uint16_t)cv[j]; }
        }
    } else {
        uint8_t* du = up + co;
        uint8_t* dv = vp + co;
        if (whole) {
            reinterpret_cast<uint32_t*>(du)[0] = pack4(cu[0], cu[1], cu[2], cu[3]);
            reinterpret_cast<uint32_t*>(dv)[0] = pack4(cv[0], cv[1], cv[2], cv[3]);
        } else {
#pragma unroll
            for (int j = 0; j < PX / 2; ++j)
                if (cx0 + j < cw) { du[j] = (uint8_t)cu[j]; dv[j] = (uint8_t)cv[j]; }
        }
    }
}

// one sample of a chroma plane row (cx inside the row)
template <bool W16> __device__ __forceinline__ int chroma422_at(const uint8_t* __restrict__ row, int cx)
{
    return W16 ? reinterpret_cast<const uint16_t*>(row)[cx] & 1023 : row[cx];
}

// Y [h][w], U [h][cw], V [h][cw] -> BGR [h][w][3] of S
template <bool W16, bool VEC, typename S, int HM>
__global__ __launch_bounds__(BX * BY) void pix422_to_bgr(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ up,
                                                          const uint8_t* __restrict__ vp, S* __restrict__ bgr, int h, int w, InvCoef c)
{
    constexpr int SH = sizeof(S) == 1 ? 16 : INV16_SH;
    constexpr int VMAX = sizeof(S) == 1 ? 255 : 65535;
    const int x0 = (blockIdx.x * BX + threadIdx.x) * PX, y = blockIdx.y * BY + threadIdx.y;
    if (x0 >= w || y >= h) return;
    const int cw = (w + 1) >> 1, cx0 = x0 >> 1;
    const bool whole = VEC && x0 + PX <= w;
    // chroma samples cx0 .. cx0 + 3 -> [1..4] (clamped into the row); the neighbours the mode taps, each one clamped load:
    // cx0 - 1 -> [0] (HM 2), cx0 + 4 -> [5] (HM 1, 2)
    int nu[PX / 2 + 2], nv[PX / 2 + 2];
    const uint8_t* ur = up + (size_t)y * cw * (W16 ? 2 : 1);
    const uint8_t* vr = vp + (size_t)y * cw * (W16 ? 2 : 1);
    if (whole) {
        if (W16) {
            const uint2 qu = *reinterpret_cast<const uint2*>(ur + 2 * cx0), qv = *reinterpret_cast<const uint2*>(vr + 2 * cx0);
            const uint32_t du[2] = {qu.x, qu.y}, dv[2] = {qv.x, qv.y};
#pragma unroll
            for (int j = 0; j < PX / 2; ++j) { nu[j + 1] = half_of(du, j) & 1023; nv[j + 1] = half_of(dv, j) & 1023; }
        } else {
            const uint32_t du = *reinterpret_cast<const uint32_t*>(ur + cx0), dv = *reinterpret_cast<const uint32_t*>(vr + cx0);
#pragma unroll
            for (int j = 0; j < PX / 2; ++j) { nu[j + 1] = byte_of(&du, j); nv[j + 1] = byte_of(&dv, j); }
        }
    } else {
#pragma unroll
        for (int j = 0; j < PX / 2; ++j) {
            const int cx = min(cx0 + j, cw - 1);
            nu[j + 1] = chroma422_at<W16>(ur, cx); nv[j + 1] = chroma422_at<W16>(vr, cx);
        }
    }
    if (HM == 2) { const int cx = max(cx0 - 1, 0); nu[0] = chroma422_at<W16>(ur, cx); nv[0] = chroma422_at<W16>(vr, cx); }
    if (HM != 0) { const int cx = min(cx0 + PX / 2, cw - 1); nu[PX / 2 + 1] = chroma422_at<W16>(ur, cx); nv[PX / 2 + 1] = chroma422_at<W16>(vr, cx); }
    const size_t o = (size_t)y * w + x0;
    int yv[PX];
    if (W16) {
        const uint16_t* s = reinterpret_cast<const uint16_t*>(yp) + o;
        if (whole) {
            const uint4 v = reinterpret_cast<const uint4*>(s)[0];
            const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < PX; ++i) yv[i] = half_of(d, i) & 1023;
        } else {
#pragma unroll
            for (int i = 0; i < PX; ++i) yv[i] = x0 + i < w ? s[i] & 1023 : 0;
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
    if constexpr (HM == 0) {
        // the chroma terms of a sample are shared by its two pixels
#pragma unroll
        for (int j = 0; j < PX / 2; ++j) {
            const int u = nu[j + 1] - c.coff, v = nv[j + 1] - c.coff;
            const int tr = c.rv * v + (1 << (SH - 1)), tg = c.gu * u + c.gv * v + (1 << (SH - 1)), tb = c.bu * u + (1 << (SH - 1));
#pragma unroll
            for (int i = 2 * j; i < 2 * j + 2; ++i) {
                const int yy = c.ky * (yv[i] - c.yoff);
                px[3 * i] = clampi((yy + tb) >> SH, VMAX);
                px[3 * i + 1] = clampi((yy + tg) >> SH, VMAX);
                px[3 * i + 2] = clampi((yy + tr) >> SH, VMAX);
            }
        }
    } else {
        typedef typename Acc422<S, HM>::type Acc;
        constexpr int DL = HM == 1 ? 1 : 2, s = SH + DL;
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            const int j = (i >> 1) + 1;
            int u, v;
            if (HM == 1) {
                u = i & 1 ? nu[j] + nu[j + 1] : 2 * nu[j];
                v = i & 1 ? nv[j] + nv[j + 1] : 2 * nv[j];
            } else {
                u = i & 1 ? 3 * nu[j] + nu[j + 1] : nu[j - 1] + 3 * nu[j];
                v = i & 1 ? 3 * nv[j] + nv[j + 1] : nv[j - 1] + 3 * nv[j];
            }
            u -= c.coff << DL; v -= c.coff << DL;
            const Acc yy = (Acc)(c.ky * (yv[i] - c.yoff)) * (1 << DL) + ((Acc)1 << (s - 1));
            px[3 * i] = clampi((int)((yy + (Acc)c.bu * u) >> s), VMAX);
            px[3 * i + 1] = clampi((int)((yy + (Acc)c.gu * u + (Acc)c.gv * v) >> s), VMAX);
            px[3 * i + 2] = clampi((int)((yy + (Acc)c.rv * v) >> s), VMAX);
        }
    }
    S* dst = bgr + o * 3;
    if (whole) {
        if constexpr (sizeof(S) == 1) {
#pragma unroll
            for (int q = 0; q < 3; ++q)
                reinterpret_cast<uint2*>(dst)[q] = make_uint2(pack4(px[8 * q], px[8 * q + 1], px[8 * q + 2], px[8 * q + 3]),
                                                              pack4(px[8 * q + 4], px[8 * q + 5], px[8 * q + 6], px[8 * q + 7]));
        } else {
#pragma unroll
            for (int q = 0; q < 3; ++q)
                reinterpret_cast<uint4*>(dst)[q] = make_uint4(pack2(px[8 * q], px[8 * q + 1]), pack2(px[8 * q + 2], px[8 * q + 3]),
                                                              pack2(px[8 * q + 4], px[8 * q + 5]), pack2(px[8 * q + 6], px[8 * q + 7]));
        }
    } else {
#pragma unroll
        for (int i = 0; i < 3 * PX; ++i)
            if (x0 + i / 3 < w) dst[i] = (S)px[i];
    }
}

// u8 BGR <-> u16 BGR, 8 samples per thread: v * 257 is exact (v / 255 = 257 v / 65535); rint(v / 257) never meets a tie (257 is
// odd), so it is floor((v + 128) / 257)
constexpr int WN = 8;
template <bool VEC>
__global__ __launch_bounds__(256) void pix_widen(const uint8_t* __restrict__ src, uint16_t* __restrict__ dst, size_t n)
{
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * WN;
    if (i0 >= n) return;
    if (VEC && i0 + WN <= n) {
        const uint2 v = *reinterpret_cast<const uint2*>(src + i0);
        const uint32_t d[2] = {v.x, v.y};
        *reinterpret_cast<uint4*>(dst + i0) = make_uint4(pack2(byte_of(d, 0) * 257, byte_of(d, 1) * 257), pack2(byte_of(d, 2) * 257, byte_of(d, 3) * 257),
                                                         pack2(byte_of(d, 4) * 257, byte_of(d, 5) * 257), pack2(byte_of(d, 6) * 257, byte_of(d, 7) * 257));
    } else {
        for (size_t i = i0; i < n && i < i0 + WN; ++i) dst[i] = (uint16_t)(src[i] * 257);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void pix_narrow(const uint16_t* __restrict__ src, uint8_t* __restrict__ dst, size_t n)
{
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * WN;
    if (i0 >= n) return;
    auto nar = [](int v) __attribute__((always_inline)) { return (v + 128) / 257; };
    if (VEC && i0 + WN <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(src + i0);
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
        *reinterpret_cast<uint2*>(dst + i0) = make_uint2(pack4(nar(half_of(d, 0)), nar(half_of(d, 1)), nar(half_of(d, 2)), nar(half_of(d, 3))),
                                                         pack4(nar(half_of(d, 4)), nar(half_of(d, 5)), nar(half_of(d, 6)), nar(half_of(d, 7))));
    } else {
        for (size_t i = i0; i < n && i < i0 + WN; ++i) dst[i] = (uint8_t)nar(src[i]);
    }
}

// the planes of a frame of `fmt` at `base`
void planes(int fmt, const uint8_t* base, int h, int w, const uint8_t** yp, const uint8_t** up, const uint8_t** vp)
{
    const size_t cw = (size_t)(w + 1) / 2, ch = (size_t)(h + 1) / 2, wh = (size_t)w * h;
    *yp = base;
    if (fmt == PIX_YUV420P) { *up = base + wh; *vp = base + wh + cw * ch; }
    else if (fmt == PIX_YUV420P10LE) { *up = base + 2 * wh; *vp = base + 2 * (wh + cw * ch); }
    else if (fmt == PIX_NV12) { *up = base + wh; *vp = nullptr; }
    else if (fmt == PIX_YUV422P) { *up = base + wh; *vp = base + wh + cw * h; }
    else if (fmt == PIX_YUV422P10LE) { *up = base + 2 * wh; *vp = base + 2 * (wh + cw * h); }
    else { *up = base + 2 * wh; *vp = nullptr; }
}

// the wide accesses need w % 8 == 0 (every row, plane and chroma row then starts on a multiple of 8 pixels) and aligned bases
bool vec_ok(const void* a, const void* b, int w) { return w % PX == 0 && ((uintptr_t)a | (uintptr_t)b) % 16 == 0; }

dim3 grid_of(int h, int w) { return dim3((unsigned)((w + PX * BX - 1) / (PX * BX)), (unsigned)((h + 2 * BY - 1) / (2 * BY))); }

// 4:2:2: a thread's 4 chroma samples move as one access of 4 bytes (8 bits) or 8 (10 bits), so the U and V planes -- w h and
// w h + cw h samples into the frame -- must start on such a multiple as well; a row of threads covers one row
bool is422(int fmt) { return fmt == PIX_YUV422P || fmt == PIX_YUV422P10LE; }
bool vec422_ok(const void* bgr, const void* frame, const uint8_t* up, const uint8_t* vp, int w, int fmt)
{
    const uintptr_t ca = fmt == PIX_YUV422P10LE ? 8 : 4;
    return vec_ok(bgr, frame, w) && ((uintptr_t)up | (uintptr_t)vp) % ca == 0;
}
dim3 grid422_of(int h, int w) { return dim3((unsigned)((w + PX * BX - 1) / (PX * BX)), (unsigned)((h + BY - 1) / BY)); }

}  // namespace

namespace {
int depth_of(int fmt) { return fmt == PIX_P010LE || fmt == PIX_YUV420P10LE || fmt == PIX_YUV422P10LE ? 10 : 8; }

// pix_chroma_mode -> the 4:2:2 kernels' horizontal mode: left and topleft are both co-sited on this axis
int hmode422(int colour) { const int m = pix_chroma_mode(colour); return m == 0 ? 0 : (m == 2 ? 2 : 1); }

template <typename S>
hipError_t from_bgr422(hipStream_t stream, int fmt, int colour, const S* bgr, void* dst, int h, int w)
{
    if (grid422_of(h, w).y > 65535) return hipErrorInvalidValue;
    const uint8_t *yp, *up, *vp;
    planes(fmt, (const uint8_t*)dst, h, w, &yp, &up, &vp);
    const FwdCoef c = fwd_coef(colour, depth_of(fmt), sizeof(S) == 2);
    const bool vec = vec422_ok(bgr, dst, up, vp, w, fmt);
    const dim3 grid = grid422_of(h, w), block(BX, BY);
    uint8_t *y = const_cast<uint8_t*>(yp), *u = const_cast<uint8_t*>(up), *v = const_cast<uint8_t*>(vp);
#define UVA_PIX422_LAUNCH_M(W16, M)                                                                                         \
    do {                                                                                                                    \
        if (vec) hipLaunchKernelGGL((pix422_from_bgr<W16, true, S, M>), grid, block, 0, stream, bgr, y, u, v, h, w, c);    \
        else hipLaunchKernelGGL((pix422_from_bgr<W16, false, S, M>), grid, block, 0, stream, bgr, y, u, v, h, w, c);       \
    } while (0)
#define UVA_PIX422_LAUNCH(W16)                                                                                              \
    do {                                                                                                                    \
        switch (hmode422(colour)) {                                                                                         \
        case 0: UVA_PIX422_LAUNCH_M(W16, 0); break;                                                                         \
        case 1: UVA_PIX422_LAUNCH_M(W16, 1); break;                                                                         \
        default: UVA_PIX422_LAUNCH_M(W16, 2); break;                                                                        \
        }                                                                                                                   \
    } while (0)
    if (fmt == PIX_YUV422P10LE) UVA_PIX422_LAUNCH(true);
    else UVA_PIX422_LAUNCH(false);
#undef UVA_PIX422_LAUNCH
#undef UVA_PIX422_LAUNCH_M
    return hipGetLastError();
}

template <typename S>
hipError_t to_bgr422(hipStream_t stream, int fmt, int colour, const void* src, S* bgr, int h, int w)
{
    if (grid422_of(h, w).y > 65535) return hipErrorInvalidValue;
    const uint8_t *y, *u, *v;
    planes(fmt, (const uint8_t*)src, h, w, &y, &u, &v);
    const InvCoef c = inv_coef(colour, depth_of(fmt), sizeof(S) == 2);
    const bool vec = vec422_ok(bgr, src, u, v, w, fmt);
    const dim3 grid = grid422_of(h, w), block(BX, BY);
#define UVA_PIX422_LAUNCH_M(W16, M)                                                                                         \
    do {                                                                                                                    \
        if (vec) hipLaunchKernelGGL((pix422_to_bgr<W16, true, S, M>), grid, block, 0, stream, y, u, v, bgr, h, w, c);      \
        else hipLaunchKernelGGL((pix422_to_bgr<W16, false, S, M>), grid, block, 0, stream, y, u, v, bgr, h, w, c);         \
    } while (0)
#define UVA_PIX422_LAUNCH(W16)                                                                                              \
    do {                                                                                                                    \
        switch (hmode422(colour)) {                                                                                         \
        case 0: UVA_PIX422_LAUNCH_M(W16, 0); break;                                                                         \
        case 1: UVA_PIX422_LAUNCH_M(W16, 1); break;                                                                         \
        default: UVA_PIX422_LAUNCH_M(W16, 2); break;                                                                        \
        }                                                                                                                   \
    } while (0)
    if (fmt == PIX_YUV422P10LE) UVA_PIX422_LAUNCH(true);
    else UVA_PIX422_LAUNCH(false);
#undef UVA_PIX422_LAUNCH
#undef UVA_PIX422_LAUNCH_M
    return hipGetLastError();
}

template <typename S>
hipError_t from_bgr(hipStream_t stream, int fmt, int colour, const S* bgr, void* dst, int h, int w)
{
    if (h <= 0 || w <= 0 || !pix_colour_ok(colour) || grid_of(h, w).y > 65535) return hipErrorInvalidValue;
    if (is422(fmt)) return from_bgr422<S>(stream, fmt, colour, bgr, dst, h, w);
    const uint8_t *yp, *up, *vp;
    planes(fmt, (const uint8_t*)dst, h, w, &yp, &up, &vp);
    const FwdCoef c = fwd_coef(colour, depth_of(fmt), sizeof(S) == 2);
    const bool vec = vec_ok(bgr, dst, w);
    const dim3 grid = grid_of(h, w), block(BX, BY);
    uint8_t *y = const_cast<uint8_t*>(yp), *u = const_cast<uint8_t*>(up), *v = const_cast<uint8_t*>(vp);
#define UVA_PIX_LAUNCH_M(F, M)                                                                                              \
    do {                                                                                                                    \
        if (vec) hipLaunchKernelGGL((pix_from_bgr<F, true, S, M>), grid, block, 0, stream, bgr, y, u, v, h, w, c);         \
        else hipLaunchKernelGGL((pix_from_bgr<F, false, S, M>), grid, block, 0, stream, bgr, y, u, v, h, w, c);            \
    } while (0)
#define UVA_PIX_LAUNCH(F)                                                                                                   \
    do {                                                                                                                    \
        switch (pix_chroma_mode(colour)) {                                                                                  \
        case 0: UVA_PIX_LAUNCH_M(F, 0); break;                                                                              \
        case 1: UVA_PIX_LAUNCH_M(F, 1); break;                                                                              \
        case 2: UVA_PIX_LAUNCH_M(F, 2); break;                                                                              \
        default: UVA_PIX_LAUNCH_M(F, 3); break;                                                                             \
        }                                                                                                                   \
    } while (0)
    switch (fmt) {
    case PIX_YUV420P: UVA_PIX_LAUNCH(PIX_YUV420P); break;
    case PIX_NV12: UVA_PIX_LAUNCH(PIX_NV12); break;
    case PIX_P010LE: UVA_PIX_LAUNCH(PIX_P010LE); break;
    case PIX_YUV420P10LE: UVA_PIX_LAUNCH(PIX_YUV420P10LE); break;
    default: return hipErrorInvalidValue;
    }
#undef UVA_PIX_LAUNCH
#undef UVA_PIX_LAUNCH_M
    return hipGetLastError();
}

template <typename S>
hipError_t to_bgr(hipStream_t stream, int fmt, int colour, const void* src, S* bgr, int h, int w)
{
    if (h <= 0 || w <= 0 || !pix_colour_ok(colour) || grid_of(h, w).y > 65535) return hipErrorInvalidValue;
    if (is422(fmt)) return to_bgr422<S>(stream, fmt, colour, src, bgr, h, w);
    const uint8_t *y, *u, *v;
    planes(fmt, (const uint8_t*)src, h, w, &y, &u, &v);
    const InvCoef c = inv_coef(colour, depth_of(fmt), sizeof(S) == 2);
    const bool vec = vec_ok(bgr, src, w);
    const dim3 grid = grid_of(h, w), block(BX, BY);
#define UVA_PIX_LAUNCH_M(F, M)                                                                                              \
    do {                                                                                                                    \
        if (vec) hipLaunchKernelGGL((pix_to_bgr<F, true, S, M>), grid, block, 0, stream, y, u, v, bgr, h, w, c);         \
        else hipLaunchKernelGGL((pix_to_bgr<F, false, S, M>), grid, block, 0, stream, y, u, v, bgr, h, w, c);            \
    } while (0)
#define UVA_PIX_LAUNCH(F)                                                                                                   \
    do {                                                                                                                    \
        switch (pix_chroma_mode(colour)) {                                                                                  \
        case 0: UVA_PIX_LAUNCH_M(F, 0); break;                                                                              \
        case 1: UVA_PIX_LAUNCH_M(F, 1); break;                                                                              \
        case 2: UVA_PIX_LAUNCH_M(F, 2); break;                                                                              \
        default: UVA_PIX_LAUNCH_M(F, 3); break;                                                                             \
        }                                                                                                                   \
    } while (0)
    switch (fmt) {
    case PIX_YUV420P: UVA_PIX_LAUNCH(PIX_YUV420P); break;
    case PIX_NV12: UVA_PIX_LAUNCH(PIX_NV12); break;
    case PIX_P010LE: UVA_PIX_LAUNCH(PIX_P010LE); break;
    case PIX_YUV420P10LE: UVA_PIX_LAUNCH(PIX_YUV420P10LE); break;
    default: return hipErrorInvalidValue;
    }
#undef UVA_PIX_LAUNCH
#undef UVA_PIX_LAUNCH_M
    return hipGetLastError();
}

dim3 flat_grid(size_t n) { return dim3((unsigned)((n + 256 * WN - 1) / (256 * WN))); }
}  // namespace

hipError_t launch_pix_from_bgr(hipStream_t stream, int fmt, int colour, const uint8_t* bgr, void* dst, int h, int w)
{
    return from_bgr<uint8_t>(stream, fmt, colour, bgr, dst, h, w);
}

hipError_t launch_pix_to_bgr(hipStream_t stream, int fmt, int colour, const void* src, uint8_t* bgr, int h, int w)
{
    return to_bgr<uint8_t>(stream, fmt, colour, src, bgr, h, w);
}

hipError_t launch_pix16_from_bgr(hipStream_t stream, int fmt, int colour, const uint16_t* bgr, void* dst, int h, int w)
{
    if (fmt != PIX_BGR24) return from_bgr<uint16_t>(stream, fmt, colour, bgr, dst, h, w);
    if (h <= 0 || w <= 0 || !pix_colour_ok(colour)) return hipErrorInvalidValue;
    const size_t n = (size_t)3 * w * h;
    if (flat_grid(n).x == 0 || n / (256 * WN) >= 0x7fffffffu) return hipErrorInvalidValue;
    if ((((uintptr_t)bgr % 16) | ((uintptr_t)dst % 8)) == 0) hipLaunchKernelGGL((pix_narrow<true>), flat_grid(n), dim3(256), 0, stream, bgr, (uint8_t*)dst, n);
    else hipLaunchKernelGGL((pix_narrow<false>), flat_grid(n), dim3(256), 0, stream, bgr, (uint8_t*)dst, n);
    return hipGetLastError();
}

hipError_t launch_pix16_to_bgr(hipStream_t stream, int fmt, int colour, const void* src, uint16_t* bgr, int h, int w)
{
    if (fmt != PIX_BGR24) return to_bgr<uint16_t>(stream, fmt, colour, src, bgr, h, w);
    if (h <= 0 || w <= 0 || !pix_colour_ok(colour)) return hipErrorInvalidValue;
    const size_t n = (size_t)3 * w * h;
    if (flat_grid(n).x == 0 || n / (256 * WN) >= 0x7fffffffu) return hipErrorInvalidValue;
    if ((((uintptr_t)src % 8) | ((uintptr_t)bgr % 16)) == 0) hipLaunchKernelGGL((pix_widen<true>), flat_grid(n), dim3(256), 0, stream, (const uint8_t*)src, bgr, n);
    else hipLaunchKernelGGL((pix_widen<false>), flat_grid(n), dim3(256), 0, stream, (const uint8_t*)src, bgr, n);
    return hipGetLastError();
}

}  // namespace uva
