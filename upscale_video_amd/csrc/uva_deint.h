// uva_deint.h -- yadif deinterlacing on the raw-video route (include/uva.h uva_deint_*).  Two halves:
//   csrc/uva_deint_host.cpp  plain C++ without HIP: the table of a format's component planes, the refusals and a scalar
//                            implementation of the rule (uva_debug_deint_host).  Functions of their arguments; built alone by
//                            tests/test_deint_sanitized.py.
//   csrc/uva_deint.hip       the kernel: deint_kernel<BYTES, STRIDE>.
// The rule is yadif's spatio-temporal one as tests/yadif_ref.py states it for this project; parity with ffmpeg's filter is
// unpinned (section 7.13).  The arithmetic of one sample, deint_rule, is written once here for both halves, so the HIP
// declarations sit behind __HIPCC__ and the shared functions carry UVA_DEINT_HD.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define UVA_DEINT_HD __host__ __device__ __forceinline__
#else
#define UVA_DEINT_HD inline
#endif

namespace uva {

// The pixel-format codes of uva_pixfmt.h, restated so that the host file needs no HIP header (uva_deint.hip asserts they agree).
enum { DEINT_BGR24 = 0, DEINT_YUV420P = 1, DEINT_NV12 = 2, DEINT_P010LE = 3, DEINT_YUV420P10LE = 5, DEINT_BGR48LE = 6, DEINT_YUV422P = 7,
       DEINT_YUV422P10LE = 8 };
enum { DEINT_FIELD = 1, DEINT_BFF = 2, DEINT_FLAGS = 3 };      // include/uva.h UVA_DEINT_*

// A plane of ROWS as they lie in memory: `ph` rows of `row_bytes` bytes from byte `off` of the frame, each holding `stride`
// interleaved component planes of `pw` samples (1: a planar plane; 2: nv12 / p010le chroma; 3: packed BGR) -- sample j of a row
// is sample j / stride of component j % stride, and "x +- k" of the rule is sample j +- k * stride.
struct DeintPlane {
    size_t off, row_bytes;
    int pw, ph, stride;
};
// how a format's words are read and written: bytes per sample (1 / 2; 0: unknown format), code value = (word >> shift) & mask,
// and a clean word = value << shift
struct DeintFormat {
    int bytes, shift, mask, nplanes;
    DeintPlane plane[3];
    size_t frame_bytes;
};
// the table for h x w frames of fmt (bytes == 0: unknown format); sizes are not judged here
DeintFormat deint_format(int fmt, int h, int w);

// nullptr, or why uva_deint_* refuses h x w frames of fmt with these flags
const char* deint_error(int fmt, int h, int w, int flags);

// out_a / out_b (either may be null) <- the outputs A and B of `cur` between `prev` and `next` (null: cur), on the host
void deint_host(const uint8_t* prev, const uint8_t* cur, const uint8_t* next, int fmt, int h, int w, int flags, uint8_t* out_a, uint8_t* out_b);

// the parity (y & 1) of the rows that output A interpolates; B interpolates the others.  tff: even rows are the first field, A
// keeps them.
UVA_DEINT_HD int deint_parity_a(int flags) { return (flags & DEINT_BFF) ? 0 : 1; }

UVA_DEINT_HD int deint_abs(int v) { return v < 0 ? -v : v; }
UVA_DEINT_HD int deint_min(int a, int b) { return a < b ? a : b; }
UVA_DEINT_HD int deint_max(int a, int b) { return a > b ? a : b; }

// One interpolated sample, in three parts.  cm[k] / cp[k]: cur[ym][x - 3 + k] / cur[yp][x - 3 + k] of the sample's component
// (k = 3 alone is read unless `inner`); c, e = cm[3], cp[3]; p2y, n2y: p2[y][x], n2[y][x]; pm, pp / nm, np: prev / next at rows
// ym, yp; `full`: rows y -+ 2 exist, and then p2mm, n2mm / p2pp, n2pp are p2 and n2 at rows ymm / ypp.
// the temporal half: d and the final diff
UVA_DEINT_HD void deint_temporal(int c, int e, int p2y, int n2y, int pm, int pp, int nm, int np, bool full, int p2mm, int n2mm, int p2pp,
                                 int n2pp, int* d_out, int* diff_out)
{
    const int d = (p2y + n2y) >> 1;
    const int t0 = deint_abs(p2y - n2y);
    const int t1 = (deint_abs(pm - c) + deint_abs(pp - e)) >> 1;
    const int t2 = (deint_abs(nm - c) + deint_abs(np - e)) >> 1;
    int diff = deint_max(deint_max(t0 >> 1, t1), t2);
    {
        const int b = (p2mm + n2mm) >> 1, f = (p2pp + n2pp) >> 1;
        const int mx = deint_max(deint_max(d - e, d - c), deint_min(b - c, f - e));
        const int mn = deint_min(deint_min(d - e, d - c), deint_max(b - c, f - e));
        diff = full ? deint_max(deint_max(diff, mn), -mx) : diff;
    }
    *d_out = d;
    *diff_out = diff;
}

// the spatial half: the prediction from the better of five directions
UVA_DEINT_HD int deint_spatial(const int cm[7], const int cp[7], bool inner)
{
    int sp = (cm[3] + cp[3]) >> 1;
    if (inner) {
        // S(j) = sum over k = -1, 0, 1 of |cur[ym][x + k + j] - cur[yp][x + k - j]|
#define UVA_DEINT_S(j) (deint_abs(cm[2 + (j)] - cp[2 - (j)]) + deint_abs(cm[3 + (j)] - cp[3 - (j)]) + deint_abs(cm[4 + (j)] - cp[4 - (j)]))
        int score = UVA_DEINT_S(0) - 1;
        const int sm1 = UVA_DEINT_S(-1), sm2 = UVA_DEINT_S(-2), sp1 = UVA_DEINT_S(1), sp2 = UVA_DEINT_S(2);
#undef UVA_DEINT_S
        // (selects, not branches: the +-2 step counts only where the +-1 step of its sign improved the score)
        const bool m1 = sm1 < score;
        score = m1 ? sm1 : score; sp = m1 ? (cm[2] + cp[4]) >> 1 : sp;
        const bool m2 = m1 && sm2 < score;
        score = m2 ? sm2 : score; sp = m2 ? (cm[1] + cp[5]) >> 1 : sp;
        const bool p1 = sp1 < score;
        score = p1 ? sp1 : score; sp = p1 ? (cm[4] + cp[2]) >> 1 : sp;
        const bool p2 = p1 && sp2 < score;
        sp = p2 ? (cm[5] + cp[1]) >> 1 : sp;
    }
    return sp;
}

UVA_DEINT_HD int deint_clamp(int sp, int d, int diff) { return deint_max(deint_min(sp, d + diff), d - diff); }

UVA_DEINT_HD int deint_rule(const int cm[7], const int cp[7], bool inner, int p2y, int n2y, int pm, int pp, int nm, int np, bool full,
                            int p2mm, int n2mm, int p2pp, int n2pp)
{
    int d, diff;
    deint_temporal(cm[3], cp[3], p2y, n2y, pm, pp, nm, np, full, p2mm, n2mm, p2pp, n2pp, &d, &diff);
    return deint_clamp(deint_spatial(cm, cp, inner), d, diff);
}

// the rows of the rule for row y of a plane of ph >= 2 rows
struct DeintRows {
    int ym, yp, ymm, ypp;
    bool full;
};
UVA_DEINT_HD DeintRows deint_rows(int y, int ph)
{
    DeintRows r;
    r.ym = y > 0 ? y - 1 : y + 1;
    r.yp = y + 1 < ph ? y + 1 : y - 1;
    r.full = !(y == 1 || y + 2 == ph);
    r.ymm = r.full ? (y > 0 ? y - 2 : y + 2) : y;
    r.ypp = r.full ? (y + 1 < ph ? y + 2 : y - 2) : y;
    return r;
}

// the code value of sample j of the row at `row` (BYTES per sample)
template <int BYTES>
UVA_DEINT_HD int deint_read(const uint8_t* row, size_t j, int shift, int mask)
{
    if (BYTES == 1) return row[j];
#ifdef __HIP_DEVICE_COMPILE__
    const uint32_t word = *(const uint16_t*)(row + 2 * j);       // (frames start at 16-byte aligned addresses there)
#else
    const uint32_t word = row[2 * j] | ((uint32_t)row[2 * j + 1] << 8);      // little-endian words at any address
#endif
    return (int)((word >> shift) & (uint32_t)mask);
}

// Sample j of row y of one plane, straight from memory: prev / cur / next / p2 / n2 point at the PLANE in their frames.  Every
// index is inside the plane (ph >= 2); a column within three samples of its component's ends takes no spatial search.
template <int BYTES>
UVA_DEINT_HD int deint_sample_mem(const uint8_t* prev, const uint8_t* cur, const uint8_t* next, const uint8_t* p2, const uint8_t* n2,
                                  size_t row_bytes, int pw, int ph, int stride, int shift, int mask, int y, int j)
{
    const DeintRows r = deint_rows(y, ph);
    const int x = j / stride;
    const bool inner = x >= 3 && x < pw - 3;
    const size_t oy = (size_t)y * row_bytes, om = (size_t)r.ym * row_bytes, op = (size_t)r.yp * row_bytes;
    int cm[7], cp[7];
    for (int k = 0; k < 7; ++k) {
        const bool have = inner || k == 3;
        cm[k] = have ? deint_read<BYTES>(cur + om, (size_t)(j + (k - 3) * stride), shift, mask) : 0;
        cp[k] = have ? deint_read<BYTES>(cur + op, (size_t)(j + (k - 3) * stride), shift, mask) : 0;
    }
    const size_t omm = (size_t)r.ymm * row_bytes, opp = (size_t)r.ypp * row_bytes;
    return deint_rule(cm, cp, inner, deint_read<BYTES>(p2 + oy, j, shift, mask), deint_read<BYTES>(n2 + oy, j, shift, mask),
                      deint_read<BYTES>(prev + om, j, shift, mask), deint_read<BYTES>(prev + op, j, shift, mask),
                      deint_read<BYTES>(next + om, j, shift, mask), deint_read<BYTES>(next + op, j, shift, mask), r.full,
                      deint_read<BYTES>(p2 + omm, j, shift, mask), deint_read<BYTES>(n2 + omm, j, shift, mask),
                      deint_read<BYTES>(p2 + opp, j, shift, mask), deint_read<BYTES>(n2 + opp, j, shift, mask));
}

}  // namespace uva

#ifdef __HIPCC__
namespace uva {

// d_out_a / d_out_b (either may be null, not both; frames of the input's format and size in HBM) <- the outputs of d_cur between
// d_prev and d_next on `stream`: one kernel.  Every frame starts at a 16-byte aligned address.  max_groups > 0 bounds the grid
// below the kernel's own bound (tests: the grid-stride walk on a small frame).
hipError_t launch_deint(hipStream_t stream, const void* d_prev, const void* d_cur, const void* d_next, int fmt, int h, int w, int flags,
                        void* d_out_a, void* d_out_b, int max_groups = 0);

}  // namespace uva
#endif
