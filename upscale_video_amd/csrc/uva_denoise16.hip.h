// uva_denoise16.hip.h -- `-m n=K` at --bit-depth 16: the stage of uva_denoise.hip.h on u16 samples.
//   1. BGR16 -> Lab16 (the frame taken as LINEAR light): L16 = L * 65535 / 100, a16 = (a + 128) * 257, b16 alike -- the
//      8-bit planes' scales x 257 -- from the CIE formulas in fixed point: a 2^15-scaled matrix in unsigned 32 bits, a table
//      of 2^16 f(t / 65535) for every 16-bit t, 2^20-scaled affine maps in 64 bits;
//   2. non-local means on the L16 plane with h and on the 2-channel (a16, b16) image with hColor: template 5x5, search 9x9,
//      reflect-101 border of 6, as at 8 bits.  A sample difference is squared in unsigned 32 bits and shifted `>> 8` BEFORE
//      any summing (25 * 2 samples stay below 2^31, and the patch distance stays a box sum of per-pixel integers), the
//      table index is the distance `>> 9` -- bins sixteen times finer than the 8-bit table's -- and the weight is the 8-bit
//      stage's function of the mean squared patch difference in 8-bit units^2, so K means the same at both depths;
//      64-bit accumulators (81 * F * 65535 does not fit 32 bits), OpenCV's rounded unsigned division;
//   3. Lab16 -> BGR16: f at 2^24 = 1.0 in 64 bits, the integer cube, a 2^14-scaled matrix.
// The definition is tests/nlm16_ref.py (integer numpy, written first); the kernels are held to it bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "uva_denoise.hip.h"
#include "uva_denoise16_tables.h"

namespace uva {

__device__ __forceinline__ uint16_t lab16_sat(int64_t v) { return (uint16_t)(v < 0 ? 0 : v > 65535 ? 65535 : v); }

// planes: L [h][w] u16, ab [h][w][2] u16; bgr rows `stride` BYTES apart
__global__ void nlm_bgr2lab16(const uint16_t* bgr, size_t stride, int h, int w, uint16_t* L, uint16_t* ab, const Lab16Tables* t)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const uint16_t* s = (const uint16_t*)((const char*)bgr + (size_t)y * stride) + (size_t)x * 3;
    const uint32_t B = s[0], G = s[1], R = s[2];
    uint32_t F[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t sum = t->fwd[3 * k] * R + t->fwd[3 * k + 1] * G + t->fwd[3 * k + 2] * B;      // < 2^32
        F[k] = t->ftab[min((sum + (1u << 14)) >> 15, 65535u)];
    }
    const int64_t fX = F[0], fY = F[1], fZ = F[2], half = 1 << 19, off = (int64_t)LAB16_AB_OFF << 20;
    const size_t i = (size_t)y * w + x;
    L[i] = lab16_sat((fY * t->l_mul - t->l_sub + half) >> 20);
    ab[2 * i] = lab16_sat(((fX - fY) * t->a_mul + off + half) >> 20);
    ab[2 * i + 1] = lab16_sat(((fY - fZ) * t->b_mul + off + half) >> 20);
}

__device__ __forceinline__ int64_t lab16_f_inv(int64_t f24, const Lab16Tables* t)
{
    if (f24 > t->f_thr) return (((f24 * f24) >> 24) * f24) >> 24;
    return ((f24 - t->f_bias) * t->lin_mul) >> 20;
}

__global__ void nlm_lab2bgr16(const uint16_t* L, const uint16_t* ab, int h, int w, uint16_t* bgr, size_t stride, const Lab16Tables* t)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const size_t i = (size_t)y * w + x;
    const int64_t LL = L[i], aa = ab[2 * i], bb = ab[2 * i + 1];
    const int64_t fy = (LL * t->il_mul + t->il_add + (1 << 15)) >> 16;
    const int64_t fx = fy + (((aa - LAB16_AB_OFF) * t->ia_mul + (1 << 15)) >> 16);
    const int64_t fz = fy - (((bb - LAB16_AB_OFF) * t->ib_mul + (1 << 15)) >> 16);
    const int64_t xx = lab16_f_inv(fx, t), yy = lab16_f_inv(fy, t), zz = lab16_f_inv(fz, t);
    uint16_t* d = (uint16_t*)((char*)bgr + (size_t)y * stride) + (size_t)x * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {        // R, G, B rows of the matrix -> samples 2, 1, 0
        int64_t v = (t->inv[3 * k] * xx + t->inv[3 * k + 1] * yy + t->inv[3 * k + 2] * zz + (1 << 13)) >> 14;
        v = v < 0 ? 0 : v > (1 << 24) ? (1 << 24) : v;
        d[2 - k] = (uint16_t)((v * 65535 + (1 << 23)) >> 24);
    }
}

// nlm_plane's shape (uva_denoise.hip.h) on u16 samples: 16 x 16 output pixels per 256-thread workgroup, their 28 x 28
// neighbourhood staged in LDS once (one 32-bit word per pixel at CN = 2: both channels come with one ds_read_b32), one column
// of five squared differences per thread and offset through a double-buffered LDS array, one barrier per offset, then five
// neighbouring column sums: 6.25 squared differences per pixel and offset.  The weight table stays in HBM (785 entries at
// K = 3, cn = 1; 156 745 at K = 30, cn = 2): the low indices every similar patch hits sit in L2.
template <int CN>
__global__ __launch_bounds__(NLM_BLK * NLM_BLK) void nlm_plane16(const uint16_t* src, int h, int w, const int* weight_table,
                                                                  int table_size, uint16_t* dst)
{
    static_assert(CN == 1 || CN == 2, "one plane, or two interleaved");
    using px_t = typename std::conditional<CN == 2, uint32_t, uint16_t>::type;
    constexpr int VW = NLM_BLK + 2 * NLM_T;
    __shared__ px_t tile[NLM_TILE * NLM_TILE];
    __shared__ uint32_t vsum[2][NLM_BLK * VW];
    const px_t* const spx = (const px_t*)src;
    const int bx = blockIdx.x * NLM_BLK, by = blockIdx.y * NLM_BLK;
    for (int i = threadIdx.x; i < NLM_TILE * NLM_TILE; i += NLM_BLK * NLM_BLK) {
        const int ty = i / NLM_TILE, tx = i - ty * NLM_TILE;
        const int sy = reflect101(by + ty - NLM_B, h), sx = reflect101(bx + tx - NLM_B, w);
        tile[i] = spx[(size_t)sy * w + sx];
    }
    __syncthreads();
    const int lx = threadIdx.x % NLM_BLK, ly = threadIdx.x / NLM_BLK;
    const int x = bx + lx, y = by + ly;
    const int cx = lx + NLM_B, cy = ly + NLM_B;
    // (d * d) of a 17-bit signed d in UNSIGNED 32 bits: 65535^2 < 2^32, a signed product would overflow
    auto sqd = [](uint32_t a, uint32_t b) {
        const uint32_t d = a - b;
        return (d * d) >> NLM16_SQ_SHIFT;
    };
    auto colsum = [&](int r, int c, int sy, int sx) {
        const int tx = NLM_B - NLM_T + c;
        uint32_t v = 0;
#pragma unroll
        for (int ty = -NLM_T; ty <= NLM_T; ++ty) {
            const uint32_t a = tile[(r + NLM_B + ty) * NLM_TILE + tx];
            const uint32_t b = tile[(r + NLM_B + ty + sy) * NLM_TILE + tx + sx];
            if (CN == 2) v += sqd(a & 0xffffu, b & 0xffffu) + sqd(a >> 16, b >> 16);
            else v += sqd(a, b);
        }
        return v;
    };
    uint64_t est[CN];
#pragma unroll
    for (int c = 0; c < CN; ++c) est[c] = 0;
    uint32_t wsum = 0;                                            // <= 81 * 103969
    int buf = 0;
    for (int sy = -NLM_S; sy <= NLM_S; ++sy)
        for (int sx = -NLM_S; sx <= NLM_S; ++sx) {
            uint32_t* const vb = vsum[buf];
            vb[ly * VW + lx] = colsum(ly, lx, sy, sx);
            if (threadIdx.x < NLM_BLK * 2 * NLM_T) {              // the four extra columns of the 16 rows
                const int r = threadIdx.x / (2 * NLM_T), c = NLM_BLK + threadIdx.x % (2 * NLM_T);
                vb[r * VW + c] = colsum(r, c, sy, sx);
            }
            __syncthreads();                                      // (the other buffer is free again after the NEXT barrier)
            uint32_t dist = 0;                                    // <= 25 * 2 * (65535^2 >> 8) < 2^31
#pragma unroll
            for (int t = 0; t <= 2 * NLM_T; ++t) dist += vb[ly * VW + lx + t];
            const uint32_t idx = min(dist >> NLM16_IDX_SHIFT, (uint32_t)(table_size - 1));
            const uint32_t wgt = (uint32_t)weight_table[idx];
            const uint32_t p = tile[(cy + sy) * NLM_TILE + cx + sx];
            if (CN == 2) {
                est[0] += (uint64_t)wgt * (p & 0xffffu);          // one 32 x 32 -> 64 multiply-add each
                est[CN - 1] += (uint64_t)wgt * (p >> 16);
            } else {
                est[0] += (uint64_t)wgt * p;
            }
            wsum += wgt;
            buf ^= 1;
        }
    if (x >= w || y >= h) return;
#pragma unroll
    for (int c = 0; c < CN; ++c) {
        const uint64_t q = (est[c] + wsum / 2) / wsum;           // divByWeightsSum; the centre patch weighs F: wsum > 0
        dst[((size_t)y * w + x) * CN + c] = (uint16_t)(q < 65535 ? q : 65535);
    }
}

}  // namespace uva
