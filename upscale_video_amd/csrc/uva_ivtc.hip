// uva_ivtc.hip -- the kernel behind uva_ivtc_metrics and uva_ivtc_push (uva_ivtc.h).
//
// ivtc_metrics_kernel<BYTES>: three packed frames of one format in HBM (prev, cur, next) -> the comb metric (N, M) of the three
// frames that weave cur's first field with the second field of cur, prev and next, on plane 0, in ONE pass: six exact 64-bit sums.
//
// It keeps the footprint of its siblings (csrc/uva_repeat.hip, csrc/uva_deint.hip): 256 threads, 192 bytes of static LDS, no
// scratch, no floating point, a bounded grid that walks the plane in strides.  The rule is vertical only, so there is no halo:
// a lane owns 16 bytes of a row and loads the same 16 bytes of the rows above and below.  The three candidates of a row share
// the rows of cur (a kept row: the row itself; a row of the other field: its two neighbours) and differ in the rows of cur, prev
// or next around or between them, which are loaded one candidate at a time; the rows of prev and next that no candidate uses --
// those of the first field -- are never loaded.  A row is a neighbour of two rows, so a launch asks for it up to three
// times; it comes from HBM once and from the caches after that.
#include "uva_ivtc.h"

#include "uva_pixfmt.h"

namespace uva {

namespace {

constexpr int IV_THREADS = 256;        // four waves
constexpr int IV_WAVES = IV_THREADS / 64;
constexpr int IV_MAX_GROUPS = 1024;    // four workgroups per compute unit: beyond that a wave walks the rows in grid strides

struct IvtcArgs {
    const uint8_t *prev, *cur, *next;
    unsigned long long* stats;         // N_c, M_c, N_p, M_p, N_n, M_n
    uint32_t row_bytes, ph;            // plane 0: it starts the frame
    uint32_t runs;                     // runs of 64 slots in a row
    uint32_t shift, mask, thr, first;
};

// The nb (0 ... 16) bytes at p, the bytes beyond nb as zeros.  A whole slot is one 16-byte load -- of whatever alignment the row
// has: the copy leaves the choice of instructions to the compiler, which knows what the target may do with an address that is
// no multiple of 16.  A row's ragged end is the one slot with nb < 16: its bytes come one by one through a 128-bit shift
// register, in a loop that is not unrolled, and nothing beyond the row's last byte is read.  (One lane of a row's last wave runs it.)
__device__ __forceinline__ uint4 iv_load(const uint8_t* p, uint32_t nb)
{
    uint4 v = make_uint4(0, 0, 0, 0);
    if (nb == 16u) {
        __builtin_memcpy(&v, p, 16);
    } else {
#pragma unroll 1
        for (uint32_t k = nb; k-- > 0;) {
            v.w = (v.w << 8) | (v.z >> 24);
            v.z = (v.z << 8) | (v.y >> 24);
            v.y = (v.y << 8) | (v.x >> 24);
            v.x = (v.x << 8) | p[k];
        }
    }
    return v;
}

// the code value of sample k of a word
template <int BYTES>
__device__ __forceinline__ int iv_sample(uint32_t word, int k, uint32_t shift, uint32_t mask)
{
    if (BYTES == 1) return (int)((word >> (8 * k)) & 255u);
    return (int)((word >> (16 * k + shift)) & mask);      // (shift + the mask's bits stay inside the 16-bit word)
}

// one candidate's share of a word of a slot: rows y - 1, y, y + 1 of its woven frame.  Masked bytes are zero in all three rows:
// d1 = d2 = 0, not combed.  `n` counts samples and `m` sums at most 16 * 255 or 8 * 65535 < 2^20 per slot; the caller adds both
// to wider sums.
template <int BYTES>
__device__ __forceinline__ void iv_comb(uint32_t wa, uint32_t wb, uint32_t wc, uint32_t shift, uint32_t mask, uint32_t thr, uint32_t& n,
                                        uint32_t& m)
{
#pragma unroll
    for (int k = 0; k < 4 / BYTES; ++k) {
        const int a = iv_sample<BYTES>(wa, k, shift, mask), b = iv_sample<BYTES>(wb, k, shift, mask), c = iv_sample<BYTES>(wc, k, shift, mask);
        const int d1 = b - a, d2 = b - c;
        const int a1 = d1 < 0 ? -d1 : d1, a2 = d2 < 0 ? -d2 : d2;
        const uint32_t mn = (uint32_t)(a1 < a2 ? a1 : a2);
        // the same sign and both non-zero: mn > thr >= 0 says non-zero, the sign bits say the rest
        const bool hit = ((d1 ^ d2) >= 0) && mn > thr;
        n += hit ? 1u : 0u;
        m += hit ? mn : 0u;
    }
}

// the unit moves on by a word, around: after four steps it is as it was
__device__ __forceinline__ void iv_rotate(uint4& v)
{
    const uint32_t x = v.x;
    v.x = v.y; v.y = v.z; v.z = v.w; v.w = x;
}

// Lane per 16-byte slot of a row (counted from the row's first byte), wave per run of 64 slots of ONE row: the row, its parity
// and every base address are the wave's, in scalar registers.
//
// A slot is worked on a word of four bytes at a time, one candidate after the other, in loops that are NOT unrolled: after a
// step every unit moves on by a word, around, and after a candidate the three pairs of sums move on by one, around, so the body
// is the same code on the same registers and only a word's samples are unpacked at any time.  Unrolled, the kernel needs more
// than a hundred registers, or scratch under a bound (uva_deint.hip has the same lesson).
//
// The accumulators cannot overflow: check_dims admits h * w <= 2^28 and the widest plane 0 has three samples per pixel, so a
// launch sees fewer than 3 * 2^28 < 2^32 samples per candidate and a 32-bit count holds them all, even on one workgroup; M adds
// per slot less than 2^20 into 64 bits, and 3 * 2^28 * 65535 < 2^46.
template <int BYTES>
__global__ __launch_bounds__(IV_THREADS, 7) void ivtc_metrics_kernel(IvtcArgs a)
{
    uint32_t cnt0 = 0, cnt1 = 0, cnt2 = 0;
    unsigned long long sum0 = 0, sum1 = 0, sum2 = 0;
    const uint32_t lane = threadIdx.x & 63u;
    // (blockIdx.y walks the runs and the waves of blockIdx.x the rows: no division, which would be floating point here)
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * IV_WAVES + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * IV_WAVES;
    const uint32_t row_bytes = a.row_bytes, shift = a.shift, mask = a.mask, thr = a.thr;
    for (uint32_t run = blockIdx.y; run < a.runs; run += gridDim.y)
    for (uint32_t y = 1u + wave; y + 1u < a.ph; y += nwaves) {
        const uint32_t cb = (run * 64u + lane) * 16u;
        const uint32_t nb = cb < row_bytes ? (row_bytes - cb < 16u ? row_bytes - cb : 16u) : 0u;
        // (plane 0 has fewer than 6 * 2^28 < 2^32 bytes: 32-bit offsets)
        const uint32_t o = y * row_bytes + cb;
        const bool kept = (y & 1u) == a.first;
        // a kept row is cur's, between the candidate's rows; a row of the other field is the candidate's, between cur's
        uint4 r0 = iv_load(a.cur + (kept ? o : o - row_bytes), nb), r1 = make_uint4(0, 0, 0, 0);
        if (!kept) r1 = iv_load(a.cur + o + row_bytes, nb);
        const uint8_t* fx = a.cur;
#pragma unroll 1
        for (int x = 0; x < 3; ++x) {
            uint32_t n = 0, m = 0;
            if (kept) {
                uint4 ra = iv_load(fx + o - row_bytes, nb), rc = iv_load(fx + o + row_bytes, nb);
#pragma unroll 1
                for (int q = 0; q < 4; ++q) {
                    iv_comb<BYTES>(ra.x, r0.x, rc.x, shift, mask, thr, n, m);
                    iv_rotate(ra); iv_rotate(r0); iv_rotate(rc);
                }
            } else {
                uint4 rb = iv_load(fx + o, nb);
#pragma unroll 1
                for (int q = 0; q < 4; ++q) {
                    iv_comb<BYTES>(r0.x, rb.x, r1.x, shift, mask, thr, n, m);
                    iv_rotate(r0); iv_rotate(rb); iv_rotate(r1);
                }
            }
            // the sums move on by one candidate, around: c, p, n are back in their places after the third
            const uint32_t c = cnt0 + n;
            const unsigned long long t = sum0 + m;
            cnt0 = cnt1; cnt1 = cnt2; cnt2 = c;
            sum0 = sum1; sum1 = sum2; sum2 = t;
            fx = x == 0 ? a.prev : a.next;
        }
    }
    const uint32_t cnt[3] = {cnt0, cnt1, cnt2};
    const unsigned long long sum[3] = {sum0, sum1, sum2};
    // lanes of a wave through __shfl_xor, the four waves through LDS, then one set of integer atomics per workgroup: integer sums
    // do not depend on the order of arrival, the six numbers are exact
    __shared__ unsigned long long s_sum[IV_WAVES][6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        uint32_t c = cnt[k], lo = (uint32_t)sum[k], hi = (uint32_t)(sum[k] >> 32);
        unsigned long long s = sum[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            c += __shfl_xor(c, off, 64);
            s += ((unsigned long long)__shfl_xor(hi, off, 64) << 32) | __shfl_xor(lo, off, 64);
            lo = (uint32_t)s; hi = (uint32_t)(s >> 32);
        }
        if (lane == 0) {
            s_sum[threadIdx.x >> 6][2 * k] = c;
            s_sum[threadIdx.x >> 6][2 * k + 1] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        unsigned long long t = 0;
        for (int k = 0; k < IV_WAVES; ++k) t += s_sum[k][threadIdx.x];
        if (t) atomicAdd(&a.stats[threadIdx.x], t);      // (a workgroup that found no comb has nothing to add)
    }
}

}  // namespace

hipError_t launch_ivtc_metrics(hipStream_t stream, const void* d_prev, const void* d_cur, const void* d_next, int fmt, int h, int w,
                               int flags, int T, unsigned long long* d_stats, int max_groups)
{
    if (ivtc_error(fmt, h, w, flags, T, 0) || !d_prev || !d_cur || !d_next || !d_stats) return hipErrorInvalidValue;
    if ((((uintptr_t)d_prev | (uintptr_t)d_cur | (uintptr_t)d_next) & 15) != 0 || ((uintptr_t)d_stats & 7) != 0) return hipErrorInvalidValue;
    const DeintFormat f = deint_format(fmt, h, w);
    const DeintPlane& q = f.plane[0];
    if (q.off != 0 || q.ph < 3 || q.row_bytes * (size_t)q.ph > 0xffffffffull) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_stats, 0, 6 * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    IvtcArgs a = {};
    a.prev = (const uint8_t*)d_prev; a.cur = (const uint8_t*)d_cur; a.next = (const uint8_t*)d_next;
    a.stats = d_stats;
    a.row_bytes = (uint32_t)q.row_bytes; a.ph = (uint32_t)q.ph;
    a.runs = (uint32_t)((q.row_bytes + 1023) / 1024);
    a.shift = (uint32_t)f.shift; a.mask = (uint32_t)f.mask; a.thr = ivtc_threshold(f, T); a.first = (uint32_t)ivtc_first(flags);
    // gy workgroups share the runs of a row, gx times four waves the rows: gx * gy workgroups, IV_MAX_GROUPS at most
    const uint32_t cap = max_groups > 0 && max_groups < IV_MAX_GROUPS ? (uint32_t)max_groups : (uint32_t)IV_MAX_GROUPS;
    const uint32_t gy = a.runs < cap ? a.runs : cap, want = (a.ph - 2u + IV_WAVES - 1) / IV_WAVES;
    const uint32_t gx = want < cap / gy ? want : cap / gy;
    const dim3 groups(gx < 1 ? 1u : gx, gy);
    if (f.bytes == 1) hipLaunchKernelGGL(ivtc_metrics_kernel<1>, groups, dim3(IV_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(ivtc_metrics_kernel<2>, groups, dim3(IV_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_ivtc_weave(hipStream_t stream, const void* d_cur, const void* d_x, int fmt, int h, int w, int flags, void* d_out)
{
    if (ivtc_error(fmt, h, w, flags, 0, 0) || !d_cur || !d_x || !d_out) return hipErrorInvalidValue;
    const DeintFormat f = deint_format(fmt, h, w);
    hipError_t e = hipMemcpyAsync(d_out, d_cur, f.frame_bytes, hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess || d_x == d_cur) return e;
    const int other = 1 - ivtc_first(flags);
    for (int p = 0; p < f.nplanes && e == hipSuccess; ++p) {
        const DeintPlane& pl = f.plane[p];
        const int rows = (pl.ph - other + 1) / 2;        // rows other, other + 2, ... of the plane
        if (rows <= 0) continue;
        const size_t o = pl.off + (size_t)other * pl.row_bytes;
        e = hipMemcpy2DAsync((uint8_t*)d_out + o, 2 * pl.row_bytes, (const uint8_t*)d_x + o, 2 * pl.row_bytes, pl.row_bytes, (size_t)rows,
                             hipMemcpyDeviceToDevice, stream);
    }
    return e;
}

}  // namespace uva
