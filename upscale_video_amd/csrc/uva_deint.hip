// uva_deint.hip -- the kernel behind uva_deint_frames and uva_deint_push (uva_deint.h).
//
// deint_kernel<BYTES, STRIDE>: three packed frames of one format in HBM (prev, cur, next) -> output A, output B or both of the
// middle one: the rows of one field copied, the rows of the other interpolated by yadif's spatio-temporal rule (deint_rule).  One
// launch covers every plane of the frame, and in `field` mode it writes both outputs: every row is then copied into one of them
// and interpolated into the other, so all lanes of a launch do the same work.
//
// It runs on a stream of its own while a net's persistent kernels own the compute units, so it keeps frame_diff_kernel's
// footprint (csrc/uva_repeat.hip): 256 threads, no LDS, no scratch, a bounded grid that walks the frame in strides.
#include "uva_deint.h"

#include "uva_pixfmt.h"

namespace uva {

static_assert(DEINT_BGR24 == PIX_BGR24 && DEINT_YUV420P == PIX_YUV420P && DEINT_NV12 == PIX_NV12 && DEINT_P010LE == PIX_P010LE &&
              DEINT_YUV420P10LE == PIX_YUV420P10LE && DEINT_BGR48LE == PIX_BGR48LE && DEINT_YUV422P == PIX_YUV422P &&
              DEINT_YUV422P10LE == PIX_YUV422P10LE, "uva_deint.h restates uva_pixfmt.h's format codes");

namespace {

constexpr int DI_THREADS = 256;        // four waves
constexpr int DI_MAX_GROUPS = 1024;    // four workgroups per compute unit: beyond that a workgroup walks the slots in grid strides

struct DeintArgs {
    const uint8_t *prev, *cur, *next;
    uint8_t *out_a, *out_b;            // either may be null
    uint32_t off[3], row_bytes[3];     // (a frame has at most 6 * 2^28 bytes: fits 32 bits)
    uint32_t slots[3];                 // 16-byte slots that a row can touch, at most
    int pw[3], ph[3];
    int n, shift, mask, par_a;
};

// The 16 bytes at p, an address that is a multiple of wd (1, 2, 4, 8 or 16; at least the sample's width): 16 / wd loads of wd
// bytes.  Where crop_sums_kernel (csrc/uva_crop.hip) picks the width per load from the address, the rows here lie a whole number
// of rows from a slot that is 16-byte aligned, so the width is a property of the plane's row length: the same in every lane,
// and the branches are scalar.
template <int BYTES>
__device__ __forceinline__ uint4 load_unit(const uint8_t* p, uint32_t wd)
{
    if (wd >= 16) return *(const uint4*)p;
    if (wd == 8) {
        const uint2 a = *(const uint2*)p, b = *(const uint2*)(p + 8);
        return make_uint4(a.x, a.y, b.x, b.y);
    }
    if (wd == 4) {
        const uint32_t* q = (const uint32_t*)p;
        return make_uint4(q[0], q[1], q[2], q[3]);
    }
    if (BYTES == 2 || wd == 2) {
        const uint16_t* q = (const uint16_t*)p;
        return make_uint4(q[0] | ((uint32_t)q[1] << 16), q[2] | ((uint32_t)q[3] << 16), q[4] | ((uint32_t)q[5] << 16),
                          q[6] | ((uint32_t)q[7] << 16));
    }
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        w[k] = p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// the code value of the sample at byte `o` (a constant once unrolled) of the words w
template <int BYTES>
__device__ __forceinline__ int unit_sample(const uint32_t* w, int o, int shift, int mask)
{
    if (BYTES == 1) return (int)((w[o >> 2] >> (8 * (o & 3))) & 255u);
    return (int)((((w[o >> 2] >> (8 * (o & 2))) & 0xffffu) >> shift) & (uint32_t)mask);
}

template <int BYTES>
__device__ __forceinline__ int unit_sample(const uint4& v, int o, int shift, int mask)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    return unit_sample<BYTES>(w, o, shift, mask);
}

// One row of the search, cur[ym] or cur[yp]: the slot's 16 bytes with the unit on either side, and for the one format whose
// halo of 3 * ST samples is longer than a unit (bgr48le: 18 bytes) the word beyond each.  The slot is worked on a word of four
// bytes at a time; next() moves the window on by a word, so the taps of a step sit at the same places of w in every step.
template <int BYTES, int ST>
struct SearchRow {
    static constexpr int HB = 3 * ST * BYTES;      // halo bytes on either side
    uint32_t w[12];
    uint32_t xl, xr;
    // the row at `row` (the same in every lane), the slot cb >= max(16, HB) bytes into it
    __device__ __forceinline__ void load(const uint8_t* row, uint32_t cb, uint32_t wd)
    {
        const uint8_t* p = row + (cb - 16u);       // (a scalar base and one 32-bit lane offset; the rest are immediates)
        const uint4 l = load_unit<BYTES>(p, wd), m = load_unit<BYTES>(p + 16, wd), r = load_unit<BYTES>(p + 32, wd);
        w[0] = l.x; w[1] = l.y; w[2] = l.z; w[3] = l.w;
        w[4] = m.x; w[5] = m.y; w[6] = m.z; w[7] = m.w;
        w[8] = r.x; w[9] = r.y; w[10] = r.z; w[11] = r.w;
        xl = xr = 0;
        if (HB > 16) {
            xl = *(const uint16_t*)(row + (cb - 18u));
            xr = *(const uint16_t*)(p + 48);
        }
    }
    // the sample `rel` bytes from the window's word in work, -HB <= rel < 4 + HB
    __device__ __forceinline__ int at(int rel, int shift, int mask) const
    {
        if (rel < -16) return (int)(((xl & 0xffffu) >> shift) & (uint32_t)mask);
        return unit_sample<BYTES>(w, rel + 16, shift, mask);
    }
    __device__ __forceinline__ void next()
    {
        if (HB > 16) xl = w[0] >> 16;
#pragma unroll
        for (int i = 0; i < 11; ++i) w[i] = w[i + 1];
        w[11] = xr;
    }
};

__device__ __forceinline__ void next_word(uint4& v) { v.x = v.y; v.y = v.z; v.z = v.w; }

// The slot of row y of plane p that begins `cb` bytes into the row and has `nb` bytes (16 unless it is the row's first or last):
// the interpolated samples go to `out`.  y and every pointer are the same in all lanes of a wave -- rows of the plane in the
// frames, `out` the row in the output -- and cb is the lane's own, so an access is a scalar base with a 32-bit lane offset.  A
// whole slot with a unit (bgr48le: 18 bytes) of the row on either side takes the wide path: every sample of it is an inner
// column.  The slots at a row's two ends go sample by sample through deint_sample_mem, which knows the edge columns.
template <int BYTES, int ST>
__device__ __forceinline__ void deint_slot(const DeintArgs& a, int p, int y, uint32_t cb, uint32_t nb, const uint8_t* prev, const uint8_t* cur,
                                           const uint8_t* next, const uint8_t* p2, const uint8_t* n2, uint8_t* out)
{
    constexpr int HB = 3 * ST * BYTES, HBR = HB > 16 ? HB : 16;
    const uint32_t row_bytes = a.row_bytes[p];
    // the load width of the rows one (w1) and two (w2) above and below a 16-byte aligned slot: the largest power of two, 16 at
    // most, that divides the row length (a multiple of BYTES), and that of twice the row length
    const uint32_t g = row_bytes & 15u, w1 = g ? (g & (0u - g)) : 16u, w2 = w1 >= 8 ? 16u : 2 * w1;
    const int shift = a.shift, mask = a.mask;
    const DeintRows r = deint_rows(y, a.ph[p]);
    if (nb == 16 && cb >= (uint32_t)HBR && cb + 16 + HBR <= row_bytes) {
        const size_t oy = (size_t)y * row_bytes, om = (size_t)r.ym * row_bytes, op = (size_t)r.yp * row_bytes;
        // First the temporal half, from the slot's own 16 bytes of twelve rows: d and the final diff of every sample, packed into
        // eight words.  Then the search over cur[ym] and cur[yp] with their halos.  Either half is a loop of four steps, a word of
        // four bytes each, that is NOT unrolled: after a step every unit moves on by a word, so the body is the same code on the
        // same registers.  Unrolled, the sixteen samples' unpacked taps are all in flight at once and the kernel needs more than
        // a hundred registers, or scratch under a bound; like this it needs 72 at the most, for a register move per word and step.
        constexpr int SPW = 4 / BYTES;      // samples of a word
        constexpr uint32_t VM = BYTES == 1 ? 0xffu : 0xffffu;
        uint32_t dd[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) dd[k] = 0;
        {
            uint4 cm = load_unit<BYTES>(cur + om + cb, w1), cp = load_unit<BYTES>(cur + op + cb, w1);
            uint4 p2y = load_unit<BYTES>(p2 + oy + cb, 16), n2y = load_unit<BYTES>(n2 + oy + cb, 16);
            uint4 pm = load_unit<BYTES>(prev + om + cb, w1), pp = load_unit<BYTES>(prev + op + cb, w1);
            uint4 nm = load_unit<BYTES>(next + om + cb, w1), np = load_unit<BYTES>(next + op + cb, w1);
            // (a row without rows y -+ 2 reads row y in their place, deint_rows, and the rule then ignores what it read)
            const size_t omm = (size_t)r.ymm * row_bytes, opp = (size_t)r.ypp * row_bytes;
            uint4 p2mm = load_unit<BYTES>(p2 + omm + cb, w2), n2mm = load_unit<BYTES>(n2 + omm + cb, w2);
            uint4 p2pp = load_unit<BYTES>(p2 + opp + cb, w2), n2pp = load_unit<BYTES>(n2 + opp + cb, w2);
#pragma unroll 1
            for (int q = 0; q < 4; ++q) {
                uint32_t lo2 = 0, hi2 = 0;
#pragma unroll
                for (int k = 0; k < SPW; ++k) {
                    const int o = k * BYTES;
                    int d, diff;
                    deint_temporal(unit_sample<BYTES>(cm, o, shift, mask), unit_sample<BYTES>(cp, o, shift, mask),
                                   unit_sample<BYTES>(p2y, o, shift, mask), unit_sample<BYTES>(n2y, o, shift, mask),
                                   unit_sample<BYTES>(pm, o, shift, mask), unit_sample<BYTES>(pp, o, shift, mask),
                                   unit_sample<BYTES>(nm, o, shift, mask), unit_sample<BYTES>(np, o, shift, mask), r.full,
                                   unit_sample<BYTES>(p2mm, o, shift, mask), unit_sample<BYTES>(n2mm, o, shift, mask),
                                   unit_sample<BYTES>(p2pp, o, shift, mask), unit_sample<BYTES>(n2pp, o, shift, mask), &d, &diff);
                    // (both are code values: 8 * BYTES bits each, d in the low half of the sample's 16 * BYTES bits)
                    const uint32_t both = ((uint32_t)d | ((uint32_t)diff << (8 * BYTES))) << (8 * ((2 * o) & 3));
                    if (2 * o < 4) lo2 |= both;
                    else hi2 |= both;
                }
#pragma unroll
                for (int k = 0; k < 6; ++k) dd[k] = dd[k + 2];
                dd[6] = lo2; dd[7] = hi2;
                next_word(cm); next_word(cp); next_word(p2y); next_word(n2y); next_word(pm); next_word(pp); next_word(nm); next_word(np);
                next_word(p2mm); next_word(n2mm); next_word(p2pp); next_word(n2pp);
            }
        }
        SearchRow<BYTES, ST> sm, sq;
        sm.load(cur + om, cb, w1);
        sq.load(cur + op, cb, w1);
        uint32_t res[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (int q = 0; q < 4; ++q) {
            uint32_t word = 0;
#pragma unroll
            for (int k = 0; k < SPW; ++k) {
                const int o = k * BYTES;
                int tm[7], tp[7];
#pragma unroll
                for (int t = 0; t < 7; ++t) {
                    tm[t] = sm.at(o + (t - 3) * ST * BYTES, shift, mask);
                    tp[t] = sq.at(o + (t - 3) * ST * BYTES, shift, mask);
                }
                const uint32_t both = dd[(2 * o) >> 2] >> (8 * ((2 * o) & 3));
                const int sp = deint_clamp(deint_spatial(tm, tp, true), (int)(both & VM), (int)((both >> (8 * BYTES)) & VM));
                word |= (BYTES == 1 ? (uint32_t)sp : (uint32_t)sp << shift) << (8 * o);
            }
            res[0] = res[1]; res[1] = res[2]; res[2] = res[3]; res[3] = word;
#pragma unroll
            for (int k = 0; k < 6; ++k) dd[k] = dd[k + 2];
            sm.next();
            sq.next();
        }
        *(uint4*)(out + cb) = make_uint4(res[0], res[1], res[2], res[3]);
        return;
    }
    for (uint32_t b = cb; b < cb + nb; b += BYTES) {
        const int sp = deint_sample_mem<BYTES>(prev, cur, next, p2, n2, row_bytes, a.pw[p], a.ph[p], ST, shift, mask, y, (int)(b / BYTES));
        if (BYTES == 1) out[b] = (uint8_t)sp;
        else *(uint16_t*)(out + b) = (uint16_t)((uint32_t)sp << shift);
    }
}

// Lane per 16-byte slot of a row, wave per run of 64 slots of ONE row, the slots counted from the 16-byte boundary at or below
// the row's first byte: the frames start at 16-byte aligned addresses, so a slot is aligned in every frame and in the outputs,
// and the copy of a kept row and the store of an interpolated one are 16-byte accesses except at a row's ragged ends.  The row,
// its field and with them every base address are the wave's, in scalar registers.  Every byte of an output is written by exactly
// one lane.  STRIDE 2 (nv12, p010le): plane 0 is the luma plane, of stride 1.
template <int BYTES, int ST>
__device__ __forceinline__ void deint_plane(const DeintArgs& a, int p, uint32_t lane, uint32_t wave, uint32_t nwaves)
{
    const uint32_t row_bytes = a.row_bytes[p], runs = (a.slots[p] + 63u) / 64u;
    const uint32_t total = (uint32_t)a.ph[p] * runs;
    for (uint32_t c = wave; c < total; c += nwaves) {
        const uint32_t y = c / runs, s = (c % runs) * 64u + lane;
        const uint32_t row_lo = a.off[p] + y * row_bytes, row_hi = row_lo + row_bytes;
        const uint32_t slot = (row_lo & ~15u) + 16u * s;
        const uint32_t lo = slot > row_lo ? slot : row_lo, hi = slot + 16 < row_hi ? slot + 16 : row_hi;
        if (lo >= hi) continue;
        const uint32_t cb = lo - row_lo, nb = hi - lo;
        const bool in_a = (int)(y & 1) == a.par_a;               // the row that output A interpolates and output B keeps
        uint8_t* keep = in_a ? a.out_b : a.out_a;
        uint8_t* out = in_a ? a.out_a : a.out_b;
        if (keep) {
            const uint8_t* src = a.cur + row_lo;
            uint8_t* dst = keep + row_lo;
            if (nb == 16) {
                *(uint4*)(dst + cb) = *(const uint4*)(src + cb);
            } else {
                for (uint32_t b = cb; b < cb + nb; b += BYTES) {
                    if (BYTES == 1) dst[b] = src[b];
                    else *(uint16_t*)(dst + b) = *(const uint16_t*)(src + b);
                }
            }
        }
        if (!out) continue;
        const uint8_t *prev = a.prev + a.off[p], *cur = a.cur + a.off[p], *next = a.next + a.off[p];
        deint_slot<BYTES, ST>(a, p, (int)y, cb, nb, prev, cur, next, in_a ? prev : cur, in_a ? cur : next, out + row_lo);
    }
}

template <int BYTES, int STRIDE>
__global__ __launch_bounds__(DI_THREADS, 7) void deint_kernel(DeintArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (DI_THREADS / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (DI_THREADS / 64);
    if (STRIDE == 2) {
        deint_plane<BYTES, 1>(a, 0, lane, wave, nwaves);
        deint_plane<BYTES, 2>(a, 1, lane, wave, nwaves);
    } else {
        for (int p = 0; p < a.n; ++p) deint_plane<BYTES, STRIDE>(a, p, lane, wave, nwaves);
    }
}

}  // namespace

hipError_t launch_deint(hipStream_t stream, const void* d_prev, const void* d_cur, const void* d_next, int fmt, int h, int w, int flags,
                        void* d_out_a, void* d_out_b, int max_groups)
{
    if (deint_error(fmt, h, w, flags) || !d_prev || !d_cur || !d_next || (!d_out_a && !d_out_b)) return hipErrorInvalidValue;
    if ((((uintptr_t)d_prev | (uintptr_t)d_cur | (uintptr_t)d_next | (uintptr_t)d_out_a | (uintptr_t)d_out_b) & 15) != 0) return hipErrorInvalidValue;
    const DeintFormat f = deint_format(fmt, h, w);
    DeintArgs a = {};
    a.prev = (const uint8_t*)d_prev; a.cur = (const uint8_t*)d_cur; a.next = (const uint8_t*)d_next;
    a.out_a = (uint8_t*)d_out_a; a.out_b = (uint8_t*)d_out_b;
    a.n = f.nplanes; a.shift = f.shift; a.mask = f.mask; a.par_a = deint_parity_a(flags);
    unsigned long long work = 0;
    int stride = 1;
    for (int p = 0; p < f.nplanes; ++p) {
        const DeintPlane& q = f.plane[p];
        if (q.off + q.row_bytes * (size_t)q.ph > 0xffffffffull || q.ph < 2) return hipErrorInvalidValue;
        a.off[p] = (uint32_t)q.off; a.row_bytes[p] = (uint32_t)q.row_bytes; a.pw[p] = q.pw; a.ph[p] = q.ph;
        a.slots[p] = (uint32_t)(q.row_bytes / 16 + 2);
        const unsigned long long t = (unsigned long long)q.ph * a.slots[p];
        work = t > work ? t : work;
        stride = q.stride > stride ? q.stride : stride;
    }
    const unsigned long long want = (work + DI_THREADS - 1) / DI_THREADS;
    uint32_t groups = want < 1 ? 1u : (want > (unsigned long long)DI_MAX_GROUPS ? (uint32_t)DI_MAX_GROUPS : (uint32_t)want);
    if (max_groups > 0 && groups > (uint32_t)max_groups) groups = (uint32_t)max_groups;
#define UVA_DEINT_LAUNCH(B, S) hipLaunchKernelGGL((deint_kernel<B, S>), dim3(groups), dim3(DI_THREADS), 0, stream, a)
    if (f.bytes == 1) {
        if (stride == 1) UVA_DEINT_LAUNCH(1, 1);
        else if (stride == 2) UVA_DEINT_LAUNCH(1, 2);
        else UVA_DEINT_LAUNCH(1, 3);
    } else {
        if (stride == 1) UVA_DEINT_LAUNCH(2, 1);
        else if (stride == 2) UVA_DEINT_LAUNCH(2, 2);
        else UVA_DEINT_LAUNCH(2, 3);
    }
#undef UVA_DEINT_LAUNCH
    return hipGetLastError();
}

}  // namespace uva
