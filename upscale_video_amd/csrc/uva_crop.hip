// uva_crop.hip -- the kernels behind uva_crop_sums and the input window (uva_crop.h).
//
// crop_sums_kernel: one pass over the luma plane of a Y'CbCr frame, or over all of a packed BGR frame, in HBM -> the exact sum of
// every row and of every column as 64-bit integers (check_dims admits h * w <= 2^28 pixels: a line sum of 16-bit samples does not
// fit 32 bits in general).  pix_window_kernel: the rows of a window as they were uploaded at full width -> the dense window frame,
// its columns compacted.
//
// Both run on a net's upload stream while that net's persistent kernels own the compute units, so they keep frame_diff_kernel's
// footprint (csrc/uva_repeat.hip): 256 threads, a kilobyte of static LDS at most, no dynamic LDS, no scratch, a bounded grid that
// walks the frame in strides -- they fit beside a resident workgroup of any of the nets' kernels instead of waiting for one to leave.
#include "uva_crop.h"

#include "uva_pixfmt.h"

namespace uva {

static_assert(CROP_BGR24 == PIX_BGR24 && CROP_YUV420P == PIX_YUV420P && CROP_NV12 == PIX_NV12 && CROP_P010LE == PIX_P010LE &&
              CROP_YUV420P10LE == PIX_YUV420P10LE && CROP_BGR48LE == PIX_BGR48LE && CROP_YUV422P == PIX_YUV422P &&
              CROP_YUV422P10LE == PIX_YUV422P10LE, "uva_crop.h restates uva_pixfmt.h's format codes");

namespace {

constexpr int CS_THREADS = 256;        // four waves
constexpr int CS_WAVES = CS_THREADS / 64;
constexpr int CS_MAX_GROUPS = 1024;    // four workgroups per compute unit: beyond that a workgroup walks the tiles in grid strides
constexpr int CS_BAND = 64;            // the most rows of a tile

// The 16 bytes at p, which lies `al` (= address & 15) past a 16-byte boundary: one 16-byte load where al is 0, else loads of the
// widest power of two that divides al, down to the sample's own width -- al is a multiple of BYTES.  al is the same for every
// lane of a wave (a row's alignment), so the branches are uniform.
template <int BYTES>
__device__ __forceinline__ uint4 load_unit(const uint8_t* p, uint32_t al)
{
    uint4 v;
    if ((al & 15) == 0) {
        v = *(const uint4*)p;
    } else if ((al & 7) == 0) {
        const uint2 a = *(const uint2*)p, b = *(const uint2*)(p + 8);
        v = make_uint4(a.x, a.y, b.x, b.y);
    } else if ((al & 3) == 0) {
        const uint32_t* q = (const uint32_t*)p;
        v = make_uint4(q[0], q[1], q[2], q[3]);
    } else if (BYTES == 2 || (al & 1) == 0) {
        const uint16_t* q = (const uint16_t*)p;
        v = make_uint4(q[0] | ((uint32_t)q[1] << 16), q[2] | ((uint32_t)q[3] << 16), q[4] | ((uint32_t)q[5] << 16),
                       q[6] | ((uint32_t)q[7] << 16));
    } else {
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            w[k] = p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
        v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return v;
}

// the first nbytes (< 16, a multiple of BYTES) bytes at p with loads of the sample's own width, the rest zero: nothing is read
// past p + nbytes
template <int BYTES>
__device__ __forceinline__ uint4 load_partial(const uint8_t* p, uint32_t nbytes)
{
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t j = 0; j < nbytes; j += BYTES) {
        const uint32_t s = BYTES == 1 ? (uint32_t)p[j] : (uint32_t)(*(const uint16_t*)(p + j));
        w[j >> 2] |= s << (8 * (j & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// A tile is up to `band` rows of one span of 256 units of 16 bytes (4096 bytes of every row, the units counted from the row's
// first byte): lane t of the workgroup owns unit span * 256 + t and walks the band's rows with it, so it holds the sums of its
// 16 / BYTES sample columns in registers (a band has at most 64 rows: 64 * 65535 fits 32 bits) and adds them to col_sums once
// per tile.  Every row's 256 unit sums are combined through __shfl_xor within a wave and through LDS between the four waves;
// thread r of the workgroup then adds row r's sum (at most 2048 * 65535 < 2^28) to row_sums.  So a workgroup issues one integer
// atomic per line of its tile -- two for a packed BGR column whose three samples lie in two lanes' units -- and none for a line
// whose sum is zero.  Integer sums do not depend on the order of arrival: the results are exact.
// comps: samples per pixel of a row (3: packed BGR, sample j of a row belongs to column j / 3; 1: a luma plane).
template <int BYTES>
__global__ __launch_bounds__(CS_THREADS) void crop_sums_kernel(const uint8_t* __restrict__ frame, uint32_t h, uint32_t w, uint32_t comps,
                                                               uint32_t shift, uint32_t mask, uint32_t band, uint32_t nspans,
                                                               uint32_t ntiles, unsigned long long* __restrict__ row_sums,
                                                               unsigned long long* __restrict__ col_sums)
{
    constexpr int SPU = 16 / BYTES;                          // samples per unit
    __shared__ uint32_t s_row[CS_WAVES][CS_BAND];
    const uint32_t row_bytes = w * comps * BYTES;            // <= 6 * 2^28: fits 32 bits
    const uint32_t full = row_bytes / 16, tail = row_bytes % 16;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t span = tile % nspans, r0 = (tile / nspans) * band;
        const uint32_t nr = h - r0 < band ? h - r0 : band;
        const uint32_t u = span * CS_THREADS + threadIdx.x;
        const uint32_t have = u < full ? 16u : (u == full ? tail : 0u);      // bytes of this lane's unit inside the row
        uint32_t acc[SPU];
#pragma unroll
        for (int k = 0; k < SPU; ++k) acc[k] = 0;
        // four rows' loads are issued before the first of them is used: the loop is bound by their latency, not by the adds
        for (uint32_t i0 = 0; i0 < nr; i0 += 4) {
            uint4 v4[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v4[q] = make_uint4(0, 0, 0, 0);
                if (i0 + q < nr) {
                    const size_t off = (size_t)(r0 + i0 + q) * row_bytes;
                    if (have == 16) v4[q] = load_unit<BYTES>(frame + off + (size_t)u * 16, (uint32_t)(off & 15));
                    else if (have) v4[q] = load_partial<BYTES>(frame + off + (size_t)u * 16, have);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t wd[4] = {v4[q].x, v4[q].y, v4[q].z, v4[q].w};
                uint32_t s = 0;
                if (BYTES == 1) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        s = __builtin_amdgcn_sad_u8(wd[k], 0u, s);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[4 * k + j] += (wd[k] >> (8 * j)) & 255u;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            // (a partial unit's missing samples and a missing row are zero words: shift and mask keep them zero)
                            const uint32_t c = (((wd[k] >> (16 * j)) & 0xffffu) >> shift) & mask;
                            acc[2 * k + j] += c;
                            s += c;
                        }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
                if (lane == 0 && i0 + q < nr) s_row[wave][i0 + q] = s;
            }
        }
        __syncthreads();
        if (threadIdx.x < nr) {
            unsigned long long t = 0;
#pragma unroll
            for (int k = 0; k < CS_WAVES; ++k) t += s_row[k][threadIdx.x];
            if (t) atomicAdd(&row_sums[r0 + threadIdx.x], t);
        }
        __syncthreads();                                      // (the next tile writes s_row again)
        // this lane's columns: sample j of the row belongs to column j / comps; neighbours of one column go as one atomic
        const uint32_t j0 = u * SPU, nj = have / BYTES;
        uint32_t col = 0, part = 0;
        for (uint32_t k = 0; k < (uint32_t)SPU; ++k) {
            if (k >= nj) break;
            const uint32_t c = (j0 + k) / comps;
            if (k && c != col) {
                if (part) atomicAdd(&col_sums[col], (unsigned long long)part);
                part = 0;
            }
            col = c;
            uint32_t a = 0;
#pragma unroll
            for (int q = 0; q < SPU; ++q) a = (uint32_t)q == k ? acc[q] : a;      // (acc stays in registers: no dynamic index)
            part += a;
        }
        if (nj && part) atomicAdd(&col_sums[col], (unsigned long long)part);
    }
}

struct WinArgs {
    unsigned long long src_off[3], dst_off[3];      // bytes: the plane's first window row in the staging (its column 0), the plane in dst
    uint32_t src_row[3], dst_row[3], xbytes[3], rows[3];
    uint32_t slots[3];                              // 16-byte slots of dst that a row can touch, at most
    int n;
};

// Thread per 16-byte slot of the dense window frame: a slot that lies whole inside a row is gathered from the staging -- whose
// address for it has any alignment, hence load_unit -- and stored as one 16-byte unit; the slots at a row's two ends, which the row
// shares with its neighbours, go sample by sample.  Every byte of dst is written by exactly one thread.
template <int BYTES>
__global__ __launch_bounds__(CS_THREADS) void pix_window_kernel(const uint8_t* __restrict__ stage, uint8_t* __restrict__ dst, WinArgs a)
{
    for (int p = 0; p < a.n; ++p) {
        const unsigned long long total = (unsigned long long)a.rows[p] * a.slots[p];
        const uint32_t src_row = a.src_row[p], dst_row = a.dst_row[p], slots = a.slots[p];
        for (unsigned long long i = (unsigned long long)blockIdx.x * CS_THREADS + threadIdx.x; i < total;
             i += (unsigned long long)gridDim.x * CS_THREADS) {
            const uint32_t r = (uint32_t)(i / slots), s = (uint32_t)(i % slots);
            const unsigned long long row_lo = a.dst_off[p] + (unsigned long long)r * dst_row, row_hi = row_lo + dst_row;
            const unsigned long long slot = (row_lo & ~15ull) + 16ull * s;
            const unsigned long long lo = slot > row_lo ? slot : row_lo, hi = slot + 16 < row_hi ? slot + 16 : row_hi;
            if (lo >= hi) continue;
            const uint8_t* src = stage + a.src_off[p] + (unsigned long long)r * src_row + a.xbytes[p] + (lo - row_lo);
            if (hi - lo == 16) {
                *(uint4*)(dst + lo) = load_unit<BYTES>(src, (uint32_t)((uintptr_t)src & 15));
            } else {
                for (uint32_t j = 0; j < (uint32_t)(hi - lo); j += BYTES) {
                    if (BYTES == 1) dst[lo + j] = src[j];
                    else *(uint16_t*)(dst + lo + j) = *(const uint16_t*)(src + j);
                }
            }
        }
    }
}

}  // namespace

hipError_t launch_crop_sums(hipStream_t stream, const void* d_frame, int fmt, int h, int w, unsigned long long* d_rows,
                            unsigned long long* d_cols, int max_groups)
{
    const CropSample cs = crop_sample(fmt);
    if (!cs.bytes || !d_frame || !d_rows || !d_cols || h < 1 || w < 1 || (long long)h * w > (1ll << 28) || ((uintptr_t)d_frame & 15) != 0)
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_rows, 0, sizeof(unsigned long long) * (size_t)h, stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(d_cols, 0, sizeof(unsigned long long) * (size_t)w, stream);
    if (e != hipSuccess) return e;
    const unsigned long long row_bytes = (unsigned long long)w * cs.comps * cs.bytes;
    const unsigned long long units = (row_bytes + 15) / 16;
    const uint32_t nspans = (uint32_t)((units + CS_THREADS - 1) / CS_THREADS);
    // shorter bands while the frame has few tiles, so that a 1080p plane spreads over some compute units -- but not short ones:
    // every tile ends in an atomic per column, and the w counters of col_sums lie in a few L2 channels that take them one by one
    uint32_t band = CS_BAND;
    while (band > 16 && (unsigned long long)nspans * ((h + band - 1) / band) < 32) band /= 2;
    const unsigned long long tiles = (unsigned long long)nspans * (((uint32_t)h + band - 1) / band);
    if (tiles > 0xffffffffull) return hipErrorInvalidValue;
    uint32_t groups = tiles > (unsigned long long)CS_MAX_GROUPS ? (uint32_t)CS_MAX_GROUPS : (uint32_t)tiles;
    if (max_groups > 0 && groups > (uint32_t)max_groups) groups = (uint32_t)max_groups;
    if (cs.bytes == 1)
        hipLaunchKernelGGL(crop_sums_kernel<1>, dim3(groups), dim3(CS_THREADS), 0, stream, (const uint8_t*)d_frame, (uint32_t)h, (uint32_t)w,
                           (uint32_t)cs.comps, (uint32_t)cs.shift, (uint32_t)cs.mask, band, nspans, (uint32_t)tiles, d_rows, d_cols);
    else
        hipLaunchKernelGGL(crop_sums_kernel<2>, dim3(groups), dim3(CS_THREADS), 0, stream, (const uint8_t*)d_frame, (uint32_t)h, (uint32_t)w,
                           (uint32_t)cs.comps, (uint32_t)cs.shift, (uint32_t)cs.mask, band, nspans, (uint32_t)tiles, d_rows, d_cols);
    return hipGetLastError();
}

hipError_t launch_pix_window(hipStream_t stream, const void* d_stage, const size_t* stage_off, void* d_dst, const WindowPlane* planes, int n,
                             int bytes)
{
    if (!d_stage || !stage_off || !d_dst || !planes || n < 1 || n > 3 || (bytes != 1 && bytes != 2) || ((uintptr_t)d_dst & 15) != 0)
        return hipErrorInvalidValue;
    WinArgs a = {};
    unsigned long long work = 0;
    for (int p = 0; p < n; ++p) {
        const WindowPlane& q = planes[p];
        if (q.src_row > 0xffffffffull || q.dst_row > 0xffffffffull || q.xbytes + q.dst_row > q.src_row || q.rows < 1 || !q.dst_row)
            return hipErrorInvalidValue;
        a.src_off[p] = stage_off[p]; a.dst_off[p] = q.dst_off;
        a.src_row[p] = (uint32_t)q.src_row; a.dst_row[p] = (uint32_t)q.dst_row; a.xbytes[p] = (uint32_t)q.xbytes; a.rows[p] = (uint32_t)q.rows;
        a.slots[p] = (uint32_t)(q.dst_row / 16 + 2);
        const unsigned long long t = (unsigned long long)q.rows * a.slots[p];
        work = t > work ? t : work;
    }
    a.n = n;
    const unsigned long long want = (work + CS_THREADS - 1) / CS_THREADS;
    const uint32_t groups = want < 1 ? 1u : (want > (unsigned long long)CS_MAX_GROUPS ? (uint32_t)CS_MAX_GROUPS : (uint32_t)want);
    if (bytes == 1) hipLaunchKernelGGL(pix_window_kernel<1>, dim3(groups), dim3(CS_THREADS), 0, stream, (const uint8_t*)d_stage, (uint8_t*)d_dst, a);
    else hipLaunchKernelGGL(pix_window_kernel<2>, dim3(groups), dim3(CS_THREADS), 0, stream, (const uint8_t*)d_stage, (uint8_t*)d_dst, a);
    return hipGetLastError();
}

}  // namespace uva
