// uva_repeat.hip -- the frame-difference kernel behind uva_frame_diff and the raw-video route's --skip-repeats (DESIGN.md section
// 7.8).  Two packed frames of one pixel format in HBM, a threshold T in code values -> three integers: how many samples differ by
// more than T, the largest absolute difference, the sum of absolute differences.
//
// The kernel runs on a net's upload stream while that net's persistent kernels own the compute units, so it is kept small: 256
// threads, 64 bytes of static LDS, no dynamic LDS, no scratch and a handful of VGPRs -- it fits beside a resident workgroup of
// any of them instead of waiting for one to leave.
#include "uva_repeat.h"

#include "uva_pixfmt.h"

namespace uva {

namespace {

constexpr int FD_THREADS = 256;        // four waves
constexpr int FD_WAVES = FD_THREADS / 64;
constexpr int FD_MAX_GROUPS = 1024;    // four workgroups per compute unit: beyond that a lane walks the frame in grid strides

// one 32-bit word of each frame: four byte samples, or two 16-bit words that are shifted and masked the way the input conversion
// reads them
template <int BYTES>
__device__ __forceinline__ void fd_word(uint32_t x, uint32_t y, uint32_t T, uint32_t shift, uint32_t mask, uint32_t& over,
                                        uint32_t& mx, uint32_t& sad)
{
    if (BYTES == 1) {
        sad = __builtin_amdgcn_sad_u8(x, y, sad);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t a = (x >> (8 * k)) & 255u, b = (y >> (8 * k)) & 255u;
            const uint32_t d = a > b ? a - b : b - a;
            mx = d > mx ? d : mx;
            over += d > T ? 1u : 0u;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint32_t a = (((x >> (16 * k)) & 0xffffu) >> shift) & mask, b = (((y >> (16 * k)) & 0xffffu) >> shift) & mask;
            const uint32_t d = a > b ? a - b : b - a;
            mx = d > mx ? d : mx;
            over += d > T ? 1u : 0u;
            sad += d;
        }
    }
}

// a, b: the frames as 16-byte units, nunits whole ones followed by tail_bytes (< 16, a multiple of BYTES) more bytes.
// The accumulators cannot overflow: check_dims admits h * w <= 2^28, the widest frame has three samples per pixel, so a frame
// has at most 3 * 2^28 < 2^32 samples and `over` fits 32 bits even in a lane that saw every one of them; a unit's sum is at most
// 16 * 255 or 8 * 65535 < 2^20 and goes into a 64-bit sum that 3 * 2^28 * 65535 < 2^46 cannot fill.
template <int BYTES>
__global__ __launch_bounds__(FD_THREADS) void frame_diff_kernel(const uint4* __restrict__ a, const uint4* __restrict__ b,
                                                                uint32_t nunits, uint32_t tail_bytes, uint32_t T, uint32_t shift,
                                                                uint32_t mask, FrameDiffStats* __restrict__ stats)
{
    uint32_t over = 0, mx = 0;
    unsigned long long sad = 0;
    const uint32_t stride = gridDim.x * FD_THREADS;     // nunits <= 6 * 2^28 / 16, stride <= 2^18: i + stride stays in 32 bits
    for (uint32_t i = blockIdx.x * FD_THREADS + threadIdx.x; i < nunits; i += stride) {
        const uint4 x = a[i], y = b[i];
        // equal units -- all of a repeated frame -- cost the two loads and this test
        if (((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) == 0) continue;
        uint32_t s = 0;
        fd_word<BYTES>(x.x, y.x, T, shift, mask, over, mx, s);
        fd_word<BYTES>(x.y, y.y, T, shift, mask, over, mx, s);
        fd_word<BYTES>(x.z, y.z, T, shift, mask, over, mx, s);
        fd_word<BYTES>(x.w, y.w, T, shift, mask, over, mx, s);
        sad += s;
    }
    // the last partial unit, sample by sample with loads of the sample's own width: nothing is read past the frame's last byte
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint8_t* ta = (const uint8_t*)(a + nunits);
        const uint8_t* tb = (const uint8_t*)(b + nunits);
        for (uint32_t j = 0; j < tail_bytes; j += BYTES) {
            uint32_t p, q;
            if (BYTES == 1) {
                p = ta[j]; q = tb[j];
            } else {
                p = ((uint32_t)(*(const uint16_t*)(ta + j)) >> shift) & mask;
                q = ((uint32_t)(*(const uint16_t*)(tb + j)) >> shift) & mask;
            }
            const uint32_t d = p > q ? p - q : q - p;
            mx = d > mx ? d : mx;
            over += d > T ? 1u : 0u;
            sad += d;
        }
    }
    // lanes of a wave through __shfl_xor, the four waves through LDS, then one set of integer atomics per workgroup: integer sums
    // do not depend on the order of arrival, the three numbers are exact
    uint32_t sad_lo = (uint32_t)sad, sad_hi = (uint32_t)(sad >> 32);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        over += __shfl_xor(over, off, 64);
        const uint32_t m = __shfl_xor(mx, off, 64);
        mx = m > mx ? m : mx;
        const unsigned long long o = ((unsigned long long)__shfl_xor(sad_hi, off, 64) << 32) | __shfl_xor(sad_lo, off, 64);
        sad += o;
        sad_lo = (uint32_t)sad; sad_hi = (uint32_t)(sad >> 32);
    }
    __shared__ uint32_t s_over[FD_WAVES], s_max[FD_WAVES];
    __shared__ unsigned long long s_sad[FD_WAVES];
    if ((threadIdx.x & 63) == 0) {
        s_over[threadIdx.x >> 6] = over;
        s_max[threadIdx.x >> 6] = mx;
        s_sad[threadIdx.x >> 6] = sad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < FD_WAVES; ++k) {
            over += s_over[k];
            mx = s_max[k] > mx ? s_max[k] : mx;
            sad += s_sad[k];
        }
        if (mx) {          // (a workgroup that found no difference has nothing to add)
            atomicAdd(&stats->over, (unsigned long long)over);
            atomicMax(&stats->max_abs, (unsigned long long)mx);
            atomicAdd(&stats->sad, sad);
        }
    }
}

}  // namespace

int frame_diff_sample(int fmt, unsigned* shift, unsigned* mask)
{
    unsigned sh = 0, mk = 0xffffu;
    int bytes = 0;
    switch (fmt) {
    case PIX_BGR24: case PIX_YUV420P: case PIX_NV12: case PIX_YUV422P: bytes = 1; mk = 0xffu; break;
    case PIX_P010LE: bytes = 2; sh = 6; break;
    case PIX_YUV420P10LE: case PIX_YUV422P10LE: bytes = 2; mk = 1023u; break;
    case PIX_BGR48LE: bytes = 2; break;
    default: break;
    }
    if (shift) *shift = sh;
    if (mask) *mask = mk;
    return bytes;
}

hipError_t launch_frame_diff(hipStream_t stream, const void* d_a, const void* d_b, size_t bytes, int fmt, unsigned threshold,
                             FrameDiffStats* d_stats)
{
    unsigned shift = 0, mask = 0;
    const int sb = frame_diff_sample(fmt, &shift, &mask);
    if (!sb || !d_a || !d_b || !d_stats || !bytes || bytes % (size_t)sb || bytes / 16 > 0xffffffffull ||
        (((uintptr_t)d_a | (uintptr_t)d_b) & 15) != 0)
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_stats, 0, sizeof(FrameDiffStats), stream);
    if (e != hipSuccess) return e;
    const uint32_t nunits = (uint32_t)(bytes / 16), tail = (uint32_t)(bytes % 16);
    const uint32_t want = (nunits + FD_THREADS - 1) / FD_THREADS;
    const uint32_t groups = want < 1 ? 1 : (want > (uint32_t)FD_MAX_GROUPS ? (uint32_t)FD_MAX_GROUPS : want);
    if (sb == 1)
        hipLaunchKernelGGL(frame_diff_kernel<1>, dim3(groups), dim3(FD_THREADS), 0, stream, (const uint4*)d_a, (const uint4*)d_b, nunits,
                           tail, threshold, shift, mask, d_stats);
    else
        hipLaunchKernelGGL(frame_diff_kernel<2>, dim3(groups), dim3(FD_THREADS), 0, stream, (const uint4*)d_a, (const uint4*)d_b, nunits,
                           tail, threshold, shift, mask, d_stats);
    return hipGetLastError();
}

}  // namespace uva
