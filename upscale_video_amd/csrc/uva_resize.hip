// uva_resize.hip -- the resampler of the raw-video route: BGR frames of u8 or u16 samples to any output
// size within [1/4, 4] per axis, by a separable polyphase filter (lanczos-3, Keys bicubic, bilinear) with integer taps.
//
// The arithmetic, in the order the kernel adds (restated in tests/resize_ref.py):
//   tables   per axis n_in -> n_out: output sample d sits at c = (d + 0.5) n_in / n_out - 0.5; fs = max(1, n_in / n_out);
//            T = 2 ceil(a fs) taps starting at first = floor(c - a fs) + 1, weight f((k - c) / fs), normalised to sum 1, times
//            2^14, floored, the missing units given one each to the largest remainders (ties: lowest index); a tap beyond the
//            plane reads the nearest sample inside.
//   pass 1   VERTICAL, over every sample of the source columns a tile needs: s = sum_k taps_y[oy][k] * src[clamp(first_y[oy] + k)]
//            in int32, k ascending (exact: 65535 * sum|taps| < 2^31, so the order cannot matter); u8 keeps m = (s + 64) >> 7,
//            u16 keeps m = s.
//   pass 2   HORIZONTAL: s = sum_k taps_x[ox][k] * m[clamp(first_x[ox] + k)], k ascending, int32 for u8 and int64 for u16
//            (v_mad_i64_i32); the result is clamp((s + 2^20) >> 21, 0, 255) resp. clamp((s + 2^27) >> 28, 0, 65535).
//
// One launch per frame.  A workgroup of 192 threads owns a tile of 16 x 64 output pixels; the intermediate m of the tile -- 16
// rows of the source columns the tile's taps reach -- lives in LDS and never in HBM.  Pass 1 is channel-agnostic: a lane takes
// four neighbouring samples of a source row with one 4- (u8) or 8-byte (u16) load where the rows are aligned, sample by sample
// at the row's end and for unaligned frames; the row's taps and row addresses are wave-uniform, and the loads of all taps are
// in flight together (pass 1 is instantiated per tap-count class like pass 2, picked by a uniform switch).  Pass 2: thread t owns column-channel t of the
// tile (64 pixels x 3), keeps its taps and LDS offsets in registers (the kernel is instantiated per tap-count class, shorter
// rows padded with zero taps) and walks the 16 rows; neighbouring lanes read LDS words 1 (within a pixel) or 3 n apart.
#include "uva_own.h"
#include "uva_resize.h"

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <list>
#include <mutex>

namespace uva {

namespace {

constexpr int RS_TOH = 16, RS_TOW = 64, RS_THREADS = RS_TOW * 3, RS_WAVES = RS_THREADS / 64;
constexpr size_t RS_LDS_MAX = 64 * 1024;

struct ResizeArgs {
    const void* src;
    void* dst;
    const int32_t* first_x;
    const int16_t* taps_x;    // [ow][TXC], zero beyond tx
    const int32_t* first_y;
    const int16_t* taps_y;    // [oh][typ], zero beyond ty
    int h, w, oh, ow, tx, ty, typ;
    int pitch;                // words per LDS row (a multiple of 4)
    int wide;                 // source rows start at multiples of four samples' bytes: pass 1 may load four samples at once
    long long in_stride, out_stride;   // bytes
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// four samples s .. s + 3 of a row of n samples (s a multiple of 4); samples past the row's end read as 0 (nobody uses them)
template <typename T>
__device__ __forceinline__ void load4(const T* row, int s, int n, bool wide, int v[4])
{
    if (wide && s + 4 <= n) {
        if constexpr (sizeof(T) == 1) {
            const uint32_t x = *reinterpret_cast<const uint32_t*>(row + s);
            v[0] = x & 255; v[1] = (x >> 8) & 255; v[2] = (x >> 16) & 255; v[3] = x >> 24;
        } else {
            const uint2 x = *reinterpret_cast<const uint2*>(row + s);
            v[0] = x.x & 0xffff; v[1] = x.x >> 16; v[2] = x.y & 0xffff; v[3] = x.y >> 16;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = s + i < n ? (int)row[s + i] : 0;
    }
}

// pass 1, TYC taps at a time (taps_y rows are a.typ = nch * TYC long, zero beyond ty): the TYC loads of a lane's four samples
// are independent and issued together -- with a loop over a run-time tap count every load waits for the one before it, and the
// pass is bound by that latency (measured: 3x the time).  The two longest classes (16 and 24 taps: ratios below 1/2) go in two
// halves that add up in LDS -- unrolled in one piece they run the scalar registers over, and every instantiation pays for it.
template <typename T, int TYC>
__device__ __forceinline__ void resize_pass1(const ResizeArgs& a, int32_t* mid, int oy0, int nrows, int s0, int nq, int wave, int lane, int nch)
{
    constexpr bool U8 = sizeof(T) == 1;
    const int rowsamp = a.w * 3;
    for (int r = wave; r < nrows; r += RS_WAVES) {
        const int fy = a.first_y[oy0 + r];
        for (int c = 0; c < nch; ++c) {
        // wave-uniform, so they live in scalar registers: the taps two to a word, the rows as 32-bit byte offsets (the host
        // refuses source frames whose byte offsets pass 32 bits)
        const int32_t* tp = reinterpret_cast<const int32_t*>(a.taps_y + (size_t)(oy0 + r) * a.typ + c * TYC);
        int t2[TYC / 2];
        uint32_t rowoff[TYC];
#pragma unroll
        for (int k = 0; k < TYC / 2; ++k) t2[k] = tp[k];
#pragma unroll
        for (int k = 0; k < TYC; ++k) rowoff[k] = (uint32_t)clampi(fy + c * TYC + k, 0, a.h - 1) * (uint32_t)a.in_stride;
        const char* base = static_cast<const char*>(a.src);
        auto tap = [&](int k) { return k & 1 ? t2[k >> 1] >> 16 : (int)(int16_t)(t2[k >> 1] & 0xffff); };
        for (int q = lane; q < nq; q += 64) {
            const int s = s0 + 4 * q;
            int4* m4 = reinterpret_cast<int4*>(mid + r * a.pitch + 4 * q);
            int acc[4] = {0, 0, 0, 0};
            if (c) { const int4 m = *m4; acc[0] = m.x; acc[1] = m.y; acc[2] = m.z; acc[3] = m.w; }     // (this lane's own words)
            if (a.wide && s + 4 <= rowsamp) {
                // (the words as loaded stay in registers until their tap's turn: unpacked early they would take four each)
                using Raw = typename std::conditional<U8, uint32_t, uint2>::type;
                Raw raw[TYC];
#pragma unroll
                for (int k = 0; k < TYC; ++k) raw[k] = *reinterpret_cast<const Raw*>(base + (rowoff[k] + (uint32_t)s * (uint32_t)sizeof(T)));
#pragma unroll
                for (int k = 0; k < TYC; ++k) {
                    int v[4];
                    if constexpr (U8) {
                        v[0] = raw[k] & 255; v[1] = (raw[k] >> 8) & 255; v[2] = (raw[k] >> 16) & 255; v[3] = raw[k] >> 24;
                    } else {
                        v[0] = raw[k].x & 0xffff; v[1] = raw[k].x >> 16; v[2] = raw[k].y & 0xffff; v[3] = raw[k].y >> 16;
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] += v[i] * tap(k);
                }
            } else {
                // sample by sample (a row's last group, unaligned frames): four loads per tap, so a few taps at a time
                constexpr int CH = TYC % 4 == 0 ? 4 : (TYC % 3 == 0 ? 3 : 2);
#pragma unroll
                for (int k0 = 0; k0 < TYC; k0 += CH) {
                    int v[CH][4];
#pragma unroll
                    for (int k = 0; k < CH; ++k) load4<T>(reinterpret_cast<const T*>(base + rowoff[k0 + k]), s, rowsamp, false, v[k]);
#pragma unroll
                    for (int k = 0; k < CH; ++k) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[i] += v[k][i] * tap(k0 + k);
                    }
                }
            }
            if constexpr (U8) {
                if (c == nch - 1) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = (acc[i] + 64) >> 7;
                }
            }
            *m4 = make_int4(acc[0], acc[1], acc[2], acc[3]);
        }
        }
    }
}

template <typename T, int TXC>
__global__ __launch_bounds__(RS_THREADS) void resize_kernel(ResizeArgs a)
{
    extern __shared__ int32_t rs_mid[];     // [RS_TOH][pitch]
    constexpr bool U8 = sizeof(T) == 1;
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * RS_TOW, oy0 = blockIdx.y * RS_TOH;
    const int oxl = min(ox0 + RS_TOW, a.ow) - 1;
    const int nrows = min(RS_TOH, a.oh - oy0);
    // the source columns this tile's taps reach, and the first of them rounded down to a multiple of four samples
    const int xlo = clampi(a.first_x[ox0], 0, a.w - 1), xhi = clampi(a.first_x[oxl] + a.tx - 1, 0, a.w - 1);
    const int s0 = (xlo * 3) & ~3;
    const int nq = (xhi * 3 + 3 - s0 + 3) >> 2;

    // pass 1: vertical, wave-uniform output row, lanes over groups of four samples
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    switch (a.typ) {        // (uniform: the class of the vertical tap count)
    case 2: resize_pass1<T, 2>(a, rs_mid, oy0, nrows, s0, nq, wave, lane, 1); break;
    case 4: resize_pass1<T, 4>(a, rs_mid, oy0, nrows, s0, nq, wave, lane, 1); break;
    case 6: resize_pass1<T, 6>(a, rs_mid, oy0, nrows, s0, nq, wave, lane, 1); break;
    case 8: resize_pass1<T, 8>(a, rs_mid, oy0, nrows, s0, nq, wave, lane, 1); break;
    case 12: resize_pass1<T, 12>(a, rs_mid, oy0, nrows, s0, nq, wave, lane, 1); break;
    case 16: resize_pass1<T, 8>(a, rs_mid, oy0, nrows, s0, nq, wave, lane, 2); break;
    default: resize_pass1<T, 12>(a, rs_mid, oy0, nrows, s0, nq, wave, lane, 2); break;
    }
    __syncthreads();

    // pass 2: horizontal, thread = column-channel of the tile
    const int px = tid / 3, ch = tid - 3 * px, ox = ox0 + px;
    if (ox >= a.ow) return;
    int off[TXC], tap[TXC];
    const int fx = a.first_x[ox];
#pragma unroll
    for (int k = 0; k < TXC; ++k) {
        off[k] = clampi(fx + k, xlo, xhi) * 3 + ch - s0;       // (a padding tap, weight 0, stays inside the tile's columns)
        tap[k] = a.taps_x[(size_t)ox * TXC + k];
    }
    for (int r = 0; r < nrows; ++r) {
        const int32_t* m = rs_mid + r * a.pitch;
        T* out = reinterpret_cast<T*>(static_cast<char*>(a.dst) + (size_t)(oy0 + r) * a.out_stride) + ox * 3 + ch;
        if constexpr (U8) {
            int s = 0;
#pragma unroll
            for (int k = 0; k < TXC; ++k) s += __mul24(m[off[k]], tap[k]);      // (m has 17 bits, a tap 16: the full-rate multiply)
            *out = (T)clampi((s + (1 << 20)) >> 21, 0, 255);
        } else {
            long long s = 0;
#pragma unroll
            for (int k = 0; k < TXC; ++k) s += (long long)m[off[k]] * tap[k];
            s = (s + (1ll << 27)) >> 28;
            *out = (T)(s < 0 ? 0 : (s > 65535 ? 65535 : s));
        }
    }
}

// ---- the tables (host) --------------------------------------------------------------------------------------------------
const double RS_PI = 3.14159265358979323846;
const int RS_SUPPORT[RESIZE_NFILTER] = {3, 2, 1};

double sinc(double x) { return x == 0.0 ? 1.0 : std::sin(RS_PI * x) / (RS_PI * x); }

double weight(int filter, double x)
{
    x = std::fabs(x);
    switch (filter) {
    case RESIZE_LANCZOS: return x < 3.0 ? sinc(x) * sinc(x / 3.0) : 0.0;
    case RESIZE_BICUBIC:        // Keys, a = -0.5
        if (x < 1.0) return (1.5 * x - 2.5) * x * x + 1.0;
        if (x < 2.0) return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
        return 0.0;
    default: return x < 1.0 ? 1.0 - x : 0.0;
    }
}

// the tap-count classes resize_kernel is instantiated for
int tap_class(int t)
{
    for (int c : {2, 4, 6, 8, 12, 16, 24})
        if (t <= c) return c;
    return 0;
}

struct Table {
    int device, n_in, n_out, filter, t, pitch;
    std::vector<int32_t> first;      // host copy: the launch sizes the LDS rows from it
    DevPtr<int32_t> d_first;
    DevPtr<int16_t> d_taps;          // [n_out][pitch]
};
std::mutex g_rs_mu;
// (a list: entries stay where they are while others are added; never destroyed: no HIP call at process exit)
std::list<Table>& g_tables = *new std::list<Table>;
constexpr size_t RS_MAX_TABLES = 64;

void free_tables(int device)          // (g_rs_mu held; device < 0: all)
{
    for (auto it = g_tables.begin(); it != g_tables.end();) {
        if (device >= 0 && it->device != device) { ++it; continue; }
        (void)hipSetDevice(it->device);
        it = g_tables.erase(it);
    }
}

const Table* get_table(int device, int n_in, int n_out, int filter, std::string* err)
{
    for (const Table& t : g_tables)
        if (t.device == device && t.n_in == n_in && t.n_out == n_out && t.filter == filter) return &t;
    Table t{device, n_in, n_out, filter, 0, 0, {}, {}, {}};
    std::vector<int16_t> taps;
    t.t = resize_build_taps(n_in, n_out, filter, t.first, taps);
    if (!t.t) { *err = "resize: bad axis"; return nullptr; }
    t.pitch = tap_class(t.t);
    std::vector<int16_t> padded((size_t)n_out * t.pitch, 0);
    for (int d = 0; d < n_out; ++d) std::copy(taps.begin() + (size_t)d * t.t, taps.begin() + (size_t)(d + 1) * t.t, padded.begin() + (size_t)d * t.pitch);
    // synchronous copies: the table may be used from any stream as soon as this returns
    hipError_t e = alloc_into(t.d_first, (size_t)n_out * 4);
    if (e == hipSuccess) e = alloc_into(t.d_taps, padded.size() * 2);
    if (e == hipSuccess) e = hipMemcpy(t.d_first, t.first.data(), (size_t)n_out * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t.d_taps, padded.data(), padded.size() * 2, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        *err = std::string("resize tables: ") + hipGetErrorString(e);
        return nullptr;
    }
    g_tables.push_back(std::move(t));
    return &g_tables.back();
}

template <typename T, int TXC>
hipError_t launch_t(hipStream_t stream, dim3 grid, size_t lds, const ResizeArgs& a)
{
    hipLaunchKernelGGL((resize_kernel<T, TXC>), grid, dim3(RS_THREADS), lds, stream, a);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_c(int txc, hipStream_t stream, dim3 grid, size_t lds, const ResizeArgs& a)
{
    switch (txc) {
    case 2: return launch_t<T, 2>(stream, grid, lds, a);
    case 4: return launch_t<T, 4>(stream, grid, lds, a);
    case 6: return launch_t<T, 6>(stream, grid, lds, a);
    case 8: return launch_t<T, 8>(stream, grid, lds, a);
    case 12: return launch_t<T, 12>(stream, grid, lds, a);
    case 16: return launch_t<T, 16>(stream, grid, lds, a);
    case 24: return launch_t<T, 24>(stream, grid, lds, a);
    }
    return hipErrorInvalidValue;
}

}  // namespace

int resize_ntaps(int n_in, int n_out, int filter)
{
    if (resize_axis_error(n_in, n_out, filter)) return 0;
    const long long a = RS_SUPPORT[filter];
    // 2 ceil(a max(1, n_in / n_out)) in integers
    return (int)(2 * (n_in > n_out ? (a * n_in + n_out - 1) / n_out : a));
}

int resize_build_taps(int n_in, int n_out, int filter, std::vector<int32_t>& first, std::vector<int16_t>& taps)
{
    const int t = resize_ntaps(n_in, n_out, filter);
    if (!t) return 0;
    const double r = (double)n_in / (double)n_out, fs = r > 1.0 ? r : 1.0, a = RS_SUPPORT[filter];
    first.assign(n_out, 0);
    taps.assign((size_t)n_out * t, 0);
    double wgt[RESIZE_MAX_TAPS], rem[RESIZE_MAX_TAPS];
    int q[RESIZE_MAX_TAPS];
    for (int d = 0; d < n_out; ++d) {
        const double c = (d + 0.5) * n_in / n_out - 0.5;
        const int f = (int)std::floor(c - a * fs) + 1;
        double sum = 0.0;
        for (int k = 0; k < t; ++k) { wgt[k] = weight(filter, ((f + k) - c) / fs); sum += wgt[k]; }
        int total = 0, abs_total = 0;
        for (int k = 0; k < t; ++k) {
            const double v = wgt[k] / sum * RESIZE_ONE, fl = std::floor(v);
            q[k] = (int)fl; rem[k] = v - fl; total += q[k];
        }
        for (int left = RESIZE_ONE - total; left > 0; --left) {      // largest remainders first, ties: lowest index
            int best = 0;
            for (int k = 1; k < t; ++k)
                if (rem[k] > rem[best]) best = k;
            ++q[best]; rem[best] = -1.0;
        }
        for (int k = 0; k < t; ++k) abs_total += q[k] < 0 ? -q[k] : q[k];
        if (abs_total > 32767) return 0;         // pass 1's int32 sums rely on it (never seen: at most 1.55 * 2^14)
        first[d] = f;
        for (int k = 0; k < t; ++k) taps[(size_t)d * t + k] = (int16_t)q[k];
    }
    return t;
}

int launch_resize(hipStream_t stream, int device, const void* d_in, int h, int w, size_t in_stride, void* d_out, int oh, int ow,
                  size_t out_stride, int filter, int bits, std::string* err)
{
    if (bits != 8 && bits != 16) { *err = "resize: bits must be 8 or 16"; return 1; }
    if (const char* e = resize_axis_error(w, ow, filter)) { *err = e; return 1; }
    if (const char* e = resize_axis_error(h, oh, filter)) { *err = e; return 1; }
    if (!d_in || !d_out) { *err = "null frame pointer"; return 1; }
    const size_t bps = bits / 8;
    if (in_stride < (size_t)w * 3 * bps || out_stride < (size_t)ow * 3 * bps) { *err = "row stride too small"; return 1; }
    if (bits == 16 && ((((uintptr_t)d_in | (uintptr_t)d_out | in_stride | out_stride) & 1) != 0)) { *err = "16-bit frames need 2-byte aligned rows"; return 1; }
    if ((long long)h * w > (1ll << 28) || (long long)oh * ow > (1ll << 28)) { *err = "bad image size"; return 1; }
    if ((unsigned long long)in_stride * (unsigned long long)h > 0xffffffffull) { *err = "resize: source frames whose byte offsets pass 32 bits are not taken"; return 1; }
    std::lock_guard<std::mutex> lk(g_rs_mu);
    if (g_tables.size() + 2 > RS_MAX_TABLES) {
        // a caller that keeps changing geometry: this device's tables go, once nothing queued can still read one
        if (hipDeviceSynchronize() != hipSuccess) { *err = "hipDeviceSynchronize failed"; return 1; }
        free_tables(device);
        (void)hipSetDevice(device);
    }
    const Table* tx = get_table(device, w, ow, filter, err);
    const Table* ty = tx ? get_table(device, h, oh, filter, err) : nullptr;      // (a list: tx stays where it is)
    if (!tx || !ty) return 1;
    // the widest tile's LDS row, by the kernel's own formulas
    int pitch = 4;
    for (int ox0 = 0; ox0 < ow; ox0 += RS_TOW) {
        const int oxl = std::min(ox0 + RS_TOW, ow) - 1;
        const int xlo = std::min(std::max(tx->first[ox0], 0), w - 1), xhi = std::min(std::max(tx->first[oxl] + tx->t - 1, 0), w - 1);
        const int s0 = (xlo * 3) & ~3;
        pitch = std::max(pitch, ((xhi * 3 + 3 - s0 + 3) >> 2) * 4);
    }
    const size_t lds = (size_t)RS_TOH * pitch * 4;
    if (lds > RS_LDS_MAX) { *err = "resize: tile does not fit LDS"; return 1; }
    ResizeArgs a;
    a.src = d_in; a.dst = d_out;
    a.first_x = tx->d_first; a.taps_x = tx->d_taps; a.first_y = ty->d_first; a.taps_y = ty->d_taps;
    a.h = h; a.w = w; a.oh = oh; a.ow = ow; a.tx = tx->t; a.ty = ty->t; a.typ = ty->pitch;
    a.pitch = pitch;
    const size_t align = 4 * bps;
    a.wide = ((uintptr_t)d_in % align == 0 && in_stride % align == 0) ? 1 : 0;
    a.in_stride = (long long)in_stride; a.out_stride = (long long)out_stride;
    const dim3 grid((unsigned)((ow + RS_TOW - 1) / RS_TOW), (unsigned)((oh + RS_TOH - 1) / RS_TOH));
    const hipError_t e = bits == 8 ? launch_c<uint8_t>(tx->pitch, stream, grid, lds, a) : launch_c<uint16_t>(tx->pitch, stream, grid, lds, a);
    if (e != hipSuccess) { *err = std::string("resize_kernel: ") + hipGetErrorString(e); return 1; }
    return 0;
}

void resize_release_all()
{
    std::lock_guard<std::mutex> lk(g_rs_mu);
    free_tables(-1);
}

}  // namespace uva
