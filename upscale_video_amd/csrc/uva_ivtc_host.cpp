// uva_ivtc_host.cpp -- the host half of the inverse telecine (uva_ivtc.h): plain C++, no HIP, every
// function a function of its arguments.  The refusals, the weave and the metric of tests/ivtc_ref.py sample by sample, the
// decision and the decimator; uva_ivtc_push decides with the same ivtc_choose and IvtcDecimator.
#include "uva_ivtc.h"

#include <string.h>

namespace uva {

const char* ivtc_error(int fmt, int h, int w, int flags, int T, int L)
{
    if (flags & ~IVTC_FLAGS) return "detelecine: unknown flag bits (UVA_IVTC_BFF | UVA_IVTC_KEEP_COMBED | UVA_IVTC_KEEP_ALL)";
    if (const char* e = deint_error(fmt, h, w, 0)) return e;
    if (T < 0 || T > 255) return "detelecine: the comb threshold T is 0 ... 255 on the 8-bit scale";
    if (L < 0 || L > 1000000) return "detelecine: the combed limit L is 0 ... 1000000 parts per million";
    return nullptr;
}

void ivtc_weave_host(const uint8_t* cur, const uint8_t* x, int fmt, int h, int w, int flags, uint8_t* out)
{
    const DeintFormat f = deint_format(fmt, h, w);
    const int first = ivtc_first(flags);
    for (int p = 0; p < f.nplanes; ++p) {
        const DeintPlane& pl = f.plane[p];
        for (int y = 0; y < pl.ph; ++y) {
            const size_t o = pl.off + (size_t)y * pl.row_bytes;
            memcpy(out + o, ((y & 1) == first ? cur : x) + o, pl.row_bytes);
        }
    }
}

namespace {

template <int BYTES>
void ivtc_metric_one(const uint8_t* cur, const uint8_t* x, const DeintFormat& f, int first, unsigned thr, unsigned long long* n_out,
                     unsigned long long* m_out)
{
    const DeintPlane& pl = f.plane[0];
    const size_t n = (size_t)pl.pw * pl.stride;
    unsigned long long count = 0, sum = 0;
    for (int y = 1; y + 1 < pl.ph; ++y) {
        // row r of the woven frame lies in cur (first field) or in x
        const bool kept = (y & 1) == first;
        const uint8_t* ra = (kept ? x : cur) + pl.off + (size_t)(y - 1) * pl.row_bytes;
        const uint8_t* rb = (kept ? cur : x) + pl.off + (size_t)y * pl.row_bytes;
        const uint8_t* rc = (kept ? x : cur) + pl.off + (size_t)(y + 1) * pl.row_bytes;
        for (size_t j = 0; j < n; ++j) {
            const int a = deint_read<BYTES>(ra, j, f.shift, f.mask), b = deint_read<BYTES>(rb, j, f.shift, f.mask),
                      c = deint_read<BYTES>(rc, j, f.shift, f.mask);
            const int d1 = b - a, d2 = b - c;
            const int m = deint_min(deint_abs(d1), deint_abs(d2));
            if (((d1 > 0 && d2 > 0) || (d1 < 0 && d2 < 0)) && (unsigned)m > thr) {
                ++count;
                sum += (unsigned)m;
            }
        }
    }
    *n_out = count;
    *m_out = sum;
}

}  // namespace

void ivtc_metrics_host(const uint8_t* prev, const uint8_t* cur, const uint8_t* next, int fmt, int h, int w, int flags, int T,
                       unsigned long long* stats)
{
    const DeintFormat f = deint_format(fmt, h, w);
    const uint8_t* x[3] = {cur, prev ? prev : cur, next ? next : cur};
    const unsigned thr = ivtc_threshold(f, T);
    for (int k = 0; k < 3; ++k) {
        if (f.bytes == 1) ivtc_metric_one<1>(cur, x[k], f, ivtc_first(flags), thr, &stats[2 * k], &stats[2 * k + 1]);
        else ivtc_metric_one<2>(cur, x[k], f, ivtc_first(flags), thr, &stats[2 * k], &stats[2 * k + 1]);
    }
}

bool ivtc_choose(const unsigned long long* stats, int rows, long long samples_per_row, int L, int* match)
{
    int k = IVTC_C;
    if (stats[2 * IVTC_P + 1] < stats[2 * k + 1]) k = IVTC_P;
    if (stats[2 * IVTC_N + 1] < stats[2 * k + 1]) k = IVTC_N;
    *match = k;
    // N <= 3 * 2^28 and 10^6 < 2^20; L * rows * samples <= 10^6 * 3 * 2^28: both sides fit 64 bits
    return stats[2 * k] * 1000000ull > (unsigned long long)L * (unsigned long long)rows * (unsigned long long)samples_per_row;
}

void IvtcDecimator::reset(bool keep_all_frames)
{
    *this = IvtcDecimator();
    keep_all = keep_all_frames;
}

void IvtcDecimator::put(long long frame)
{
    if (len < QUEUE) queue[(head + len++) % QUEUE] = frame;      // (never full: see the struct's comment)
}

void IvtcDecimator::add(unsigned long long d)
{
    if (keep_all) {
        put(base++);
        return;
    }
    diff[pos++] = d;
    if (pos < CYCLE) return;
    int drop = 0;
    for (int k = 1; k < CYCLE; ++k)
        if (diff[k] < diff[drop]) drop = k;              // (strictly smaller: ties drop the earliest)
    for (int k = 0; k < CYCLE; ++k)
        if (k != drop) put(base + k);
    ++dropped;
    base += CYCLE;
    pos = 0;
}

void IvtcDecimator::end()
{
    for (int k = 0; k < pos; ++k) put(base + k);
    base += pos;
    pos = 0;
}

bool IvtcDecimator::pop(long long* frame)
{
    if (!len) return false;
    *frame = queue[head];
    head = (head + 1) % QUEUE;
    --len;
    return true;
}

}  // namespace uva
