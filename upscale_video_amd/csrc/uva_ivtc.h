// uva_ivtc.h -- inverse telecine on the raw-video route (include/uva.h uva_ivtc_*): field matching
// and decimation for 2:3 pulldown.  Two halves:
//   csrc/uva_ivtc_host.cpp  plain C++ without HIP: the refusals, a scalar restatement of the weave and the metric, the decision
//                           (ivtc_choose) and the decimator, a small state machine.  Functions of their arguments; built alone
//                           by tests/test_ivtc_sanitized.py.  The GPU path calls the same ivtc_choose and decimator.
//   csrc/uva_ivtc.hip       the kernel: ivtc_metrics_kernel<BYTES>.
// The rule is the one tests/ivtc_ref.py states for this project; parity with ffmpeg's fieldmatch / decimate is unpinned
// (section 7.15).  Formats and planes are those of uva_deint.h (deint_format): the table is not restated.
#pragma once
#include "uva_deint.h"

namespace uva {

enum { IVTC_BFF = 1, IVTC_KEEP_COMBED = 2, IVTC_KEEP_ALL = 4, IVTC_FLAGS = 7 };      // include/uva.h UVA_IVTC_*
enum { IVTC_C = 0, IVTC_P = 1, IVTC_N = 2 };                                          // the candidates, in the order of `stats`

// nullptr, or why uva_ivtc_* refuses h x w frames of fmt with these flags, T (8-bit scale) and L (parts per million)
const char* ivtc_error(int fmt, int h, int w, int flags, int T, int L);

// the parity (y & 1) of the rows that every candidate takes from cur: the first field
inline int ivtc_first(int flags) { return (flags & IVTC_BFF) ? 1 : 0; }
// the flags of the yadif output that keeps the same field (uva_deint.h: A keeps the first field)
inline int ivtc_deint_flags(int flags) { return (flags & IVTC_BFF) ? DEINT_BFF : 0; }
// the metric's threshold in code values of the format
inline unsigned ivtc_threshold(const DeintFormat& f, int T) { return (unsigned)T << (f.mask == 255 ? 0 : (f.mask == 1023 ? 2 : 8)); }

// out <- W_X: the rows of the first field of every plane from cur, the others from x, byte for byte
void ivtc_weave_host(const uint8_t* cur, const uint8_t* x, int fmt, int h, int w, int flags, uint8_t* out);

// stats[6] <- (N_c, M_c, N_p, M_p, N_n, M_n) of cur between prev and next (null: cur), on the host
void ivtc_metrics_host(const uint8_t* prev, const uint8_t* cur, const uint8_t* next, int fmt, int h, int w, int flags, int T,
                       unsigned long long* stats);

// the decision: *match <- the candidate with the smallest M (ties: c, p, n); returns whether it is combed,
// N * 10^6 > L * rows * samples_per_row (rows = ph - 2 of plane 0) -- in 64-bit integers that both sides fit, nothing rounds
bool ivtc_choose(const unsigned long long* stats, int rows, long long samples_per_row, int L, int* match);
// rows and samples per row of the metric for this format
inline void ivtc_metric_extent(const DeintFormat& f, int* rows, long long* samples)
{
    *rows = f.plane[0].ph - 2;
    *samples = (long long)f.plane[0].pw * f.plane[0].stride;
}

// The decimator.  Final frames are numbered from 0 since the last reset; add() takes the next one's diff, end() closes the
// stream (a trailing cycle of fewer than five loses none), pop() hands out the number of the next frame to deliver.  A full
// cycle is decided when its fifth diff arrives: the four that stay are queued, so at most one frame need leave per added
// frame and the queue never holds more than eight.
struct IvtcDecimator {
    static constexpr int CYCLE = 5, QUEUE = 16;
    bool keep_all = false;
    int pos = 0;                          // frames of the open cycle
    long long base = 0;                   // number of the open cycle's first frame
    unsigned long long diff[CYCLE] = {};
    long long queue[QUEUE] = {};
    int head = 0, len = 0;
    long long dropped = 0;

    void reset(bool keep_all_frames);
    void add(unsigned long long d);
    void end();
    bool pop(long long* frame);

private:
    void put(long long frame);
};
constexpr unsigned long long IVTC_FIRST_DIFF = ~0ull;

}  // namespace uva

#ifdef __HIPCC__
namespace uva {

// d_stats[6] (zeroed here, on `stream`) <- the six sums of d_cur between d_prev and d_next: one kernel.  Every frame starts at a
// 16-byte aligned address.  max_groups > 0 bounds the grid below the kernel's own bound (tests).
hipError_t launch_ivtc_metrics(hipStream_t stream, const void* d_prev, const void* d_cur, const void* d_next, int fmt, int h, int w,
                               int flags, int T, unsigned long long* d_stats, int max_groups = 0);

// d_out <- W_X of d_cur and d_x on `stream`: one strided 2-D copy per plane over a copy of d_cur (d_x == d_cur: the copy alone)
hipError_t launch_ivtc_weave(hipStream_t stream, const void* d_cur, const void* d_x, int fmt, int h, int w, int flags, void* d_out);

}  // namespace uva
#endif
