// uva_sub10.h -- what the host side (uva_api.hip) needs of sub10_kernel (csrc/uva_sub10.hip.h; its own translation unit,
// uva_sub10.hip): constants of the row lists, the argument block and the launcher.
//
// sub10_kernel runs the WHOLE 1x HurrDeblur SubCompact net (models/1x_HurrDeblur_SubCompact_nf24-nc8_244k_net_g.param:3-26:
// conv 3->24, 8 x conv 24->24, conv 24->3, + input; the reference's apply_model, upscale/upscale_processing.py:258-299) in one
// launch, u8 in -> u8 out -- and, since round 6, up to S10_MAXB FRAMES of one geometry in that one launch:
// a frame's strips are dealt out to the 256 workgroups in segments that each pay 20 warm-up rows and the launch pays the
// pipeline's 20 steps of fill and drain once, so k frames in one launch pay both once per k.
// sub10_kernel16 is the same net on one u16 frame (u16 in -> u16 out).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "uva_devutil.hip.h"

namespace uva {

// (the row lists' constants S10_WC, S10_NL, S10_VALID, S10_MAX_ROWS, S10_MAXB, S10_YBIAS, S10_FSHIFT, S10_MAX_H: uva_plan.h, through uva_devutil.hip.h)
constexpr int S10_NW = 12;                       // waves: 8 trunk layers, the first and the last layer on two waves each
constexpr int S10_DRAIN = 2 * S10_NL;            // steps after the last row went in until it has come out

struct Sub10Args {
    const uint8_t* src[S10_MAXB]; // u8 HWC BGR frames (one plane = a whole frame: apply_model, :263-288), one geometry
    uint8_t* dst[S10_MAXB];
    size_t src_stride;
    size_t dst_stride;
    int h, w;
    const uint4* rows;            // [gridDim.x][max_rows]: x = plane row y (may be outside), y = plane column of computed
                                  // column 0, z = 1: the last layer's row is written out; z >> 8 = the frame; w = rows to the
                                  // nearest row of the segment that is written out
    const int* nrows;             // [gridDim.x]
    int max_rows;
    const half8* wpk[S10_NL];     // pack_sub16 images
    const float* bias[S10_NL];    // [32] each, zero padded
    const float* slope[S10_NL];   // [32] each (none for the last layer)
    unsigned long long* dbg;      // UVA_INSTRUMENT builds: workgroup 0 stamps [step][wave][4] here
};

// sub10_kernel16's arguments: ONE u16 HWC BGR frame (the 16-bit route).  Strides are in bytes and even,
// like the pointers; the tail waves read the residual from `src` while neighbouring strips store to `dst`, so the two frames
// must not overlap.  Row lists, weights, biases and slopes are sub10_kernel's.
struct Sub10Args16 {
    const uint16_t* src;
    uint16_t* dst;
    size_t src_stride;
    size_t dst_stride;
    int h, w;
    const uint4* rows;
    const int* nrows;
    int max_rows;
    const half8* wpk[S10_NL];
    const float* bias[S10_NL];
    const float* slope[S10_NL];
    unsigned long long* dbg;
};

// One launch of sub10_kernel on `grid` workgroups of 768 threads.  Returns hipSuccess or the failing call's error.
hipError_t launch_sub10_kernel(hipStream_t stream, int grid, const Sub10Args& a);
// ... of sub10_kernel16 (row lists built for one frame)
hipError_t launch_sub10_kernel16(hipStream_t stream, int grid, const Sub10Args16& a);

}  // namespace uva
