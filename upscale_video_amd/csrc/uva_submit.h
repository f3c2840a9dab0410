// uva_submit.h -- the pipelined host route's arguments and arithmetic (uva_net_submit_* / uva_net_process_u8 / _u16 in
// csrc/uva_api.hip): what a call asks for (SubmitSpec) and everything that follows from that alone
// (SubmitPlan, csrc/uva_submit.cpp).  Plain C++ without HIP and without uva_net: functions of their arguments, built alone by
// tests/test_submit_plan.py and tests/test_submit_sanitized.py.
#pragma once
#include <stddef.h>

#include "uva_crop.h"
#include "uva_pixfmt.h"

namespace uva {

// one call of the route; the frame is h x w, strides are in bytes
struct SubmitSpec {
    int h = 0, w = 0;
    size_t in_stride = 0, out_stride = 0;    // of BGR frames (a packed frame of another format is dense; out_stride: of the frame that leaves)
    int tile_size = 0, border = 0;
    int in_fmt = PIX_BGR24, out_fmt = PIX_BGR24, colour = 0;
    int bits = 8;                            // 8: the net's frames are u8 BGR (BGR24); 16: u16 BGR (BGR48LE)
    int rs_oh = 0, rs_ow = 0, rs_filter = 0; // > 0 and other than the net's result size: the result is resampled to rs_oh x rs_ow
    void* png_ws = nullptr;                  // the PNG route: the result stays in HBM, its deflate blocks go to this page-locked
    size_t png_ws_bytes = 0;                 // workspace
    bool may_skip = false;                   // takes part in uva_net_set_skip_repeats (the uva_net_submit_* entries, not the PNG ones)
    bool windowed = false;                   // a pixel-format entry: uva_net_set_input_window applies
};

// uva_net_set_input_window: `in` is a dense src_h x src_w frame of in_fmt and the call's h x w the window at (x, y) of it
struct SubmitWindow {
    int src_h = 0, src_w = 0, x = 0, y = 0;
};

// the arguments a kept frame ran with (uva_net_set_skip_repeats: a frame is compared with the kept one only under the same key)
struct SubmitKey {
    int h, w, in_fmt, out_fmt, colour, u16, tile_size, border, res_h, res_w, filter;
    bool operator==(const SubmitKey& o) const
    {
        return h == o.h && w == o.w && in_fmt == o.in_fmt && out_fmt == o.out_fmt && colour == o.colour && u16 == o.u16 &&
               tile_size == o.tile_size && border == o.border && res_h == o.res_h && res_w == o.res_w && filter == o.filter;
    }
};

struct SubmitPlan {
    bool window_refused = false;             // the refusal returned is the window's (those come before the caller's pointer checks)
    // the net's frames
    size_t bps = 1;                          // bytes per sample
    size_t in_row = 0, out_row = 0, in_bytes = 0, out_bytes = 0;
    int out_h = 0, out_w = 0;                // the net's result: h x w times the scale
    int native = PIX_BGR24;                  // their format: BGR24 or BGR48LE
    // the frame that leaves: the net's result, or that resampled
    bool rs = false;
    int res_h = 0, res_w = 0;
    size_t res_row = 0, res_bytes = 0;
    // packed frames: in_fmt / out_fmt other than native
    bool pin = false, pout = false;
    size_t pin_bytes = 0, pout_bytes = 0;
    // the input window.  win_rows: a packed frame's planes go up as row ranges; win_cols: at full width into the staging, and
    // pix_window_kernel compacts the columns.  A window of a native frame is the frame at in_offset with the source's stride.
    bool win = false, win_rows = false, win_cols = false;
    WindowPlane wpl[3] = {};
    int wn = 0;
    size_t wstage[3] = {0, 0, 0}, wstage_bytes = 0;
    size_t in_offset = 0, in_stride = 0, out_stride = 0;   // (out_stride: the PNG route's is out_row)
    // the upload without win_rows: h2d_rows rows of h2d_row bytes (a packed frame is one row); packed_bytes: what then lies in HBM
    // (d_pin or d_in); h_in_bytes: the staging an unpinned source goes through
    size_t h2d_row = 0, packed_bytes = 0, h_in_bytes = 0;
    int h2d_rows = 0;
    // the download: dl_bytes, of the packed frame or of the frame that leaves.  Through the staging of an unpinned destination it
    // is dl_rows rows of dl_row bytes, dl_user_stride apart at the caller's; a packed frame is pout_bytes rows of one byte
    size_t dl_bytes = 0, dl_row = 0, dl_user_stride = 0;
    int dl_rows = 0;
    SubmitKey key = {};
};

// *out <- the plan of `spec` on a net of `scale` (win: the input window in force, null: none); returns null, or why the call is
// refused
const char* submit_plan(const SubmitSpec& spec, int scale, const SubmitWindow* win, SubmitPlan* out);

}  // namespace uva
