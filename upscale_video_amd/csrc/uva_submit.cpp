// uva_submit.cpp -- the plan of one call of the pipelined host route (uva_submit.h): sizes, branches and refusals that follow
// from the arguments alone.  No HIP call, nothing of uva_net.
#include "uva_submit.h"

#include <limits.h>

namespace uva {

const char* submit_plan(const SubmitSpec& sp, int scale, const SubmitWindow* win, SubmitPlan* out)
{
    SubmitPlan& p = *out;
    p = SubmitPlan();
    const int h = sp.h, w = sp.w, s = scale;
    const bool u16 = sp.bits == 16;
    // only the upload knows of a window: it leaves the dense window frame where a whole frame's upload would
    p.win = win != nullptr;
    if (p.win) {
        if (const char* e = crop_window_error(sp.in_fmt, win->src_h, win->src_w, win->x, win->y, h, w)) {
            p.window_refused = true;
            return e;
        }
        p.wn = crop_window_planes(sp.in_fmt, win->src_h, win->src_w, win->x, win->y, h, w, p.wpl);
    }
    p.bps = u16 ? 2 : 1;
    p.in_row = (size_t)w * 3 * p.bps;
    p.out_row = (size_t)w * s * 3 * p.bps;
    p.out_h = h * s;
    p.out_w = w * s;
    p.rs = sp.rs_oh > 0 && sp.rs_ow > 0 && !(sp.rs_oh == p.out_h && sp.rs_ow == p.out_w);
    p.res_h = p.rs ? sp.rs_oh : p.out_h;
    p.res_w = p.rs ? sp.rs_ow : p.out_w;
    p.res_row = (size_t)p.res_w * 3 * p.bps;
    p.res_bytes = p.res_row * (size_t)p.res_h;
    p.in_stride = sp.in_stride;
    p.out_stride = sp.png_ws ? p.out_row : sp.out_stride;
    if (p.in_stride < p.in_row || p.out_stride < p.res_row) return "row stride too small";
    p.in_bytes = p.in_row * h;
    p.out_bytes = p.out_row * (size_t)h * s;
    p.native = u16 ? PIX_BGR48LE : PIX_BGR24;
    p.pin = sp.in_fmt != p.native;
    p.pout = sp.out_fmt != p.native;
    if (p.win && !p.pin) {
        // the net's own BGR layout: the window is the frame at an offset with the source's row stride, which the upload takes as it is
        p.in_offset = (size_t)p.wpl[0].row0 * p.wpl[0].src_row + p.wpl[0].xbytes;
        p.in_stride = p.wpl[0].src_row;
    }
    // a window over whole rows (a letterbox) is a contiguous row range of every plane; a narrower one goes up at full width and
    // pix_window_kernel compacts its columns
    p.win_rows = p.win && p.pin;
    p.win_cols = p.win_rows && p.wpl[0].dst_row != p.wpl[0].src_row;
    p.wstage_bytes = p.win_cols ? pix_window_staging(p.wpl, p.wn, p.wstage) : 0;
    p.pin_bytes = pix_frame_bytes(sp.in_fmt, h, w);
    p.pout_bytes = pix_frame_bytes(sp.out_fmt, p.res_h, p.res_w);
    if (p.pout_bytes > (size_t)INT_MAX) return "result frame of 2 GB or more";
    // (a packed frame goes up as one row of pin_bytes)
    p.h2d_row = p.pin ? p.pin_bytes : p.in_row;
    p.h2d_rows = p.pin ? 1 : h;
    p.packed_bytes = p.pin ? p.pin_bytes : p.in_bytes;
    p.h_in_bytes = p.win_cols ? p.wstage_bytes : p.packed_bytes;
    // what comes down: the BGR rows of the frame that leaves, or the packed frame -- as "rows" of one byte, so that a band is a
    // byte range (collect copies it with one memcpy)
    p.dl_bytes = p.pout ? p.pout_bytes : p.res_bytes;
    p.dl_row = p.pout ? 1 : p.res_row;
    p.dl_rows = p.pout ? (int)p.pout_bytes : p.res_h;
    p.dl_user_stride = p.pout ? 1 : p.out_stride;
    p.key = {h, w, sp.in_fmt, sp.out_fmt, sp.colour, u16 ? 1 : 0, sp.tile_size, sp.border, p.res_h, p.res_w, p.rs ? sp.rs_filter : 0};
    return nullptr;
}

}  // namespace uva
