"""Numpy restatement of the 4:2:2 formats yuv422p / yuv422p10le (csrc/uva_pixfmt.hip) -- TESTS ONLY.

One chroma row per luma row: the horizontal axis of sections 7.3 / 7.5 (chroma_ref.up_axis / down_axis on axis 1) and nothing
on the vertical one.  Coefficients and shifts are pixfmt_ref's (u8 BGR) and pixfmt16_ref's (u16 BGR).  Every sum is added in
the kernels' order and asserted to fit the kernels' accumulator: int32 everywhere but the u16 inverse of the interpolating
modes, which is int64.  Every other format is handed to chroma_ref, so the calls here take all of ncnn.PIX_FORMATS_ALL.
Beside the fixed point, the float64 definition it approximates."""
import numpy as np

import chroma_ref as cr
import pixfmt16_ref as ref16
import pixfmt_ref as ref8

FORMATS422 = ("yuv422p", "yuv422p10le")
HCOSITED = {"left": True, "center": False, "topleft": True}       # the horizontal part of a siting: all a 4:2:2 format reads


def depth_of(fmt):
    return 10 if fmt == "yuv422p10le" else (8 if fmt == "yuv422p" else ref16.depth_of(fmt))


def frame_bytes(fmt, h, w):
    if fmt not in FORMATS422:
        return ref16.frame_bytes(fmt, h, w)
    return (w * h + 2 * ((w + 1) // 2) * h) * (2 if fmt == "yuv422p10le" else 1)


def planes(frame, fmt, h, w):
    """flat frame -> (Y [h][w], U [h][cw], V [h][cw]) int64 sample values (10 bits: word & 1023)"""
    cw = (w + 1) // 2
    a = np.asarray(frame, np.uint8).reshape(-1)
    assert a.size == frame_bytes(fmt, h, w)
    a = a.view("<u2").astype(np.int64) & 1023 if fmt == "yuv422p10le" else a.astype(np.int64)
    return a[:h * w].reshape(h, w), a[h * w:h * w + cw * h].reshape(h, cw), a[h * w + cw * h:].reshape(h, cw)


def pack(fmt, y, u, v):
    """sample planes -> flat u8 frame (10 bits: little-endian words, the high six bits zero)"""
    a = np.concatenate([np.asarray(t).ravel() for t in (y, u, v)])
    return a.astype("<u2").view(np.uint8) if fmt == "yuv422p10le" else a.astype(np.uint8)


def _route(u16):
    """(coefficient module, forward shift, inverse shift, largest BGR code)"""
    return (ref16, ref16.FWD_SH, ref16.INV_SH, 65535) if u16 else (ref8, 16, 16, 255)


# ---- per-sample fixed point, the kernels' order and accumulators ---------------------------------------------------------
def fwd_luma(r, g, b, matrix="bt601", full=False, depth=8, u16=False):
    mod, sh, _, _ = _route(u16)
    (cr_, cg, cb), _, _, yoff, _, maxv = mod.fwd_coefs(matrix, full, depth)
    r, g, b = (np.asarray(t, np.int64) for t in (r, g, b))
    return np.clip(cr._acc(32, cr_ * r, cg * g, cb * b, yoff << sh, 1 << (sh - 1)) >> sh, 0, maxv)


def fwd_chroma(sr, sg, sb, dl, matrix="bt601", full=False, depth=8, u16=False):
    """chroma from the (weighted) SUMS of R, G, B over 2^dl, dl a number or an array; int32 on both routes"""
    mod, sh, _, _ = _route(u16)
    _, (ur, ug, ub), (vr, vg, vb), _, coff, maxv = mod.fwd_coefs(matrix, full, depth)
    sr, sg, sb = (np.asarray(t, np.int64) for t in (sr, sg, sb))
    s = sh + np.asarray(dl, np.int64)
    u = np.clip(cr._acc(32, ur * sr, ug * sg, ub * sb, coff << s, 1 << (s - 1)) >> s, 0, maxv)
    v = np.clip(cr._acc(32, vr * sr, vg * sg, vb * sb, coff << s, 1 << (s - 1)) >> s, 0, maxv)
    return u, v


def inv_pixel_replicate(y, u, v, matrix="bt601", full=False, depth=8, u16=False):
    """Y' and its pair's chroma sample -> (b, g, r); int32 on both routes"""
    mod, _, sh, vmax = _route(u16)
    ky, rv, gu, gv, bu, yoff, coff = mod.inv_coefs(matrix, full, depth)
    yy = cr._acc(32, ky * (np.asarray(y, np.int64) - yoff))
    u = np.asarray(u, np.int64) - coff
    v = np.asarray(v, np.int64) - coff
    half = 1 << (sh - 1)
    tr, tg, tb = cr._acc(32, rv * v, half), cr._acc(32, gu * u, gv * v, half), cr._acc(32, bu * u, half)
    b, g, r = (np.clip(cr._acc(32, yy, t) >> sh, 0, vmax) for t in (tb, tg, tr))
    return b, g, r


def inv_pixel(y, us, vs, dl, matrix="bt601", full=False, depth=8, u16=False):
    """Y' and the chroma SUMS over 2^dl -> (b, g, r): section 7.5's form (int32 on the u8 route, int64 on the u16 route)"""
    return cr.inv_pixel(y, us, vs, dl, matrix, full, depth, u16)


# ---- float64 ---------------------------------------------------------------------------------------------------------
def float_inv_pixel(y, us, vs, dl, matrix="bt601", full=False, depth=8, u16=False):
    return cr.float_inv_pixel(y, us, vs, dl, matrix, full, depth, u16)


def float_fwd_chroma(sr, sg, sb, dl, matrix="bt601", full=False, depth=8, u16=False):
    return cr.float_fwd_chroma(sr, sg, sb, dl, matrix, full, depth, u16)


# ---- whole frames ------------------------------------------------------------------------------------------------------
def pix_to_bgr(frame, fmt, h, w, matrix="bt601", full=False, chroma_filter="replicate", chroma_loc="left", u16=False):
    """flat frame of `fmt` -> u8 (or, u16=True, u16) [h][w][3]"""
    if fmt not in FORMATS422:
        return cr.pix_to_bgr(frame, fmt, h, w, matrix, full, chroma_filter, chroma_loc, u16)
    y, u, v = planes(frame, fmt, h, w)
    if chroma_filter == "replicate":
        up = lambda a: np.repeat(a, 2, 1)[:, :w]   # noqa: E731
        b, g, r = inv_pixel_replicate(y, up(u), up(v), matrix, full, depth_of(fmt), u16)
    else:
        us, dl = cr.up_axis(u, w, HCOSITED[chroma_loc], 1)
        vs, _ = cr.up_axis(v, w, HCOSITED[chroma_loc], 1)
        b, g, r = inv_pixel(y, us, vs, dl, matrix, full, depth_of(fmt), u16)
    return np.stack([b, g, r], axis=-1).astype(np.uint16 if u16 else np.uint8)


def bgr_to_pix(bgr, fmt, matrix="bt601", full=False, chroma_filter="replicate", chroma_loc="left", u16=False):
    """u8 (or, u16=True, u16) [h][w][3] -> flat u8 frame of `fmt`"""
    if fmt not in FORMATS422:
        return cr.bgr_to_pix(bgr, fmt, matrix, full, chroma_filter, chroma_loc, u16)
    bgr = np.asarray(bgr, np.uint16 if u16 else np.uint8)
    h, w, _ = bgr.shape
    depth = depth_of(fmt)
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    y = fwd_luma(r, g, b, matrix, full, depth, u16)
    if chroma_filter == "replicate":
        cw = (w + 1) // 2
        pair = lambda a: np.pad(a, ((0, 0), (0, 2 * cw - w))).reshape(h, cw, 2).sum(axis=2)   # noqa: E731
        dl = np.where(np.arange(cw) * 2 + 1 < w, 1, 0)[None, :]        # a lone pixel at an odd right edge: >> SH
        sr, sg, sb = pair(r), pair(g), pair(b)
    else:
        (sr, dl), (sg, _), (sb, _) = (cr.down_axis(t, HCOSITED[chroma_loc], 1) for t in (r, g, b))
    u, v = fwd_chroma(sr, sg, sb, dl, matrix, full, depth, u16)
    return pack(fmt, y, u, v)


def convert(frame, in_fmt, out_fmt, h, w, matrix="bt601", full=False, chroma_filter="replicate", chroma_loc="left", bit_depth=8):
    """uva_pix_convert (bit_depth 8) / uva_pix_convert16 (16): in_fmt -> out_fmt through u8 / u16 BGR; a copy when the formats are equal"""
    if in_fmt == out_fmt:
        return np.asarray(frame).reshape(-1).view(np.uint8).copy()
    u16 = bit_depth == 16
    bgr = pix_to_bgr(frame, in_fmt, h, w, matrix, full, chroma_filter, chroma_loc, u16)
    return np.asarray(bgr_to_pix(bgr, out_fmt, matrix, full, chroma_filter, chroma_loc, u16)).reshape(-1).view(np.uint8)


def random_frame(rng, fmt, h, w):
    """a frame of random bytes: for the 10-bit format that is random words, garbage in the high six bits included"""
    return rng.integers(0, 256, frame_bytes(fmt, h, w), dtype=np.uint8)


def squeeze_to_420(frame, fmt, h, w, chroma_loc=None):
    """a 4:2:2 frame -> its 4:2:0 sibling (yuv420p / yuv420p10le) by the project's forward filter on the vertical axis alone: the
    pair's rounded mean (chroma_loc None: replicate's box) or the siting's vertical taps, rounded; Y' is kept"""
    y, u, v = planes(frame, fmt, h, w)
    out = []
    for c in (u, v):
        if chroma_loc is None:
            s, d = cr.down_axis(c, False, 0)
        else:
            s, d = cr.down_axis(c, cr.COSITED[chroma_loc][1], 0)
        out.append((s + (1 << (d - 1))) >> d)
    return ref16.pack("yuv420p10le" if fmt == "yuv422p10le" else "yuv420p", y, *out)
