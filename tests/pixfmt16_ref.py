"""Numpy restatement of the 16-bit route's conversions (csrc/uva_pixfmt.hip) -- TESTS ONLY.

u16 BGR (unorm16, v / 65535) <-> yuv420p / nv12 / p010le / yuv420p10le, bgr24 <-> u16 (v * 257, rint(v / 257)), and the 8-bit
route's yuv420p10le (p010le's arithmetic in planar words).  Fixed point exactly as the kernels (int32 sums: asserted here), and
the float64 formulas it approximates.  Frames are flat u8 arrays in ffmpeg's rawvideo layouts; u16 BGR frames are u16 [h][w][3]."""
import numpy as np

import pixfmt_ref as ref8

FORMATS16 = ("bgr24", "yuv420p", "nv12", "p010le", "yuv420p10le", "bgr48le")
FWD_SH, INV_SH = 19, 13
MATRICES = ref8.MATRICES


def frame_bytes(fmt, h, w):
    c = 2 * ((w + 1) // 2) * ((h + 1) // 2)
    return {"bgr24": 3 * w * h, "yuv420p": w * h + c, "nv12": w * h + c, "p010le": 2 * (w * h + c), "yuv420p10le": 2 * (w * h + c),
            "bgr48le": 6 * w * h}[fmt]


def depth_of(fmt):
    return 10 if fmt in ("p010le", "yuv420p10le") else 8


def _fix(c, sh):
    return int(np.floor(np.ldexp(c, sh) + 0.5))


def fwd_coefs(matrix, full, depth):
    kr, kb = MATRICES[matrix]
    kg = 1 - kr - kb
    ys, cs, yoff = ref8._ranges(full, depth)
    sy, sc = ys / 65535.0, cs / 65535.0
    f = lambda c: _fix(c, FWD_SH)   # noqa: E731
    y = [f(kr * sy), f(kg * sy), f(kb * sy)]
    u = [f(-kr / (2 * (1 - kb)) * sc), f(-kg / (2 * (1 - kb)) * sc), f(0.5 * sc)]
    v = [f(0.5 * sc), f(-kg / (2 * (1 - kr)) * sc), f(-kb / (2 * (1 - kr)) * sc)]
    return y, u, v, yoff, 1 << (depth - 1), (1 << depth) - 1


def inv_coefs(matrix, full, depth):
    kr, kb = MATRICES[matrix]
    kg = 1 - kr - kb
    ys, cs, yoff = ref8._ranges(full, depth)
    ky, kc = 65535.0 / ys, 65535.0 / cs
    f = lambda c: _fix(c, INV_SH)   # noqa: E731
    return (f(ky), f(2 * (1 - kr) * kc), f(-2 * kb * (1 - kb) / kg * kc), f(-2 * kr * (1 - kr) / kg * kc), f(2 * (1 - kb) * kc),
            yoff, 1 << (depth - 1))


def _i32(*parts):
    """the kernels add left to right in int32: every partial sum must fit"""
    acc = np.zeros((), np.int64)
    for p in parts:
        acc = acc + p
        assert np.all(np.abs(acc) < 2 ** 31), "int32 overflow"
    return acc


def fwd_luma(r, g, b, matrix="bt601", full=False, depth=10):
    (cr, cg, cb), _, _, yoff, _, maxv = fwd_coefs(matrix, full, depth)
    r, g, b = (np.asarray(t, np.int64) for t in (r, g, b))
    return np.clip(_i32(cr * r, cg * g, cb * b, yoff << FWD_SH, 1 << (FWD_SH - 1)) >> FWD_SH, 0, maxv)


def fwd_chroma(sr, sg, sb, n_log2, matrix="bt601", full=False, depth=10):
    """chroma from the SUMS of a block of 2^n_log2 u16 pixels"""
    _, (ur, ug, ub), (vr, vg, vb), _, coff, maxv = fwd_coefs(matrix, full, depth)
    sr, sg, sb = (np.asarray(t, np.int64) for t in (sr, sg, sb))
    s = FWD_SH + np.asarray(n_log2, np.int64)
    u = np.clip(_i32(ur * sr, ug * sg, ub * sb, coff << s, 1 << (s - 1)) >> s, 0, maxv)
    v = np.clip(_i32(vr * sr, vg * sg, vb * sb, coff << s, 1 << (s - 1)) >> s, 0, maxv)
    return u, v


def inv_pixel(y, u, v, matrix="bt601", full=False, depth=10):
    """-> (b, g, r) u16 codes"""
    ky, rv, gu, gv, bu, yoff, coff = inv_coefs(matrix, full, depth)
    yy = ky * (np.asarray(y, np.int64) - yoff)
    u = np.asarray(u, np.int64) - coff
    v = np.asarray(v, np.int64) - coff
    half = 1 << (INV_SH - 1)
    r = np.clip(_i32(yy, rv * v + half) >> INV_SH, 0, 65535)
    g = np.clip(_i32(yy, gu * u + gv * v + half) >> INV_SH, 0, 65535)
    b = np.clip(_i32(yy, bu * u + half) >> INV_SH, 0, 65535)
    return b, g, r


def widen(bgr8):
    return np.asarray(bgr8, np.uint16) * np.uint16(257)


def narrow(bgr16):
    """rint(v / 257): 257 is odd, so there is no tie and this is floor((v + 128) / 257)"""
    return ((np.asarray(bgr16, np.int64) + 128) // 257).astype(np.uint8)


# ---- float64 ------------------------------------------------------------------------------------------------------
def float_fwd(r, g, b, matrix="bt601", full=False, depth=10):
    """u16 samples -> (Y, Cb, Cr) float64 codes, unrounded"""
    return ref8.float_fwd(*(np.asarray(t, np.float64) * (255.0 / 65535.0) for t in (r, g, b)), matrix=matrix, full=full, depth=depth)


def float_inv(y, u, v, matrix="bt601", full=False, depth=10):
    """-> (b, g, r) float64 in 0..65535 units, unrounded and unclamped"""
    return tuple(t * (65535.0 / 255.0) for t in ref8.float_inv(y, u, v, matrix, full, depth))


# ---- layouts ------------------------------------------------------------------------------------------------------
def pack(fmt, y, u, v):
    """sample planes (int) -> flat u8 frame of a Y'CbCr format"""
    if fmt == "yuv420p":
        return np.concatenate([y.ravel(), u.ravel(), v.ravel()]).astype(np.uint8)
    if fmt == "yuv420p10le":
        return np.concatenate([y.ravel(), u.ravel(), v.ravel()]).astype("<u2").view(np.uint8)
    uv = np.stack([u, v], axis=-1).ravel()
    if fmt == "nv12":
        return np.concatenate([y.ravel(), uv]).astype(np.uint8)
    return (np.concatenate([y.ravel(), uv]).astype("<u2") << 6).view(np.uint8)


def planes(frame, fmt, h, w):
    """flat frame -> (Y, U, V) int64 sample values (p010le: word >> 6; yuv420p10le: word & 1023)"""
    if fmt in ("yuv420p", "nv12", "p010le"):
        return ref8.pix_planes(frame, fmt, h, w)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    a = np.asarray(frame, np.uint8).reshape(-1).view("<u2").astype(np.int64) & 1023
    return a[:h * w].reshape(h, w), a[h * w:h * w + cw * ch].reshape(ch, cw), a[h * w + cw * ch:].reshape(ch, cw)


def p010_to_yuv420p10(frame, h, w):
    """the same samples repacked: nv12's interleave in high bits -> planar in low bits"""
    return pack("yuv420p10le", *ref8.pix_planes(frame, "p010le", h, w))


def _blocks(h, w):
    ch, cw = (h + 1) // 2, (w + 1) // 2
    pad = lambda a: np.pad(a, ((0, 2 * ch - h), (0, 2 * cw - w)))   # noqa: E731
    blk = lambda a: pad(a).reshape(ch, 2, cw, 2).sum(axis=(1, 3))   # noqa: E731
    rows = np.where(np.arange(ch) * 2 + 1 < h, 2, 1)[:, None]
    cols = np.where(np.arange(cw) * 2 + 1 < w, 2, 1)[None, :]
    return blk, (rows - 1) + (cols - 1)


# ---- whole frames: the 16-bit route ---------------------------------------------------------------------------------
def bgr16_to_pix(bgr16, fmt, matrix="bt601", full=False):
    """u16 [h][w][3] -> flat u8 frame of `fmt` (bgr24: rint(v / 257); bgr48le: the samples)"""
    bgr16 = np.asarray(bgr16, np.uint16)
    if fmt == "bgr48le":
        return bgr16.astype("<u2").reshape(-1).view(np.uint8).copy()
    if fmt == "bgr24":
        return narrow(bgr16).reshape(-1)
    h, w, _ = bgr16.shape
    depth = depth_of(fmt)
    b, g, r = (bgr16[..., k].astype(np.int64) for k in range(3))
    y = fwd_luma(r, g, b, matrix, full, depth)
    blk, n_log2 = _blocks(h, w)
    u, v = fwd_chroma(blk(r), blk(g), blk(b), n_log2, matrix, full, depth)
    return pack(fmt, y, u, v)


def pix_to_bgr16(frame, fmt, h, w, matrix="bt601", full=False):
    """flat frame of `fmt` -> u16 [h][w][3] (bgr24: v * 257)"""
    if fmt == "bgr48le":
        return np.asarray(frame, np.uint8).reshape(-1).view("<u2").reshape(h, w, 3).astype(np.uint16)
    if fmt == "bgr24":
        return widen(np.asarray(frame, np.uint8).reshape(h, w, 3))
    y, u, v = planes(frame, fmt, h, w)
    up = lambda a: np.repeat(np.repeat(a, 2, 0), 2, 1)[:h, :w]   # noqa: E731
    b, g, r = inv_pixel(y, up(u), up(v), matrix, full, depth_of(fmt))
    return np.stack([b, g, r], axis=-1).astype(np.uint16)


def convert16(frame, in_fmt, out_fmt, h, w, matrix="bt601", full=False):
    """uva_pix_convert16: in_fmt -> out_fmt through u16 BGR (a copy when the formats are equal)"""
    if in_fmt == out_fmt:
        return np.asarray(frame).reshape(-1).view(np.uint8).copy()
    return bgr16_to_pix(pix_to_bgr16(frame, in_fmt, h, w, matrix, full), out_fmt, matrix, full)


# ---- the 8-bit route's yuv420p10le (u8 BGR <-> p010le's arithmetic, planar low-bit words) ------------------------
def bgr_to_pix8(bgr, fmt, matrix="bt601", full=False):
    if fmt == "yuv420p10le":
        h, w, _ = np.asarray(bgr).shape
        return p010_to_yuv420p10(ref8.bgr_to_pix(bgr, "p010le", matrix, full), h, w)
    return ref8.bgr_to_pix(bgr, fmt, matrix, full)


def pix_to_bgr8(frame, fmt, h, w, matrix="bt601", full=False):
    if fmt == "yuv420p10le":
        y, u, v = planes(frame, fmt, h, w)
        up = lambda a: np.repeat(np.repeat(a, 2, 0), 2, 1)[:h, :w]   # noqa: E731
        b, g, r = ref8.inv_pixel(y, up(u), up(v), matrix, full, 10)
        return np.stack([b, g, r], axis=-1).astype(np.uint8)
    return ref8.pix_to_bgr(frame, fmt, h, w, matrix, full)


def convert8(frame, in_fmt, out_fmt, h, w, matrix="bt601", full=False):
    """uva_pix_convert with yuv420p10le among the formats"""
    if in_fmt == out_fmt:
        return np.asarray(frame, np.uint8).reshape(-1).copy()
    return bgr_to_pix8(pix_to_bgr8(frame, in_fmt, h, w, matrix, full), out_fmt, matrix, full)
