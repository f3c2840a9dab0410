"""Numpy restatement of the raw-video pixel formats (csrc/uva_pixfmt.hip) -- TESTS ONLY.

fixed-point functions (what the kernels must give bit for bit) and the float64 textbook formulas they approximate.
Frames are flat u8 arrays in ffmpeg's rawvideo layouts; BGR frames are u8 [h][w][3]."""
import numpy as np

FORMATS = ("bgr24", "yuv420p", "nv12", "p010le")
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def frame_bytes(fmt, h, w):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return {"bgr24": 3 * w * h, "yuv420p": w * h + 2 * cw * ch, "nv12": w * h + 2 * cw * ch, "p010le": 2 * (w * h + 2 * cw * ch)}[fmt]


def _fix16(c):
    return int(np.floor(c * 65536.0 + 0.5))


def _ranges(full, depth):
    ys = (1 << depth) - 1 if full else 219 << (depth - 8)
    cs = (1 << depth) - 1 if full else 224 << (depth - 8)
    return ys, cs, 0 if full else 16 << (depth - 8)


def fwd_coefs(matrix, full, depth):
    kr, kb = MATRICES[matrix]
    kg = 1 - kr - kb
    ys, cs, yoff = _ranges(full, depth)
    sy, sc = ys / 255.0, cs / 255.0
    y = [_fix16(kr * sy), _fix16(kg * sy), _fix16(kb * sy)]
    u = [_fix16(-kr / (2 * (1 - kb)) * sc), _fix16(-kg / (2 * (1 - kb)) * sc), _fix16(0.5 * sc)]
    v = [_fix16(0.5 * sc), _fix16(-kg / (2 * (1 - kr)) * sc), _fix16(-kb / (2 * (1 - kr)) * sc)]
    return y, u, v, yoff, 1 << (depth - 1), (1 << depth) - 1


def inv_coefs(matrix, full, depth):
    kr, kb = MATRICES[matrix]
    kg = 1 - kr - kb
    ys, cs, yoff = _ranges(full, depth)
    ky, kc = 255.0 / ys, 255.0 / cs
    return (_fix16(ky), _fix16(2 * (1 - kr) * kc), _fix16(-2 * kb * (1 - kb) / kg * kc), _fix16(-2 * kr * (1 - kr) / kg * kc),
            _fix16(2 * (1 - kb) * kc), yoff, 1 << (depth - 1))


# ---- per-sample fixed point (int64 numpy; the kernels' int32 sums never overflow) ------------------------------
def fwd_luma(r, g, b, matrix="bt601", full=False, depth=8):
    (cr, cg, cb), _, _, yoff, _, maxv = fwd_coefs(matrix, full, depth)
    r, g, b = (np.asarray(t, np.int64) for t in (r, g, b))
    return np.clip((cr * r + cg * g + cb * b + (yoff << 16) + 32768) >> 16, 0, maxv)


def fwd_chroma(sr, sg, sb, n_log2, matrix="bt601", full=False, depth=8):
    """chroma from the SUMS of a block of 2^n_log2 pixels"""
    _, (ur, ug, ub), (vr, vg, vb), _, coff, maxv = fwd_coefs(matrix, full, depth)
    sr, sg, sb = (np.asarray(t, np.int64) for t in (sr, sg, sb))
    s = 16 + np.asarray(n_log2, np.int64)
    u = np.clip((ur * sr + ug * sg + ub * sb + (coff << s) + (1 << (s - 1))) >> s, 0, maxv)
    v = np.clip((vr * sr + vg * sg + vb * sb + (coff << s) + (1 << (s - 1))) >> s, 0, maxv)
    return u, v


def inv_pixel(y, u, v, matrix="bt601", full=False, depth=8):
    """-> (b, g, r) u8"""
    ky, rv, gu, gv, bu, yoff, coff = inv_coefs(matrix, full, depth)
    yy = ky * (np.asarray(y, np.int64) - yoff)
    u = np.asarray(u, np.int64) - coff
    v = np.asarray(v, np.int64) - coff
    r = np.clip((yy + rv * v + 32768) >> 16, 0, 255)
    g = np.clip((yy + gu * u + gv * v + 32768) >> 16, 0, 255)
    b = np.clip((yy + bu * u + 32768) >> 16, 0, 255)
    return b, g, r


# ---- float64 textbook formulas --------------------------------------------------------------------------------
def float_fwd(r, g, b, matrix="bt601", full=False, depth=8):
    """-> (Y, Cb, Cr) float64 codes, unrounded"""
    kr, kb = MATRICES[matrix]
    kg = 1 - kr - kb
    ys, cs, yoff = _ranges(full, depth)
    r, g, b = (np.asarray(t, np.float64) / 255.0 for t in (r, g, b))
    ey = kr * r + kg * g + kb * b
    return yoff + ys * ey, (1 << (depth - 1)) + cs * (b - ey) / (2 * (1 - kb)), (1 << (depth - 1)) + cs * (r - ey) / (2 * (1 - kr))


def float_inv(y, u, v, matrix="bt601", full=False, depth=8):
    """-> (b, g, r) float64 in 0..255 units, unrounded and unclamped"""
    kr, kb = MATRICES[matrix]
    kg = 1 - kr - kb
    ys, cs, yoff = _ranges(full, depth)
    ey = (np.asarray(y, np.float64) - yoff) / ys
    pb = (np.asarray(u, np.float64) - (1 << (depth - 1))) / cs
    pr = (np.asarray(v, np.float64) - (1 << (depth - 1))) / cs
    r = ey + 2 * (1 - kr) * pr
    b = ey + 2 * (1 - kb) * pb
    g = (ey - kr * r - kb * b) / kg
    return 255 * b, 255 * g, 255 * r


# ---- whole frames ---------------------------------------------------------------------------------------------
def bgr_to_pix(bgr, fmt, matrix="bt601", full=False):
    """u8 [h][w][3] -> flat u8 frame of `fmt`"""
    bgr = np.asarray(bgr, np.uint8)
    if fmt == "bgr24":
        return bgr.reshape(-1).copy()
    h, w, _ = bgr.shape
    depth = 10 if fmt == "p010le" else 8
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    y = fwd_luma(r, g, b, matrix, full, depth)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    pad = lambda a: np.pad(a, ((0, 2 * ch - h), (0, 2 * cw - w)))   # noqa: E731
    blk = lambda a: pad(a).reshape(ch, 2, cw, 2).sum(axis=(1, 3))   # noqa: E731
    rows = np.where(np.arange(ch) * 2 + 1 < h, 2, 1)[:, None]
    cols = np.where(np.arange(cw) * 2 + 1 < w, 2, 1)[None, :]
    n_log2 = (rows - 1) + (cols - 1)
    u, v = fwd_chroma(blk(r), blk(g), blk(b), n_log2, matrix, full, depth)
    if fmt == "yuv420p":
        return np.concatenate([y.ravel(), u.ravel(), v.ravel()]).astype(np.uint8)
    uv = np.stack([u, v], axis=-1).ravel()
    if fmt == "nv12":
        return np.concatenate([y.ravel(), uv]).astype(np.uint8)
    return (np.concatenate([y.ravel(), uv]).astype("<u2") << 6).view(np.uint8)


def pix_planes(frame, fmt, h, w):
    """flat frame -> (Y [h][w], U [ch][cw], V [ch][cw]) as int64 sample values (p010le: the 10-bit values)"""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    a = np.asarray(frame, np.uint8).reshape(-1)
    if fmt == "p010le":
        a = a.view("<u2").astype(np.int64) >> 6
    else:
        a = a.astype(np.int64)
    y = a[:h * w].reshape(h, w)
    if fmt == "yuv420p":
        return y, a[h * w:h * w + cw * ch].reshape(ch, cw), a[h * w + cw * ch:].reshape(ch, cw)
    uv = a[h * w:].reshape(ch, cw, 2)
    return y, uv[..., 0], uv[..., 1]


def pix_to_bgr(frame, fmt, h, w, matrix="bt601", full=False):
    """flat frame of `fmt` -> u8 [h][w][3]"""
    if fmt == "bgr24":
        return np.asarray(frame, np.uint8).reshape(h, w, 3).copy()
    y, u, v = pix_planes(frame, fmt, h, w)
    up = lambda a: np.repeat(np.repeat(a, 2, 0), 2, 1)[:h, :w]   # noqa: E731
    b, g, r = inv_pixel(y, up(u), up(v), matrix, full, 10 if fmt == "p010le" else 8)
    return np.stack([b, g, r], axis=-1).astype(np.uint8)


def convert(frame, in_fmt, out_fmt, h, w, matrix="bt601", full=False):
    """flat / [h][w][3] frame of in_fmt -> flat u8 frame of out_fmt (through u8 BGR; a copy when the formats are equal)"""
    if in_fmt == out_fmt:
        return np.asarray(frame, np.uint8).reshape(-1).copy()
    bgr = pix_to_bgr(frame, in_fmt, h, w, matrix, full)
    return bgr_to_pix(bgr, out_fmt, matrix, full)
