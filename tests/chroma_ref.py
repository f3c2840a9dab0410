"""Numpy restatement of the sited, interpolating 4:2:0 chroma modes (csrc/uva_pixfmt.hip) -- TESTS ONLY.

chroma_filter "replicate" is sections 7.3 / 7.4 (pixfmt_ref.py, pixfmt16_ref.py) and is handed to them.  "bilinear" with a
siting (ffmpeg's chroma_sample_location names) interpolates: integer weighted sums, the weights' power of two folded into the
final shift, taps beyond a plane's edge replicated.  The u8 route adds in int32, the u16 route in int64 with section 7.4's
coefficients: every partial sum is asserted to fit.  Beside them the float64 definition they approximate."""
import numpy as np

import pixfmt16_ref as ref16
import pixfmt_ref as ref8

SITINGS = ("left", "center", "topleft")
COSITED = {"left": (True, False), "center": (False, False), "topleft": (True, True)}     # siting -> (horizontal, vertical)
MODES = (("replicate", "left"),) + tuple(("bilinear", s) for s in SITINGS)
YUV = ("yuv420p", "nv12", "p010le", "yuv420p10le")


def up_axis(c, n, cosited, axis):
    """chroma plane -> n luma positions along `axis`: (integer weighted sums, log2 of the weights' sum).  Also takes floats."""
    c = np.moveaxis(np.asarray(c), axis, 0)
    m = c.shape[0]
    k = np.arange(n) // 2
    odd = (np.arange(n) % 2 == 1).reshape((-1,) + (1,) * (c.ndim - 1))
    at = lambda i: c[np.clip(i, 0, m - 1)]   # noqa: E731
    if cosited:       # chroma sits on luma 2k: 2k <- C[k], 2k+1 <- (C[k] + C[k+1]) / 2
        out, dl = np.where(odd, at(k) + at(k + 1), 2 * at(k)), 1
    else:             # midway between 2k and 2k+1: 2k <- (C[k-1] + 3 C[k]) / 4, 2k+1 <- (3 C[k] + C[k+1]) / 4
        out, dl = np.where(odd, 3 * at(k) + at(k + 1), at(k - 1) + 3 * at(k)), 2
    return np.moveaxis(out, 0, axis), dl


def down_axis(p, cosited, axis):
    """luma-resolution plane -> ceil(n/2) chroma positions along `axis`: (weighted sums, log2 of the weights' sum)"""
    p = np.asarray(p)
    n = p.shape[axis]
    k = np.arange((n + 1) // 2)
    at = lambda i: np.take(p, np.clip(i, 0, n - 1), axis=axis)   # noqa: E731
    if cosited:       # [1 2 1] / 4 centred on luma 2k
        return at(2 * k - 1) + 2 * at(2 * k) + at(2 * k + 1), 2
    return at(2 * k) + at(2 * k + 1), 1     # [1 1] / 2: the box on this axis


def upsample(c, h, w, loc):
    """chroma plane [ch][cw] -> [h][w] sums and the log2 of their denominator (8 left, 16 center, 4 topleft)"""
    hco, vco = COSITED[loc]
    a, d0 = up_axis(c, h, vco, 0)
    a, d1 = up_axis(a, w, hco, 1)
    return a, d0 + d1


def downsample(p, loc):
    """[h][w] plane -> [ch][cw] sums over the siting's window (3x2 left, 2x2 center, 3x3 topleft) and the log2 of the denominator"""
    hco, vco = COSITED[loc]
    a, d0 = down_axis(p, vco, 0)
    a, d1 = down_axis(a, hco, 1)
    return a, d0 + d1


def _acc(bits, *parts):
    """the kernels add left to right in int32 (u8 route) or int64 (u16 route): every partial sum must fit"""
    acc = np.zeros((), np.int64)
    lim = 2 ** (bits - 1)
    for p in parts:
        p = np.asarray(p, np.int64)
        if bits == 64:      # int64 numpy cannot show its own overflow: bound the sum first
            assert float(np.abs(acc).max()) + float(np.abs(p).max()) < 2.0 ** 62, "int64 overflow"
        acc = acc + p
        assert np.all(acc < lim) and np.all(acc >= -lim), "int%d overflow" % bits
    return acc


def _route(u16):
    """(coefficient module, forward shift, inverse shift, accumulator bits, largest BGR code)"""
    return (ref16, ref16.FWD_SH, ref16.INV_SH, 64, 65535) if u16 else (ref8, 16, 16, 32, 255)


# ---- per-sample fixed point ---------------------------------------------------------------------------------------
def inv_pixel(y, us, vs, dl, matrix="bt601", full=False, depth=8, u16=False):
    """Y' and the chroma SUMS over 2^dl -> (b, g, r)"""
    mod, _, sh, bits, vmax = _route(u16)
    ky, rv, gu, gv, bu, yoff, coff = mod.inv_coefs(matrix, full, depth)
    s = sh + dl
    u = np.asarray(us, np.int64) - (coff << dl)
    v = np.asarray(vs, np.int64) - (coff << dl)
    yy = _acc(32, ky * (np.asarray(y, np.int64) - yoff))           # (an int32 product on both routes)
    base = _acc(bits, yy * (1 << dl), 1 << (s - 1))
    b = np.clip(_acc(bits, base, bu * u) >> s, 0, vmax)
    g = np.clip(_acc(bits, base, gu * u, gv * v) >> s, 0, vmax)
    r = np.clip(_acc(bits, base, rv * v) >> s, 0, vmax)
    return b, g, r


def fwd_chroma(sr, sg, sb, dl, matrix="bt601", full=False, depth=8, u16=False):
    """chroma from the weighted SUMS of R, G, B over 2^dl"""
    mod, sh, _, bits, _ = _route(u16)
    _, (ur, ug, ub), (vr, vg, vb), _, coff, maxv = mod.fwd_coefs(matrix, full, depth)
    sr, sg, sb = (np.asarray(t, np.int64) for t in (sr, sg, sb))
    s = sh + dl
    u = np.clip(_acc(bits, ur * sr, ug * sg, ub * sb, coff << s, 1 << (s - 1)) >> s, 0, maxv)
    v = np.clip(_acc(bits, vr * sr, vg * sg, vb * sb, coff << s, 1 << (s - 1)) >> s, 0, maxv)
    return u, v


def fwd_luma(r, g, b, matrix="bt601", full=False, depth=8, u16=False):
    return _route(u16)[0].fwd_luma(r, g, b, matrix, full, depth)


# ---- float64: interpolate or filter in float, then the float matrix --------------------------------------------------
def float_inv_pixel(y, us, vs, dl, matrix="bt601", full=False, depth=8, u16=False):
    f = ref16.float_inv if u16 else ref8.float_inv
    return f(y, np.asarray(us, np.float64) / (1 << dl), np.asarray(vs, np.float64) / (1 << dl), matrix, full, depth)


def float_fwd_chroma(sr, sg, sb, dl, matrix="bt601", full=False, depth=8, u16=False):
    f = ref16.float_fwd if u16 else ref8.float_fwd
    _, u, v = f(*(np.asarray(t, np.float64) / (1 << dl) for t in (sr, sg, sb)), matrix=matrix, full=full, depth=depth)
    return u, v


# ---- whole frames -------------------------------------------------------------------------------------------------
def pix_to_bgr(frame, fmt, h, w, matrix="bt601", full=False, chroma_filter="replicate", chroma_loc="left", u16=False):
    """flat frame of `fmt` -> u8 (or, u16=True, u16) [h][w][3]"""
    if chroma_filter == "replicate" or fmt not in YUV:
        return ref16.pix_to_bgr16(frame, fmt, h, w, matrix, full) if u16 else ref16.pix_to_bgr8(frame, fmt, h, w, matrix, full)
    y, u, v = ref16.planes(frame, fmt, h, w)
    us, dl = upsample(u, h, w, chroma_loc)
    vs, _ = upsample(v, h, w, chroma_loc)
    b, g, r = inv_pixel(y, us, vs, dl, matrix, full, ref16.depth_of(fmt), u16)
    return np.stack([b, g, r], axis=-1).astype(np.uint16 if u16 else np.uint8)


def bgr_to_pix(bgr, fmt, matrix="bt601", full=False, chroma_filter="replicate", chroma_loc="left", u16=False):
    """u8 (or, u16=True, u16) [h][w][3] -> flat u8 frame of `fmt`"""
    if chroma_filter == "replicate" or fmt not in YUV:
        return ref16.bgr16_to_pix(bgr, fmt, matrix, full) if u16 else ref16.bgr_to_pix8(bgr, fmt, matrix, full)
    bgr = np.asarray(bgr, np.uint16 if u16 else np.uint8)
    depth = ref16.depth_of(fmt)
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    y = fwd_luma(r, g, b, matrix, full, depth, u16)
    (sr, dl), (sg, _), (sb, _) = (downsample(t, chroma_loc) for t in (r, g, b))
    u, v = fwd_chroma(sr, sg, sb, dl, matrix, full, depth, u16)
    return ref16.pack(fmt, y, u, v)


def convert(frame, in_fmt, out_fmt, h, w, matrix="bt601", full=False, chroma_filter="replicate", chroma_loc="left", bit_depth=8):
    """uva_pix_convert (bit_depth 8) / uva_pix_convert16 (16): in_fmt -> out_fmt through u8 / u16 BGR; a copy when the formats are equal"""
    if in_fmt == out_fmt:
        return np.asarray(frame).reshape(-1).view(np.uint8).copy()
    u16 = bit_depth == 16
    bgr = pix_to_bgr(frame, in_fmt, h, w, matrix, full, chroma_filter, chroma_loc, u16)
    return np.asarray(bgr_to_pix(bgr, out_fmt, matrix, full, chroma_filter, chroma_loc, u16)).reshape(-1).view(np.uint8)


# ---- the quality experiment's frame and measure -----------------------------------------------------------------------
def edges_frame(h=270, w=480, seed=7):
    """29 x 23-pixel patches of random saturated colour (every channel 0 or 255, never all equal) -> u8 BGR [h][w][3]"""
    rng = np.random.default_rng(seed)
    ph, pw = 23, 29
    gh, gw = (h + ph - 1) // ph, (w + pw - 1) // pw
    pal = np.array([[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)][1:-1], np.uint8)
    cells = pal[rng.integers(0, len(pal), (gh, gw))]
    return np.repeat(np.repeat(cells, ph, 0), pw, 1)[:h, :w].copy()


def psnr(a, b, peak=255.0):
    mse = float(((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).mean())
    return 99.0 if mse == 0 else 10 * np.log10(peak * peak / mse)
