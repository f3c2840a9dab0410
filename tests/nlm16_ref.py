"""nlm16_ref.py -- TEST INFRASTRUCTURE ONLY (never imported by the product).

The DEFINITION of `-m n=K` at --bit-depth 16: integer numpy, written before the kernels, which
are held to it bit for bit (csrc/uva_denoise16.hip.h).  The stage has the 8-bit stage's shape (oracle/nlm_oracle.py): BGR ->
Lab, non-local means on L and on (a, b), Lab -> BGR -- on u16 samples.

Lab at 16 bits: the colour science of nlm_oracle.bgr2lab_cie / lab2bgr_cie (input taken as linear light, as OpenCV's LBGR2Lab
takes it), L16 = L * 65535 / 100, a16 = (a + 128) * 257, b16 = (b + 128) * 257 (the 8-bit planes' scales x 257), saturated.
Fixed point, every table built in float64 with one operation per statement:
  forward   t = min((sum C15 * v + 2^14) >> 15, 65535)   C15 = rint(2^15 M / white), unsigned 32 bits
            F = ftab[t]                                  ftab[t] = rint(2^16 f(t / 65535)), 65536 entries
            L16 = sat((F_y * l_mul - l_sub + 2^19) >> 20), a16 = sat(((F_x - F_y) * a_mul + (32896 << 20) + 2^19) >> 20), b16 alike
  inverse   f24 of y from L16, of x and z from a16 / b16, all at 2^24 = 1.0 in 64 bits; x = f^3 by integer cube above the CIE
            threshold, the line below it; the 2^14-scaled matrix; rounded to 2^24, clipped, rounded to 65535.

NLM at 16 bits: template 5, search 9, reflect-101 border 6, as at 8 bits.  A sample difference d (17 bits signed) is squared in
unsigned 32 bits and shifted `>> 8` BEFORE any summing, so a patch distance is a box sum of per-pixel integers (at most
25 * 2 * (65535^2 >> 8) < 2^31).  The weight is the 8-bit stage's function of the mean squared patch difference in 8-bit
units^2 (one code16 = 1/257 unit): index = distance >> 9 (sixteen times finer than the 8-bit table's `>> 5` bins),
weight = rint(F exp(-index * m16 / (h^2 cn))) with m16 = 2^9 * 2^8 / (257^2 * 25), F = 103969, weights below F / 1000 dropped;
the table is cut at its first zero and the index clamped to it.  64-bit accumulators, OpenCV's rounded unsigned division,
saturated to 65535.
"""
import numpy as np

from oracle import nlm_oracle as no

T, S, B = no.T, no.S, no.B
SQ_SHIFT = 8                       # per squared sample difference, before summing
IDX_SHIFT = 9                      # patch distance -> table index
FIXED = no.INT_MAX // (81 * 255)   # 103969, as at 8 bits
TABLE_LIMIT = 1 << 22              # (no h <= 30 comes near: 156 641 entries at h = 30, cn = 2)


def weight_table16(h, cn):
    """int64 [n]: monotone, t[0] == FIXED, t[-1] == 0 and no zero before it"""
    mult = (512.0 * 256.0) / (257.0 * 257.0 * 25.0)
    hh = float(np.float32(h))
    den = hh * hh * cn
    out = []
    start = 0
    while start < TABLE_LIMIT:
        i = np.arange(start, start + 65536, dtype=np.float64)
        dist = i * mult
        w = np.exp(-dist / den)
        tab = np.rint(FIXED * w).astype(np.int64)
        tab[tab < 0.001 * FIXED] = 0
        z = np.nonzero(tab == 0)[0]
        if len(z):
            out.append(tab[:z[0] + 1])
            return np.concatenate(out)
        out.append(tab)
        start += 65536
    raise ValueError("weight table does not end")


def nlm_plane16(plane, h):
    """plane: u16 [H][W] or [H][W][cn] -> same shape"""
    img = np.asarray(plane)
    assert img.dtype == np.uint16
    a = img[..., None] if img.ndim == 2 else img
    H, W, cn = a.shape
    tab = weight_table16(h, cn)
    ext = np.pad(a.astype(np.int64), ((B, B), (B, B), (0, 0)), mode="reflect")
    est = np.zeros((H, W, cn), np.int64)
    wsum = np.zeros((H, W), np.int64)
    c0 = ext[S:S + H + 2 * T, S:S + W + 2 * T]
    k = 2 * T + 1
    for sy in range(-S, S + 1):
        for sx in range(-S, S + 1):
            sh = ext[S + sy:S + sy + H + 2 * T, S + sx:S + sx + W + 2 * T]
            d2 = (((c0 - sh) ** 2) >> SQ_SHIFT).sum(axis=2)
            cs = np.pad(d2, ((1, 0), (1, 0))).cumsum(0).cumsum(1)
            dist = cs[k:, k:] - cs[:-k, k:] - cs[k:, :-k] + cs[:-k, :-k]
            wgt = tab[np.minimum(dist >> IDX_SHIFT, len(tab) - 1)]
            p = ext[B + sy:B + sy + H, B + sx:B + sx + W]
            est += wgt[..., None] * p
            wsum += wgt
    out = (est + (wsum // 2)[..., None]) // wsum[..., None]
    out = np.clip(out, 0, 65535).astype(np.uint16)
    return out[..., 0] if img.ndim == 2 else out


# ---- Lab at 16 bits ----------------------------------------------------------------------------------------------------
_RGB2XYZ = [[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]]
_XYZ2RGB = [[3.240479, -1.53715, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]]
_D65 = [0.950456, 1.0, 1.088754]
AB_OFF = 32896                     # 128 * 257
_tables = None


def _rint(v):
    return int(np.rint(np.float64(v)))


def lab16_tables():
    """dict of the stage's constants, every value an integer; float64, one operation per statement"""
    global _tables
    if _tables is not None:
        return _tables
    t = {}
    x = np.arange(65536, dtype=np.float64) / 65535.0
    bias = 16.0 / 116.0
    lin = 7.787 * x
    lin = lin + bias
    f = np.where(x > 0.008856, np.cbrt(x), lin)
    t["ftab"] = np.rint(65536.0 * f).astype(np.int64)
    fwd, inv = np.zeros((3, 3), np.int64), np.zeros((3, 3), np.int64)
    for i in range(3):
        for j in range(3):
            v = 32768.0 * _RGB2XYZ[i][j]
            fwd[i, j] = _rint(v / _D65[i])
            v = 16384.0 * _XYZ2RGB[i][j]
            inv[i, j] = _rint(v * _D65[j])
    t["fwd"], t["inv"] = fwd, inv
    q20, q24, q40 = 1048576.0, 16777216.0, 1099511627776.0
    lscale = 116.0 * 655.35                     # L16 per unit of f
    t["l_mul"] = _rint(q20 * (lscale / 65536.0))
    t["l_sub"] = _rint(q20 * (16.0 * 655.35))
    t["a_mul"] = _rint(q20 * (128500.0 / 65536.0))      # 500 * 257
    t["b_mul"] = _rint(q20 * (51400.0 / 65536.0))       # 200 * 257
    t["il_mul"] = _rint(q40 / lscale)
    t["il_add"] = _rint(q40 * bias)
    t["ia_mul"] = _rint(q40 / 128500.0)
    t["ib_mul"] = _rint(q40 / 51400.0)
    thr = 7.787 * 0.008856
    thr = thr + bias
    t["f_thr"] = _rint(q24 * thr)
    t["f_bias"] = _rint(q24 * bias)
    t["lin_mul"] = _rint(q20 / 7.787)
    _tables = t
    return t


def _sat16(v):
    return np.clip(v, 0, 65535)


def bgr2lab16(bgr16):
    """u16 [..][3] BGR (linear light) -> u16 [..][3] (L16, a16, b16)"""
    t = lab16_tables()
    img = np.asarray(bgr16)
    assert img.dtype == np.uint16
    Bv, Gv, Rv = (img[..., k].astype(np.int64) for k in range(3))
    C = t["fwd"]
    F = []
    for k in range(3):
        s = C[k, 0] * Rv + C[k, 1] * Gv + C[k, 2] * Bv          # < 2^32
        F.append(t["ftab"][np.minimum((s + (1 << 14)) >> 15, 65535)])
    half = 1 << 19
    L = (F[1] * t["l_mul"] - t["l_sub"] + half) >> 20
    a = ((F[0] - F[1]) * t["a_mul"] + (AB_OFF << 20) + half) >> 20
    b = ((F[1] - F[2]) * t["b_mul"] + (AB_OFF << 20) + half) >> 20
    return np.stack([_sat16(L), _sat16(a), _sat16(b)], axis=-1).astype(np.uint16)


def _f_inv24(f24, t):
    """2^24-scaled f -> 2^24-scaled X / Xn (Y, Z / Zn): the integer cube above the threshold, the line below"""
    sq = (f24 * f24) >> 24
    cube = (sq * f24) >> 24
    lin = ((f24 - t["f_bias"]) * t["lin_mul"]) >> 20
    return np.where(f24 > t["f_thr"], cube, lin)


def lab2bgr16(lab16):
    """u16 [..][3] (L16, a16, b16) -> u16 [..][3] BGR"""
    t = lab16_tables()
    lab = np.asarray(lab16)
    assert lab.dtype == np.uint16
    L, a, b = (lab[..., k].astype(np.int64) for k in range(3))
    fy = (L * t["il_mul"] + t["il_add"] + (1 << 15)) >> 16
    fx = fy + (((a - AB_OFF) * t["ia_mul"] + (1 << 15)) >> 16)
    fz = fy - (((b - AB_OFF) * t["ib_mul"] + (1 << 15)) >> 16)
    x, y, z = _f_inv24(fx, t), _f_inv24(fy, t), _f_inv24(fz, t)
    C = t["inv"]
    out = []
    for k in (2, 1, 0):                                          # B, G, R
        v = (C[k, 0] * x + C[k, 1] * y + C[k, 2] * z + (1 << 13)) >> 14
        v = np.clip(v, 0, 1 << 24)
        out.append((v * 65535 + (1 << 23)) >> 24)
    return np.stack(out, axis=-1).astype(np.uint16)


def denoise16(bgr16, K):
    """the whole stage: u16 [H][W][3] BGR -> the same"""
    lab = bgr2lab16(bgr16)
    L = nlm_plane16(np.ascontiguousarray(lab[..., 0]), K)
    ab = nlm_plane16(np.ascontiguousarray(lab[..., 1:]), K)
    return lab2bgr16(np.concatenate([L[..., None], ab], axis=-1))


# ---- the colour science in float64 (what the fixed-point scheme is measured against) --------------------------------------
def _f64(x):
    return np.where(x > 0.008856, np.cbrt(x), 7.787 * x + 16.0 / 116.0)


def bgr2lab16_float(bgr16):
    """nlm_oracle.bgr2lab_cie's formulas in float64 on u16 input, in 16-bit codes, unrounded and unclipped: float64 [..][3]"""
    v = np.asarray(bgr16).astype(np.float64) / 65535.0
    b, g, r = v[..., 0], v[..., 1], v[..., 2]
    X = (0.412453 * r + 0.357580 * g + 0.180423 * b) / 0.950456
    Y = 0.212671 * r + 0.715160 * g + 0.072169 * b
    Z = (0.019334 * r + 0.119193 * g + 0.950227 * b) / 1.088754
    fx, fy, fz = _f64(X), _f64(Y), _f64(Z)
    L = np.where(Y > 0.008856, 116.0 * fy - 16.0, 903.3 * Y)
    return np.stack([L * 655.35, (500.0 * (fx - fy) + 128.0) * 257.0, (200.0 * (fy - fz) + 128.0) * 257.0], axis=-1)


def colour_set():
    """the fixed colours of the Lab checks: the 64-level cube widened x 257, 2^20 seeded random 16-bit colours, the eight
    corners: u16 [N][3] (N = 64^3 + 2^20 + 8, shaped [1316][997][3] minus padding by the caller if it wants an image)"""
    g = (np.arange(64, dtype=np.int64) * 255 // 63 * 257).astype(np.uint16)
    cube = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rnd = np.random.default_rng(16).integers(0, 65536, (1 << 20, 3), dtype=np.uint16)
    c = np.array([0, 65535], np.uint16)
    corners = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([cube, rnd, corners], axis=0)
