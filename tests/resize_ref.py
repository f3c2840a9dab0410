"""The resampler's arithmetic (csrc/uva_resize.hip) restated in numpy, sum for sum in the kernel's order,
with every partial sum asserted to fit the type the kernel holds it in.

    tables   ideal_weights(): float64 weights of one axis as the issue defines them; int_taps(): the library's rule for turning
             them into integers that sum to 2^14.  The bit-exact comparisons take the LIBRARY's table (ncnn.resize_taps): `sin`
             may differ in the last bit between the C library and numpy, and one flipped unit would break them for no reason.
    pass 1   vertical, int32, taps ascending; u8 keeps (s + 64) >> 7, u16 keeps s.
    pass 2   horizontal, taps ascending, int32 (u8) / int64 (u16); result clamp((s + 2^20) >> 21) / clamp((s + 2^27) >> 28).
"""
import math

import numpy as np

ONE = 1 << 14
SUPPORT = {"lanczos": 3, "bicubic": 2, "bilinear": 1}
FILTERS = tuple(SUPPORT)


def kernel(name, x):
    x = np.abs(np.asarray(x, np.float64))
    if name == "lanczos":
        return np.where(x < 3.0, np.sinc(x) * np.sinc(x / 3.0), 0.0)
    if name == "bicubic":        # Keys, a = -0.5
        return np.where(x < 1.0, (1.5 * x - 2.5) * x * x + 1.0, np.where(x < 2.0, ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0, 0.0))
    if name == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    raise ValueError(name)


def ntaps(n_in, n_out, name):
    a = SUPPORT[name]
    return 2 * (-(-a * n_in // n_out) if n_in > n_out else a)


def ideal_weights(n_in, n_out, name):
    """-> (first int64 [n_out], weights float64 [n_out][T], every row normalised to sum 1)"""
    a = SUPPORT[name]
    r = n_in / n_out
    fs = max(1.0, r)
    t = ntaps(n_in, n_out, name)
    d = np.arange(n_out, dtype=np.float64)
    c = (d + 0.5) * n_in / n_out - 0.5
    first = np.floor(c - a * fs).astype(np.int64) + 1
    k = first[:, None] + np.arange(t)[None, :]
    w = kernel(name, (k - c[:, None]) / fs)
    return first, w / w.sum(axis=1, keepdims=True)


def int_taps(weights):
    """rows of float64 weights that sum to 1 -> int64 taps that sum to exactly 2^14: floor, then the missing units one each to
    the largest remainders (ties: lowest index)"""
    v = weights * ONE
    q = np.floor(v).astype(np.int64)
    rem = v - q
    for d in range(q.shape[0]):
        left = ONE - int(q[d].sum())
        assert 0 <= left <= q.shape[1]
        order = np.argsort(-rem[d], kind="stable")
        q[d, order[:left]] += 1
    return q


def _gather_idx(first, t, n_in):
    return np.clip(np.asarray(first, np.int64)[:, None] + np.arange(t)[None, :], 0, n_in - 1)


def resize(img, size, tables):
    """img u8 / u16 [h][w][3] -> [oh][ow][3]; tables = ((first_y, taps_y), (first_x, taps_x)), taps [n_out][T] integers"""
    img = np.asarray(img)
    assert img.dtype in (np.uint8, np.uint16) and img.ndim == 3 and img.shape[2] == 3
    u8 = img.dtype == np.uint8
    h, w, _ = img.shape
    oh, ow = size
    (fy, ty), (fx, tx) = tables
    ty, tx = np.asarray(ty, np.int64), np.asarray(tx, np.int64)
    assert ty.shape[0] == oh and tx.shape[0] == ow
    assert (ty.sum(axis=1) == ONE).all() and (tx.sum(axis=1) == ONE).all()
    x = img.astype(np.int64)
    # pass 1: vertical, int32
    iy = _gather_idx(fy, ty.shape[1], h)
    mid = np.zeros((oh, w, 3), np.int64)
    for k in range(ty.shape[1]):
        mid += ty[:, k, None, None] * x[iy[:, k]]
        assert np.abs(mid).max() < 2 ** 31, "pass 1 partial sum leaves int32"
    if u8:
        mid = (mid + 64) >> 7
    assert np.abs(mid).max() < 2 ** 31
    # pass 2: horizontal, int32 (u8) / int64 (u16)
    ix = _gather_idx(fx, tx.shape[1], w)
    out = np.zeros((oh, ow, 3), np.int64)
    for k in range(tx.shape[1]):
        if not u8:       # (int64 sums: bound them before numpy could wrap)
            assert float(np.abs(out).max()) + float(np.abs(mid).max()) * float(np.abs(tx[:, k]).max()) < 2.0 ** 63
        out += tx[None, :, k, None] * mid[:, ix[:, k]]
        if u8:
            assert np.abs(out).max() < 2 ** 31 - (1 << 20), "pass 2 partial sum leaves int32"
    if u8:
        return np.clip((out + (1 << 20)) >> 21, 0, 255).astype(np.uint8)
    return np.clip((out + (1 << 27)) >> 28, 0, 65535).astype(np.uint16)


def resize_float(img, size, tables_or_weights):
    """float64 evaluation, unrounded and unclamped: rows of weights (float, sum 1) or of integer taps (sum 2^14)"""
    x = np.asarray(img, np.float64)
    h, w, _ = x.shape
    (fy, ty), (fx, tx) = tables_or_weights
    ty, tx = np.asarray(ty, np.float64), np.asarray(tx, np.float64)
    ty, tx = ty / ty.sum(axis=1, keepdims=True), tx / tx.sum(axis=1, keepdims=True)
    iy, ix = _gather_idx(fy, ty.shape[1], h), _gather_idx(fx, tx.shape[1], w)
    mid = np.einsum("ok,okwc->owc", ty, x[iy])
    return np.einsum("pk,opkc->opc", tx, mid[:, ix])


def library_tables(h, w, oh, ow, name):
    from upscale_video_amd import ncnn
    return ncnn.resize_taps(h, oh, name), ncnn.resize_taps(w, ow, name)


def own_tables(h, w, oh, ow, name):
    """the same tables from this file's float64 weights (differ from the library's by a unit where `sin` does)"""
    fy, wy = ideal_weights(h, oh, name)
    fx, wx = ideal_weights(w, ow, name)
    return (fy, int_taps(wy)), (fx, int_taps(wx))


def ideal_tables(h, w, oh, ow, name):
    return ideal_weights(h, oh, name), ideal_weights(w, ow, name)


def point_sample(img, size):
    h, w, _ = img.shape
    oh, ow = size
    iy = np.clip(np.floor((np.arange(oh) + 0.5) * h / oh).astype(int), 0, h - 1)
    ix = np.clip(np.floor((np.arange(ow) + 0.5) * w / ow).astype(int), 0, w - 1)
    return img[iy][:, ix]


def out_scale_size(h, w, f):
    return tuple(max(2, 2 * int(math.floor(n * f / 2 + 0.5))) for n in (h, w))
