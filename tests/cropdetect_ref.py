"""ffmpeg cropdetect's rule in numpy: the DEFINITION of the crop detector for this project.  ffmpeg is on
none of the project's machines, so parity with ffmpeg itself is unpinned; what the library computes (uva_crop_sums,
uva_crop_bounds, uva_crop_rect, ncnn.CropDetector) is held to this file bit for bit.

Samples are code values as the input conversion reads them; a LINE is a row or column of the luma plane, or of all three
components of a packed BGR frame."""
import numpy as np

DEPTH = {"bgr24": 8, "yuv420p": 8, "nv12": 8, "yuv422p": 8, "p010le": 10, "yuv420p10le": 10, "yuv422p10le": 10, "bgr48le": 16}
PACKED = ("bgr24", "bgr48le")


def samples(frame, fmt, h, w):
    """the samples the detector reads of a dense h x w frame (flat bytes) -> uint64 [h][w * comps]"""
    raw = np.ascontiguousarray(frame).reshape(-1).view(np.uint8)
    comps = 3 if fmt in PACKED else 1
    n = h * w * comps
    if DEPTH[fmt] == 8:
        v = raw[:n].astype(np.uint64)
    else:
        words = raw[:2 * n].view("<u2").astype(np.uint64)
        v = words >> np.uint64(6) if fmt == "p010le" else (words & np.uint64(1023) if DEPTH[fmt] == 10 else words)
    return v.reshape(h, w * comps)


def line_sums(frame, fmt, h, w):
    """-> (rows uint64 [h], cols uint64 [w])"""
    s = samples(frame, fmt, h, w)
    comps = 3 if fmt in PACKED else 1
    return s.sum(axis=1, dtype=np.uint64), s.reshape(h, w, comps).sum(axis=(0, 2), dtype=np.uint64)


def bounds(rows, cols, fmt, h, w, limit=24):
    """(first bright row, last bright row, first bright column, last bright column), -1 where there is none: a line with sum S
    over n samples is bright iff S // n > limit << (depth - 8)"""
    comps = 3 if fmt in PACKED else 1
    lim = limit << (DEPTH[fmt] - 8)
    out = []
    for sums, n in ((rows, w * comps), (cols, h * comps)):
        bright = [i for i, s in enumerate(sums) if int(s) // n > lim]
        out += [bright[0], bright[-1]] if bright else [-1, -1]
    return tuple(out)


def update(state, b):
    """the running state (x1, y1, x2, y2) after a frame with bounds b; a frame with no bright line leaves it unchanged"""
    x1, y1, x2, y2 = state
    r0, r1, c0, c1 = b
    if r0 >= 0:
        y1, y2 = min(y1, r0), max(y2, r1)
    if c0 >= 0:
        x1, x2 = min(x1, c0), max(x2, c1)
    return x1, y1, x2, y2


def initial(h, w):
    return w - 1, h - 1, 0, 0


def effective_round(r):
    r = 16 if r <= 1 else r
    return 2 * r if r % 2 else r


def rect(state, round=16):
    """(W, H, X, Y) or None"""
    R = effective_round(round)
    x1, y1, x2, y2 = state
    x, y = (x1 + 1) & ~1, (y1 + 1) & ~1
    cw, ch = x2 - x + 1, y2 - y + 1
    if cw <= 0 or ch <= 0:
        return None
    k = cw % R
    cw, x = cw - k, x + ((k // 2 + 1) & ~1)
    k = ch % R
    ch, y = ch - k, y + ((k // 2 + 1) & ~1)
    if cw <= 0 or ch <= 0:
        return None
    return cw, ch, x, y


class Detector:
    """ncnn.CropDetector's twin on the host"""

    def __init__(self, h, w, fmt, limit=24, round=16, gpu=0):
        self.h, self.w, self.fmt, self.limit, self.round = h, w, fmt, limit, round
        self.state = initial(h, w)

    def update(self, frame):
        self.state = update(self.state, bounds(*line_sums(frame, self.fmt, self.h, self.w), self.fmt, self.h, self.w, self.limit))
        return self.state

    def rect(self):
        return rect(self.state, self.round)


def window(frame, fmt, src_h, src_w, x, y, h, w):
    """numpy slicing of every plane at its own resolution -> the dense h x w frame as flat bytes"""
    raw = np.ascontiguousarray(frame).reshape(-1).view(np.uint8)
    b = 1 if DEPTH[fmt] == 8 else 2
    if fmt in PACKED:
        return raw.reshape(src_h, src_w, 3 * b)[y:y + h, x:x + w].reshape(-1).copy()
    v420 = fmt in ("yuv420p", "nv12", "p010le", "yuv420p10le")
    scw, cw = (src_w + 1) // 2, (w + 1) // 2
    sch = (src_h + 1) // 2 if v420 else src_h
    cy, chh = (y // 2, (h + 1) // 2) if v420 else (y, h)
    ny = src_h * src_w * b
    parts = [raw[:ny].reshape(src_h, src_w, b)[y:y + h, x:x + w]]
    if fmt in ("nv12", "p010le"):
        parts.append(raw[ny:ny + sch * scw * 2 * b].reshape(sch, scw, 2 * b)[cy:cy + chh, x // 2:x // 2 + cw])
    else:
        for p in range(2):
            o = ny + p * sch * scw * b
            parts.append(raw[o:o + sch * scw * b].reshape(sch, scw, b)[cy:cy + chh, x // 2:x // 2 + cw])
    return np.concatenate([p.reshape(-1) for p in parts])


def letterboxed_stream(h, w, n, seed=5):
    """n yuv420p frames: a bright picture in rows 16 ... 79, noise below the limit in the bars; frames 11 and 12 all black,
    frame 40 with a bright subtitle in the lower bar"""
    rng = np.random.default_rng(seed)
    out = np.empty((n, h * w * 3 // 2), np.uint8)
    for i in range(n):
        y = rng.integers(0, 12, (h, w), dtype=np.uint8)
        y[16:80] = rng.integers(60, 235, (64, w), dtype=np.uint8)
        if i in (11, 12):
            y[:] = 0
        if i == 40:
            y[84:90, 30:130] = 235
        out[i, :h * w] = y.reshape(-1)
        out[i, h * w:] = rng.integers(0, 256, h * w // 2, dtype=np.uint8)
    return out
