"""numpy restatement of the repeated-frame rule, tests only: the three numbers of the frame-difference
kernel in int64, and which frame's result every frame of a sequence gets when the comparison is always against the KEPT frame."""
import numpy as np

EIGHT_BIT = ("bgr24", "yuv420p", "nv12", "yuv422p")
SIXTEEN_BIT = ("p010le", "yuv420p10le", "yuv422p10le", "bgr48le")


def frame_bytes(fmt, h, w):
    c = 2 * ((w + 1) // 2) * ((h + 1) // 2)
    c422 = 2 * ((w + 1) // 2) * h
    return {"bgr24": 3 * w * h, "yuv420p": w * h + c, "nv12": w * h + c, "p010le": 2 * (w * h + c), "yuv420p10le": 2 * (w * h + c),
            "bgr48le": 6 * w * h, "yuv422p": w * h + c422, "yuv422p10le": 2 * (w * h + c422)}[fmt]


def samples(buf, fmt, h, w):
    """the code values of one dense frame as the input conversion reads them, int64"""
    raw = np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    assert raw.size == frame_bytes(fmt, h, w), (raw.size, fmt, h, w)
    if fmt in EIGHT_BIT:
        return raw.astype(np.int64)
    assert fmt in SIXTEEN_BIT, fmt
    words = raw.view("<u2").astype(np.int64)
    if fmt == "p010le":
        return words >> 6
    if fmt == "bgr48le":
        return words
    return words & 1023


def frame_diff(a, b, fmt, h, w, T):
    """(over, max_abs, sad): samples with |a - b| > T, the largest |a - b|, the sum of |a - b|"""
    d = np.abs(samples(a, fmt, h, w) - samples(b, fmt, h, w))
    return int((d > T).sum()), int(d.max()), int(d.sum())


def kept_indices(frames, fmt, h, w, T):
    """for each frame, the index of the frame whose result it gets: its own when it runs (and becomes the kept frame), the kept
    frame's when no sample differs from that frame's by more than T"""
    out, kept = [], None
    for k, f in enumerate(frames):
        if kept is None or frame_diff(frames[kept], f, fmt, h, w, T)[0] != 0:
            kept = k
        out.append(kept)
    return out


def skipped(indices):
    return sum(1 for k, i in enumerate(indices) if i != k)
