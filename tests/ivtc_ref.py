"""The inverse-telecine rule of the raw-video route in numpy: the definition that the kernel
(csrc/uva_ivtc.hip), the host restatement (csrc/uva_ivtc_host.cpp) and the handle (uva_ivtc_push) are held to, bit for bit.

It is field matching followed by decimation, for 2:3 pulldown only.  PARITY WITH ffmpeg's fieldmatch / decimate FILTERS IS
UNPINNED: ffmpeg is on none of the project's machines, so no constant, metric or tie rule here has been checked against them.
The rule is fixed here so that the implementations agree on it.

Formats, planes, sample reading, "first field" and the null-neighbour convention are those of tests/yadif_ref.py: planes are per
component plane, chroma rows alternate fields on their own row index, samples are code values as the input conversion reads
them, first = 0 for tff (default) and 1 for bff, prev / next None mean cur.

1. Candidates.  For X in {c: cur, p: prev, n: next} the woven frame W_X has, in every plane, the rows with y % 2 == first from
   cur (the kept field) and the other rows from X, copied byte for byte.
2. Metric, on plane 0 only (luma, or all of a packed BGR frame).  For every row 1 <= y <= ph-2 and every sample of the row:
   a = W[y-1], b = W[y], c = W[y+1], d1 = b-a, d2 = b-c, m = min(|d1|, |d2|); the sample is combed when d1 and d2 have the same
   sign, both are non-zero and m > T << (depth - 8).  N_X: combed samples; M_X: the sum of m over them.
   stats = (N_c, M_c, N_p, M_p, N_n, M_n).
3. Match: the X with the smallest M_X; ties go to c, then p, then n.
4. The matched frame is combed when N_X * 10^6 > L * (ph-2) * (samples per row).
5. Policy "yadif": a combed frame is replaced by output A of the yadif rule on the same three source frames with the same field
   order; "keep": the matched frame stands.
6. Decimation: the final frames are grouped in cycles of five from the start of the stream; the diff of a frame is the sum of
   absolute differences of code values against the final frame before it, every plane (the first frame: 2^64-1); of a full
   cycle the frame with the smallest diff is dropped, ties drop the earliest; a trailing cycle of fewer than five loses none.
"""
import numpy as np

import yadif_ref
from yadif_ref import FORMATS, _READ, depth, frame_bytes, memory_planes, words  # noqa: F401

MATCHES = "cpn"
FIRST_DIFF = (1 << 64) - 1


def first_of(field_order):
    return 1 if field_order == "bff" else 0


def weave(cur, x, fmt, h, w, field_order="tff"):
    """W_X: flat u8; rows y % 2 == first of every plane from cur, the others from x"""
    nb = _READ[fmt][0]
    first = first_of(field_order)
    out = np.array(np.ascontiguousarray(cur).reshape(-1).view(np.uint8), copy=True)
    src = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
    for off, ph, pw, st in memory_planes(fmt, h, w):
        rb = pw * st * nb
        o = out[off * nb:off * nb + ph * rb].reshape(ph, rb)
        s = src[off * nb:off * nb + ph * rb].reshape(ph, rb)
        o[1 - first::2] = s[1 - first::2]
    return out


def plane0(frame, fmt, h, w):
    """int64 [ph][samples per row] code values of plane 0"""
    _, shift, mask = _READ[fmt]
    off, ph, pw, st = memory_planes(fmt, h, w)[0]
    return ((words(frame, fmt)[off:off + ph * pw * st].reshape(ph, pw * st).astype(np.int64) >> shift) & mask)


def comb_metric(frame, fmt, h, w, T=9):
    """(N, M) of one woven frame"""
    v = plane0(frame, fmt, h, w)
    a, b, c = v[:-2], v[1:-1], v[2:]
    d1, d2 = b - a, b - c
    m = np.minimum(np.abs(d1), np.abs(d2))
    hit = (d1 * d2 > 0) & (m > (int(T) << (depth(fmt) - 8)))
    return int(np.count_nonzero(hit)), int(m[hit].sum())


def metrics(prev, cur, nxt, fmt, h, w, field_order="tff", T=9):
    """-> (N_c, M_c, N_p, M_p, N_n, M_n)"""
    if h < 4 or w < 1:
        raise ValueError("detelecine: h >= 4 and w >= 1")
    prev = cur if prev is None else prev
    nxt = cur if nxt is None else nxt
    out = []
    for x in (cur, prev, nxt):
        out += comb_metric(weave(cur, x, fmt, h, w, field_order), fmt, h, w, T)
    return tuple(out)


def choose(stats, fmt, h, w, L=1000):
    """-> (match 0 / 1 / 2 for c / p / n, combed)"""
    ms = [stats[1], stats[3], stats[5]]
    k = ms.index(min(ms))
    _, ph, pw, st = memory_planes(fmt, h, w)[0]
    return k, stats[2 * k] * 10 ** 6 > L * (ph - 2) * (pw * st)


def final_frame(prev, cur, nxt, fmt, h, w, field_order="tff", T=9, L=1000, combed="yadif"):
    """-> (flat u8 final frame, match, combed)"""
    st = metrics(prev, cur, nxt, fmt, h, w, field_order, T)
    k, cb = choose(st, fmt, h, w, L)
    if cb and combed == "yadif":
        return yadif_ref.deinterlace(prev, cur, nxt, fmt, h, w, field_order)[0], k, cb
    x = (cur, cur if prev is None else prev, cur if nxt is None else nxt)[k]
    return weave(cur, x, fmt, h, w, field_order), k, cb


def frame_sad(a, b, fmt):
    _, shift, mask = _READ[fmt]
    x = (words(a, fmt).astype(np.int64) >> shift) & mask
    y = (words(b, fmt).astype(np.int64) >> shift) & mask
    return int(np.abs(x - y).sum())


def decimate(diffs, keep_all=False):
    """the indices of the frames that stay"""
    n = len(diffs)
    if keep_all:
        return list(range(n))
    keep = []
    for c in range(0, n, 5):
        cyc = list(range(c, min(c + 5, n)))
        if len(cyc) == 5:
            d = [diffs[i] for i in cyc]
            cyc.pop(d.index(min(d)))
        keep += cyc
    return keep


def detelecine(frames, fmt, h, w, field_order="tff", T=9, L=1000, combed="yadif", keep_all=False):
    """a whole stream -> (the output frames in order, info): info has "match" (a string of c / p / n), "combed" (list of bool),
    "diffs", "kept" (indices of the final frames that stay) and "stats" (the seven counters of uva_ivtc_stats)"""
    finals, match, cmb = [], "", []
    for k, cur in enumerate(frames):
        f, m, cb = final_frame(frames[k - 1] if k else None, cur, frames[k + 1] if k + 1 < len(frames) else None, fmt, h, w,
                               field_order, T, L, combed)
        finals.append(f)
        match += MATCHES[m]
        cmb.append(bool(cb))
    diffs = [FIRST_DIFF if k == 0 else frame_sad(finals[k], finals[k - 1], fmt) for k in range(len(finals))]
    kept = decimate(diffs, keep_all)
    n = len(frames)
    info = dict(match=match, combed=cmb, diffs=diffs, kept=kept,
                stats=(n, len(kept), match.count("c"), match.count("p"), match.count("n"), sum(cmb), n - len(kept)))
    return [finals[i] for i in kept], info


# ---- synthetic material ---------------------------------------------------------------------------------------------------
def film_frames(fmt, n, h, w, seed=0, noise=3):
    """n progressive frames of fmt: every component plane is a pattern that moves horizontally by several samples a frame (so
    that fields of different frames comb) with per-sample noise of 0 ... noise-1 code values of 8 bits (below T = 9)"""
    nb, shift, mask = _READ[fmt]
    dp = depth(fmt)
    rng = np.random.default_rng(seed)
    frames = [np.zeros(frame_bytes(fmt, h, w) // nb, np.uint8 if nb == 1 else "<u2") for _ in range(n)]
    for k, (off, ph, pw, st) in enumerate(memory_planes(fmt, h, w)):
        for c in range(st):
            y, x = np.mgrid[0:ph, 0:pw]
            for t in range(n):
                v = (((x + 5 * t + 2 * (y // 3) + 3 * c + k) % 8) < 4) * 160 + 40 + rng.integers(0, noise, (ph, pw))
                rows = frames[t][off:off + ph * pw * st].reshape(ph, pw * st)
                rows[:, c::st] = ((v << (dp - 8)) << shift).astype(rows.dtype)
    return [f.view(np.uint8) for f in frames]


def pulldown(film, fmt, h, w, n_out, phase=0, field_order="tff"):
    """2:3 pulldown: n_out video frames from the film frames.  Film frame A B C D -> video AA AB BC CC DD (first field, second
    field), the cycle started `phase` frames in.  -> (video frames, per video frame the film indices (first, second))"""
    pat = [(0, 0), (0, 1), (1, 2), (2, 2), (3, 3)]
    video, src = [], []
    for j in range(n_out):
        q, r = divmod(j + phase, 5)
        a, b = 4 * q + pat[r][0], 4 * q + pat[r][1]
        video.append(weave(film[a], film[b], fmt, h, w, field_order))
        src.append((a, b))
    return video, src
