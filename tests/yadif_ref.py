"""The deinterlacing rule of the raw-video route in numpy: the definition that the kernel
(csrc/uva_deint.hip) and the host restatement (csrc/uva_deint_host.cpp) are held to, bit for bit.

It is yadif's spatio-temporal rule, restated.  PARITY WITH ffmpeg's yadif FILTER IS UNPINNED: ffmpeg is on none of the project's
machines, so no constant, edge rule or field choice here has been checked against the filter.  The rule is fixed here so that the
three implementations agree on it.

The rule works per component plane (pw x ph samples; "x +- j" is the j-th neighbour of the same component): each of Y, Cb, Cr
of a planar format, the two halves of the interleaved chroma plane of nv12 / p010le, the three components of bgr24 / bgr48le.
The chroma rows of a 4:2:0 frame alternate fields as luma rows do.  Samples are code values as the input conversion reads them:
bytes; word >> 6 for p010le; word & 1023 for yuv420p10le / yuv422p10le; whole words for bgr48le.

tff (default): even rows are the first field in time; bff: odd rows.  prev / next None mean cur.  Output A keeps the rows of the
first field and interpolates the others with p2 = prev, n2 = cur; output B keeps the second field's rows, p2 = cur, n2 = next.
Kept rows are copied byte for byte (ignored bits too); an interpolated sample is written as a clean code value in the format's
placement.  For row y, column x of a component plane, in signed 32-bit integers:

    ym = y-1 if y > 0 else y+1        yp = y+1 if y+1 < ph else y-1
    c = cur[ym][x]   e = cur[yp][x]   d = (p2[y][x] + n2[y][x]) >> 1
    t0 = |p2[y][x] - n2[y][x]|
    t1 = (|prev[ym][x] - c| + |prev[yp][x] - e|) >> 1
    t2 = (|next[ym][x] - c| + |next[yp][x] - e|) >> 1
    diff = max(t0 >> 1, t1, t2)       sp = (c + e) >> 1
    if 3 <= x < pw-3:
        S(j) = |cur[ym][x-1+j] - cur[yp][x-1-j]| + |cur[ym][x+j] - cur[yp][x-j]| + |cur[ym][x+1+j] - cur[yp][x+1-j]|
        score = S(0) - 1
        for s in (-1, +1):
            if S(s) < score:  score = S(s); sp = (cur[ym][x+s] + cur[yp][x-s]) >> 1
                if S(2s) < score:  score = S(2s); sp = (cur[ym][x+2s] + cur[yp][x-2s]) >> 1
    if not (y == 1 or y+2 == ph):
        ymm = y-2 if y > 0 else y+2    ypp = y+2 if y+1 < ph else y-2
        b = (p2[ymm][x] + n2[ymm][x]) >> 1   f = (p2[ypp][x] + n2[ypp][x]) >> 1
        mx = max(d-e, d-c, min(b-c, f-e))    mn = min(d-e, d-c, max(b-c, f-e))
        diff = max(diff, mn, -mx)
    sp = min(sp, d+diff); sp = max(sp, d-diff)
"""
import numpy as np

FORMATS = ("bgr24", "yuv420p", "nv12", "p010le", "yuv420p10le", "bgr48le", "yuv422p", "yuv422p10le")
# bytes per sample, shift, mask
_READ = {"bgr24": (1, 0, 255), "yuv420p": (1, 0, 255), "nv12": (1, 0, 255), "yuv422p": (1, 0, 255), "p010le": (2, 6, 1023),
         "yuv420p10le": (2, 0, 1023), "yuv422p10le": (2, 0, 1023), "bgr48le": (2, 0, 65535)}


def depth(fmt):
    return {255: 8, 1023: 10, 65535: 16}[_READ[fmt][2]]


def memory_planes(fmt, h, w):
    """[(offset in samples, ph, pw, stride)]: the planes of rows as they lie in memory, `stride` components interleaved"""
    if fmt in ("bgr24", "bgr48le"):
        return [(0, h, w, 3)]
    cw, ch = (w + 1) // 2, (h if fmt.startswith("yuv422") else (h + 1) // 2)
    if fmt in ("nv12", "p010le"):
        return [(0, h, w, 1), (h * w, ch, cw, 2)]
    return [(0, h, w, 1), (h * w, ch, cw, 1), (h * w + ch * cw, ch, cw, 1)]


def frame_bytes(fmt, h, w):
    return sum(ph * pw * st for _, ph, pw, st in memory_planes(fmt, h, w)) * _READ[fmt][0]


def words(frame, fmt):
    """the frame's samples as stored: a flat u8 or little-endian u16 view"""
    a = np.ascontiguousarray(frame).reshape(-1).view(np.uint8)
    return a if _READ[fmt][0] == 1 else a.view("<u2")


def component_planes(frame, fmt, h, w):
    """[(memory plane index, component index, int32 [ph][pw] code values)]"""
    wd = words(frame, fmt)
    _, shift, mask = _READ[fmt]
    out = []
    for k, (off, ph, pw, st) in enumerate(memory_planes(fmt, h, w)):
        rows = wd[off:off + ph * pw * st].reshape(ph, pw * st)
        for c in range(st):
            out.append((k, c, ((rows[:, c::st].astype(np.int32) >> shift) & mask)))
    return out


class Census:
    """per interpolated sample: the chosen spatial step, the clamp, the temporal term that set diff, what raised it, the column
    class and the row class"""

    def __init__(self):
        self.step = {s: 0 for s in (-2, -1, 0, 1, 2)}
        self.clamp = {"upper": 0, "lower": 0, "none": 0}
        self.term = {"t0": 0, "t1": 0, "t2": 0}
        self.raised = {"mn": 0, "-mx": 0, "none": 0}
        self.column = {"edge": 0, "inner": 0}
        self.row = {"full": 0, "short": 0}

    def classes(self):
        return {name: dict(getattr(self, name)) for name in ("step", "clamp", "term", "raised", "column", "row")}

    def empty(self):
        return [(name, k) for name, d in self.classes().items() for k, v in d.items() if v == 0]


def interp_row(prev, cur, nxt, p2, n2, y, census=None):
    """row y of one component plane (int32 [ph][pw] arrays) -> int32 [pw]"""
    ph, pw = cur.shape
    ym = y - 1 if y > 0 else y + 1
    yp = y + 1 if y + 1 < ph else y - 1
    c, e = cur[ym], cur[yp]
    d = (p2[y] + n2[y]) >> 1
    t0 = np.abs(p2[y] - n2[y])
    t1 = (np.abs(prev[ym] - c) + np.abs(prev[yp] - e)) >> 1
    t2 = (np.abs(nxt[ym] - c) + np.abs(nxt[yp] - e)) >> 1
    diff = np.maximum(np.maximum(t0 >> 1, t1), t2)
    term = np.where((t0 >> 1) >= np.maximum(t1, t2), 0, np.where(t1 >= t2, 1, 2))
    sp = (c + e) >> 1
    step = np.zeros(pw, np.int32)
    if pw >= 7:
        x = np.arange(3, pw - 3)

        def S(j):
            return (np.abs(c[x - 1 + j] - e[x - 1 - j]) + np.abs(c[x + j] - e[x - j]) + np.abs(c[x + 1 + j] - e[x + 1 - j]))
        score = S(0) - 1
        spi, sti = sp[x].copy(), np.zeros(x.size, np.int32)
        for s in (-1, 1):
            m1 = S(s) < score
            score = np.where(m1, S(s), score)
            spi = np.where(m1, (c[x + s] + e[x - s]) >> 1, spi)
            sti = np.where(m1, s, sti)
            m2 = m1 & (S(2 * s) < score)
            score = np.where(m2, S(2 * s), score)
            spi = np.where(m2, (c[x + 2 * s] + e[x - 2 * s]) >> 1, spi)
            sti = np.where(m2, 2 * s, sti)
        sp = sp.copy()
        sp[x] = spi
        step[x] = sti
    full = not (y == 1 or y + 2 == ph)
    raised = np.zeros(pw, np.int32)
    if full:
        ymm = y - 2 if y > 0 else y + 2
        ypp = y + 2 if y + 1 < ph else y - 2
        b = (p2[ymm] + n2[ymm]) >> 1
        f = (p2[ypp] + n2[ypp]) >> 1
        mx = np.maximum(np.maximum(d - e, d - c), np.minimum(b - c, f - e))
        mn = np.minimum(np.minimum(d - e, d - c), np.maximum(b - c, f - e))
        raised = np.where((mn > diff) & (mn >= -mx), 1, np.where(-mx > diff, 2, 0))
        diff = np.maximum(np.maximum(diff, mn), -mx)
    out = np.maximum(np.minimum(sp, d + diff), d - diff)
    if census is not None:
        for s in census.step:
            census.step[s] += int(np.count_nonzero(step == s))
        census.clamp["upper"] += int(np.count_nonzero(sp > d + diff))
        census.clamp["lower"] += int(np.count_nonzero(sp < d - diff))
        census.clamp["none"] += int(np.count_nonzero((sp <= d + diff) & (sp >= d - diff)))
        for k, name in enumerate(("t0", "t1", "t2")):
            census.term[name] += int(np.count_nonzero(term == k))
        for k, name in enumerate(("none", "mn", "-mx")):
            census.raised[name] += int(np.count_nonzero(raised == k))
        inner = max(0, pw - 6)
        census.column["inner"] += inner
        census.column["edge"] += pw - inner
        census.row["full" if full else "short"] += pw
    return out


def deinterlace(prev, cur, nxt, fmt, h, w, field_order="tff", census=None):
    """-> (A, B): flat u8 frames.  prev / nxt None mean cur.  census: a Census, or a pair of them for A and B."""
    if h < 4 or w < 1:
        raise ValueError("deinterlace: h >= 4 and w >= 1")
    prev = cur if prev is None else prev
    nxt = cur if nxt is None else nxt
    _, shift, _ = _READ[fmt]
    pa = 0 if field_order == "bff" else 1            # the parity of the rows that A interpolates
    cp, cc, cn = (component_planes(f, fmt, h, w) for f in (prev, cur, nxt))
    outs = []
    for o in range(2):
        out = np.array(words(cur, fmt), copy=True)
        par = pa if o == 0 else 1 - pa
        cen = census[o] if isinstance(census, (tuple, list)) else census
        mp = memory_planes(fmt, h, w)
        for (k, c, pv), (_, _, cu), (_, _, nx) in zip(cp, cc, cn):
            off, ph, pw, st = mp[k]
            p2, n2 = (pv, cu) if o == 0 else (cu, nx)
            rows = out[off:off + ph * pw * st].reshape(ph, pw * st)
            for y in range(par, ph, 2):
                rows[y, c::st] = (interp_row(pv, cu, nx, p2, n2, y, cen) << shift).astype(rows.dtype)
        outs.append(out.view(np.uint8))
    return outs[0], outs[1]


def deinterlace_sequence(frames, fmt, h, w, mode="frame", field_order="tff"):
    """a whole stream -> the list of output frames, in order (A, or A then B, per input frame)"""
    out = []
    for k, cur in enumerate(frames):
        a, b = deinterlace(frames[k - 1] if k else None, cur, frames[k + 1] if k + 1 < len(frames) else None, fmt, h, w, field_order)
        out.append(a)
        if mode == "field":
            out.append(b)
    return out


def census(frames, fmt, h, w, field_order="tff"):
    """-> (Census of every output A, Census of every output B) over the stream"""
    ca, cb = Census(), Census()
    for k, cur in enumerate(frames):
        deinterlace(frames[k - 1] if k else None, cur, frames[k + 1] if k + 1 < len(frames) else None, fmt, h, w, field_order, (ca, cb))
    return ca, cb


def interlaced_sequence(n, h, w, depth=8, seed=0):
    """n planes [h][w] of code values of `depth` bits whose two fields belong to different instants, in thirds by width: a static
    gradient with a little noise, diagonals that move (slopes +1, -1, +2, -2 in four row bands), white noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    s = np.array([1, -1, 2, -2])[np.minimum(3, y * 4 // h)]
    out = []
    for t in range(n):
        left = (3 * x + 5 * y) % 97 + 60 + rng.integers(0, 3, (h, w))
        mid = (((x - s * y - 3 * t - (y & 1)) % 12) < 5) * 150 + 40
        right = rng.integers(0, 256, (h, w))
        v = np.where(x < w // 3, left, np.where(x < 2 * w // 3, mid, right))
        out.append((v * ((1 << depth) - 1) // 255).astype(np.int64))
    return out


def sequence_frames(fmt, n, h, w, seed=0, dirty=False):
    """n frames of fmt whose every component plane is an interlaced_sequence of its own.  dirty: the bits that the converter
    ignores in a 10-bit format are random instead of zero."""
    nb, shift, mask = _READ[fmt]
    rng = np.random.default_rng(seed + 1000)
    frames = [np.zeros(frame_bytes(fmt, h, w) // nb, np.uint8 if nb == 1 else "<u2") for _ in range(n)]
    for k, (off, ph, pw, st) in enumerate(memory_planes(fmt, h, w)):
        for c in range(st):
            seq = interlaced_sequence(n, ph, pw, depth(fmt), seed * 31 + 7 * k + c)
            for t in range(n):
                rows = frames[t][off:off + ph * pw * st].reshape(ph, pw * st)
                rows[:, c::st] = (seq[t] << shift).astype(rows.dtype)
    if dirty and nb == 2 and mask == 1023:
        junk = (1 << 6) - 1 if shift else 0xfc00
        for f in frames:
            f |= rng.integers(0, 65536, f.size).astype(f.dtype) & junk
    return [f.view(np.uint8) for f in frames]
