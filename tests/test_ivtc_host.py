"""The inverse telecine's host half against tests/ivtc_ref.py, without a GPU: the library's scalar
restatement of weave, metric and decision (uva_debug_ivtc_host), its decimator driven as uva_ivtc_push drives it
(uva_debug_ivtc_decimate), every refusal, the exported symbols, the command line's refusals and the reader."""
import io

import numpy as np
import pytest

import ivtc_ref as ref
import yadif_ref

FORMATS = list(ref.FORMATS)
ORDERS = ["tff", "bff"]
SIZES = [(4, 1), (5, 7), (9, 6), (16, 48), (37, 53)]


def neighbours(fr, k):
    return (fr[k - 1] if k else None), fr[k], (fr[k + 1] if k + 1 < len(fr) else None)


def check(uva, trio, fmt, h, w, order, T=9, L=1000):
    for policy in ("yadif", "keep"):
        st, woven, chosen, match, combed = uva.ivtc_metrics(*trio, fmt, h, w, order, thresh=T, host=True, combed=policy, combed_limit=L)
        assert st == ref.metrics(*trio, fmt, h, w, order, T), (fmt, h, w, order, T)
        cur = trio[1]
        for k, x in enumerate((cur, cur if trio[0] is None else trio[0], cur if trio[2] is None else trio[2])):
            assert np.array_equal(woven[k], ref.weave(cur, x, fmt, h, w, order)), (fmt, h, w, order, k)
        want, m, cb = ref.final_frame(*trio, fmt, h, w, order, T, L, policy)
        assert (match, combed) == (m, bool(cb)) and np.array_equal(chosen, want), (fmt, h, w, order, policy)
    return st, match, combed


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("h,w", SIZES)
def test_host_against_the_reference(uva, fmt, h, w):
    """first / middle / last frame of a stream with dirty ignored bits, both orders, several T and L"""
    fr = yadif_ref.sequence_frames(fmt, 3, h, w, seed=h + w, dirty=True)
    for order in ORDERS:
        for k in range(3):
            check(uva, neighbours(fr, k), fmt, h, w, order)
        check(uva, neighbours(fr, 1), fmt, h, w, order, T=0, L=0)
        check(uva, neighbours(fr, 1), fmt, h, w, order, T=255, L=1000000)


@pytest.mark.parametrize("fmt", ["p010le", "yuv420p10le", "yuv422p10le"])
def test_bits_the_converter_ignores_do_not_count(uva, fmt):
    h, w = 9, 6
    clean = yadif_ref.sequence_frames(fmt, 3, h, w, seed=2)
    dirty = yadif_ref.sequence_frames(fmt, 3, h, w, seed=2, dirty=True)
    assert not np.array_equal(clean[1], dirty[1])
    a = uva.ivtc_metrics(*clean, fmt, h, w, host=True)
    b = uva.ivtc_metrics(*dirty, fmt, h, w, host=True)
    assert a[0] == b[0] and (a[3], a[4]) == (b[3], b[4])
    assert np.array_equal(b[1][1], ref.weave(dirty[1], dirty[0], fmt, h, w))         # ... and woven rows keep them


@pytest.mark.parametrize("fmt", FORMATS)
def test_saturated_frames(uva, fmt):
    """all 0, all maximum, rows alternating 0 / maximum: the maximum of N and M"""
    h, w = 16, 48
    nb = ref.frame_bytes(fmt, h, w)
    top = {8: 255, 10: 1023, 16: 65535}[ref.depth(fmt)]
    word = top << (6 if fmt == "p010le" else 0)
    zero = np.zeros(nb, np.uint8)
    full = (np.full(nb, word, np.uint8) if ref.depth(fmt) == 8 else np.full(nb // 2, word, "<u2").view(np.uint8))
    comb = full.copy()
    for off, ph, pw, st in ref.memory_planes(fmt, h, w):
        ref.words(comb, fmt)[off:off + ph * pw * st].reshape(ph, pw * st)[0::2] = 0
    _, ph, pw, st = ref.memory_planes(fmt, h, w)[0]
    for trio in ((zero, zero, zero), (full, full, full), (comb, comb, comb), (zero, comb, full), (full, comb, zero), (comb, full, comb)):
        for order in ORDERS:
            check(uva, trio, fmt, h, w, order)
            check(uva, trio, fmt, h, w, order, T=0)
    stats, match, combed = check(uva, (comb, comb, comb), fmt, h, w, "tff", L=999999)
    every = (ph - 2) * pw * memory_stride(fmt)
    assert stats[:2] == (every, every * top)
    assert match == 0 and combed
    assert not check(uva, (comb, comb, comb), fmt, h, w, "tff", L=1000000)[2]        # N * 10^6 > L * all is strict


def memory_stride(fmt):
    return ref.memory_planes(fmt, 4, 4)[0][3]


def test_ties(uva):
    fmt, h, w = "yuv420p", 16, 48
    f = ref.film_frames(fmt, 2, h, w)
    st, match, combed = check(uva, (f[0], f[0], f[0]), fmt, h, w, "tff")
    assert match == 0 and not combed and st[0:2] == st[2:4] == st[4:6]
    # p and n equal and better than c: p
    mixed = ref.weave(f[0], f[1], fmt, h, w)
    st, match, _ = check(uva, (f[0], mixed, f[0]), fmt, h, w, "tff")
    assert st[3] == st[5] < st[1] and match == 1
    # equal diffs drop the earliest; the first frame's diff is 2^64 - 1
    big = ref.FIRST_DIFF
    assert uva.ivtc_decimate([big, 5, 3, 3, 9]) == [0, 1, 3, 4]
    assert uva.ivtc_decimate([big, big, big, big, big]) == [1, 2, 3, 4]


def test_the_decimator_against_the_reference(uva):
    rng = np.random.default_rng(5)
    for n in range(0, 28):
        diffs = [ref.FIRST_DIFF] * min(n, 1) + [int(v) for v in rng.integers(0, 4, max(0, n - 1))]       # (many ties)
        assert uva.ivtc_decimate(diffs) == ref.decimate(diffs), diffs
        assert len(ref.decimate(diffs)) == n - n // 5
        assert uva.ivtc_decimate(diffs, keep_all=True) == list(range(n))
    diffs = [int(v) for v in rng.integers(0, 1 << 63, 25)]
    assert uva.ivtc_decimate(diffs) == ref.decimate(diffs)


def test_every_refusal(uva):
    from upscale_video_amd import _lib
    L = _lib.load()
    YUV = uva.PIX_FORMATS_ALL["yuv420p"]
    for name in ("uva_ivtc_check", "uva_ivtc_metrics", "uva_ivtc_metrics_device", "uva_debug_ivtc_metrics", "uva_debug_ivtc_host",
                 "uva_debug_ivtc_decimate", "uva_ivtc_create", "uva_ivtc_push", "uva_ivtc_reset", "uva_ivtc_stats", "uva_ivtc_destroy"):
        assert name in _lib.OPTIONAL_SYMBOLS and hasattr(L, name), name
    assert L.uva_abi_version() == 15
    bad = [(4, 8, 8, 0, 9, 1000, "unknown pixel format"), (99, 8, 8, 0, 9, 1000, "unknown pixel format"), (YUV, 3, 8, 0, 9, 1000, "fewer than 4 rows"),
           (YUV, 0, 8, 0, 9, 1000, "bad image size"), (YUV, 8, 0, 0, 9, 1000, "bad image size"), (YUV, 1 << 15, (1 << 13) + 1, 0, 9, 1000, "bad image size"),
           (YUV, 8, 8, 8, 9, 1000, "unknown flag bits"), (YUV, 8, 8, -1, 9, 1000, "unknown flag bits"), (YUV, 8, 8, 0, -1, 1000, "threshold T"),
           (YUV, 8, 8, 0, 256, 1000, "threshold T"), (YUV, 8, 8, 0, 9, -1, "limit L"), (YUV, 8, 8, 0, 9, 1000001, "limit L")]
    frame = np.zeros(ref.frame_bytes("yuv420p", 8, 8), np.uint8)
    st = np.zeros(6, np.uint64)
    import ctypes
    handle = ctypes.c_void_p()
    for fmt, h, w, flags, T, Lm, text in bad:
        assert L.uva_ivtc_check(fmt, h, w, flags, T, Lm) == 1 and text in L.uva_last_error().decode(), (fmt, h, w, flags, T, Lm)
        # the entries that would use a GPU refuse before they look for one
        if Lm == 1000:
            assert L.uva_ivtc_metrics(0, None, frame.ctypes.data, None, fmt, h, w, flags, T, st.ctypes.data) == 1
            assert text in L.uva_last_error().decode()
            assert L.uva_debug_ivtc_metrics(0, None, frame.ctypes.data, None, fmt, h, w, flags, T, st.ctypes.data, 1) == 1
            assert L.uva_ivtc_metrics_device(0, None, frame.ctypes.data, None, fmt, h, w, flags, T, st.ctypes.data) == 1
        assert L.uva_ivtc_create(0, fmt, h, w, flags, T, Lm, ctypes.byref(handle)) == 1 and text in L.uva_last_error().decode()
        assert handle.value is None
        assert L.uva_debug_ivtc_host(None, frame.ctypes.data, None, fmt, h, w, flags, T, Lm, st.ctypes.data, None, None, None) == 1
    assert L.uva_ivtc_check(YUV, 4, 1, 7, 255, 1000000) == 0 and L.uva_ivtc_check(YUV, 1 << 14, 1 << 14, 0, 0, 0) == 0
    assert L.uva_ivtc_metrics(0, None, None, None, YUV, 8, 8, 0, 9, st.ctypes.data) == 1 and "null" in L.uva_last_error().decode()
    assert L.uva_debug_ivtc_metrics(0, None, frame.ctypes.data, None, YUV, 8, 8, 0, 9, st.ctypes.data, -1) == 1
    assert L.uva_debug_ivtc_host(None, None, None, YUV, 8, 8, 0, 9, 1000, st.ctypes.data, None, None, None) == 1
    assert L.uva_ivtc_push(None, None, None, None) == 1 and L.uva_ivtc_reset(None) == 1 and L.uva_ivtc_stats(None, None) == 1
    L.uva_ivtc_destroy(None)
    with pytest.raises(ValueError):
        uva.ivtc_flags("top")
    with pytest.raises(ValueError):
        uva.ivtc_flags(combed="bob")
    with pytest.raises(_lib.UvaError, match="fewer than 4 rows"):
        uva.ivtc_check("yuv420p", 3, 8)
    uva.ivtc_check("bgr48le", 4, 1, "bff", 0, "keep", 0, True)


def test_the_command_line_refuses_before_any_gpu_work(capsys):
    from upscale_video_amd import rawvideo
    for argv, text in ((["--detelecine", "--deinterlace", "frame"], "exclude each other"),
                       (["--detelecine-thresh", "5"], "--detelecine-thresh needs --detelecine"),
                       (["--detelecine-combed", "keep"], "--detelecine-combed needs --detelecine"),
                       (["--detelecine-combed-limit", "5"], "--detelecine-combed-limit needs --detelecine"),
                       (["--detelecine-keep-all"], "--detelecine-keep-all needs --detelecine"),
                       (["--field-order", "bff"], "--field-order needs --deinterlace frame|field or --detelecine"),
                       (["--detelecine", "--field-order", "top"], "--field-order takes tff or bff"),
                       (["--detelecine", "--detelecine-combed", "bob"], "--detelecine-combed takes yadif or keep"),
                       (["--detelecine", "--detelecine-thresh", "256"], "--detelecine-thresh is 0 ... 255"),
                       (["--detelecine", "--detelecine-thresh", "-1"], "--detelecine-thresh is 0 ... 255"),
                       (["--detelecine", "--detelecine-combed-limit", "1000001"], "--detelecine-combed-limit is 0 ... 1000000"),
                       (["--detelecine", "-H", "3"], "fewer than 4 rows")):
        with pytest.raises(SystemExit):
            rawvideo.main(["-W", "8", "-H", "8"] + argv)
        assert text in capsys.readouterr().err, argv
    with pytest.raises(SystemExit):
        rawvideo.main(["--help"])
    out = capsys.readouterr().out
    assert "4/5" in out and "unpinned" in out and "guess" in out


class StandIn:
    """a Detelecine that hands frames through with the handle's timing: a full five is delivered over the next four calls"""

    def __init__(self, uva, keep_all=False):
        self.uva, self.keep_all, self.diffs, self.frames, self.queue, self.ended, self.flushes = uva, keep_all, [], [], [], False, 0

    def _deliver(self, out):
        want = self.uva.ivtc_decimate(self.diffs, self.keep_all) if self.ended else None
        if want is None:                 # frames of complete cycles only
            full = len(self.diffs) // 5 * 5 if not self.keep_all else len(self.diffs)
            want = self.uva.ivtc_decimate(self.diffs[:full], self.keep_all)
        if len(self.queue) < len(want):
            j = want[len(self.queue)]
            self.queue.append(j)
            out[:] = self.frames[j]
            return 1
        return 0

    def push(self, frame, out):
        assert not self.ended
        self.frames.append(np.array(frame, copy=True))
        self.diffs.append(ref.FIRST_DIFF if len(self.frames) == 1 else 1 + len(self.frames) % 3)
        return self._deliver(out)

    def flush(self, out):
        self.ended = True
        self.flushes += 1
        k = self._deliver(out)
        if not k:
            self.__init__(self.uva, self.keep_all)
        return k


def test_the_reader_flushes_until_empty(uva):
    from upscale_video_amd import rawvideo
    nb = 12
    frames = [np.full(nb, k, np.uint8) for k in range(13)]
    data = b"".join(f.tobytes() for f in frames)
    for max_frames, n_in in ((None, 13), (12, 12), (5, 5), (4, 4), (0, 0)):
        dt, raw, out = StandIn(uva), np.empty(nb, np.uint8), np.empty(nb, np.uint8)
        got = []
        for k in rawvideo.detelecined(io.BytesIO(data), dt, raw, lambda: [out], max_frames):
            assert k in (0, 1)
            if k:
                got.append(int(out[0]))
        diffs = [ref.FIRST_DIFF] * min(1, n_in) + [1 + (k + 1) % 3 for k in range(1, n_in)]
        assert got == ref.decimate(diffs) and len(got) == n_in - n_in // 5, (max_frames, got)
    with pytest.raises(ValueError):
        next(rawvideo.detelecined(io.BytesIO(data), StandIn(uva), raw, lambda: [out], None, lead=True))
    spec = rawvideo.DetelecineSpec("bff", 12, "keep", 500, True)
    assert spec.per_frame == 1 and spec.out_frames(20) == 20 and rawvideo.DetelecineSpec().out_frames(23) == 19
    assert rawvideo._front_reader(spec) is rawvideo.detelecined and rawvideo._front_reader(rawvideo.DeintSpec()) is rawvideo.deinterlaced
    for bad in (dict(thresh=256), dict(combed_limit=-1), dict(field_order="top"), dict(combed="bob")):
        with pytest.raises(ValueError):
            rawvideo.DetelecineSpec(**bad)
    with pytest.raises(ValueError, match="not cut into segments"):
        rawvideo.stream_segments("a.raw", "b.raw", 8, 8, [[], []], 1, deint=rawvideo.DetelecineSpec())
