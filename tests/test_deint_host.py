"""The deinterlacer without a GPU: the rule's definition tests/yadif_ref.py takes every one of its
branches on the test sequence, the library's host restatement (uva_debug_deint_host, csrc/uva_deint_host.cpp) equals it bit for
bit for every format, field order, output and position in a stream, and every refusal comes with its text before a GPU is looked
for."""
import ctypes

import numpy as np
import pytest

import yadif_ref as ref

FORMATS = list(ref.FORMATS)
SIZES = [(4, 1), (5, 7), (9, 6), (16, 48), (37, 53)]


def test_the_census_sequence_takes_every_branch():
    """four frames of 16 x 48: every spatial step, both clamps, every temporal term, both raises, edge and inner columns, full
    and short rows, in output A and in output B"""
    frames = ref.sequence_frames("yuv420p", 4, 16, 48, seed=1)
    for order in ("tff", "bff"):
        for which, c in zip("AB", ref.census(frames, "yuv420p", 16, 48, order)):
            print(order, which, c.classes())
            assert c.empty() == [], (order, which, c.classes())


@pytest.mark.parametrize("h,w", [(5, 7), (9, 6), (4, 1)])
def test_small_frames_take_the_edge_and_short_row_branches(h, w):
    frames = ref.sequence_frames("yuv420p", 4, h, w, seed=2)
    both = [c for order in ("tff", "bff") for c in ref.census(frames, "yuv420p", h, w, order)]
    # (which output meets a short row -- y == 1 or y + 2 == ph -- depends on the field order and on ph being even or odd)
    assert sum(c.row["short"] for c in both) > 0 and sum(c.row["full"] for c in both) > 0
    for c in both:
        assert c.column["edge"] > 0 and (c.column["inner"] > 0) == (w >= 7)


def test_kept_rows_are_the_frames_bytes():
    for fmt in FORMATS:
        h, w = 9, 6
        fr = ref.sequence_frames(fmt, 3, h, w, seed=4, dirty=True)
        for order, pa in (("tff", 1), ("bff", 0)):
            a, b = ref.deinterlace(fr[0], fr[1], fr[2], fmt, h, w, order)
            for off, ph, pw, st in ref.memory_planes(fmt, h, w):
                rows = [ref.words(x, fmt)[off:off + ph * pw * st].reshape(ph, pw * st) for x in (a, b, fr[1])]
                # A keeps the rows it does not interpolate, B the others: together the kept rows are the whole frame
                assert np.array_equal(rows[0][1 - pa::2], rows[2][1 - pa::2]) and np.array_equal(rows[1][pa::2], rows[2][pa::2])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("h,w", SIZES)
def test_host_restatement_equals_the_reference(uva, fmt, h, w):
    n = 4
    fr = ref.sequence_frames(fmt, n, h, w, seed=h * 100 + w)
    assert fr[0].size == uva.pix_frame_bytes(fmt, h, w) == ref.frame_bytes(fmt, h, w)
    for order in ("tff", "bff"):
        for k in range(n):                              # the first frame, middle frames, the last frame
            p, c, nx = (fr[k - 1] if k else None), fr[k], (fr[k + 1] if k + 1 < n else None)
            want_a, want_b = ref.deinterlace(p, c, nx, fmt, h, w, order)
            a, b = uva.deint_frames(p, c, nx, fmt, h, w, "field", order, host=True)
            assert np.array_equal(a, want_a), (fmt, h, w, order, k, "A")
            assert np.array_equal(b, want_b), (fmt, h, w, order, k, "B")
            a, b = uva.deint_frames(p, c, nx, fmt, h, w, "frame", order, host=True)
            assert b is None and np.array_equal(a, want_a)


@pytest.mark.parametrize("fmt", ["p010le", "yuv420p10le", "yuv422p10le"])
def test_ignored_bits_leave_interpolated_samples_alone_and_stay_in_kept_rows(uva, fmt):
    h, w = 16, 48
    clean = ref.sequence_frames(fmt, 3, h, w, seed=5)
    dirty = ref.sequence_frames(fmt, 3, h, w, seed=5, dirty=True)
    assert not np.array_equal(clean[1], dirty[1])
    got = uva.deint_frames(dirty[0], dirty[1], dirty[2], fmt, h, w, "field", host=True)
    base = uva.deint_frames(clean[0], clean[1], clean[2], fmt, h, w, "field", host=True)
    want = ref.deinterlace(dirty[0], dirty[1], dirty[2], fmt, h, w)
    for o in range(2):
        assert np.array_equal(got[o], want[o])
        par = 1 - o                                     # tff: A interpolates the odd rows, B the even ones
        for off, ph, pw, st in ref.memory_planes(fmt, h, w):
            g, b, d = (ref.words(x, fmt)[off:off + ph * pw * st].reshape(ph, pw * st) for x in (got[o], base[o], dirty[1]))
            assert np.array_equal(g[par::2], b[par::2])
            assert np.array_equal(g[1 - par::2], d[1 - par::2])


@pytest.mark.parametrize("fmt", ["yuv420p", "bgr24", "yuv420p10le", "p010le", "bgr48le"])
def test_saturated_sequences(uva, fmt):
    """all 0, all maximum, rows alternating 0 / maximum between the fields: at 16 bits |65535 - 0| summed three times"""
    h, w = 16, 48
    nb = ref.frame_bytes(fmt, h, w)
    top = {8: 255, 10: 1023, 16: 65535}[ref.depth(fmt)] << (6 if fmt == "p010le" else 0)
    zero = np.zeros(nb, np.uint8)
    full = np.full(nb, top, np.uint8) if ref.depth(fmt) == 8 else np.full(nb // 2, top, "<u2").view(np.uint8)
    comb = full.copy()
    for off, ph, pw, st in ref.memory_planes(fmt, h, w):
        ref.words(comb, fmt)[off:off + ph * pw * st].reshape(ph, pw * st)[0::2] = 0
    for trio in ((zero, zero, zero), (full, full, full), (comb, comb, comb), (zero, comb, full), (full, comb, zero), (comb, full, comb)):
        for order in ("tff", "bff"):
            want = ref.deinterlace(*trio, fmt, h, w, order)
            got = uva.deint_frames(*trio, fmt, h, w, "field", order, host=True)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            assert int(ref.words(got[0], fmt).max()) <= top


def test_refusals_come_with_their_texts_before_a_gpu_is_looked_for(uva):
    from upscale_video_amd import _lib
    L = _lib.load()
    assert L.uva_abi_version() == 15
    for name in ("uva_deint_check", "uva_deint_frames", "uva_deint_frames_device", "uva_debug_deint_frames", "uva_debug_deint_host",
                 "uva_deint_create", "uva_deint_push", "uva_deint_reset", "uva_deint_destroy"):
        assert name in _lib.OPTIONAL_SYMBOLS and hasattr(L, name), name
    err = lambda: L.uva_last_error().decode()          # noqa: E731
    YUV, FIELD = uva.PIX_FORMATS_ALL["yuv420p"], 1
    for args, text in (((4, 8, 8, 0), "unknown pixel format"), ((9, 8, 8, 0), "unknown pixel format"), ((YUV, 8, 8, 4), "unknown flag bits"),
                       ((YUV, 0, 8, 0), "bad image size"), ((YUV, 8, 0, 0), "bad image size"), ((YUV, 1 << 15, (1 << 13) + 1, 0), "bad image size"),
                       ((YUV, 3, 8, 0), "fewer than 4 rows")):
        assert L.uva_deint_check(*args) != 0 and text in err(), (args, err())
    assert L.uva_deint_check(YUV, 4, 1, 3) == 0
    with pytest.raises(_lib.UvaError, match="fewer than 4 rows"):
        uva.deint_check("nv12", 2, 16)
    with pytest.raises(ValueError, match="unknown deinterlace mode"):
        uva.deint_flags("bob")
    with pytest.raises(ValueError, match="unknown field order"):
        uva.deint_flags("frame", "top")
    # the stateless entries: every refusal of the check, then null pointers and outputs that do not exist
    buf = np.zeros(uva.pix_frame_bytes("yuv420p", 8, 8), np.uint8)
    p, o1, o2 = buf.ctypes.data, buf.copy(), buf.copy()
    entries = (lambda *a: L.uva_deint_frames(0, *a), lambda *a: L.uva_deint_frames_device(0, *a), lambda *a: L.uva_debug_deint_frames(0, *a, 0),
               lambda *a: L.uva_debug_deint_host(*a))
    for call in entries:
        for args, text in (((p, p, p, YUV, 3, 8, 0, o1.ctypes.data, None), "fewer than 4 rows"),
                           ((p, p, p, 4, 8, 8, 0, o1.ctypes.data, None), "unknown pixel format"),
                           ((p, p, p, YUV, 8, 8, 8, o1.ctypes.data, None), "unknown flag bits"),
                           ((p, None, p, YUV, 8, 8, 0, o1.ctypes.data, None), "null frame pointer"),
                           ((p, p, p, YUV, 8, 8, FIELD, None, None), "neither output"),
                           ((p, p, p, YUV, 8, 8, 0, o1.ctypes.data, o2.ctypes.data), "UVA_DEINT_FIELD only")):
            assert call(*args) != 0 and text in err(), (args, err())
    assert L.uva_debug_deint_frames(0, p, p, p, YUV, 8, 8, 0, o1.ctypes.data, None, -1) != 0 and "max_groups" in err()
    assert L.uva_deint_frames_device(0, p + 1, p, p, YUV, 8, 8, 0, o1.ctypes.data, None) != 0 and "16-byte aligned" in err()
    # the handle's entries refuse null pointers and sizes without touching a GPU
    h = ctypes.c_void_p()
    assert L.uva_deint_create(0, YUV, 3, 8, 0, ctypes.byref(h)) != 0 and "fewer than 4 rows" in err() and not h.value
    assert L.uva_deint_create(0, YUV, 8, 8, 0, None) != 0 and "null pointer" in err()
    n = ctypes.c_int(7)
    assert L.uva_deint_push(None, p, o1.ctypes.data, None, ctypes.byref(n)) != 0 and "null pointer" in err()
    assert L.uva_deint_reset(None) != 0 and "null pointer" in err()
    L.uva_deint_destroy(None)
    # B alone is a legal call of the host restatement
    a, b = uva.deint_frames(None, buf, None, "yuv420p", 8, 8, "field", host=True)
    only_b = buf.copy()
    assert L.uva_debug_deint_host(None, p, None, YUV, 8, 8, FIELD, None, only_b.ctypes.data) == 0 and np.array_equal(only_b, b)


def test_the_command_line_refuses_before_any_gpu_work(capsys):
    from upscale_video_amd import rawvideo
    for argv, text in ((["--deinterlace", "bob"], "--deinterlace takes frame or field"),
                       (["--deinterlace", "frame", "--field-order", "top"], "--field-order takes tff or bff"),
                       (["--field-order", "bff"], "--field-order needs --deinterlace"),
                       (["--deinterlace", "field", "-H", "3"], "fewer than 4 rows")):
        with pytest.raises(SystemExit):
            rawvideo.main(["-W", "8", "-H", "8"] + argv)
        assert text in capsys.readouterr().err


def test_the_reader_counts_input_frames_and_discards_context():
    """deinterlaced() with a stand-in for the Deinterlacer: --frames counts input frames, a leading context frame's outputs are
    dropped, a trailing one replaces the flush"""
    import io
    from upscale_video_amd import rawvideo

    class Fake:
        def __init__(self):
            self.log, self.n = [], 0

        def push(self, frame, outs):
            self.log.append(int(frame[0]))
            self.n += 1
            return 0 if self.n == 1 else 2

        def flush(self, outs):
            self.log.append("flush")
            k, self.n = (2 if self.n else 0), 0
            return k

        def reset(self):
            self.log.append("reset")
            self.n = 0
    data = bytes(range(6))                               # six frames of one byte
    raw = np.zeros(1, np.uint8)
    for kw, log, counts in ((dict(), [0, 1, 2, 3, 4, 5, "flush"], [0, 2, 2, 2, 2, 2, 2]),
                            (dict(max_frames=3), [0, 1, 2, "flush"], [0, 2, 2, 2]),
                            (dict(max_frames=3, trail=True), [0, 1, 2, 3, "reset"], [0, 2, 2, 2]),
                            (dict(max_frames=2, lead=True, trail=True), [0, 1, 2, 3, "reset"], [0, 0, 2, 2]),
                            (dict(max_frames=5, lead=True, trail=True), [0, 1, 2, 3, 4, 5, "flush"], [0, 0, 2, 2, 2, 2, 2])):
        fake = Fake()
        got = list(rawvideo.deinterlaced(io.BytesIO(data), fake, raw, lambda: None, **kw))
        assert fake.log == log and got == counts, (kw, fake.log, got)
