"""Deinterlacing on the MI355X (-m gpu).  Everything is integer arithmetic and every comparison is bit for
bit: deint_kernel against tests/yadif_ref.py for every format, field order and mode, the stateful handle against the stateless
calls, and the command line file to file against runs on frames that the reference deinterlaced."""
import functools
import io

import numpy as np
import pytest

import yadif_ref as ref
from conftest import load_net
from upscale_video_amd import rawvideo

pytestmark = pytest.mark.gpu

FORMATS = list(ref.FORMATS)
ORDERS = ["tff", "bff"]


@functools.lru_cache(maxsize=None)
def sequence(fmt, n, h, w, dirty=False):
    return tuple(ref.sequence_frames(fmt, n, h, w, seed=h * 100 + w, dirty=dirty))


@functools.lru_cache(maxsize=None)
def expected(fmt, n, h, w, k, order, dirty=False):
    """the reference's (A, B) of frame k of sequence(fmt, n, h, w)"""
    fr = sequence(fmt, n, h, w, dirty)
    return ref.deinterlace(fr[k - 1] if k else None, fr[k], fr[k + 1] if k + 1 < n else None, fmt, h, w, order)


def neighbours(fr, k):
    return (fr[k - 1] if k else None), fr[k], (fr[k + 1] if k + 1 < len(fr) else None)


# ---- the kernel against the reference ---------------------------------------------------------------------------------------
# 4 x 1, 5 x 7, 9 x 6: every column an edge column, short rows, chroma planes of two and three rows; 16 x 48: the census sequence
# (tests/test_deint_host.py: no branch of the rule is left out); 37 x 53: odd, ragged rows, less than one workgroup
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("h,w", [(4, 1), (5, 7), (9, 6), (16, 48), (37, 53)])
def test_kernel_against_the_reference(uva, fmt, h, w):
    n = 4
    fr = sequence(fmt, n, h, w)
    for order in ORDERS:
        for k in range(n):                          # first frame (prev None), middle frames, last frame (next None)
            want_a, want_b = expected(fmt, n, h, w, k, order)
            a, b = uva.deint_frames(*neighbours(fr, k), fmt, h, w, "field", order)
            assert np.array_equal(a, want_a), (fmt, h, w, order, k, "A")
            assert np.array_equal(b, want_b), (fmt, h, w, order, k, "B")
            a, b = uva.deint_frames(*neighbours(fr, k), fmt, h, w, "frame", order)
            assert b is None and np.array_equal(a, want_a), (fmt, h, w, order, k, "frame")


# 70 x 300: rows of 300, 600, 900 or 1800 bytes start at every alignment that the sample width allows and end in ragged 16-byte
# units; 130 x 1030: several runs of slots per row and many rows -- on a grid of 3 workgroups or of 1 every wave walks many
@pytest.mark.parametrize("fmt", ["yuv420p", "p010le", "bgr48le"])
@pytest.mark.parametrize("h,w,max_groups", [(70, 300, None), (130, 1030, None), (130, 1030, 3), (130, 1030, 1)])
def test_kernel_on_larger_frames(uva, fmt, h, w, max_groups):
    fr = sequence(fmt, 3, h, w)
    for order in ORDERS:
        want_a, want_b = expected(fmt, 3, h, w, 1, order)
        a, b = uva.deint_frames(fr[0], fr[1], fr[2], fmt, h, w, "field", order, max_groups=max_groups)
        assert np.array_equal(a, want_a) and np.array_equal(b, want_b), (fmt, h, w, order, max_groups)


def test_a_null_neighbour_is_the_frame_itself(uva):
    fmt, h, w = "nv12", 37, 53
    fr = sequence(fmt, 4, h, w)
    a, b = uva.deint_frames(None, fr[0], None, fmt, h, w, "field")
    a2, b2 = uva.deint_frames(fr[0], fr[0], fr[0], fmt, h, w, "field")
    want = ref.deinterlace(None, fr[0], None, fmt, h, w)
    assert np.array_equal(a, want[0]) and np.array_equal(b, want[1]) and np.array_equal(a, a2) and np.array_equal(b, b2)


@pytest.mark.parametrize("fmt", ["p010le", "yuv420p10le", "yuv422p10le"])
def test_bits_the_converter_ignores(uva, fmt):
    """they leave interpolated samples unchanged, and kept rows keep them"""
    h, w = 37, 53
    clean, dirty = sequence(fmt, 4, h, w), sequence(fmt, 4, h, w, True)
    assert not np.array_equal(clean[1], dirty[1])
    want = expected(fmt, 4, h, w, 1, "tff", True)
    got = uva.deint_frames(dirty[0], dirty[1], dirty[2], fmt, h, w, "field")
    base = uva.deint_frames(clean[0], clean[1], clean[2], fmt, h, w, "field")
    for o in range(2):
        assert np.array_equal(got[o], want[o])
        (off, ph, pw, st) = ref.memory_planes(fmt, h, w)[0]
        g, b, d = (x.view("<u2")[:ph * pw].reshape(ph, pw) for x in (got[o], base[o], dirty[1]))
        par = 1 - o                                                  # tff: A interpolates the odd rows, B the even ones
        assert np.array_equal(g[par::2], b[par::2])                  # interpolated: clean, and what clean frames give
        assert np.array_equal(g[1 - par::2], d[1 - par::2])          # kept: cur's bytes, ignored bits too


@pytest.mark.parametrize("fmt", ["yuv420p", "yuv422p10le", "p010le", "bgr48le"])
def test_saturated_frames(uva, fmt):
    """all 0, all maximum, and rows alternating 0 / maximum between the fields: 16-bit differences summed three times"""
    h, w = 16, 48
    nb = ref.frame_bytes(fmt, h, w)
    top = {8: 255, 10: 1023, 16: 65535}[ref.depth(fmt)] << (6 if fmt == "p010le" else 0)
    zero = np.zeros(nb, np.uint8)
    full = (np.full(nb, top, np.uint8) if ref.depth(fmt) == 8 else np.full(nb // 2, top, "<u2").view(np.uint8))
    comb = full.copy()
    for off, ph, pw, st in ref.memory_planes(fmt, h, w):
        rows = ref.words(comb, fmt)[off:off + ph * pw * st].reshape(ph, pw * st)
        rows[0::2] = 0
    for trio in ((zero, zero, zero), (full, full, full), (comb, comb, comb), (zero, comb, full), (full, comb, zero), (comb, full, comb)):
        for order in ORDERS:
            want = ref.deinterlace(*trio, fmt, h, w, order)
            got = uva.deint_frames(*trio, fmt, h, w, "field", order)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_frames_in_hbm(uva):
    import torch
    fmt, h, w = "p010le", 70, 300
    fr = sequence(fmt, 3, h, w)
    d = [torch.from_numpy(f.copy()).cuda() for f in fr]
    oa, ob = torch.zeros_like(d[0]), torch.zeros_like(d[0])
    torch.cuda.synchronize()
    uva.deint_frames(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), fmt, h, w, "field", "bff", device=True, out_a=oa.data_ptr(),
                     out_b=ob.data_ptr())
    want = expected(fmt, 3, h, w, 1, "bff")
    assert np.array_equal(oa.cpu().numpy(), want[0]) and np.array_equal(ob.cpu().numpy(), want[1])
    # the ends of a stream, and output B alone
    ob.zero_()
    torch.cuda.synchronize()
    uva.deint_frames(None, d[1].data_ptr(), None, fmt, h, w, "field", "bff", device=True, out_b=ob.data_ptr())
    assert np.array_equal(ob.cpu().numpy(), ref.deinterlace(None, fr[1], None, fmt, h, w, "bff")[1])


# ---- the stateful handle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,mode", [("yuv420p", "field"), ("bgr24", "frame"), ("yuv420p10le", "field")])
def test_handle_against_the_stateless_calls(uva, fmt, mode):
    h, w, n = 37, 53, 5
    fr = sequence(fmt, n, h, w)
    per = 2 if mode == "field" else 1
    want = ref.deinterlace_sequence(fr, fmt, h, w, mode, "bff")
    outs = [np.empty(fr[0].size, np.uint8) for _ in range(2)]

    def run(di, frames):
        got, counts = [], []
        for f in frames:
            k = di.push(f, outs)
            counts.append(k)
            got += [o.copy() for o in outs[:k]]
        k = di.flush(outs)
        counts.append(k)
        got += [o.copy() for o in outs[:k]]
        return got, counts
    with uva.Deinterlacer(fmt, h, w, mode, "bff") as di:
        assert di.flush(outs) == 0                                   # nothing pushed: nothing to flush
        got, counts = run(di, fr)
        assert counts == [0] + [per] * n
        assert len(got) == len(want) and all(np.array_equal(g, x) for g, x in zip(got, want))
        for k in range(n):                                           # ... and frame for frame the stateless calls
            a, b = uva.deint_frames(*neighbours(fr, k), fmt, h, w, mode, "bff")
            assert np.array_equal(got[per * k], a) and (per == 1 or np.array_equal(got[per * k + 1], b))
        # a second stream after the flush equals a fresh handle's; reset in mid-stream forgets the frames pushed
        again, _ = run(di, fr[1:4])
        want2 = ref.deinterlace_sequence(fr[1:4], fmt, h, w, mode, "bff")
        assert all(np.array_equal(g, x) for g, x in zip(again, want2)) and len(again) == len(want2)
        assert di.push(fr[0], outs) == 0 and di.push(fr[4], outs) == per
        di.reset()
        third, counts = run(di, fr[1:4])
        assert counts == [0, per, per, per] and all(np.array_equal(g, x) for g, x in zip(third, want2))


# ---- the route ------------------------------------------------------------------------------------------------------------------
H, W, N = 64, 96, 6


@pytest.fixture(scope="module")
def films(tmp_path_factory):
    """six interlaced frames per format as files, and the reference's deinterlaced streams next to them"""
    d = tmp_path_factory.mktemp("deint")

    def film(fmt, mode="field", order="tff", n=N):
        src, want = d / ("%s.raw" % fmt), d / ("%s_%s_%s_%d.raw" % (fmt, mode, order, n))
        fr = sequence(fmt, N, H, W)
        if not src.exists():
            src.write_bytes(b"".join(f.tobytes() for f in fr))
        if not want.exists():
            want.write_bytes(b"".join(f.tobytes() for f in ref.deinterlace_sequence(fr[:n], fmt, H, W, mode, order)))
        return str(src), str(want)
    return d, film


def run_main(argv):
    assert rawvideo.main(argv) == 0


def read(path):
    with open(path, "rb") as f:
        return f.read()


SIZE = ["-W", str(W), "-H", str(H)]


def yuv(fmt="yuv420p"):
    return ["--in-pix-fmt", fmt, "--out-pix-fmt", fmt]


@pytest.mark.parametrize("extra", [[], ["--frames", "5"], ["--crop", "64:32:16:8"], ["--skip-repeats", "0"]],
                         ids=["plain", "frames5", "crop", "skip-repeats"])
def test_cli_field_mode_gives_the_bytes_of_a_run_on_deinterlaced_frames(uva, films, extra):
    d, film = films
    n_in = 5 if "--frames" in extra else N
    src, pre = film("yuv420p", n=n_in)
    out_a, out_b = str(d / "a.raw"), str(d / "b.raw")
    # the reference's frames through the same command without the option (--frames counts input frames: twice as many there)
    plain = [v if v != "5" else "10" for v in extra]
    run_main(["-i", pre, "-o", out_a, "-s", "2"] + SIZE + yuv() + plain)
    run_main(["-i", src, "-o", out_b, "-s", "2", "--deinterlace", "field"] + SIZE + yuv() + extra)
    want = read(out_a)
    oh, ow = (64, 128) if "--crop" in extra else (2 * H, 2 * W)
    assert len(want) == 2 * n_in * uva.pix_frame_bytes("yuv420p", oh, ow) and read(out_b) == want


def test_cli_segments_read_context_frames(uva, films, monkeypatch):
    """-g 0,0 file to file: two segments of three frames; the second reads frame 2 as leading context, the first frame 3 as
    trailing context, and the file is byte for byte the single lane's"""
    d, film = films
    monkeypatch.setenv("UVA_RAW_TMPFS_SEGMENTS", "1")        # (segments also where the output lies on tmpfs)
    out_a, out_b = str(d / "c.raw"), str(d / "e.raw")
    for mode in ("field", "frame"):
        src, pre = film("yuv420p", mode=mode, order="bff")
        run_main(["-i", pre, "-o", out_a, "-s", "2"] + SIZE + yuv())
        run_main(["-i", src, "-o", out_b, "-s", "2", "-g", "0,0", "--deinterlace", mode, "--field-order", "bff"] + SIZE + yuv())
        want = read(out_a)
        assert len(want) == (2 if mode == "field" else 1) * N * uva.pix_frame_bytes("yuv420p", 2 * H, 2 * W) and read(out_b) == want
    # five frames in two segments (2 + 3): the last segment flushes at frame 4, frame 5 is never read
    src, pre = film("yuv420p", n=5)
    run_main(["-i", pre, "-o", out_a, "-s", "2"] + SIZE + yuv())
    run_main(["-i", src, "-o", out_b, "-s", "2", "-g", "0,0", "--frames", "5", "--deinterlace", "field"] + SIZE + yuv())
    assert read(out_b) == read(out_a)


def test_cli_p010le_at_16_bits(uva, films):
    d, film = films
    src, pre = film("p010le")
    out_a, out_b = str(d / "f.raw"), str(d / "g.raw")
    args = ["-s", "2", "--bit-depth", "16"] + SIZE + yuv("p010le")
    run_main(["-i", pre, "-o", out_a] + args)
    run_main(["-i", src, "-o", out_b, "--deinterlace", "field"] + args)
    want = read(out_a)
    assert len(want) == 2 * N * uva.pix_frame_bytes("p010le", 2 * H, 2 * W) and read(out_b) == want


def test_cli_copy_through_is_a_deinterlace_only_run(uva, films):
    d, film = films
    out = str(d / "h.raw")
    for mode in ("field", "frame"):
        src, pre = film("bgr24", mode=mode)
        run_main(["-i", src, "-o", out, "-s", "1", "--deinterlace", mode] + SIZE)
        assert read(out) == read(pre)
    src, pre = film("bgr24", n=4)
    run_main(["-i", src, "-o", out, "-s", "1", "--deinterlace", "field", "--frames", "4"] + SIZE)
    assert read(out) == read(pre)


def test_pipe_form_with_two_lanes(uva, films):
    """stream() over in-memory streams, the frames dealt round-robin to two lanes"""
    d, film = films
    src, pre = film("yuv420p")
    pix = rawvideo.PixFormats("yuv420p", "yuv420p")
    nets = [[(load_net(uva, "2x"), 0)], [(load_net(uva, "2x"), 0)]]
    want, got = io.BytesIO(), io.BytesIO()
    assert rawvideo.stream(io.BytesIO(read(pre)), want, H, W, nets, pix=pix) == 2 * N
    assert rawvideo.stream(io.BytesIO(read(src)), got, H, W, nets, pix=pix, deint=rawvideo.DeintSpec("field")) == 2 * N
    assert got.getvalue() == want.getvalue() and len(want.getvalue()) == 2 * N * uva.pix_frame_bytes("yuv420p", 2 * H, 2 * W)
