"""Crop detection and cropped frames on the MI355X (-m gpu).  Everything is integer arithmetic and every
comparison is bit for bit: crop_sums_kernel against numpy, the detector end to end against tests/cropdetect_ref.py,
uva_pix_window against numpy slicing of every plane, a submit with an input window against a submit of the host-cropped frame,
and the command line file to file."""
import numpy as np
import pytest

import cropdetect_ref as ref
from conftest import load_net
from upscale_video_amd import rawvideo

pytestmark = pytest.mark.gpu

FORMATS = ["bgr24", "yuv420p", "nv12", "p010le", "yuv420p10le", "bgr48le", "yuv422p", "yuv422p10le"]


def random_frame(uva, fmt, h, w, rng, garbage=False):
    """raw bytes of one frame with legal code values; garbage: the bits the converter ignores are random instead of zero"""
    n = uva.pix_frame_bytes(fmt, h, w)
    if ref.DEPTH[fmt] == 8:
        return rng.integers(0, 256, n, dtype=np.uint8)
    words = rng.integers(0, 65536 if fmt == "bgr48le" else 1024, n // 2).astype("<u2")
    if fmt == "p010le":
        words = (words << 6).astype("<u2")
        if garbage:
            words |= rng.integers(0, 64, n // 2).astype("<u2")
    elif garbage and fmt != "bgr48le":
        words |= (rng.integers(0, 64, n // 2) << 10).astype("<u2")
    return words.view(np.uint8).copy()


# ---- the sums ---------------------------------------------------------------------------------------------------------------
# 37 x 53: less than one workgroup, odd; 70 x 300: a ragged 16-byte end in every row (300 % 16 = 12, and rows of 300 or 900 bytes
# start at every alignment); 130 x 1030: several tiles in both directions -- on a grid of 3 workgroups every workgroup walks
# several of them
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("h,w,max_groups", [(37, 53, None), (70, 300, None), (130, 1030, None), (130, 1030, 3), (130, 1030, 1)])
def test_sums_against_numpy(uva, fmt, h, w, max_groups):
    rng = np.random.default_rng(h * 1000 + w + len(fmt))
    frame = random_frame(uva, fmt, h, w, rng)
    want_r, want_c = ref.line_sums(frame, fmt, h, w)
    got_r, got_c = uva.crop_sums(frame, fmt, h, w, max_groups=max_groups)
    assert got_r.dtype == np.uint64 and np.array_equal(got_r, want_r), (fmt, h, w, "rows")
    assert np.array_equal(got_c, want_c), (fmt, h, w, "columns")
    if max_groups is None and (h, w) == (70, 300):
        # saturated samples: the sums of 16-bit words at their largest; and a black frame: all zero, not what the last call left
        top = np.full(frame.size, 255, np.uint8)
        r, c = uva.crop_sums(top, fmt, h, w)
        assert np.array_equal(r, ref.line_sums(top, fmt, h, w)[0]) and np.array_equal(c, ref.line_sums(top, fmt, h, w)[1])
        r, c = uva.crop_sums(np.zeros(frame.size, np.uint8), fmt, h, w)
        assert not r.any() and not c.any()


@pytest.mark.parametrize("fmt", ["p010le", "yuv420p10le", "yuv422p10le"])
def test_bits_the_converter_ignores_make_no_difference(uva, fmt):
    h, w = 70, 300
    clean = random_frame(uva, fmt, h, w, np.random.default_rng(3))
    dirty = random_frame(uva, fmt, h, w, np.random.default_rng(3), garbage=True)
    assert not np.array_equal(clean, dirty)
    a, b = uva.crop_sums(clean, fmt, h, w), uva.crop_sums(dirty, fmt, h, w)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], ref.line_sums(dirty, fmt, h, w)[0])


def test_sums_of_a_frame_in_hbm(uva):
    import torch
    h, w, fmt = 70, 300, "nv12"
    frame = random_frame(uva, fmt, h, w, np.random.default_rng(4))
    d = torch.from_numpy(frame.copy()).cuda()
    torch.cuda.synchronize()
    r, c = uva.crop_sums(d.data_ptr(), fmt, h, w, device=True)
    want = ref.line_sums(frame, fmt, h, w)
    assert np.array_equal(r, want[0]) and np.array_equal(c, want[1])


# ---- the detector, end to end ---------------------------------------------------------------------------------------------
def boxed_frame(uva, fmt, h, w, box, rng, spike=None):
    """a frame of fmt: a bright picture in rows box[0] ... box[1] - 1 and columns box[2] ... box[3] - 1, noise below the limit
    (24 of 255) around it, chroma of any value; spike (row, col): one saturated pixel there"""
    depth = ref.DEPTH[fmt]
    comps = 3 if fmt in ref.PACKED else 1
    scale = 1 << (depth - 8)
    y = rng.integers(0, 12 * scale, (h, w, comps))
    y[box[0]:box[1], box[2]:box[3]] = rng.integers(60 * scale, 236 * scale, (box[1] - box[0], box[3] - box[2], comps))
    if spike is not None:
        y[spike[0], spike[1]] = (1 << depth) - 1
    frame = random_frame(uva, fmt, h, w, rng, garbage=True)          # chroma planes, and garbage in the ignored bits
    if depth == 8:
        frame[:h * w * comps] = y.reshape(-1).astype(np.uint8)
    else:
        words = frame.view("<u2")
        keep = words[:h * w * comps] & (63 if fmt == "p010le" else (0xfc00 if depth == 10 else 0))
        words[:h * w * comps] = ((y.reshape(-1) << (6 if fmt == "p010le" else 0)).astype("<u2")) | keep
    return frame


@pytest.mark.parametrize("fmt", ["yuv420p", "nv12", "p010le", "bgr24", "bgr48le", "yuv422p10le"])
def test_detector_against_the_reference(uva, fmt):
    h, w = 96, 160
    rng = np.random.default_rng(11 + len(fmt))
    frames = [
        boxed_frame(uva, fmt, h, w, (16, 80, 0, 160), rng),                       # letterbox, noise below the limit in the bars
        boxed_frame(uva, fmt, h, w, (16, 80, 0, 160), rng, spike=(5, 77)),        # one saturated pixel in the upper bar
        boxed_frame(uva, fmt, h, w, (20, 70, 34, 120), rng),                      # bars on all four sides, inside the first
        boxed_frame(uva, fmt, h, w, (16, 80, 0, 160), rng, spike=(90, 3)),
    ]
    got, want = uva.CropDetector(h, w, fmt), ref.Detector(h, w, fmt)
    for f in frames:
        assert got.update(f) == want.update(f)
        assert got.rect() == want.rect()
    assert got.state == (0, 16, 159, 79) and got.rect() == (160, 64, 0, 16)
    # all four sides alone, and another limit and round
    four, four_ref = uva.CropDetector(h, w, fmt, limit=40, round=4), ref.Detector(h, w, fmt, limit=40, round=4)
    assert four.update(frames[2]) == four_ref.update(frames[2]) == (34, 20, 119, 69)
    assert four.rect() == four_ref.rect() == (84, 48, 36, 22)
    black = np.zeros(frames[0].size, np.uint8)
    assert four.update(black) == (34, 20, 119, 69)                                # no bright line: unchanged


# ---- the window outside a net ---------------------------------------------------------------------------------------------
def windows_of(fmt, sh, sw):
    """(x, y, h, w): windows at each edge and one in the middle, on the grid the format's chroma allows (an odd source's last
    column or row cannot be reached by an even window: those stop at the last boundary that can)"""
    ex = 1 if fmt in ref.PACKED else 2
    ey = 2 if fmt in ("yuv420p", "nv12", "p010le", "yuv420p10le") else 1
    right, bottom = sw - sw % ex, sh - sh % ey
    w, h = 40 - 40 % ex + (0 if fmt not in ref.PACKED else 1), 24 + (1 if ey == 1 else 0)
    return [(0, 0, h, w), (right - w, 0, h, w), (0, bottom - h, h, w), (right - w, bottom - h, h, w), (3 * ex + 16, 5 * ey + 8, h, w),
            (0, 4 * ey, h, right), (3 * ex, 0, bottom, w), (0, 0, bottom, right)]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("sh,sw", [(71, 131), (72, 132)])
def test_pix_window_against_numpy_slicing(uva, fmt, sh, sw):
    rng = np.random.default_rng(sh + len(fmt))
    frame = random_frame(uva, fmt, sh, sw, rng, garbage=True)
    for x, y, h, w in windows_of(fmt, sh, sw):
        got = uva.pix_window(frame, fmt, sh, sw, x, y, h, w)
        want = ref.window(frame, fmt, sh, sw, x, y, h, w)
        assert got.nbytes == uva.pix_frame_bytes(fmt, h, w) == want.size, (fmt, x, y, h, w)
        assert np.array_equal(np.ascontiguousarray(got).reshape(-1).view(np.uint8), want), (fmt, x, y, h, w)


def test_pix_window_of_a_frame_in_hbm(uva):
    import ctypes

    import torch
    from upscale_video_amd import _lib
    fmt, sh, sw, (x, y, h, w) = "yuv420p10le", 72, 132, (34, 10, 40, 60)
    frame = random_frame(uva, fmt, sh, sw, np.random.default_rng(8))
    d_in = torch.from_numpy(frame.copy()).cuda()
    d_out = torch.zeros(uva.pix_frame_bytes(fmt, h, w), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.load().uva_pix_window_device(0, ctypes.c_void_p(d_in.data_ptr()), uva.PIX_FORMATS_ALL[fmt], sh, sw, x, y, h, w,
                                                 ctypes.c_void_p(d_out.data_ptr())))
    assert np.array_equal(d_out.cpu().numpy(), ref.window(frame, fmt, sh, sw, x, y, h, w))


# ---- the window in front of a net -------------------------------------------------------------------------------------------
SH, SW = 96, 160
LETTERBOX, PILLARBOX = (160, 64, 0, 16), (96, 96, 32, 0)        # W:H:X:Y


@pytest.fixture(scope="module")
def net2x(uva):
    return load_net(uva, "2x")


def route_kw(route):
    return {"yuv420p": dict(in_fmt="yuv420p", out_fmt="yuv420p"), "p010le": dict(in_fmt="p010le", out_fmt="p010le", bit_depth=16)}[route]


def submit_all(net, frames, h, w, kw, pinned_in=None):
    """every frame through submit_pix / collect_u8, three in flight -> the results' bytes"""
    out, tickets = [], []
    for i, f in enumerate(frames):
        if pinned_in is not None:
            buf = pinned_in[i % len(pinned_in)]
            buf[:] = f
            f = buf
        tickets.append(net.submit_pix(f, h, w, **kw))
        if len(tickets) == 3:
            out.append(net.collect_u8(tickets.pop(0)).tobytes())
    while tickets:
        out.append(net.collect_u8(tickets.pop(0)).tobytes())
    return out


@pytest.mark.parametrize("route", ["yuv420p", "p010le"])
@pytest.mark.parametrize("crop", [LETTERBOX, PILLARBOX])
@pytest.mark.parametrize("pinned", [False, True])
def test_a_windowed_submit_equals_a_submit_of_the_cropped_frame(uva, net2x, route, crop, pinned):
    kw = route_kw(route)
    fmt = kw["in_fmt"]
    cw, ch, x, y = crop
    rng = np.random.default_rng(21)
    distinct = [random_frame(uva, fmt, SH, SW, rng) for _ in range(3)]
    frames = [distinct[i] for i in (0, 0, 1, 1, 1, 2, 0)]                          # a stream that repeats frames
    cut = [ref.window(f, fmt, SH, SW, x, y, ch, cw) for f in frames]
    net = net2x
    net.set_input_window()
    net.set_skip_repeats(None)
    want = submit_all(net, cut, ch, cw, kw)
    assert len(want[0]) == uva.pix_frame_bytes(fmt, 2 * ch, 2 * cw)
    sized = dict(kw, out_size=(2 * ch - 10, 2 * cw + 6), resize_filter="bicubic")
    want_sized = submit_all(net, cut[:3], ch, cw, sized)
    net.set_skip_repeats(0)
    assert submit_all(net, cut, ch, cw, kw) == want
    want_stats = net.skip_stats()
    assert want_stats == (7, 3)
    net.set_skip_repeats(None)
    # the same calls with the window set and the frames as they come off the input
    ring = [uva.pinned_empty((uva.pix_frame_bytes(fmt, SH, SW),)) for _ in range(4)] if pinned else None
    net.set_input_window(SH, SW, x, y)
    try:
        assert submit_all(net, frames, ch, cw, kw, ring) == want
        assert submit_all(net, frames[:3], ch, cw, sized, ring) == want_sized
        net.set_skip_repeats(0)
        assert submit_all(net, frames, ch, cw, kw, ring) == want
        assert net.skip_stats() == want_stats
        # a window the format's chroma grid does not allow is refused by the submit call, never rounded
        from upscale_video_amd._lib import UvaError
        with pytest.raises(UvaError, match="input window"):
            net.submit_pix(frames[0], ch - 1, cw, **kw)
    finally:
        net.set_skip_repeats(None)
        net.set_input_window()


@pytest.mark.parametrize("route", ["yuv420p", "p010le"])
def test_a_whole_frame_window_gives_the_bytes_with_no_window(uva, net2x, route):
    kw = route_kw(route)
    frames = [random_frame(uva, kw["in_fmt"], SH, SW, np.random.default_rng(22))]
    net2x.set_input_window()
    want = submit_all(net2x, frames, SH, SW, kw)
    net2x.set_input_window(SH, SW, 0, 0)
    try:
        assert submit_all(net2x, frames, SH, SW, kw) == want
    finally:
        net2x.set_input_window()
    assert submit_all(net2x, frames, SH, SW, kw) == want


def test_a_bgr24_window_takes_any_offset(uva, net2x):
    """the net's own layout: the window is uploaded with the source's row stride, odd offsets and sizes included"""
    frame = random_frame(uva, "bgr24", SH, SW, np.random.default_rng(23))
    x, y, h, w = 33, 7, 51, 77
    net2x.set_input_window()
    want = submit_all(net2x, [ref.window(frame, "bgr24", SH, SW, x, y, h, w)], h, w, dict(in_fmt="bgr24"))
    net2x.set_input_window(SH, SW, x, y)
    try:
        assert submit_all(net2x, [frame], h, w, dict(in_fmt="bgr24")) == want
    finally:
        net2x.set_input_window()


# ---- the command line, file to file ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def letterboxed(tmp_path_factory):
    """130 yuv420p frames of 96 x 160 with the picture in rows 16 ... 79 (two frames all black, one with a bright subtitle in the
    bar), and the same stream cropped on the host"""
    d = tmp_path_factory.mktemp("crop")
    frames = ref.letterboxed_stream(SH, SW, 130)
    src, cut = d / "in.yuv", d / "cut.yuv"
    src.write_bytes(frames.tobytes())
    cut.write_bytes(b"".join(ref.window(f, "yuv420p", SH, SW, 0, 16, 64, 160).tobytes() for f in frames))
    return d, str(src), str(cut)


def run_main(argv):
    assert rawvideo.main(argv) == 0


YUV = ["--in-pix-fmt", "yuv420p", "--out-pix-fmt", "yuv420p"]


def test_cli_crop_gives_the_bytes_of_a_run_on_a_cropped_file(uva, letterboxed, capsys):
    d, src, cut = letterboxed
    out_a, out_b = str(d / "a.yuv"), str(d / "b.yuv")
    run_main(["-i", cut, "-o", out_a, "-W", "160", "-H", "64", "-s", "2", "--frames", "12"] + YUV)
    run_main(["-i", src, "-o", out_b, "-W", "160", "-H", "96", "-s", "2", "--frames", "12", "--crop", "160:64:0:16"] + YUV)
    want = open(out_a, "rb").read()
    assert len(want) == 12 * uva.pix_frame_bytes("yuv420p", 128, 320) and open(out_b, "rb").read() == want
    # --out-scale works from the cropped size: 1.5 x (64, 160) -> 96 x 240
    run_main(["-i", cut, "-o", out_a, "-W", "160", "-H", "64", "-s", "2", "--frames", "3", "--out-scale", "1.5"] + YUV)
    run_main(["-i", src, "-o", out_b, "-W", "160", "-H", "96", "-s", "2", "--frames", "3", "--out-scale", "1.5", "--crop", "crop=160:64:0:16"] + YUV)
    want = open(out_a, "rb").read()
    assert len(want) == 3 * uva.pix_frame_bytes("yuv420p", 96, 240) and open(out_b, "rb").read() == want


def test_cli_crop_auto_and_cropdetect_find_the_letterbox(uva, letterboxed, capsys):
    d, src, cut = letterboxed
    out_a, out_b = str(d / "c.yuv"), str(d / "d.yuv")
    capsys.readouterr()
    run_main(["-i", src, "-W", "160", "-H", "96", "--cropdetect"] + YUV)
    cap = capsys.readouterr()
    assert cap.out == "crop=160:64:0:16\n"
    with open(src, "rb") as f:                                  # the same through a pipe-like stream is main's other branch: the function
        assert rawvideo.detect_crop_pipe(f, SH, SW, "yuv420p", stride=10) == (160, 64, 0, 16)
    run_main(["-i", cut, "-o", out_a, "-W", "160", "-H", "64", "-s", "2"] + YUV)
    run_main(["-i", src, "-o", out_b, "-W", "160", "-H", "96", "-s", "2", "--crop", "auto"] + YUV)
    assert "crop=160:64:0:16" in capsys.readouterr().err
    want = open(out_a, "rb").read()
    assert len(want) == 130 * uva.pix_frame_bytes("yuv420p", 128, 320) and open(out_b, "rb").read() == want


@pytest.mark.parametrize("lane", [["-s", "1", "-m", "n=3"], ["-s", "1"], ["-s", "1", "--out-pix-fmt", "nv12"]])
def test_cli_lanes_without_a_net_in_front_honour_the_crop(uva, letterboxed, lane):
    d, src, cut = letterboxed
    out_a, out_b = str(d / "e.yuv"), str(d / "f.yuv")
    base = ["--frames", "4"] + YUV + lane              # (a later --out-pix-fmt wins)
    run_main(["-i", cut, "-o", out_a, "-W", "160", "-H", "64"] + base)
    run_main(["-i", src, "-o", out_b, "-W", "160", "-H", "96", "--crop", "160:64:0:16"] + base)
    want = open(out_a, "rb").read()
    assert len(want) == 4 * uva.pix_frame_bytes("yuv420p", 64, 160) and open(out_b, "rb").read() == want
    if lane == ["-s", "1"]:
        assert want == open(cut, "rb").read()[:len(want)]
