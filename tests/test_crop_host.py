"""CPU tests of the crop detector's host half and of the route's crop options: uva_crop_bounds and
uva_crop_rect against tests/cropdetect_ref.py on constructed line sums, the window validator's refusals, the host-only setter,
the sample positions of --crop auto and the option parsing.  No GPU: nothing here computes a sum."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import cropdetect_ref as ref
from conftest import ROOT, load_net

# one format per (depth, samples per pixel of a line): 8 / 10 / 16 bits, and the packed formats' n = 3w
FMTS = ["yuv420p", "p010le", "yuv420p10le", "bgr48le", "bgr24"]


def comps(fmt):
    return 3 if fmt in ref.PACKED else 1


def sums_of_means(fmt, h, w, row_means, col_means):
    """line sums of a frame whose rows / columns have exactly these mean code values"""
    return (np.array([m * w * comps(fmt) for m in row_means], np.uint64), np.array([m * h * comps(fmt) for m in col_means], np.uint64))


@pytest.mark.parametrize("fmt", FMTS)
def test_a_line_at_the_limit_is_dark_and_one_above_is_bright(uva, fmt):
    h, w, limit = 12, 20, 24
    L = limit << (ref.DEPTH[fmt] - 8)
    rows, cols = sums_of_means(fmt, h, w, [L] * h, [L] * w)
    assert uva.crop_bounds(rows, cols, fmt, h, w, limit) == ref.bounds(rows, cols, fmt, h, w, limit) == (-1, -1, -1, -1)
    # one sample short of mean L + 1 is still floor(S / n) == L: dark; mean exactly L + 1: bright
    rows[5] = (L + 1) * w * comps(fmt) - 1
    cols[7] = (L + 1) * h * comps(fmt) - 1
    assert uva.crop_bounds(rows, cols, fmt, h, w, limit) == (-1, -1, -1, -1)
    rows[5] += 1
    rows[9] = (L + 1) * w * comps(fmt)
    cols[7] += 1
    got = uva.crop_bounds(rows, cols, fmt, h, w, limit)
    assert got == ref.bounds(rows, cols, fmt, h, w, limit) == (5, 9, 7, 7)


@pytest.mark.parametrize("fmt", FMTS)
def test_an_all_dark_frame_leaves_the_state_and_gives_no_rectangle(uva, fmt):
    h, w = 70, 300
    det = uva.CropDetector(h, w, fmt)
    assert det.state == ref.initial(h, w) == (w - 1, h - 1, 0, 0)
    rows, cols = sums_of_means(fmt, h, w, [3] * h, [3] * w)
    assert det.update_sums(rows, cols) == ref.initial(h, w)
    assert det.rect() is None and ref.rect(det.state) is None


@pytest.mark.parametrize("fmt", FMTS)
def test_an_all_bright_70x300_frame_gives_288_64_6_4(uva, fmt):
    """By hand: the state becomes (0, 0, 299, 69).  x = (0 + 1) & ~1 = 0, cw = 299 - 0 + 1 = 300, k = 300 % 16 = 12, cw = 288,
    x += (12 / 2 + 1) & ~1 = 6.  y = 0, ch = 70, k = 70 % 16 = 6, ch = 64, y += (6 / 2 + 1) & ~1 = 4.  crop=288:64:6:4."""
    h, w = 70, 300
    top = (1 << ref.DEPTH[fmt]) - 1
    rows, cols = sums_of_means(fmt, h, w, [top] * h, [top] * w)
    det = uva.CropDetector(h, w, fmt)
    assert det.update_sums(rows, cols) == (0, 0, 299, 69)
    assert det.rect() == ref.rect((0, 0, 299, 69)) == (288, 64, 6, 4)


def test_the_state_over_three_frames_only_grows(uva):
    h, w, fmt = 40, 64, "yuv420p"
    det, state = uva.CropDetector(h, w, fmt), ref.initial(h, w)
    frames = [((10, 29), (8, 55)), ((12, 20), (20, 30)), ((6, 25), (16, 60))]       # bright rows, bright columns of each frame
    want = [(8, 10, 55, 29), (8, 10, 55, 29), (8, 6, 60, 29)]
    for ((r0, r1), (c0, c1)), expect in zip(frames, want):
        rows, cols = sums_of_means(fmt, h, w, [200 if r0 <= r <= r1 else 0 for r in range(h)], [200 if c0 <= c <= c1 else 0 for c in range(w)])
        prev = det.state
        state = ref.update(state, ref.bounds(rows, cols, fmt, h, w))
        got = det.update_sums(rows, cols)
        assert got == state == expect
        assert got[0] <= prev[0] and got[1] <= prev[1] and got[2] >= prev[2] and got[3] >= prev[3]
    assert det.rect() == ref.rect(state)


def test_round_0_1_and_15_mean_16_16_and_30(uva):
    assert [ref.effective_round(r) for r in (0, 1, 15, 16, 2)] == [16, 16, 30, 16, 2]
    state = (0, 0, 299, 69)
    assert uva.crop_rect(state, 0) == uva.crop_rect(state, 1) == uva.crop_rect(state, 16) == (288, 64, 6, 4)
    # R = 30: cw 300 % 30 = 0 -> 300 at x 0; ch 70 % 30 = 10 -> 60, y += (5 + 1) & ~1 = 6
    assert uva.crop_rect(state, 15) == uva.crop_rect(state, 30) == ref.rect(state, 15) == (300, 60, 0, 6)
    for r in (0, 1, 2, 7, 15, 16, 32, 33):
        assert uva.crop_rect(state, r) == ref.rect(state, r), r


def test_every_rectangle_is_even_inside_the_frame_and_a_valid_window(uva):
    """1 000 seeded random states and sizes: whatever uva_crop_rect produces has even W, H, X, Y, lies inside the frame and is a
    window the validator takes for the strictest formats (4:2:0), hence for all of them."""
    rng = np.random.default_rng(20260101)
    made = 0
    for _ in range(1000):
        h, w = int(rng.integers(1, 2200)), int(rng.integers(1, 4100))
        x1, x2 = (int(v) for v in rng.integers(0, w, 2))
        y1, y2 = (int(v) for v in rng.integers(0, h, 2))
        rnd = int(rng.choice([0, 1, 2, 3, 4, 8, 15, 16, 32, 33]))
        got = uva.crop_rect((x1, y1, x2, y2), rnd)
        assert got == ref.rect((x1, y1, x2, y2), rnd)
        if got is None:
            continue
        made += 1
        cw, ch, x, y = got
        assert cw > 0 and ch > 0 and not (cw | ch | x | y) & 1, got
        assert 0 <= x and x + cw <= w and 0 <= y and y + ch <= h, (got, h, w)
        for fmt in ("yuv420p", "nv12", "p010le", "yuv422p10le", "bgr24"):
            uva.pix_window_check(fmt, h, w, x, y, ch, cw)               # raises if refused
    assert made > 200


def test_the_window_validator_refuses_with_its_reason(uva):
    from upscale_video_amd._lib import UvaError
    uva.pix_window_check("yuv420p", 96, 160, 0, 16, 64, 160)
    uva.pix_window_check("bgr24", 71, 131, 3, 5, 7, 11)                 # packed BGR: any window
    uva.pix_window_check("bgr48le", 71, 131, 130, 70, 1, 1)
    uva.pix_window_check("yuv422p", 71, 130, 2, 5, 7, 10)               # 4:2:2: odd rows are fine
    for args in (("yuv420p", 96, 160, 0, 40, 64, 160), ("bgr24", 96, 160, 100, 0, 96, 61), ("nv12", 96, 160, -2, 0, 96, 160)):
        with pytest.raises(UvaError, match="the window leaves the frame"):
            uva.pix_window_check(*args)
    for args in (("yuv420p", 96, 160, 1, 0, 96, 100), ("yuv422p10le", 96, 160, 0, 0, 96, 99), ("p010le", 96, 160, 3, 0, 96, 11)):
        with pytest.raises(UvaError, match="x and the width must be even for a Y'CbCr format"):
            uva.pix_window_check(*args)
    for args in (("yuv420p", 96, 160, 0, 1, 64, 160), ("nv12", 96, 160, 0, 0, 63, 160), ("yuv420p10le", 96, 160, 0, 3, 5, 160)):
        with pytest.raises(UvaError, match="y and the height must be even for a 4:2:0 format"):
            uva.pix_window_check(*args)
    with pytest.raises(UvaError, match="bad image size"):
        uva.pix_window_check("bgr24", 96, 160, 0, 0, 0, 160)
    # the entries that would use the GPU refuse before they look for one
    buf, out = np.zeros(96 * 160 * 3 // 2, np.uint8), np.zeros(64 * 160 * 3 // 2, np.uint8)
    with pytest.raises(UvaError, match="the window leaves the frame"):
        uva.pix_window(buf, "yuv420p", 96, 160, 0, 40, 64, 160, out=out)


def test_refusals_of_the_detector_entries(uva):
    from upscale_video_amd import _lib
    L = _lib.load()
    rows, cols, b = np.zeros(4, np.uint64), np.zeros(6, np.uint64), np.zeros(4, np.int32)
    bp = b.ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_int))
    for limit in (-1, 256):
        assert L.uva_crop_bounds(rows.ctypes.data, cols.ctypes.data, 1, 4, 6, limit, bp) != 0
        assert b"limit is 0 ... 255" in L.uva_last_error()
    assert L.uva_crop_bounds(None, cols.ctypes.data, 1, 4, 6, 24, bp) != 0 and b"null" in L.uva_last_error()
    assert L.uva_crop_bounds(rows.ctypes.data, cols.ctypes.data, 4, 4, 6, 24, bp) != 0 and b"unknown pixel format" in L.uva_last_error()
    assert L.uva_crop_bounds(rows.ctypes.data, cols.ctypes.data, 1, 0, 6, 24, bp) != 0 and b"bad image size" in L.uva_last_error()
    assert L.uva_crop_rect(None, 16, bp) != 0 and b"null" in L.uva_last_error()
    frame = np.zeros(64, np.uint8)
    assert L.uva_crop_sums(0, None, 1, 4, 6, rows.ctypes.data, cols.ctypes.data) != 0 and b"null" in L.uva_last_error()
    assert L.uva_crop_sums(0, frame.ctypes.data, 4, 4, 6, rows.ctypes.data, cols.ctypes.data) != 0 and b"unknown pixel format" in L.uva_last_error()
    assert L.uva_crop_sums(0, frame.ctypes.data, 1, 4, 0, rows.ctypes.data, cols.ctypes.data) != 0 and b"bad image size" in L.uva_last_error()
    assert L.uva_crop_sums_device(0, None, 1, 4, 6, rows.ctypes.data, cols.ctypes.data) != 0 and b"null" in L.uva_last_error()
    assert L.uva_abi_version() == 15


def test_set_input_window_is_host_only(uva):
    """works with no GPU present: the setter touches no device"""
    from upscale_video_amd._lib import UvaError
    net = load_net(uva, "2x")
    net.set_input_window(96, 160, 0, 16)
    assert net._window == (96, 160, 0, 16)
    net.set_skip_repeats(0)
    net.set_input_window(96, 160, 32, 0)
    assert net.skip_stats() == (0, 0)
    net.set_input_window()                    # zeros: off
    assert net._window is None
    for bad in ((0, 160, 0, 0), (96, 160, 160, 0), (96, 160, 0, -1), (-96, 160, 0, 0)):
        with pytest.raises(UvaError, match="input window|uva_net_set_input_window"):
            net.set_input_window(*bad)


@pytest.mark.parametrize("n", [1, 2, 119, 120, 241, 200000])
def test_crop_sample_positions_follow_the_reference_s_recipe(n):
    """get_crop_detect (upscale/upscale_processing.py:144-152) seeks to (i + 1) * int(duration / 120) for i = 10 ... 109 and
    looks at two frames; in frames: min((i + 1) * (N // 120), N - 2), clamped at 0 for a file of one frame, duplicates dropped."""
    from upscale_video_amd.rawvideo import crop_sample_positions
    want = []
    for i in range(10, 110):
        p = max(0, min((i + 1) * (n // 120), n - 2))
        if p not in want:
            want.append(p)
    got = crop_sample_positions(n)
    assert got == want and len(set(got)) == len(got)
    assert all(0 <= p <= max(0, n - 2) for p in got)
    assert got == {1: [0], 2: [0], 119: [0]}.get(n, got)
    if n == 120:
        assert got == list(range(11, 111))
    if n == 241:
        assert got == list(range(22, 222, 2))
    if n == 200000:
        assert got[0] == 11 * 1666 and got[-1] == 110 * 1666 and len(got) == 100


def test_crop_option_parsing():
    from upscale_video_amd.rawvideo import PixFormats, parse_crop
    assert parse_crop("160:64:0:16") == parse_crop("crop=160:64:0:16") == parse_crop(" 160:64:0:16\n") == (160, 64, 0, 16)
    for bad in ("160x64", "160:64:0", "a:b:c:d", "160:64:0:-16", "0:64:0:0", ""):
        with pytest.raises(ValueError, match="--crop"):
            parse_crop(bad)
    pix = PixFormats("yuv420p", "yuv420p", crop=(160, 64, 0, 16))
    assert pix.net_size(96, 160) == (64, 160) and pix.window(96, 160) == (96, 160, 0, 16)
    assert PixFormats().net_size(96, 160) == (96, 160) and PixFormats().window(96, 160) is None
    with pytest.raises(ValueError):
        PixFormats(crop=(160, 64, 0))


def test_votes_most_frequent_then_larger_area_then_first_seen():
    from upscale_video_amd.rawvideo import CropVotes
    v = CropVotes()
    for r in [(160, 64, 0, 16), (160, 96, 0, 0), (160, 64, 0, 16), None, (160, 96, 0, 0), (144, 64, 8, 16)]:
        v.add(r)
    assert v.winner() == (160, 96, 0, 0)                      # 2 : 2 votes, the larger area
    v.add((160, 64, 0, 16))
    assert v.winner() == (160, 64, 0, 16)
    t = CropVotes()
    t.add((64, 32, 0, 0))
    t.add((32, 64, 2, 2))
    assert t.winner() == (64, 32, 0, 0)                       # equal votes and area: the first seen
    assert CropVotes().winner() is None


def test_detection_on_a_file_and_a_pipe_with_the_reference_detector(tmp_path):
    """the route's sampling and voting with tests/cropdetect_ref.py's Detector in place of the GPU's: a 130-frame letterboxed
    yuv420p file, two of its frames all black and one with a bright subtitle in the bar"""
    from upscale_video_amd.rawvideo import detect_crop_file, detect_crop_pipe
    h, w, n = 96, 160, 130
    frames = ref.letterboxed_stream(h, w, n)
    path = tmp_path / "in.yuv"
    path.write_bytes(frames.tobytes())
    assert detect_crop_file(str(path), h, w, "yuv420p", detector=ref.Detector) == (160, 64, 0, 16)
    assert detect_crop_pipe(io.BytesIO(frames.tobytes()), h, w, "yuv420p", stride=10, detector=ref.Detector) == (160, 64, 0, 16)
    black = np.zeros((3, h * w * 3 // 2), np.uint8)
    assert detect_crop_pipe(io.BytesIO(black.tobytes()), h, w, "yuv420p", stride=2, detector=ref.Detector) is None


def run_cli(*args, stdin=None):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "upscale_video_amd.rawvideo"] + list(args), input=stdin, capture_output=True, env=env,
                          cwd=ROOT, timeout=300)


def test_crop_auto_is_refused_on_a_pipe_and_bad_windows_at_the_command_line(uva):
    r = run_cli("-W", "160", "-H", "96", "-s", "1", "--in-pix-fmt", "yuv420p", "--out-pix-fmt", "yuv420p", "--crop", "auto", stdin=b"")
    assert r.returncode != 0 and b"--cropdetect" in r.stderr and b"regular file" in r.stderr
    r = run_cli("-W", "160", "-H", "96", "-s", "1", "--in-pix-fmt", "yuv420p", "--out-pix-fmt", "yuv420p", "--crop", "160:64:0:15", stdin=b"")
    assert r.returncode != 0 and b"even for a 4:2:0 format" in r.stderr
    r = run_cli("-W", "160", "-H", "96", "-s", "1", "--crop", "160:64:0:40", stdin=b"")
    assert r.returncode != 0 and b"the window leaves the frame" in r.stderr
    r = run_cli("-W", "160", "-H", "96", "-s", "1", "--crop", "160x64", stdin=b"")
    assert r.returncode != 0 and b"W:H:X:Y" in r.stderr
