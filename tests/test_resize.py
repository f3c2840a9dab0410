"""The resampler on the CPU: the library's tap tables against float64, the numpy restatement
(tests/resize_ref.py) against float64 with the same taps and with the ideal weights, what anti-aliasing buys on a zone plate, and
the raw-video route's --out-size / --out-scale / --resize-filter with a stand-in net that applies the restatement."""
import io
import math
import os

import numpy as np
import pytest

import pixfmt16_ref
import pixfmt_ref
import resize_ref as ref
from upscale_video_amd import _lib, ncnn, rawvideo

AXES = [(1, 1), (1, 3), (3, 1), (5, 7), (7, 4), (100, 25), (100, 400), (1000, 999), (2160, 1440), (3840, 2560), (1080, 1620)]
# u16 against float64 with the ideal weights: the measured maximum over test_restatement_against_float64's inputs (two-level
# content, 14-bit taps) and the bar = measured + 1 code; the issue caps the bar at 16 codes
U16_IDEAL_MEASURED = 7.9      # 7.891: lanczos, two-level content
U16_IDEAL_BAR = U16_IDEAL_MEASURED + 1.0
assert U16_IDEAL_BAR <= 16.0


# ---- the table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.FILTERS)
@pytest.mark.parametrize("n_in,n_out", AXES)
def test_table_against_float64(n_in, n_out, name):
    first, taps = ncnn.resize_taps(n_in, n_out, name)
    a = ref.SUPPORT[name]
    r = n_in / n_out
    t = 2 * math.ceil(a * max(1.0, r))
    assert taps.shape == (n_out, t) and taps.dtype == np.int16 and first.shape == (n_out,)
    assert t == ref.ntaps(n_in, n_out, name) and t <= 24
    assert (taps.astype(np.int64).sum(axis=1) == ref.ONE).all()
    want_first, w = ref.ideal_weights(n_in, n_out, name)
    assert np.array_equal(first, want_first)             # floor(c - a fs) + 1
    assert np.abs(taps - w * ref.ONE).max() <= 1.0
    assert np.abs(taps.astype(np.int64)).sum(axis=1).max() <= 32767        # pass 1's int32 sums rely on it
    if n_in == n_out:
        assert ((taps != 0).sum(axis=1) == 1).all() and taps.max() == ref.ONE
        assert np.array_equal(first + np.argmax(taps, axis=1), np.arange(n_out))
    # mirrored geometry -> mirrored table: row d over the source samples is row n_out-1-d reversed.  Compared as dense rows
    # (taps scattered over the clamped samples), within a unit: `first` is defined by a floor, so a row whose window starts
    # exactly on a sample is not the mirror image of its twin's window but that window shifted by one zero tap, and the largest-
    # remainder rule breaks ties towards the lower index on both sides
    dense = np.zeros((n_out, n_in), np.int64)
    idx = np.clip(first[:, None].astype(np.int64) + np.arange(t)[None, :], 0, n_in - 1)
    for k in range(t):
        np.add.at(dense, (np.arange(n_out), idx[:, k]), taps[:, k].astype(np.int64))
    assert np.abs(dense - dense[::-1, ::-1]).max() <= 1


def test_table_equals_own_rule_almost_everywhere():
    """the library's table is the restated rule (floor + largest remainders) applied to the C library's float64 weights: where
    numpy's `sin` agrees to the last bit the two are equal, and they never differ by more than a unit"""
    for name in ref.FILTERS:
        for n_in, n_out in AXES:
            first, taps = ncnn.resize_taps(n_in, n_out, name)
            fo, w = ref.ideal_weights(n_in, n_out, name)
            own = ref.int_taps(w)
            assert np.abs(own - taps).max() <= 1
            assert (own != taps).any(axis=1).mean() <= 0.02, (name, n_in, n_out)


def test_table_refusals():
    for n_in, n_out in ((0, 1), (1, 0), (100, 24), (24, 100), (-3, 5)):
        with pytest.raises(ValueError):
            ncnn.resize_taps(n_in, n_out, "lanczos")
    with pytest.raises(ValueError, match="filter"):
        ncnn.resize_taps(10, 10, "mitchell")
    L = _lib.load()
    import ctypes
    t = ctypes.c_int(0)
    assert L.uva_resize_taps(100, 24, 0, None, None, 0, ctypes.byref(t)) != 0 and b"[1/4, 4]" in L.uva_last_error()
    assert L.uva_resize_taps(10, 10, 3, None, None, 0, ctypes.byref(t)) != 0 and b"filter" in L.uva_last_error()
    assert L.uva_resize_taps(10, 0, 0, None, None, 0, ctypes.byref(t)) != 0 and b"at least 1" in L.uva_last_error()
    # both limits are inside
    assert ncnn.resize_taps(100, 25, "lanczos")[1].shape == (25, 24) and ncnn.resize_taps(25, 100, "lanczos")[1].shape == (100, 6)
    assert ncnn.RESIZE_FILTERS == {"lanczos": 0, "bicubic": 1, "bilinear": 2}


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _frames(h, w, dtype, seed):
    rng = np.random.default_rng(seed)
    mx = np.iinfo(dtype).max
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([(0.5 + 0.5 * np.sin(yy / 7.0 + c) * np.cos(xx / 5.0 - c)) * mx for c in range(3)], axis=2)
    return {"random": rng.integers(0, mx + 1, (h, w, 3)).astype(dtype),
            "two-level": (rng.integers(0, 2, (h, w, 3)) * mx).astype(dtype),
            "smooth": np.rint(smooth).astype(dtype)}


GEOMETRIES = [((48, 64), (31, 40)),      # shrink
              ((23, 31), (40, 57)),      # enlarge
              ((40, 30), (25, 47)),      # mixed: rows shrink, columns grow
              ((30, 40), (47, 25)),      # mixed the other way
              ((64, 48), (16, 12)),      # ratio limit 1/4
              ((9, 11), (36, 44))]       # ratio limit 4


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("name", ref.FILTERS)
def test_restatement_against_float64(dtype, name, record_property):
    mx = np.iinfo(dtype).max
    worst_same = worst_ideal = 0.0
    for (h, w), (oh, ow) in GEOMETRIES:
        tables = ref.library_tables(h, w, oh, ow, name)
        ideal = ref.ideal_tables(h, w, oh, ow, name)
        for kind, img in _frames(h, w, dtype, seed=h * 1000 + ow).items():
            got = ref.resize(img, (oh, ow), tables).astype(np.float64)             # (asserts every partial sum's range)
            same = np.clip(ref.resize_float(img, (oh, ow), tables), 0, mx)
            exact = np.clip(ref.resize_float(img, (oh, ow), ideal), 0, mx)
            worst_same = max(worst_same, np.abs(got - same).max())
            worst_ideal = max(worst_ideal, np.abs(got - exact).max())
            # flipping the frame flips the result, within a code (the tables are mirror images within a unit)
            flipped = ref.resize(img[::-1, ::-1], (oh, ow), tables)[::-1, ::-1]
            assert np.abs(flipped.astype(np.int64) - got.astype(np.int64)).max() <= 1, (kind, h, w, oh, ow)
    print("resize %s %s: max |restatement - float64|: same taps %.3f, ideal weights %.3f codes" % (np.dtype(dtype).name, name, worst_same, worst_ideal))
    record_property("same_taps", worst_same)
    record_property("ideal_weights", worst_ideal)
    # the passes' own rounding: the final round-to-nearest (0.5) + what pass 1 drops -- u8: |error| <= 0.5 of its 2^-7 units per
    # sample, times sum|taps_x| / 2^14 <= 2 -> 2^-7 codes; u16: nothing -- so below 0.51 codes; the bar is the issue's 1 code
    assert worst_same <= 1.0
    assert worst_ideal <= (1.0 if dtype == np.uint8 else U16_IDEAL_BAR)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("name", ref.FILTERS)
def test_flat_and_identity_exact(dtype, name):
    mx = np.iinfo(dtype).max
    rng = np.random.default_rng(3)
    for (h, w), (oh, ow) in GEOMETRIES:
        tables = ref.library_tables(h, w, oh, ow, name)
        for v in (0, 1, mx // 2, mx - 1, mx):
            flat = np.full((h, w, 3), v, dtype)
            flat[..., 1] = mx - v
            out = ref.resize(flat, (oh, ow), tables)
            assert (out[..., 0] == v).all() and (out[..., 1] == mx - v).all()
    img = rng.integers(0, mx + 1, (13, 17, 3)).astype(dtype)
    assert np.array_equal(ref.resize(img, (13, 17), ref.library_tables(13, 17, 13, 17, name)), img)
    # one axis kept: that axis passes through (its table is one tap of 2^14)
    one = ref.resize(img, (13, 30), ref.library_tables(13, 17, 13, 30, name))
    assert one.shape == (13, 30, 3)
    rows = ref.resize(img, (30, 17), ref.library_tables(13, 17, 30, 17, name))
    both = ref.resize(img, (30, 30), ref.library_tables(13, 17, 30, 30, name))
    assert rows.shape == (30, 17, 3) and both.shape == (30, 30, 3)


# ---- what it buys --------------------------------------------------------------------------------------------------------
def _zone_plate(h, w, gh, gw, ss):
    """0.5 + 0.45 cos(pi r^2 / (1.1 max(h, w))), r in SOURCE pixels (h x w) from the frame centre, rendered on a gh x gw grid with
    ss x ss samples per pixel"""
    y = (np.arange(gh * ss) + 0.5) / (gh * ss) * h - h / 2.0
    x = (np.arange(gw * ss) + 0.5) / (gw * ss) * w - w / 2.0
    r2 = y[:, None] ** 2 + x[None, :] ** 2
    v = 0.5 + 0.45 * np.cos(np.pi * r2 / (1.1 * max(h, w)))
    return v.reshape(gh, ss, gw, ss).mean(axis=(1, 3))


def _psnr(a, b):
    mse = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return 10 * np.log10(255.0 ** 2 / mse)


def test_zone_plate_antialiasing(record_property):
    h, w, oh, ow = 270, 480, 180, 320
    src = np.rint(_zone_plate(h, w, h, w, 4) * 255).astype(np.uint8)
    src = np.repeat(src[:, :, None], 3, axis=2)
    want = _zone_plate(h, w, oh, ow, 6) * 255
    want = np.repeat(want[:, :, None], 3, axis=2)
    psnr = {name: _psnr(ref.resize(src, (oh, ow), ref.library_tables(h, w, oh, ow, name)), want) for name in ref.FILTERS}
    psnr["point"] = _psnr(ref.point_sample(src, (oh, ow)), want)
    print("zone plate 480x270 -> 320x180, PSNR dB: " + ", ".join("%s %.1f" % kv for kv in psnr.items()))
    for k, v in psnr.items():
        record_property(k, v)
    for name in ref.FILTERS:
        assert psnr[name] > psnr["point"]
    assert psnr["lanczos"] >= psnr["point"] + 4.0 and psnr["bicubic"] >= psnr["point"] + 4.0


# ---- the command line ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,msg", [
    (["--out-size", "1440"], "--out-size"), (["--out-size", "0x10"], "--out-size"), (["--out-size", "12x-4"], "--out-size"),
    (["--out-size", "16 by 16"], "--out-size"),
    (["-s", "2", "--out-size", "65x16"], "--out-size"),           # 16 -> 65: above 4
    (["-s", "4", "--out-size", "32x7"], "--out-size"),            # 32 -> 7: below 1/4
    (["--out-scale", "9"], "--out-scale"), (["--out-scale", "0"], "--out-scale"), (["--out-scale", "-1"], "--out-scale"),
    (["--out-size", "16x16", "--out-scale", "1.5"], "--out-scale"),
    (["--out-size", "16x16", "--resize-filter", "mitchell"], "--resize-filter"),
    (["-s", "1", "-m", "n=4", "--out-size", "12x12"], "--out-size"),
])
def test_cli_errors(capsys, argv, msg):
    with pytest.raises(SystemExit) as e:
        rawvideo.main(["-W", "8", "-H", "8"] + argv)
    assert e.value.code == 2
    assert msg in capsys.readouterr().err, argv


def test_out_scale_sizes():
    assert rawvideo.out_scale_size(720, 1280, 1.5) == (1080, 1920)
    assert rawvideo.out_scale_size(480, 853, 1.5) == (720, 1280)          # 2 floor(853 * 1.5 / 2 + 0.5)
    assert rawvideo.out_scale_size(720, 1280, 3) == (2160, 3840)
    assert rawvideo.out_scale_size(1, 1, 0.5) == (2, 2)


class _Stop(Exception):
    pass


@pytest.mark.parametrize("argv,h,w,want", [
    (["-s", "2", "--out-scale", "1.5"], 720, 1280, (1080, 1920)),
    (["-s", "2", "--out-scale", "1.5"], 480, 853, (720, 1280)),
    (["-s", "4", "--out-scale", "3"], 720, 1280, (2160, 3840)),
    (["-s", "2", "--out-size", "2560x1440", "--resize-filter", "bicubic"], 1080, 1920, (1440, 2560)),
    (["-s", "2", "--out-size", "2560x1440"], 720, 1280, None),            # the net's own size: nothing to resample
])
def test_cli_sizes_reach_the_streamer(monkeypatch, tmp_path, argv, h, w, want):
    seen = {}

    class Net:
        scale = int(argv[1])
    monkeypatch.setattr(rawvideo, "load_net", lambda stem, gpu, path: Net())

    def fake_stream(fin, fout, hh, ww, nets, max_frames=None, write_threads=1, pix=None):
        seen["pix"] = pix
        raise _Stop()
    monkeypatch.setattr(rawvideo, "stream", fake_stream)
    with pytest.raises(_Stop):
        (tmp_path / "in.raw").write_bytes(b"")
        rawvideo.main(["-W", str(w), "-H", str(h), "-i", str(tmp_path / "in.raw"), "-o", str(tmp_path / "out.raw")] + argv)
    if want is None:
        assert seen["pix"].out_size is None and seen["pix"].resize_kw() == {}
    else:
        assert seen["pix"].out_size == want
        kw = seen["pix"].resize_kw()
        assert kw["out_size"] == want and (kw.get("resize_filter") == "bicubic") == ("bicubic" in argv)


# ---- the streamer ------------------------------------------------------------------------------------------------------
def _to_bgr(buf, fmt, h, w, depth):
    if depth == 16:
        return pixfmt16_ref.pix_to_bgr16(buf, fmt, h, w, "bt709")
    return pixfmt_ref.pix_to_bgr(buf, fmt, h, w, "bt709") if fmt != "bgr24" else np.asarray(buf).reshape(h, w, 3)


def _from_bgr(bgr, fmt, depth):
    if depth == 16:
        return pixfmt16_ref.bgr16_to_pix(bgr, fmt, "bt709")
    return pixfmt_ref.bgr_to_pix(bgr, fmt, "bt709") if fmt != "bgr24" else bgr.reshape(-1)


def _net_apply(bgr, scale):
    mx = np.iinfo(bgr.dtype).max
    return np.minimum(np.repeat(np.repeat(bgr.astype(np.int64), scale, 0), scale, 1) + 3, mx).astype(bgr.dtype)


class ResizeFakeNet:
    """Net.submit_pix / collect_u8 stand-in in the pattern of tests/test_pixfmt16.py's Pix16FakeNet, which also applies the
    restated resampler when out_size is given; finished only at collect time (buffer reuse mistakes show up)"""

    def __init__(self, scale):
        self.scale, self.live, self.calls = scale, 0, []

    def submit_u8(self, frame, out=None, tile_size=0, border=0):
        return self.submit_pix(frame, frame.shape[0], frame.shape[1], "bgr24", out=out, tile_size=tile_size, border=border, _u8=True)

    def submit_pix(self, buf, h, w, in_fmt, out=None, out_fmt="bgr24", colour="bt601", color_range="tv", tile_size=0, border=0,
                   _u8=False, **kw):
        assert self.live < 3
        self.live += 1
        self.calls.append(("submit_u8" if _u8 else "submit_pix", dict(kw)))
        depth = kw.get("bit_depth", 8)
        oh, ow = kw.get("out_size") or (h * self.scale, w * self.scale)
        assert out.nbytes == ncnn.pix_frame_bytes(out_fmt, oh, ow)
        return (np.array(buf).reshape(-1).view(np.uint8), h, w, in_fmt, out, out_fmt, depth, (oh, ow), kw.get("resize_filter", "lanczos"))

    def collect_u8(self, t):
        buf, h, w, in_fmt, out, out_fmt, depth, size, filt = t
        self.live -= 1
        out.reshape(-1).view(np.uint8)[...] = np.asarray(expected_frame(buf, h, w, in_fmt, out_fmt, depth, self.scale, size, filt)).reshape(-1).view(np.uint8)
        return out


def expected_frame(buf, h, w, in_fmt, out_fmt, depth, scale, size, filt):
    x = _net_apply(_to_bgr(buf, in_fmt, h, w, depth), scale)
    if size != x.shape[:2]:
        x = ref.resize(x, size, ref.library_tables(x.shape[0], x.shape[1], size[0], size[1], filt))
    return _from_bgr(x, out_fmt, depth)


CASES = [("bgr24", "bgr24", 8, (13, 21), "lanczos"), ("yuv420p", "yuv420p", 8, (14, 20), "bicubic"),
         ("yuv420p10le", "p010le", 16, (12, 26), "lanczos"), ("bgr24", "yuv420p", 8, (7, 11), "bilinear")]      # (an odd output size)


def _input_frames(in_fmt, depth, h, w, n, seed):
    rng = np.random.default_rng(seed)
    if depth == 16:
        return [np.asarray(pixfmt16_ref.bgr16_to_pix(rng.integers(0, 65536, (h, w, 3), dtype=np.uint16), in_fmt, "bt709")) for _ in range(n)]
    return [np.asarray(_from_bgr(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), in_fmt, 8)) for _ in range(n)]


@pytest.mark.parametrize("in_fmt,out_fmt,depth,size,filt", CASES)
@pytest.mark.parametrize("nlanes", [1, 2])
def test_stream_out_size(in_fmt, out_fmt, depth, size, filt, nlanes):
    h, w = 6, 8
    pix = rawvideo.PixFormats(in_fmt, out_fmt, "bt709", "tv", depth, "replicate", "left", size, filt)
    frames = _input_frames(in_fmt, depth, h, w, 9, 5)
    want = b"".join(np.asarray(expected_frame(f.reshape(-1).view(np.uint8), h, w, in_fmt, out_fmt, depth, 2, size, filt)).tobytes() for f in frames)
    lanes = [[(ResizeFakeNet(2), 32)] for _ in range(nlanes)]
    fout = io.BytesIO()
    n = rawvideo.stream(io.BytesIO(b"".join(f.tobytes() for f in frames)), fout, h, w, lanes if nlanes > 1 else lanes[0],
                        alloc=lambda s: np.zeros(s, np.uint8), pix=pix)
    assert n == len(frames) and fout.getvalue() == want
    assert len(want) == len(frames) * ncnn.pix_frame_bytes(out_fmt, *size)
    for lane in lanes:
        for name, kw in lane[0][0].calls:
            assert name == "submit_pix" and kw["out_size"] == size
            assert kw.get("resize_filter", "lanczos") == filt and ("resize_filter" in kw) == (filt != "lanczos")


def test_stream_two_stages_resamples_behind_the_last():
    """-m a in front of the 2x net: the 1x stage sees no new keyword, the last stage gets the output size"""
    h, w, size = 6, 8, (9, 13)
    pix = rawvideo.PixFormats("yuv420p", "yuv420p", "bt709", out_size=size)
    frames = _input_frames("yuv420p", 8, h, w, 7, 6)
    first, second = ResizeFakeNet(1), ResizeFakeNet(2)
    fout = io.BytesIO()
    n = rawvideo.stream(io.BytesIO(b"".join(f.tobytes() for f in frames)), fout, h, w, [(first, 0), (second, 32)],
                        alloc=lambda s: np.zeros(s, np.uint8), pix=pix)
    want = b""
    for f in frames:
        x = _net_apply(_net_apply(_to_bgr(f, "yuv420p", h, w, 8), 1), 2)
        x = ref.resize(x, size, ref.library_tables(2 * h, 2 * w, size[0], size[1], "lanczos"))
        want += np.asarray(_from_bgr(x, "yuv420p", 8)).tobytes()
    assert n == 7 and fout.getvalue() == want
    assert all("out_size" not in kw for _, kw in first.calls) and all(kw["out_size"] == size for _, kw in second.calls)


@pytest.mark.parametrize("nlanes", [1, 2])
@pytest.mark.parametrize("in_fmt,out_fmt,depth,size,filt", CASES[:3])
def test_stream_segments_out_size(tmp_path, in_fmt, out_fmt, depth, size, filt, nlanes):
    h, w = 6, 8
    pix = rawvideo.PixFormats(in_fmt, out_fmt, "bt709", "tv", depth, "replicate", "left", size, filt)
    frames = _input_frames(in_fmt, depth, h, w, 7, 8)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(b"".join(f.tobytes() for f in frames))
    lanes = [[(ResizeFakeNet(2), 32)] for _ in range(nlanes)]
    n = rawvideo.stream_segments(str(src), str(dst), h, w, lanes, 2, None, lambda s: np.zeros(s, np.uint8), open, None, 1, pix)
    want = b"".join(np.asarray(expected_frame(f.reshape(-1).view(np.uint8), h, w, in_fmt, out_fmt, depth, 2, size, filt)).tobytes() for f in frames)
    assert n == len(frames)
    assert os.path.getsize(dst) == len(frames) * ncnn.pix_frame_bytes(out_fmt, *size)
    assert dst.read_bytes() == want


def test_without_the_flags_the_net_sees_no_new_keyword():
    h, w = 6, 8
    for in_fmt, out_fmt in (("bgr24", "bgr24"), ("yuv420p", "nv12")):
        pix = rawvideo.PixFormats(in_fmt, out_fmt, "bt709")
        assert pix.resize_kw() == {} and pix.out_size is None
        net = ResizeFakeNet(2)
        frames = _input_frames(in_fmt, 8, h, w, 4, 9)
        fout = io.BytesIO()
        assert rawvideo.stream(io.BytesIO(b"".join(f.tobytes() for f in frames)), fout, h, w, [(net, 32)],
                               alloc=lambda s: np.zeros(s, np.uint8), pix=pix) == 4
        assert len(fout.getvalue()) == 4 * ncnn.pix_frame_bytes(out_fmt, 2 * h, 2 * w)
        assert [c for c in net.calls] == [("submit_u8" if in_fmt == out_fmt == "bgr24" else "submit_pix", {})] * 4


def test_lane_that_ends_in_the_denoise_stage_refuses():
    pix = rawvideo.PixFormats(out_size=(8, 8))
    with pytest.raises(ValueError, match="denoise"):
        rawvideo.Lane([(("denoise", 0, 4), 0)], 6, 8, lambda s: np.zeros(s, np.uint8), pix)


def test_python_refusals_without_a_gpu():
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match=r"\[1/4, 4\]"):
        ncnn.resize(img, (1, 8))
    with pytest.raises(ValueError, match=r"\[1/4, 4\]"):
        ncnn.resize(img, (8, 33))
    with pytest.raises(ValueError, match="at least 1"):
        ncnn.resize(img, (0, 8))
    with pytest.raises(ValueError, match="filter"):
        ncnn.resize(img, (8, 8), filter="area")
    with pytest.raises(ValueError, match="u8 or u16"):
        ncnn.resize(img.astype(np.float32), (8, 8))
    with pytest.raises(ValueError):
        rawvideo.PixFormats(resize_filter="area")
    with pytest.raises(ValueError):
        rawvideo.PixFormats(out_size=(0, 4))
