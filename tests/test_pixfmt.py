"""Raw-video pixel formats on the CPU: the numpy restatement (tests/pixfmt_ref.py) against known
answers and the float64 textbook formulas over every colour, frame sizes, the rawvideo flags, and stream() /
stream_segments() with a stand-in net whose submit_pix does the restatement's arithmetic."""
import ctypes
import io
import itertools

import numpy as np
import pytest

import pixfmt_ref as ref
from upscale_video_amd import ncnn, rawvideo

COMBOS = [(m, full) for m in ("bt601", "bt709") for full in (False, True)]


# ---- the arithmetic -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,rgb,want", [
    ("bt601", (0, 0, 0), (16, 128, 128)), ("bt601", (255, 255, 255), (235, 128, 128)), ("bt601", (255, 0, 0), (81, 90, 240)),
    ("bt601", (0, 255, 0), (145, 54, 34)), ("bt601", (0, 0, 255), (41, 240, 110)),
    ("bt709", (255, 0, 0), (63, 102, 240)), ("bt709", (0, 255, 0), (173, 42, 26)), ("bt709", (0, 0, 255), (32, 240, 118)),
])
def test_known_answers_limited_range(matrix, rgb, want):
    r, g, b = rgb
    y = ref.fwd_luma(r, g, b, matrix)
    u, v = ref.fwd_chroma(r, g, b, 0, matrix)
    assert (int(y), int(u), int(v)) == want
    # the same colour as a 2x2 block: its sums give the same chroma
    u4, v4 = ref.fwd_chroma(4 * r, 4 * g, 4 * b, 2, matrix)
    assert (int(u4), int(v4)) == want[1:]


def test_known_answers_p010_and_full_range():
    frame = np.array([[[0, 0, 0], [255, 255, 255]]], np.uint8)          # black, white (BGR)
    p = ref.bgr_to_pix(frame, "p010le").view("<u2")
    assert list(p[:2]) == [4096, 60160] and list(p[2:]) == [32768, 32768]
    for m in ("bt601", "bt709"):
        assert int(ref.fwd_luma(0, 0, 0, m, full=True)) == 0 and int(ref.fwd_luma(255, 255, 255, m, full=True)) == 255
        assert int(ref.fwd_luma(255, 255, 255, m, full=True, depth=10)) == 1023
        u, v = ref.fwd_chroma(255, 255, 255, 0, m, full=True)
        assert (int(u), int(v)) == (128, 128)
    # and back: the limited-range codes of black and white are black and white
    for depth in (8, 10):
        k = 1 << (depth - 8)
        assert [int(t) for t in ref.inv_pixel(16 * k, 128 * k, 128 * k, depth=depth)] == [0, 0, 0]
        assert [int(t) for t in ref.inv_pixel(235 * k, 128 * k, 128 * k, depth=depth)] == [255, 255, 255]


def _all_triples():
    a = np.arange(1 << 24, dtype=np.int64)
    return a >> 16, (a >> 8) & 255, a & 255


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("matrix,full", COMBOS)
def test_every_colour_forward_is_within_one_code_of_float64(matrix, full, depth):
    r, g, b = _all_triples()
    maxv = (1 << depth) - 1
    fy, fu, fv = ref.float_fwd(r, g, b, matrix, full, depth)
    y = ref.fwd_luma(r, g, b, matrix, full, depth)
    u, v = ref.fwd_chroma(r, g, b, 0, matrix, full, depth)
    for fixed, flt in ((y, fy), (u, fu), (v, fv)):
        assert np.abs(fixed - np.clip(flt, 0, maxv)).max() <= 1


@pytest.mark.parametrize("matrix,full", COMBOS)
def test_every_ycbcr_triple_inverse_is_within_one_code_of_float64(matrix, full):
    y, u, v = _all_triples()
    got = ref.inv_pixel(y, u, v, matrix, full)
    want = ref.float_inv(y, u, v, matrix, full)
    for fixed, flt in zip(got, want):
        assert np.abs(fixed - np.clip(flt, 0, 255)).max() <= 1


def test_round_trip_of_grey_is_exact():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2).repeat(2, axis=0)      # 2 x 256
    for fmt in ("yuv420p", "nv12", "p010le"):
        for m, full in COMBOS:
            back = ref.pix_to_bgr(ref.bgr_to_pix(grey, fmt, m, full), fmt, 2, 256, m, full)
            assert np.abs(back.astype(int) - grey).max() <= 1, (fmt, m, full)


# ---- frame sizes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (2, 4), (970, 965), (1080, 1920), (2160, 3840)])
def test_frame_bytes(uva, h, w):
    from upscale_video_amd import _lib
    L = _lib.load()
    cw, ch = (w + 1) // 2, (h + 1) // 2
    want = {"bgr24": 3 * w * h, "yuv420p": w * h + 2 * cw * ch, "nv12": w * h + 2 * cw * ch, "p010le": 2 * (w * h + 2 * cw * ch)}
    for fmt, code in ncnn.PIX_FORMATS.items():
        assert ncnn.pix_frame_bytes(fmt, h, w) == want[fmt] == ref.frame_bytes(fmt, h, w) == L.uva_pix_frame_bytes(code, h, w)
        assert ref.bgr_to_pix(np.zeros((h, w, 3), np.uint8), fmt).nbytes == want[fmt] if h * w < 10 ** 5 else True
    assert L.uva_pix_frame_bytes(4, h, w) == 0 and L.uva_pix_frame_bytes(1, 0, w) == 0
    with pytest.raises(ValueError):
        ncnn.pix_frame_bytes("rgb24", h, w)


def test_colour_word():
    assert ncnn.colour_word() == 0 and ncnn.colour_word("bt709", "pc") == 3 and ncnn.colour_word("bt601", "pc") == 2
    for bad in (("bt2020", "tv"), ("bt601", "mpeg")):
        with pytest.raises(ValueError):
            ncnn.colour_word(*bad)


# ---- the streamer -----------------------------------------------------------------------------------------------------
class PixFakeNet:
    """Net.submit_u8 / submit_pix / collect_u8 stand-in: nearest-neighbour upscale + 1 on the u8 BGR frame, the pixel formats
    converted with the restatement; finished only at collect time (buffer-reuse mistakes show up)."""

    def __init__(self, scale):
        self.scale, self.live, self.pix_calls = scale, 0, 0

    def submit_u8(self, img, out=None, tile_size=0, border=0):
        assert self.live < 3
        self.live += 1
        return ("bgr24", img, img.shape[0], img.shape[1], out, "bgr24", "bt601", "tv")

    def submit_pix(self, buf, h, w, in_fmt, out=None, out_fmt="bgr24", colour="bt601", color_range="tv", tile_size=0, border=0):
        assert self.live < 3 and buf.nbytes == ref.frame_bytes(in_fmt, h, w)
        assert out.nbytes == ref.frame_bytes(out_fmt, h * self.scale, w * self.scale)
        self.live += 1
        self.pix_calls += 1
        return (in_fmt, buf, h, w, out, out_fmt, colour, color_range)

    def collect_u8(self, t):
        in_fmt, buf, h, w, out, out_fmt, colour, rng = t
        self.live -= 1
        full = rng == "pc"
        res = self.apply(ref.pix_to_bgr(buf, in_fmt, h, w, colour, full), self.scale)
        out.reshape(-1)[...] = ref.bgr_to_pix(res, out_fmt, colour, full)
        return out

    @staticmethod
    def apply(bgr, scale):
        return np.repeat(np.repeat(bgr, scale, 0), scale, 1) + 1


def _frames(n, h, w, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 200, (h, w, 3), dtype=np.uint8) for _ in range(n)]


def _want(frames, pix, scales, denoise=False):
    """the per-frame composition: input format -> BGR -> (255 - x if denoised) -> nets -> output format"""
    full = pix.color_range == "pc"
    out = []
    for f in frames:
        h, w, _ = f.shape
        packed = ref.bgr_to_pix(f, pix.in_fmt, pix.colour, full)
        x = ref.pix_to_bgr(packed, pix.in_fmt, h, w, pix.colour, full)
        if denoise:
            x = 255 - x
        for s in scales:
            x = PixFakeNet.apply(x, s)
        out.append(ref.bgr_to_pix(x, pix.out_fmt, pix.colour, full).tobytes())
    return packed_input(frames, pix), b"".join(out)


def packed_input(frames, pix):
    return b"".join(ref.bgr_to_pix(f, pix.in_fmt, pix.colour, pix.color_range == "pc").tobytes() for f in frames)


@pytest.mark.parametrize("in_fmt,out_fmt", list(itertools.product(ncnn.PIX_FORMATS, repeat=2)))
@pytest.mark.parametrize("h,w", [(6, 10), (5, 7)])
@pytest.mark.parametrize("nlanes", [1, 2])
def test_stream_converts_at_both_ends(in_fmt, out_fmt, h, w, nlanes):
    pix = rawvideo.PixFormats(in_fmt, out_fmt, "bt709" if (h + nlanes) % 2 else "bt601", "pc" if nlanes == 2 else "tv")
    frames = _frames(11, h, w)
    data, want = _want(frames, pix, [1, 2])
    lanes = [[(PixFakeNet(1), 0), (PixFakeNet(2), 32)] for _ in range(nlanes)]
    fout = io.BytesIO()
    n = rawvideo.stream(io.BytesIO(data), fout, h, w, lanes if nlanes > 1 else lanes[0], alloc=lambda s: np.zeros(s, np.uint8), pix=pix)
    assert n == len(frames) and fout.getvalue() == want
    # the first net takes the input format, the last one gives the output format, nothing else converts
    first, last = lanes[0][0][0], lanes[0][1][0]
    assert (first.pix_calls > 0) == (in_fmt != "bgr24") and (last.pix_calls > 0) == (out_fmt != "bgr24")


def test_default_formats_take_the_old_path():
    """no format flags: submit_u8 only (the existing FakeNets have nothing else)"""
    h, w = 4, 6
    frames = _frames(5, h, w)
    nets = [(PixFakeNet(1), 0), (PixFakeNet(2), 0)]
    fout = io.BytesIO()
    rawvideo.stream(io.BytesIO(b"".join(f.tobytes() for f in frames)), fout, h, w, nets, alloc=lambda s: np.zeros(s, np.uint8))
    assert all(n.pix_calls == 0 for n, _ in nets)
    assert fout.getvalue() == b"".join(PixFakeNet.apply(PixFakeNet.apply(f, 1), 2).tobytes() for f in frames)


@pytest.mark.parametrize("in_fmt,out_fmt", [("yuv420p", "p010le"), ("nv12", "yuv420p"), ("p010le", "bgr24"), ("bgr24", "nv12"),
                                            ("yuv420p", "yuv420p")])
@pytest.mark.parametrize("nlanes", [1, 2, 3])
def test_segments_offsets_and_byte_counts(tmp_path, in_fmt, out_fmt, nlanes):
    h, w = 5, 9
    pix = rawvideo.PixFormats(in_fmt, out_fmt)
    frames = _frames(10, h, w)
    data, want = _want(frames, pix, [2])
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(data)
    lanes = [[(PixFakeNet(2), 0)] for _ in range(nlanes)]
    assert rawvideo.stream_segments(str(src), str(dst), h, w, lanes, 2, alloc=lambda s: np.zeros(s, np.uint8), pix=pix) == 10
    assert dst.stat().st_size == 10 * ref.frame_bytes(out_fmt, 2 * h, 2 * w) and dst.read_bytes() == want
    outs = [str(tmp_path / ("o%d.raw" % k)) for k in range(nlanes)]
    lanes = [[(PixFakeNet(2), 0)] for _ in range(nlanes)]
    assert rawvideo.stream_segments(str(src), outs, h, w, lanes, 2, alloc=lambda s: np.zeros(s, np.uint8), pix=pix, max_frames=7) == 7
    assert b"".join(open(o, "rb").read() for o in outs) == want[:7 * ref.frame_bytes(out_fmt, 2 * h, 2 * w)]
    # a file that ends inside a frame of the input format is refused
    src.write_bytes(data[:-1])
    with pytest.raises(EOFError):
        rawvideo.stream_segments(str(src), str(dst), h, w, [[(PixFakeNet(2), 0)]], 2, alloc=lambda s: np.zeros(s, np.uint8), pix=pix)


class _FakeLib:
    """uva_denoise_u8 (255 - x) and uva_pix_convert (the restatement) on host pointers"""

    def __init__(self):
        self.converts = []

    @staticmethod
    def _arr(addr, n):
        return np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(addr))

    def uva_denoise_u8(self, gpu, src, h, w, ss, dst, ds, hl, hc):
        self._arr(dst, h * w * 3)[...] = 255 - self._arr(src, h * w * 3)
        return 0

    def uva_pix_convert(self, gpu, src, in_fmt, dst, out_fmt, h, w, colour):
        names = {v: k for k, v in ncnn.PIX_FORMATS.items()}
        fi, fo = names[in_fmt], names[out_fmt]
        self.converts.append((fi, fo))
        m = "bt709" if colour & 1 else "bt601"
        res = ref.convert(self._arr(src, ref.frame_bytes(fi, h, w)), fi, fo, h, w, m, bool(colour & 2))
        self._arr(dst, res.size)[...] = res
        return 0


@pytest.mark.parametrize("in_fmt,out_fmt", [("yuv420p", "p010le"), ("nv12", "bgr24"), ("bgr24", "yuv420p")])
@pytest.mark.parametrize("with_net", [True, False])
def test_denoise_first_converts_on_the_host_route(monkeypatch, in_fmt, out_fmt, with_net):
    """`-m n=K` leading a lane takes host BGR: its input is converted with uva_pix_convert; alone (`-s 1 -m n=K`) it also
    produces the output format"""
    from upscale_video_amd import _lib
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: fake)
    monkeypatch.setattr(_lib, "check", lambda rc: None)
    h, w = 5, 6
    pix = rawvideo.PixFormats(in_fmt, out_fmt, "bt709")
    frames = _frames(8, h, w)
    data, want = _want(frames, pix, [2] if with_net else [], denoise=True)
    chain = [(("denoise", 0, 5), 0)] + ([(PixFakeNet(2), 32)] if with_net else [])
    fout = io.BytesIO()
    assert rawvideo.stream(io.BytesIO(data), fout, h, w, chain, alloc=lambda s: np.zeros(s, np.uint8), pix=pix) == 8
    assert fout.getvalue() == want
    assert ((in_fmt, "bgr24") in fake.converts) == (in_fmt != "bgr24")
    assert (("bgr24", out_fmt) in fake.converts) == (out_fmt != "bgr24" and not with_net)


# ---- the command line ------------------------------------------------------------------------------------------------
def test_cli_rejects_unknown_formats(capsys):
    for argv, msg in ((["--in-pix-fmt", "rgb24"], "invalid choice"), (["--out-pix-fmt", "yuv444p"], "invalid choice"),
                      (["--colorspace", "bt2020"], "invalid choice"), (["--color-range", "mpeg"], "invalid choice")):
        with pytest.raises(SystemExit):
            rawvideo.main(["-W", "8", "-H", "8"] + argv)
        assert msg in capsys.readouterr().err, argv


def test_cli_scale_1_copies_or_converts_once(tmp_path, monkeypatch):
    """`-s 1` without a net: equal formats are copied through in frames of that format (odd sizes too); different ones are
    converted once per frame"""
    h, w = 5, 7
    pix = rawvideo.PixFormats("yuv420p", "yuv420p")
    data = packed_input(_frames(4, h, w), pix)
    src, dst = tmp_path / "in.yuv", tmp_path / "out.yuv"
    src.write_bytes(data)
    assert rawvideo.main(["-i", str(src), "-o", str(dst), "-W", str(w), "-H", str(h), "-s", "1",
                          "--in-pix-fmt", "yuv420p", "--out-pix-fmt", "yuv420p", "--frames", "3"]) == 0
    assert dst.read_bytes() == data[:3 * ref.frame_bytes("yuv420p", h, w)]
    calls = []

    def fake_convert(buf, hh, ww, fi, fo, colour="bt601", color_range="tv", out=None, gpu=0):
        calls.append((fi, fo, colour, color_range, gpu))
        out.reshape(-1)[...] = ref.convert(buf, fi, fo, hh, ww, colour, color_range == "pc")
        return out
    monkeypatch.setattr(ncnn, "convert_pix", fake_convert)
    assert rawvideo.main(["-i", str(src), "-o", str(dst), "-W", str(w), "-H", str(h), "-s", "1", "-g", "2",
                          "--in-pix-fmt", "yuv420p", "--out-pix-fmt", "p010le", "--colorspace", "bt709", "--color-range", "pc"]) == 0
    fb = ref.frame_bytes("yuv420p", h, w)
    want = b"".join(ref.convert(np.frombuffer(data[k * fb:(k + 1) * fb], np.uint8), "yuv420p", "p010le", h, w, "bt709", True).tobytes()
                    for k in range(4))
    assert dst.read_bytes() == want and calls == [("yuv420p", "p010le", "bt709", "pc", 2)] * 4


def test_pipe_sink_refuses_a_short_ring(monkeypatch):
    import os
    monkeypatch.setenv("UVA_RAW_VMSPLICE", "1")
    r, wfd = os.pipe()
    with os.fdopen(wfd, "wb") as fout, os.fdopen(r, "rb"):
        sink = rawvideo.PipeSink(fout, ring=rawvideo.PIPE_DEPTH + 3)
        assert sink._fd is not None
        with pytest.raises(AssertionError):
            sink.write(np.zeros(1 << 22, np.uint8))
