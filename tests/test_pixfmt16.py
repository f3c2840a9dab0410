"""The 16-bit route's conversions on the CPU: the numpy restatement (tests/pixfmt16_ref.py) against known
answers and float64 over every 8-bit colour and a dense 10-bit Y'CbCr sweep, the layouts and frame sizes, the --bit-depth flag,
and stream() with a stand-in net whose submit_pix takes bit_depth=16."""
import io

import numpy as np
import pytest

import pixfmt16_ref as ref
from upscale_video_amd import ncnn, rawvideo

COMBOS = [(m, full) for m in ("bt601", "bt709") for full in (False, True)]


# ---- the arithmetic -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,full", COMBOS)
@pytest.mark.parametrize("depth", [8, 10])
def test_known_answers(matrix, full, depth):
    ys = (1 << depth) - 1 if full else 219 << (depth - 8)
    yoff = 0 if full else 16 << (depth - 8)
    coff = 1 << (depth - 1)
    for v, want_y in ((0, yoff), (65535, yoff + ys), (32768, yoff + ys * 32768 / 65535)):
        # black and white exactly; mid-grey (8-bit tv: 125.502, a near tie the 2^-19 coefficients cannot resolve) within a code
        assert abs(int(ref.fwd_luma(v, v, v, matrix, full, depth)) - want_y) <= (0 if v in (0, 65535) else 1), (v, matrix, full, depth)
        u, c = ref.fwd_chroma(4 * v, 4 * v, 4 * v, 2, matrix, full, depth)
        assert int(u) == int(c) == coff
    # back: black and white Y' with neutral chroma are 0 and 65535 exactly
    b, g, r = ref.inv_pixel(np.array([yoff, yoff + ys]), coff, coff, matrix, full, depth)
    assert list(b) == list(g) == list(r) == [0, 65535]


def test_bgr24_widen_narrow():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(ref.widen(v), v.astype(np.int64) * 257)
    assert np.array_equal(ref.narrow(ref.widen(v)), v)
    w = np.arange(65536)
    assert np.array_equal(ref.narrow(w), np.rint(w / 257.0).astype(np.uint8))


@pytest.mark.parametrize("matrix,full", COMBOS)
@pytest.mark.parametrize("depth", [8, 10])
def test_every_8bit_colour_through_u16_within_one_code(matrix, full, depth):
    """all 2^24 BGR triples, widened (v * 257): Y', and Cb / Cr of a one-pixel block, within one code of float64"""
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for r8 in range(0, 256):
        r16, g16, b16 = r8 * 257, g.ravel() * 257, b.ravel() * 257
        y = ref.fwd_luma(r16, g16, b16, matrix, full, depth)
        u, v = ref.fwd_chroma(r16, g16, b16, 0, matrix, full, depth)
        fy, fu, fv = ref.float_fwd(r16, g16, b16, matrix, full, depth)
        mx = (1 << depth) - 1
        for got, want in ((y, fy), (u, fu), (v, fv)):
            assert np.abs(got - np.clip(want, 0, mx)).max() <= 1.0, (r8, matrix, full, depth)


@pytest.mark.parametrize("matrix,full", COMBOS)
def test_dense_10bit_sweep_within_one_code(matrix, full):
    """every 10-bit Y' x a 16-step Cb / Cr grid (64 x 64 values) -> u16 BGR within one code of float64"""
    y, u, v = np.meshgrid(np.arange(1024), np.arange(0, 1024, 16), np.arange(0, 1024, 16), indexing="ij")
    b, g, r = ref.inv_pixel(y, u, v, matrix, full, 10)
    fb, fg, fr = ref.float_inv(y, u, v, matrix, full, 10)
    for got, want in ((b, fb), (g, fg), (r, fr)):
        assert np.abs(got - np.clip(want, 0, 65535)).max() <= 1.0


def test_yuv420p10le_is_p010le_repacked():
    rng = np.random.default_rng(1)
    for h, w in ((1, 1), (3, 5), (6, 8), (7, 40)):
        bgr16 = rng.integers(0, 65536, (h, w, 3), dtype=np.uint16)
        bgr8 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for m, full in COMBOS:
            p010 = ref.bgr16_to_pix(bgr16, "p010le", m, full)
            assert np.array_equal(ref.bgr16_to_pix(bgr16, "yuv420p10le", m, full), ref.p010_to_yuv420p10(p010, h, w))
            assert np.array_equal(ref.pix_to_bgr16(ref.p010_to_yuv420p10(p010, h, w), "yuv420p10le", h, w, m, full),
                                  ref.pix_to_bgr16(p010, "p010le", h, w, m, full))
            assert np.array_equal(ref.bgr_to_pix8(bgr8, "yuv420p10le", m, full),
                                  ref.p010_to_yuv420p10(ref.bgr_to_pix8(bgr8, "p010le", m, full), h, w))


def test_frame_bytes_and_buffers():
    for fmt in ref.FORMATS16:
        for h, w in ((1, 1), (3, 5), (1080, 1920)):
            assert ncnn.pix_frame_bytes(fmt, h, w) == ref.frame_bytes(fmt, h, w)
            assert ncnn.pix_empty(fmt, h, w).nbytes == ref.frame_bytes(fmt, h, w)
    assert ncnn.pix_empty("bgr48le", 2, 3).dtype == np.uint16 and ncnn.pix_empty("bgr48le", 2, 3).shape == (2, 3, 3)
    assert ncnn.PIX_FORMATS_ALL["yuv420p10le"] == 5 and ncnn.PIX_FORMATS_ALL["bgr48le"] == 6


def test_bgr48le_needs_bit_depth_16():
    with pytest.raises(ValueError, match="16-bit"):
        rawvideo.PixFormats("bgr48le", "p010le")
    with pytest.raises(ValueError, match="16-bit"):
        ncnn.convert_pix(np.zeros((2, 2, 3), np.uint16), 2, 2, "bgr48le", "p010le")
    assert rawvideo.PixFormats("bgr48le", "p010le", bit_depth=16).bit_depth == 16


# ---- the command line ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,msg", [
    (["-m", "a", "--bit-depth", "16"], "--bit-depth 16"), (["-m", "n=4", "--bit-depth", "16"], "--bit-depth 16"),
    (["-m", "r", "-s", "4", "--bit-depth", "16"], "--bit-depth 16"), (["--bit-depth", "10"], "invalid choice"),
    (["--in-pix-fmt", "bgr48le"], "needs --bit-depth 16"), (["--out-pix-fmt", "bgr48le", "--bit-depth", "8"], "needs --bit-depth 16"),
])
def test_cli_bit_depth_errors(capsys, argv, msg):
    with pytest.raises(SystemExit) as e:
        rawvideo.main(["-W", "8", "-H", "8"] + argv)
    assert e.value.code == 2
    assert msg in capsys.readouterr().err, argv


# ---- the streamer ------------------------------------------------------------------------------------------------------
class Pix16FakeNet:
    """Net.submit_pix(bit_depth=16) / collect_u8 stand-in: the restated conversions to u16 BGR, nearest-neighbour upscale
    + 3 (saturating), back to the output format; finished only at collect time (buffer reuse mistakes show up)"""

    def __init__(self, scale):
        self.scale, self.live, self.calls = scale, 0, []

    def submit_u8(self, *a, **k):
        raise AssertionError("--bit-depth 16 must not take the 8-bit route")

    def submit_pix(self, buf, h, w, in_fmt, out=None, out_fmt="bgr24", colour="bt601", color_range="tv", tile_size=0, border=0,
                   bit_depth=8):
        assert self.live < 3 and bit_depth == 16
        assert np.asarray(buf).nbytes == ref.frame_bytes(in_fmt, h, w)
        assert out.nbytes == ref.frame_bytes(out_fmt, h * self.scale, w * self.scale)
        self.live += 1
        self.calls.append((in_fmt, out_fmt))
        return (np.asarray(buf).reshape(-1).view(np.uint8), h, w, in_fmt, out, out_fmt, colour, color_range)

    def collect_u8(self, t):
        buf, h, w, in_fmt, out, out_fmt, colour, rng = t
        self.live -= 1
        full = rng == "pc"
        x = self.apply(ref.pix_to_bgr16(buf, in_fmt, h, w, colour, full), self.scale)
        out.reshape(-1).view(np.uint8)[...] = ref.bgr16_to_pix(x, out_fmt, colour, full)
        return out

    @staticmethod
    def apply(bgr16, scale):
        return np.minimum(np.repeat(np.repeat(bgr16.astype(np.int64), scale, 0), scale, 1) + 3, 65535).astype(np.uint16)


@pytest.mark.parametrize("in_fmt,out_fmt", [("yuv420p10le", "p010le"), ("p010le", "yuv420p10le"), ("bgr48le", "p010le"),
                                            ("bgr24", "bgr24"), ("yuv420p", "bgr48le")])
@pytest.mark.parametrize("nlanes", [1, 2])
def test_stream_bit_depth_16(in_fmt, out_fmt, nlanes):
    h, w = 5, 8
    pix = rawvideo.PixFormats(in_fmt, out_fmt, "bt709", "tv", bit_depth=16)
    rng = np.random.default_rng(4)
    frames = [ref.bgr16_to_pix(rng.integers(0, 65536, (h, w, 3), dtype=np.uint16), in_fmt, "bt709") for _ in range(9)]
    want = b"".join(ref.bgr16_to_pix(Pix16FakeNet.apply(ref.pix_to_bgr16(f, in_fmt, h, w, "bt709"), 2), out_fmt, "bt709").tobytes()
                    for f in frames)
    lanes = [[(Pix16FakeNet(2), 32)] for _ in range(nlanes)]
    fout = io.BytesIO()
    n = rawvideo.stream(io.BytesIO(b"".join(f.tobytes() for f in frames)), fout, h, w, lanes if nlanes > 1 else lanes[0],
                        alloc=lambda s: np.zeros(s, np.uint8), pix=pix)
    assert n == len(frames) and fout.getvalue() == want
    assert all(c == (in_fmt, out_fmt) for lane in lanes for net, _ in lane for c in net.calls)
