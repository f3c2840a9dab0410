"""The sited, interpolating 4:2:0 chroma modes without a GPU: the numpy restatement (chroma_ref.py)
against known answers, float64 and the replicate restatements; the quality ordering the modes exist for; ncnn.colour_word, the
streamer's options and stream() with a stand-in net that records its keyword arguments; what hipcc emits for the kernels."""
import io
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import chroma_ref as cr
import pixfmt16_ref as ref16
import pixfmt_ref as ref8
from upscale_video_amd import ncnn, rawvideo

COMBOS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]
SIZES = [(1, 1), (1, 2), (2, 1), (3, 5), (7, 40), (6, 9)]       # (h, w); the last: odd w, even h
# the weights section 7.5 states, per axis: up = {luma phase: {chroma offset: weight}} over `den`; down = taps around luma 2k
UP = {True: ({0: {0: 2}, 1: {0: 1, 1: 1}}, 2), False: ({0: {-1: 1, 0: 3}, 1: {0: 3, 1: 1}}, 4)}
DOWN = {True: ({-1: 1, 0: 2, 1: 1}, 4), False: ({0: 1, 1: 1}, 2)}


# ---- known answers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u16", [False, True])
@pytest.mark.parametrize("fmt", cr.YUV)
def test_flat_frame_converts_as_under_replicate(fmt, u16):
    """one colour: every mode gives replicate's bytes, both ways (the u16 route widens its sums, so it is identical too)"""
    rng = np.random.default_rng(5)
    for (h, w), (matrix, full) in zip(SIZES, itertools.cycle(COMBOS)):
        colour = rng.integers(0, 65536 if u16 else 256, 3)
        bgr = np.empty((h, w, 3), np.uint16 if u16 else np.uint8)
        bgr[...] = colour
        want = cr.bgr_to_pix(bgr, fmt, matrix, full, u16=u16)
        back = cr.pix_to_bgr(want, fmt, h, w, matrix, full, u16=u16)
        for loc in cr.SITINGS:
            assert np.array_equal(cr.bgr_to_pix(bgr, fmt, matrix, full, "bilinear", loc, u16), want), (h, w, loc)
            assert np.array_equal(cr.pix_to_bgr(want, fmt, h, w, matrix, full, "bilinear", loc, u16), back), (h, w, loc)


@pytest.mark.parametrize("loc", cr.SITINGS)
def test_impulse_responses_are_the_stated_weights(loc):
    hco, vco = cr.COSITED[loc]
    ch, cw, ky, kx = 5, 6, 2, 3
    imp = np.zeros((ch, cw), np.int64)
    imp[ky, kx] = 1
    got, dl = cr.upsample(imp, 2 * ch, 2 * cw, loc)
    (wy, dy), (wx, dx) = UP[vco], UP[hco]
    assert (1 << dl) == dy * dx == {"left": 8, "center": 16, "topleft": 4}[loc]
    want = np.zeros_like(got)
    for y in range(2 * ch):
        for x in range(2 * cw):
            want[y, x] = wy[y % 2].get(ky - y // 2, 0) * wx[x % 2].get(kx - x // 2, 0)
    assert np.array_equal(got, want) and got.sum() == 4 << dl
    # down: an impulse at luma (y, x) reaches chroma (k, j) with the tap weights around luma (2k, 2j)
    (ty, dy), (tx, dx) = DOWN[vco], DOWN[hco]
    for y, x in itertools.product(range(3, 7), range(3, 7)):
        imp = np.zeros((2 * ch, 2 * cw), np.int64)
        imp[y, x] = 1
        got, dl = cr.downsample(imp, loc)
        assert (1 << dl) == dy * dx and got.shape == (ch, cw)
        want = np.array([[ty.get(y - 2 * k, 0) * tx.get(x - 2 * j, 0) for j in range(cw)] for k in range(ch)])
        assert np.array_equal(got, want), (y, x)
    assert cr.downsample(np.ones((2 * ch, 2 * cw), np.int64), loc)[0].min() == 1 << dl      # the window: 3x2, 2x2 or 3x3


@pytest.mark.parametrize("loc", cr.SITINGS)
@pytest.mark.parametrize("h,w", SIZES)
def test_taps_beyond_the_edges_replicate(loc, h, w):
    """the plane padded by its own edge samples and filtered without clamping gives the same sums, at every edge and corner"""
    rng = np.random.default_rng(h * 100 + w)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    c = rng.integers(0, 1024, (ch, cw))
    got, dl = cr.upsample(c, h, w, loc)
    big, _ = cr.upsample(np.pad(c, 1, mode="edge"), 2 * ch + 4, 2 * cw + 4, loc)
    assert np.array_equal(got, big[2:2 + h, 2:2 + w])
    p = rng.integers(0, 65536, (h, w))
    got, dl = cr.downsample(p, loc)
    big, _ = cr.downsample(np.pad(p, ((2, 2 + h % 2), (2, 2 + w % 2)), mode="edge"), loc)
    assert got.shape == (ch, cw) and np.array_equal(got, big[1:1 + ch, 1:1 + cw])


# ---- within one code of float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("u16", [False, True])
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("matrix,full", COMBOS)
def test_inverse_is_within_one_code_of_float64(matrix, full, depth, u16):
    """every Y' of a 33-step grid x every four-sample chroma neighbourhood of a 6-level grid (Cb) with three Cr patterns, at
    every phase and edge position of each siting; the restatement asserts that every partial sum fits its accumulator"""
    maxv = (1 << depth) - 1
    lv = np.linspace(0, maxv, 6).astype(np.int64)
    nb = np.stack(np.meshgrid(lv, lv, lv, lv, indexing="ij"), 0).reshape(2, 2, -1)          # [2][2][N] chroma planes
    ys = np.unique(np.concatenate([np.linspace(0, maxv, 33).astype(np.int64), [16 << (depth - 8), 235 << (depth - 8)]]))
    vmax = 65535 if u16 else 255
    for loc in cr.SITINGS:
        us, dl = cr.upsample(nb, 4, 4, loc)
        for vplanes in (maxv - nb, nb[::-1, ::-1], np.roll(nb, 1, axis=2)):
            vs, _ = cr.upsample(vplanes, 4, 4, loc)
            got = cr.inv_pixel(ys[:, None, None, None], us[None], vs[None], dl, matrix, full, depth, u16)
            want = cr.float_inv_pixel(ys[:, None, None, None], us[None], vs[None], dl, matrix, full, depth, u16)
            for fixed, flt in zip(got, want):
                assert np.abs(fixed - np.clip(flt, 0, vmax)).max() <= 1.0, (loc, matrix, full, depth, u16)


def _windows(rng, n, top):
    """n random 3x3 windows of (r, g, b), a quarter of them with extreme samples only"""
    p = rng.integers(0, top + 1, (3, 3, 3, n))
    p[..., : n // 4] = rng.integers(0, 2, (3, 3, 3, n // 4)) * top
    return p


@pytest.mark.parametrize("u16", [False, True])
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("matrix,full", COMBOS)
def test_forward_is_within_one_code_of_float64(matrix, full, depth, u16):
    """every 8-bit BGR value as a flat window (widened for the u16 route), and a seeded sweep of 10^6 random windows, for the
    three sitings; partial sums asserted by the restatement"""
    maxv = (1 << depth) - 1
    k = 257 if u16 else 1
    for loc in cr.SITINGS:
        dl = cr.downsample(np.zeros((4, 4), np.int64), loc)[1]
        for lo in range(0, 1 << 24, 1 << 22):
            a = np.arange(lo, lo + (1 << 22), dtype=np.int64)
            r, g, b = ((a >> 16) * k) << dl, (((a >> 8) & 255) * k) << dl, ((a & 255) * k) << dl
            got = cr.fwd_chroma(r, g, b, dl, matrix, full, depth, u16)
            want = cr.float_fwd_chroma(r, g, b, dl, matrix, full, depth, u16)
            for fixed, flt in zip(got, want):
                assert np.abs(fixed - np.clip(flt, 0, maxv)).max() <= 1.0, (loc, lo)
            if lo == 0:       # (a flat window is the block of sections 7.3 / 7.4: the same code)
                old = (ref16 if u16 else ref8).fwd_chroma(r >> dl, g >> dl, b >> dl, 0, matrix, full, depth)
                assert all(np.array_equal(x, y) for x, y in zip(got, old))
        win = _windows(np.random.default_rng(11), 10 ** 6, 65535 if u16 else 255)
        (ty, _), (tx, _) = DOWN[cr.COSITED[loc][1]], DOWN[cr.COSITED[loc][0]]      # the window's weights, rows / columns -1 .. 1
        sums = [sum(wy * wx * win[c, 1 + oy, 1 + ox] for oy, wy in ty.items() for ox, wx in tx.items()) for c in range(3)]
        got = cr.fwd_chroma(*sums, dl, matrix, full, depth, u16)
        want = cr.float_fwd_chroma(*sums, dl, matrix, full, depth, u16)
        for fixed, flt in zip(got, want):
            assert np.abs(fixed - np.clip(flt, 0, maxv)).max() <= 1.0, loc


def test_worst_case_sums():
    """section 7.5's bounds: on the u8 route 16 times the worst sums of section 7.3 stay inside int32 (the restatement's
    assertions hold at the extremes); on the u16 route they pass 2^31, which is why that route adds in int64"""
    for (matrix, full), depth, loc in itertools.product(COMBOS, (8, 10), cr.SITINGS):
        maxv = (1 << depth) - 1
        dl_up = cr.upsample(np.zeros((2, 2), np.int64), 4, 4, loc)[1]
        dl_dn = cr.downsample(np.zeros((4, 4), np.int64), loc)[1]
        ext = np.array([0, maxv], np.int64) << dl_up
        y, u, v = np.meshgrid(np.array([0, maxv]), ext, ext, indexing="ij")
        rgb = np.meshgrid(*([np.array([0, 255], np.int64) << dl_dn] * 3), indexing="ij")
        cr.inv_pixel(y, u, v, dl_up, matrix, full, depth)                   # (asserts int32 inside)
        cr.fwd_chroma(*rgb, dl_dn, matrix, full, depth)
        cr.inv_pixel(y, u, v, dl_up, matrix, full, depth, u16=True)         # (asserts int64 inside)
        cr.fwd_chroma(*[t * 257 for t in rgb], dl_dn, matrix, full, depth, u16=True)
    # u16, 10-bit full range, a pure blue 3x3 window: Cb's sum no longer fits int32
    _, (ur, ug, ub), _, _, coff, _ = ref16.fwd_coefs("bt601", True, 10)
    assert ub * 16 * 65535 + (coff << (ref16.FWD_SH + 4)) > 2 ** 31
    ky = ref16.inv_coefs("bt601", False, 10)[0]
    assert ky * (1023 - 64) * 16 > 2 ** 31


# ---- the replicate path is unchanged ------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
def test_replicate_is_the_earlier_restatements(h, w):
    rng = np.random.default_rng(h * 64 + w)
    for (matrix, full), fmt in itertools.product(COMBOS, cr.YUV):
        bgr8 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        bgr16 = rng.integers(0, 65536, (h, w, 3), dtype=np.uint16)
        f8 = cr.bgr_to_pix(bgr8, fmt, matrix, full)
        f16 = cr.bgr_to_pix(bgr16, fmt, matrix, full, u16=True)
        assert np.array_equal(f8, ref16.bgr_to_pix8(bgr8, fmt, matrix, full))
        assert np.array_equal(f16, ref16.bgr16_to_pix(bgr16, fmt, matrix, full))
        if fmt in ref8.FORMATS:
            assert np.array_equal(f8, ref8.bgr_to_pix(bgr8, fmt, matrix, full))
            assert np.array_equal(cr.pix_to_bgr(f8, fmt, h, w, matrix, full), ref8.pix_to_bgr(f8, fmt, h, w, matrix, full))
        assert np.array_equal(cr.pix_to_bgr(f8, fmt, h, w, matrix, full), ref16.pix_to_bgr8(f8, fmt, h, w, matrix, full))
        assert np.array_equal(cr.pix_to_bgr(f16, fmt, h, w, matrix, full, u16=True), ref16.pix_to_bgr16(f16, fmt, h, w, matrix, full))
        other = "nv12" if fmt != "nv12" else "p010le"
        assert np.array_equal(cr.convert(f8, fmt, other, h, w, matrix, full), ref16.convert8(f8, fmt, other, h, w, matrix, full))
        assert np.array_equal(cr.convert(f16, fmt, other, h, w, matrix, full, bit_depth=16),
                              ref16.convert16(f16, fmt, other, h, w, matrix, full))
        # center's forward filter is the box on both axes: the same bytes as replicate going out
        assert np.array_equal(cr.bgr_to_pix(bgr8, fmt, matrix, full, "bilinear", "center"), f8)
        assert np.array_equal(cr.bgr_to_pix(bgr16, fmt, matrix, full, "bilinear", "center", u16=True), f16)


# ---- quality: the point of the change -------------------------------------------------------------------------------------
def quality_table(u16=False):
    """{source siting: {mode: RGB PSNR}} of the edges frame downsampled with the siting's forward filter and brought back"""
    truth = cr.edges_frame()
    h, w, _ = truth.shape
    t = truth.astype(np.uint16) * 257 if u16 else truth
    table = {}
    for src in cr.SITINGS:
        f = cr.bgr_to_pix(t, "yuv420p", "bt601", False, "bilinear", src, u16)
        table[src] = {m: cr.psnr(cr.pix_to_bgr(f, "yuv420p", h, w, "bt601", False, m[0], m[1], u16), t, 65535.0 if u16 else 255.0)
                      for m in cr.MODES}
    return table


@pytest.mark.parametrize("u16", [False, True])
def test_matched_bilinear_beats_replicate_on_edges(u16):
    table = quality_table(u16)
    for src in cr.SITINGS:
        print("source %-7s" % src, "  ".join("%s/%s %.2f dB" % (m[0], m[1], v) for m, v in table[src].items()))
    for src in cr.SITINGS:
        assert table[src][("bilinear", src)] > table[src][("replicate", "left")], (src, table[src])
    assert table["left"][("bilinear", "left")] > table["left"][("bilinear", "center")], table["left"]


# ---- Python interface and command line -------------------------------------------------------------------------------------
def test_colour_word():
    assert [ncnn.colour_word(c, r) for c in ("bt601", "bt709") for r in ("tv", "pc")] == [0, 2, 1, 3]
    assert ncnn.colour_word("bt601", "tv", "replicate", "left") == 0
    assert ncnn.colour_word("bt601", "tv", "bilinear") == 4 and ncnn.colour_word("bt709", "pc", "bilinear", "left") == 7
    assert ncnn.colour_word("bt601", "tv", "bilinear", "center") == 12 and ncnn.colour_word("bt709", "tv", "bilinear", "topleft") == 21
    for bad in (("bt601", "tv", "bicubic", "left"), ("bt601", "tv", "bilinear", "top"), ("bt601", "tv", "replicate", "center")):
        with pytest.raises(ValueError):
            ncnn.colour_word(*bad)
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "uva.h")).read()
    for name, bit in (("UVA_CHROMA_BILINEAR", 4), ("UVA_CHROMA_CENTER", 8), ("UVA_CHROMA_TOPLEFT", 16)):
        assert re.search(r"#define %s %d\b" % (name, bit), hdr)
    assert (ncnn.CHROMA_FILTERS["bilinear"], ncnn.CHROMA_LOCS["center"], ncnn.CHROMA_LOCS["topleft"]) == (4, 8, 16)


def test_cli_chroma_options(capsys):
    for argv, msg in ((["--chroma-loc", "center"], "--chroma-loc needs --chroma-filter bilinear"),
                      (["--chroma-loc", "left"], "--chroma-loc needs --chroma-filter bilinear"),
                      (["--chroma-filter", "replicate", "--chroma-loc", "topleft"], "--chroma-loc needs --chroma-filter bilinear"),
                      (["--chroma-filter", "bicubic"], "invalid choice"),
                      (["--chroma-filter", "bilinear", "--chroma-loc", "bottom"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            rawvideo.main(["-W", "8", "-H", "8"] + argv)
        assert e.value.code == 2 and msg in capsys.readouterr().err, argv
    with pytest.raises(ValueError):
        rawvideo.PixFormats("yuv420p", "nv12", chroma_loc="center")
    assert rawvideo.PixFormats("yuv420p", "nv12").chroma_kw() == {}
    assert rawvideo.PixFormats("yuv420p", "nv12", chroma_filter="bilinear").chroma_kw() == {"chroma_filter": "bilinear", "chroma_loc": "left"}


class ChromaFakeNet:
    """Net.submit_pix / collect_u8 stand-in that records its keyword arguments: the restated conversions around
    nearest-neighbour upscale + 1, finished only at collect time"""

    def __init__(self, scale):
        self.scale, self.live, self.kwargs = scale, 0, []

    def submit_u8(self, img, out=None, tile_size=0, border=0):
        raise AssertionError("Y'CbCr frames go through submit_pix")

    def submit_pix(self, buf, h, w, in_fmt, out=None, out_fmt="bgr24", colour="bt601", color_range="tv", tile_size=0, border=0, **kw):
        assert self.live < 3 and set(kw) <= {"bit_depth", "chroma_filter", "chroma_loc"}
        self.live += 1
        self.kwargs.append(dict(kw))
        return (buf, h, w, in_fmt, out, out_fmt, colour, color_range, kw)

    def collect_u8(self, t):
        buf, h, w, in_fmt, out, out_fmt, colour, rng, kw = t
        self.live -= 1
        out.reshape(-1).view(np.uint8)[...] = through(buf, h, w, in_fmt, out_fmt, colour, rng == "pc", self.scale, **kw)
        return out


def through(buf, h, w, in_fmt, out_fmt, matrix, full, scale, bit_depth=8, chroma_filter="replicate", chroma_loc="left"):
    u16 = bit_depth == 16
    x = cr.pix_to_bgr(buf, in_fmt, h, w, matrix, full, chroma_filter, chroma_loc, u16)
    x = np.repeat(np.repeat(x, scale, 0), scale, 1) + 1
    return np.asarray(cr.bgr_to_pix(x, out_fmt, matrix, full, chroma_filter, chroma_loc, u16)).reshape(-1).view(np.uint8)


@pytest.mark.parametrize("bit_depth", [8, 16])
@pytest.mark.parametrize("nlanes", [1, 2])
@pytest.mark.parametrize("mode", cr.MODES + ((None, None),))
def test_stream_passes_the_chroma_mode_exactly_when_given(mode, nlanes, bit_depth):
    h, w, n = 5, 7, 9
    in_fmt, out_fmt = ("p010le", "yuv420p10le") if bit_depth == 16 else ("yuv420p", "p010le")
    given = {} if mode[0] is None else {"chroma_filter": mode[0], "chroma_loc": mode[1]}
    pix = rawvideo.PixFormats(in_fmt, out_fmt, "bt709", "tv", bit_depth, **given)
    rng = np.random.default_rng(9)
    frames = [rng.integers(0, 256, ncnn.pix_frame_bytes(in_fmt, h, w), dtype=np.uint8) for _ in range(n)]
    lanes = [[(ChromaFakeNet(2), 32)] for _ in range(nlanes)]
    fout = io.BytesIO()
    got_n = rawvideo.stream(io.BytesIO(b"".join(f.tobytes() for f in frames)), fout, h, w, lanes if nlanes > 1 else lanes[0],
                            alloc=lambda s: np.zeros(s, np.uint8), pix=pix)
    want_kw = dict({"bit_depth": 16} if bit_depth == 16 else {}, **({} if mode[0] in (None, "replicate") else given))
    calls = [kw for lane in lanes for kw in lane[0][0].kwargs]
    assert got_n == n and len(calls) == n and all(kw == want_kw for kw in calls), calls
    fb = ncnn.pix_frame_bytes(out_fmt, 2 * h, 2 * w)
    out = fout.getvalue()
    assert len(out) == n * fb
    for k, f in enumerate(frames):
        want = through(f, h, w, in_fmt, out_fmt, "bt709", False, 2, **want_kw)
        assert out[k * fb:(k + 1) * fb] == want.tobytes(), k


def test_scale_1_and_denoise_stage_pass_the_mode_on(tmp_path, monkeypatch):
    """`-s 1` converts every frame once with the mode; a leading denoise stage converts with it at both of its ends"""
    h, w = 6, 9
    calls = []

    def fake_convert(buf, hh, ww, fi, fo, colour="bt601", color_range="tv", out=None, gpu=0, **kw):
        calls.append((fi, fo, dict(kw)))
        out.reshape(-1).view(np.uint8)[...] = cr.convert(buf, fi, fo, hh, ww, colour, color_range == "pc", **kw)
        return out
    monkeypatch.setattr(ncnn, "convert_pix", fake_convert)
    rng = np.random.default_rng(2)
    fb = ncnn.pix_frame_bytes("nv12", h, w)
    data = rng.integers(0, 256, 3 * fb, dtype=np.uint8).tobytes()
    src, dst = tmp_path / "in.nv12", tmp_path / "out.yuv"
    src.write_bytes(data)
    for argv, kw in (([], {}), (["--chroma-filter", "bilinear"], {"chroma_filter": "bilinear", "chroma_loc": "left"}),
                     (["--chroma-filter", "bilinear", "--chroma-loc", "topleft", "--bit-depth", "16"],
                      {"chroma_filter": "bilinear", "chroma_loc": "topleft", "bit_depth": 16})):
        del calls[:]
        assert rawvideo.main(["-i", str(src), "-o", str(dst), "-W", str(w), "-H", str(h), "-s", "1", "--in-pix-fmt", "nv12",
                              "--out-pix-fmt", "yuv420p10le"] + argv) == 0
        assert calls == [("nv12", "yuv420p10le", kw)] * 3, calls
        want = b"".join(cr.convert(np.frombuffer(data[k * fb:(k + 1) * fb], np.uint8), "nv12", "yuv420p10le", h, w, **kw).tobytes()
                        for k in range(3))
        assert dst.read_bytes() == want
    # the denoise stage: uva_denoise_u8 stood in by 255 - x
    import ctypes
    from upscale_video_amd import _lib

    class FakeLib:
        def uva_denoise_u8(self, gpu, src, hh, ww, sstride, dst, dstride, s_luma, s_colour):
            assert sstride == dstride == 3 * ww
            arr = lambda p: np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (hh * ww * 3,))   # noqa: E731
            arr(dst)[...] = 255 - arr(src)
            return 0
    monkeypatch.setattr(_lib, "load", lambda: FakeLib())
    monkeypatch.setattr(_lib, "check", lambda rc: None)
    pix = rawvideo.PixFormats("nv12", "yuv420p", chroma_filter="bilinear", chroma_loc="center")
    del calls[:]
    st = rawvideo.DenoiseStage(0, 5, h, w, lambda s: np.zeros(s, np.uint8), in_fmt="nv12", out_fmt="yuv420p", pix=pix)
    st.submit(np.frombuffer(data[:fb], np.uint8))
    res = st.collect()
    kw = {"chroma_filter": "bilinear", "chroma_loc": "center"}
    assert calls == [("nv12", "bgr24", kw), ("bgr24", "yuv420p", kw)]
    bgr = 255 - cr.pix_to_bgr(np.frombuffer(data[:fb], np.uint8), "nv12", h, w, chroma_filter="bilinear", chroma_loc="center")
    assert np.array_equal(res.reshape(-1), cr.bgr_to_pix(bgr, "yuv420p", chroma_filter="bilinear", chroma_loc="center"))


# ---- what hipcc emits ------------------------------------------------------------------------------------------------------
def test_interpolating_kernels_have_no_scratch(tmp_path):
    """uva_pixfmt.hip cross-compiled for gfx950: 4 formats x 2 access paths x 2 sample types x 4 modes of both kernels, none with
    scratch; the VGPR ranges section 7.5 quotes"""
    from upscale_video_amd import build
    asm = str(tmp_path / "pixfmt.s")
    cmd = [build.hipcc()] + [f for f in build.FLAGS if f != "-fPIC"] + ["-S", "--cuda-device-only", os.path.join(build.CSRC, "uva_pixfmt.hip"),
                                                                       "-o", asm]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(asm).read()
    info = {}
    for m in re.finditer(r"^_ZN3uva\w*pix_(to|from)_bgrILi(\d)ELb([01])E([ht])Li(\d)E\w*:", text, flags=re.M):
        seg = text[m.end():]
        scratch = int(re.search(r"; ScratchSize: (\d+)", seg).group(1))
        vgpr = int(re.search(r"; NumVgprs: (\d+)", seg).group(1))
        info[(m.group(1), int(m.group(5)), m.group(4), int(m.group(3)), int(m.group(2)))] = (scratch, vgpr)
    assert len(info) == 2 * 4 * 2 * 2 * 4, sorted(info)
    assert all(s == 0 for s, _ in info.values()), {k: v for k, v in info.items() if v[0]}
    for way in ("to", "from"):
        for mode in range(4):
            v = [vg for (wy, md, _, _, _), (_, vg) in info.items() if wy == way and md == mode]
            print("pix_%s_bgr mode %d: %d-%d VGPRs" % (way, mode, min(v), max(v)))
            assert max(v) <= 128        # at least four waves per SIMD
