"""The 4:2:2 formats yuv422p / yuv422p10le without a GPU: codes and sizes, the numpy restatement
(pix422_ref.py) tied to the 4:2:0 restatements it is built from, its accumulators, float64, what 4:2:2 buys over 4:2:0 on the
edges frame, stream() with a stand-in net, the command line, and what hipcc emits for the new kernels."""
import io
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import chroma_ref as cr
import pix422_ref as p422
import pixfmt16_ref as ref16
from upscale_video_amd import ncnn, rawvideo

COMBOS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]
TWIN = {"yuv422p": "yuv420p", "yuv422p10le": "yuv420p10le"}


# ---- codes and sizes ---------------------------------------------------------------------------------------------------
def test_codes_and_sizes(uva):
    from upscale_video_amd import _lib
    L = _lib.load()
    assert ncnn.PIX_FORMATS_ALL["yuv422p"] == 7 and ncnn.PIX_FORMATS_ALL["yuv422p10le"] == 8
    assert list(ncnn.PIX_FORMATS) == ["bgr24", "yuv420p", "nv12", "p010le"] and ncnn.PIX16_ONLY == ("bgr48le",)
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "uva.h")).read()
    assert re.search(r"#define UVA_PIX_YUV422P 7\b", hdr) and re.search(r"#define UVA_PIX_YUV422P10LE 8\b", hdr)
    assert re.search(r"#define UVA_ABI_VERSION 15\b", hdr)
    for h, w in ((1, 1), (3, 5), (1080, 1920)):
        cw = (w + 1) // 2
        for fmt, code, bps in (("yuv422p", 7, 1), ("yuv422p10le", 8, 2)):
            n = (w * h + 2 * cw * h) * bps
            assert ncnn.pix_frame_bytes(fmt, h, w) == n == p422.frame_bytes(fmt, h, w) == L.uva_pix_frame_bytes(code, h, w)
            e = ncnn.pix_empty(fmt, h, w)
            assert e.dtype == np.uint8 and e.shape == (n,)
    assert L.uva_pix_frame_bytes(4, 8, 8) == 0 and L.uva_pix_frame_bytes(9, 8, 8) == 0
    assert L.uva_pix_frame_bytes(7, 0, 8) == 0 and L.uva_pix_frame_bytes(8, 8, -1) == 0
    with pytest.raises(ValueError):
        ncnn.pix_frame_bytes("yuv444p", 8, 8)


# ---- ties to the 4:2:0 definition ------------------------------------------------------------------------------------------
def _same_chroma_rows(f422, fmt, f420, h, w):
    """Y' equal, and chroma rows 2k, 2k + 1 of the 4:2:2 frame both equal row k of the 4:2:0 one"""
    y2, u2, v2 = p422.planes(f422, fmt, h, w)
    y0, u0, v0 = ref16.planes(f420, TWIN[fmt], h, w)
    return np.array_equal(y2, y0) and all(np.array_equal(a, np.repeat(b, 2, 0)[:h]) for a, b in ((u2, u0), (v2, v0)))


@pytest.mark.parametrize("u16", [False, True])
@pytest.mark.parametrize("fmt", p422.FORMATS422)
@pytest.mark.parametrize("h,w", [(2, 2), (4, 5), (6, 16), (8, 23)])
def test_ties_to_the_420_restatements(h, w, fmt, u16):
    rng = np.random.default_rng(h * 100 + w + u16)
    top, dt = (65536, np.uint16) if u16 else (256, np.uint8)
    cw = (w + 1) // 2
    for matrix, full in COMBOS:
        # replicate: rows (BGR going out, chroma coming in) duplicated in pairs
        bgr = np.repeat(rng.integers(0, top, (h // 2, w, 3), dtype=dt), 2, 0)
        assert _same_chroma_rows(p422.bgr_to_pix(bgr, fmt, matrix, full, u16=u16), fmt, cr.bgr_to_pix(bgr, TWIN[fmt], matrix, full, u16=u16), h, w)
        maxv = (1 << p422.depth_of(fmt)) - 1
        y = rng.integers(0, maxv + 1, (h, w))
        u, v = (rng.integers(0, maxv + 1, (h // 2, cw)) for _ in range(2))
        f2, f0 = p422.pack(fmt, y, np.repeat(u, 2, 0), np.repeat(v, 2, 0)), ref16.pack(TWIN[fmt], y, u, v)
        assert np.array_equal(p422.pix_to_bgr(f2, fmt, h, w, matrix, full, u16=u16), cr.pix_to_bgr(f0, TWIN[fmt], h, w, matrix, full, u16=u16))
        # bilinear, all three sitings: every row equal
        bgr = np.repeat(rng.integers(0, top, (1, w, 3), dtype=dt), h, 0)
        y = np.repeat(rng.integers(0, maxv + 1, (1, w)), h, 0)
        u, v = (rng.integers(0, maxv + 1, (1, cw)) for _ in range(2))
        f2 = p422.pack(fmt, y, np.repeat(u, h, 0), np.repeat(v, h, 0))
        f0 = ref16.pack(TWIN[fmt], y, np.repeat(u, h // 2, 0), np.repeat(v, h // 2, 0))
        for loc in cr.SITINGS:
            kw = dict(chroma_filter="bilinear", chroma_loc=loc, u16=u16)
            assert _same_chroma_rows(p422.bgr_to_pix(bgr, fmt, matrix, full, **kw), fmt, cr.bgr_to_pix(bgr, TWIN[fmt], matrix, full, **kw), h, w), loc
            assert np.array_equal(p422.pix_to_bgr(f2, fmt, h, w, matrix, full, **kw), cr.pix_to_bgr(f0, TWIN[fmt], h, w, matrix, full, **kw)), loc


@pytest.mark.parametrize("u16", [False, True])
@pytest.mark.parametrize("fmt", p422.FORMATS422)
def test_left_is_topleft_and_flat_is_replicate(fmt, u16):
    rng = np.random.default_rng(3 + u16)
    top, dt = (65536, np.uint16) if u16 else (256, np.uint8)
    for (h, w), (matrix, full) in zip([(1, 1), (1, 2), (2, 3), (3, 5), (5, 8), (4, 24)], itertools.cycle(COMBOS)):
        bgr = rng.integers(0, top, (h, w, 3), dtype=dt)
        f = p422.random_frame(rng, fmt, h, w)
        a, b = (dict(chroma_filter="bilinear", chroma_loc=loc, u16=u16) for loc in ("left", "topleft"))
        assert np.array_equal(p422.bgr_to_pix(bgr, fmt, matrix, full, **a), p422.bgr_to_pix(bgr, fmt, matrix, full, **b))
        assert np.array_equal(p422.pix_to_bgr(f, fmt, h, w, matrix, full, **a), p422.pix_to_bgr(f, fmt, h, w, matrix, full, **b))
        flat = np.empty((h, w, 3), dt)
        flat[...] = rng.integers(0, top, 3)
        want = p422.bgr_to_pix(flat, fmt, matrix, full, u16=u16)
        back = p422.pix_to_bgr(want, fmt, h, w, matrix, full, u16=u16)
        for loc in cr.SITINGS:
            assert np.array_equal(p422.bgr_to_pix(flat, fmt, matrix, full, "bilinear", loc, u16), want), (h, w, loc)
            assert np.array_equal(p422.pix_to_bgr(want, fmt, h, w, matrix, full, "bilinear", loc, u16), back), (h, w, loc)
        # the 10-bit format ignores the high six bits coming in and writes them as zero
        if fmt == "yuv422p10le":
            clean = (f.view("<u2") & 1023).astype("<u2").view(np.uint8)
            assert np.array_equal(p422.pix_to_bgr(f, fmt, h, w, matrix, full, u16=u16), p422.pix_to_bgr(clean, fmt, h, w, matrix, full, u16=u16))
            assert (want.view("<u2") >> 10).max() == 0
        # equal formats are a copy; another format goes through BGR
        assert np.array_equal(p422.convert(f, fmt, fmt, h, w), f)
        assert p422.convert(f, fmt, "nv12", h, w, bit_depth=16 if u16 else 8).size == ref16.frame_bytes("nv12", h, w)


# ---- accumulators ------------------------------------------------------------------------------------------------------------
def test_every_partial_sum_fits_its_accumulator():
    """the extremes of every sum, in the kernels' order (the restatement asserts inside): int32 holds all of them but the u16
    inverse of the interpolating modes -- section 7.4's 2^13 scale times 2 or 4 passes 2^31 there, which is why it is int64"""
    for (matrix, full), depth in itertools.product(COMBOS, (8, 10)):
        maxv = (1 << depth) - 1
        for u16 in (False, True):
            top = 65535 if u16 else 255
            rgb = np.meshgrid(*([np.array([0, top], np.int64)] * 3), indexing="ij")
            p422.fwd_luma(*rgb, matrix, full, depth, u16)
            for dl in (0, 1, 2):         # a lone pixel, the pair / [1 1], [1 2 1]
                p422.fwd_chroma(*[t << dl for t in rgb], dl, matrix, full, depth, u16)
            y, u, v = np.meshgrid(*([np.array([0, maxv], np.int64)] * 3), indexing="ij")
            p422.inv_pixel_replicate(y, u, v, matrix, full, depth, u16)
            for dl in (1, 2):
                p422.inv_pixel(y, u << dl, v << dl, dl, matrix, full, depth, u16)
    ky, _, _, _, bu, _, _ = ref16.inv_coefs("bt601", False, 10)
    assert (ky * (1023 - 64) + bu * (1023 - 512)) * 2 > 2 ** 31            # the u16 inverse, co-sited: white Y' under full Cb
    _, _, (vr, _, _), _, coff, _ = ref16.fwd_coefs("bt601", True, 10)
    assert vr * 4 * 65535 + (coff << (ref16.FWD_SH + 2)) + (1 << (ref16.FWD_SH + 1)) < 2 ** 31      # the u16 forward [1 2 1]: it fits


# ---- within one code of float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u16", [False, True])
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("matrix,full", COMBOS)
def test_inverse_is_within_one_code_of_float64(matrix, full, depth, u16):
    """every Y' of a 33-step grid x every row of four chroma samples of a 6-level grid (Cb) with three Cr patterns, upsampled to
    eight luma positions: every phase and both edges of each mode"""
    maxv = (1 << depth) - 1
    lv = np.linspace(0, maxv, 6).astype(np.int64)
    nb = np.stack(np.meshgrid(lv, lv, lv, lv, indexing="ij"), -1).reshape(-1, 4)             # [N][4]: N chroma rows
    ys = np.unique(np.concatenate([np.linspace(0, maxv, 33).astype(np.int64), [16 << (depth - 8), 235 << (depth - 8)]]))
    vmax = 65535 if u16 else 255
    for vrows in (maxv - nb, nb[:, ::-1], np.roll(nb, 1, axis=0)):
        got = p422.inv_pixel_replicate(ys[:, None, None], np.repeat(nb, 2, 1)[None], np.repeat(vrows, 2, 1)[None], matrix, full, depth, u16)
        want = p422.float_inv_pixel(ys[:, None, None], np.repeat(nb, 2, 1)[None], np.repeat(vrows, 2, 1)[None], 0, matrix, full, depth, u16)
        for fixed, flt in zip(got, want):
            assert np.abs(fixed - np.clip(flt, 0, vmax)).max() <= 1.0, ("replicate", matrix, full, depth, u16)
        for hco in (True, False):
            us, dl = cr.up_axis(nb, 8, hco, 1)
            vs, _ = cr.up_axis(vrows, 8, hco, 1)
            got = p422.inv_pixel(ys[:, None, None], us[None], vs[None], dl, matrix, full, depth, u16)
            want = p422.float_inv_pixel(ys[:, None, None], us[None], vs[None], dl, matrix, full, depth, u16)
            for fixed, flt in zip(got, want):
                assert np.abs(fixed - np.clip(flt, 0, vmax)).max() <= 1.0, (hco, matrix, full, depth, u16)


@pytest.mark.parametrize("u16", [False, True])
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("matrix,full", COMBOS)
def test_forward_is_within_one_code_of_float64(matrix, full, depth, u16):
    """every 8-bit BGR value as a flat window (widened for the u16 route) and a seeded sweep of 10^6 random windows, under the
    weights of a lone pixel, the pair / [1 1] and [1 2 1]"""
    maxv = (1 << depth) - 1
    k = 257 if u16 else 1
    win = np.random.default_rng(11).integers(0, (65535 if u16 else 255) + 1, (3, 3, 10 ** 6))       # [channel][tap][N]
    win[..., : 250000] = np.random.default_rng(12).integers(0, 2, (3, 3, 250000)) * (65535 if u16 else 255)
    for dl, weights in ((0, (0, 1, 0)), (1, (0, 1, 1)), (2, (1, 2, 1))):
        for lo in range(0, 1 << 24, 1 << 22):
            a = np.arange(lo, lo + (1 << 22), dtype=np.int64)
            r, g, b = ((a >> 16) * k) << dl, (((a >> 8) & 255) * k) << dl, ((a & 255) * k) << dl
            got = p422.fwd_chroma(r, g, b, dl, matrix, full, depth, u16)
            want = p422.float_fwd_chroma(r, g, b, dl, matrix, full, depth, u16)
            for fixed, flt in zip(got, want):
                assert np.abs(fixed - np.clip(flt, 0, maxv)).max() <= 1.0, (dl, lo)
        sums = [sum(wt * win[c, t] for t, wt in enumerate(weights)) for c in range(3)]
        got = p422.fwd_chroma(*sums, dl, matrix, full, depth, u16)
        want = p422.float_fwd_chroma(*sums, dl, matrix, full, depth, u16)
        for fixed, flt in zip(got, want):
            assert np.abs(fixed - np.clip(flt, 0, maxv)).max() <= 1.0, dl


# ---- what it buys ------------------------------------------------------------------------------------------------------------
def round_trip_table():
    """{mode: (RGB PSNR through yuv422p, through yuv420p)} of the edges frame, BT.601 tv, 8 bits, forward then inverse"""
    truth = cr.edges_frame()
    h, w, _ = truth.shape
    table = {}
    for m in cr.MODES:
        f2 = p422.bgr_to_pix(truth, "yuv422p", "bt601", False, *m)
        f0 = cr.bgr_to_pix(truth, "yuv420p", "bt601", False, *m)
        table[m] = (cr.psnr(p422.pix_to_bgr(f2, "yuv422p", h, w, "bt601", False, *m), truth),
                    cr.psnr(cr.pix_to_bgr(f0, "yuv420p", h, w, "bt601", False, *m), truth))
    return table


def test_a_422_round_trip_keeps_3_db_over_420():
    table = round_trip_table()
    for m, (a, b) in table.items():
        print("%-9s %-7s through 4:2:2 %.2f dB, through 4:2:0 %.2f dB" % (m[0], m[1] if m[0] == "bilinear" else "", a, b))
    for m, (a, b) in table.items():
        assert a >= b + 3.0, (m, a, b)


# ---- the streamer and the command line ------------------------------------------------------------------------------------
class Pix422FakeNet:
    """Net.submit_pix / collect_u8 stand-in: the restated conversions (pix422_ref) around a nearest-neighbour upscale + 3
    (saturating), finished only at collect time (buffer reuse mistakes show up)"""

    def __init__(self, scale):
        self.scale, self.live, self.calls = scale, 0, []

    def submit_u8(self, *a, **k):
        raise AssertionError("a pixel format on either end must go through submit_pix")

    def submit_pix(self, buf, h, w, in_fmt, out=None, out_fmt="bgr24", colour="bt601", color_range="tv", tile_size=0, border=0,
                   bit_depth=8, chroma_filter="replicate", chroma_loc="left"):
        assert self.live < 3
        assert np.asarray(buf).nbytes == p422.frame_bytes(in_fmt, h, w)
        assert out.nbytes == p422.frame_bytes(out_fmt, h * self.scale, w * self.scale)
        self.live += 1
        self.calls.append((in_fmt, out_fmt, bit_depth))
        return (np.asarray(buf).reshape(-1).view(np.uint8), h, w, in_fmt, out, out_fmt, colour, color_range == "pc", bit_depth == 16,
                chroma_filter, chroma_loc)

    def collect_u8(self, t):
        buf, h, w, in_fmt, out, out_fmt, colour, full, u16, filt, loc = t
        self.live -= 1
        x = self.apply(p422.pix_to_bgr(buf, in_fmt, h, w, colour, full, filt, loc, u16), self.scale)
        out.reshape(-1).view(np.uint8)[...] = p422.bgr_to_pix(x, out_fmt, colour, full, filt, loc, u16)
        return out

    @staticmethod
    def apply(bgr, scale):
        top = 65535 if bgr.dtype == np.uint16 else 255
        return np.minimum(np.repeat(np.repeat(bgr.astype(np.int64), scale, 0), scale, 1) + 3, top).astype(bgr.dtype)


@pytest.mark.parametrize("in_fmt,out_fmt,bit_depth,mode", [
    ("yuv422p", "yuv420p", 8, ("replicate", "left")), ("nv12", "yuv422p", 8, ("bilinear", "center")),
    ("yuv422p10le", "p010le", 16, ("bilinear", "left")), ("yuv420p10le", "yuv422p10le", 16, ("replicate", "left")),
    ("yuv422p10le", "yuv422p", 8, ("bilinear", "topleft"))])
@pytest.mark.parametrize("nlanes", [1, 2])
def test_stream_with_a_stand_in_net(in_fmt, out_fmt, bit_depth, mode, nlanes):
    h, w = 5, 7
    pix = rawvideo.PixFormats(in_fmt, out_fmt, "bt709", "tv", bit_depth=bit_depth, chroma_filter=mode[0], chroma_loc=mode[1])
    assert pix.frame_bytes(h, w) == p422.frame_bytes(in_fmt, h, w) and pix.frame_bytes(2 * h, 2 * w, out=True) == p422.frame_bytes(out_fmt, 2 * h, 2 * w)
    rng = np.random.default_rng(4)
    u16 = bit_depth == 16
    frames = [p422.random_frame(rng, in_fmt, h, w) for _ in range(9)]
    want = b"".join(p422.bgr_to_pix(Pix422FakeNet.apply(p422.pix_to_bgr(f, in_fmt, h, w, "bt709", False, *mode, u16), 2), out_fmt, "bt709", False,
                                    *mode, u16).tobytes() for f in frames)
    assert len(want) == 9 * p422.frame_bytes(out_fmt, 2 * h, 2 * w)
    lanes = [[(Pix422FakeNet(2), 32)] for _ in range(nlanes)]
    fout = io.BytesIO()
    n = rawvideo.stream(io.BytesIO(b"".join(f.tobytes() for f in frames)), fout, h, w, lanes if nlanes > 1 else lanes[0],
                        alloc=lambda s: np.zeros(s, np.uint8), pix=pix)
    assert n == len(frames) and fout.getvalue() == want
    assert all(c == (in_fmt, out_fmt, bit_depth) for lane in lanes for net, _ in lane for c in net.calls)
    assert sum(len(net.calls) for lane in lanes for net, _ in lane) == len(frames)


def test_cli_takes_both_names(capsys):
    """argparse accepts the names on both ends (the run stops at a later, unrelated refusal); 4:4:4 is still no choice"""
    for a, b in (("yuv422p", "yuv422p10le"), ("yuv422p10le", "yuv422p")):
        with pytest.raises(SystemExit) as e:
            rawvideo.main(["-W", "8", "-H", "8", "--in-pix-fmt", a, "--out-pix-fmt", b, "--chroma-loc", "center"])
        assert e.value.code == 2 and "--chroma-loc needs --chroma-filter bilinear" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        rawvideo.main(["-W", "8", "-H", "8", "--out-pix-fmt", "yuv444p"])
    assert e.value.code == 2 and "invalid choice" in capsys.readouterr().err
    with pytest.raises(ValueError):
        rawvideo.PixFormats("yuv422p", "bgr48le")


# ---- what hipcc emits -------------------------------------------------------------------------------------------------------
def _kernels(text):
    info = {}
    for m in re.finditer(r"^(_ZN3uva\w*pix\w+):", text, flags=re.M):
        seg = text[m.end():]
        seg = seg[:seg.index("; Occupancy:") + 40]
        num = lambda pat: int(re.search(pat, seg).group(1))   # noqa: E731
        info[m.group(1)] = dict(scratch=num(r"; ScratchSize: (\d+)"), vgpr=num(r"; NumVgprs: (\d+)"), occ=num(r"; Occupancy: (\d+)"))
    return info


def test_kernel_resources(tmp_path):
    """every 4:2:2 instantiation -- 2 directions x 2 word sizes x 2 access paths x 2 sample types x 3 modes -- compiles for gfx950
    without scratch and with no more VGPRs than its 4:2:0 twin: yuv420p / yuv420p10le on the same path with the same sample type
    and mode (the co-sited mode, which left and topleft share, is held to left's twin, the smaller of the two)"""
    from upscale_video_amd import build
    asm = str(tmp_path / "pixfmt_isa.s")
    cmd = [build.hipcc()] + [f for f in build.FLAGS if f != "-fPIC"] + ["-S", "--cuda-device-only", os.path.join(build.CSRC, "uva_pixfmt.hip"), "-o", asm]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    info = _kernels(open(asm).read())
    seen = 0
    for d, w16, vec, ty, hm in itertools.product(("from_bgr", "to_bgr"), (0, 1), (0, 1), "ht", (0, 1, 2)):
        new = [v for n, v in info.items() if re.search(r"pix422_%sILb%dELb%dE%sLi%dEE" % (d, w16, vec, ty, hm), n)]
        twin = [v for n, v in info.items() if re.search(r"\d+pix_%sILi%dELb%dE%sLi%dEE" % (d, 5 if w16 else 1, vec, ty, hm), n)]
        assert len(new) == 1 and len(twin) == 1, (d, w16, vec, ty, hm, sorted(info))
        new, twin = new[0], twin[0]
        print("pix422_%s<%s, %s, %s, %d>: %d VGPRs (4:2:0 twin %d), occupancy %d, scratch %d"
              % (d, "10le" if w16 else "8", "wide" if vec else "bytes", "u8" if ty == "h" else "u16", hm, new["vgpr"], twin["vgpr"], new["occ"], new["scratch"]))
        assert new["scratch"] == 0, (d, w16, vec, ty, hm, new)
        assert new["vgpr"] <= twin["vgpr"], (d, w16, vec, ty, hm, new, twin)
        seen += 1
    assert seen == 48 and sum("pix422_" in n for n in info) == 48
