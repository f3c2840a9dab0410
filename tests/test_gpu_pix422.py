"""The 4:2:2 formats yuv422p / yuv422p10le on the MI355X (-m gpu): the kernels bit for bit against the
numpy restatement (tests/pix422_ref.py) on both access paths, from unaligned bases, around the net with three frames in flight,
with a resampled result, through the streamer (files, pipes, two lanes), and what a 4:2:2 source keeps through the 2x net."""
import itertools
import subprocess
import sys

import numpy as np
import pytest

import chroma_ref as cr
import pix422_ref as p422
from conftest import ROOT, load_net
from parity_report import psnr_u8, record

pytestmark = pytest.mark.gpu

COLOURS = [(m, r) for m in ("bt601", "bt709") for r in ("tv", "pc")]
# (h, w): a lone pixel; one pair; odd widths, whose last chroma sample belongs to one pixel; the wide path (w % 8 == 0) with odd
# heights, one thread and five threads a row, the neighbour taps clamped at both row ends; four whole threads and a one-pixel
# tail in a row (w % 8 != 0: the byte path); the wide path with an even height
SHAPES = [(1, 1), (1, 2), (2, 3), (3, 5), (5, 8), (7, 40), (5, 33), (4, 24)]


def _kw(m, rng_name, mode, bit_depth):
    return dict(colour=m, color_range=rng_name, bit_depth=bit_depth, chroma_filter=mode[0], chroma_loc=mode[1])


@pytest.mark.parametrize("bit_depth", [8, 16])
@pytest.mark.parametrize("fmt", p422.FORMATS422)
def test_conversion_kernels_are_bit_exact(uva, fmt, bit_depth):
    """every shape x matrix x range x mode, both directions, through bgr24 (8-bit route) / bgr48le (16-bit route); the 10-bit
    input is random words, garbage in the high six bits included"""
    u16 = bit_depth == 16
    bgr_fmt = "bgr48le" if u16 else "bgr24"
    rng = np.random.default_rng(422 + bit_depth + len(fmt))
    for (h, w), (m, rn), mode in itertools.product(SHAPES, COLOURS, cr.MODES):
        full = rn == "pc"
        kw = _kw(m, rn, mode, bit_depth)
        bgr = rng.integers(0, 65536 if u16 else 256, (h, w, 3), dtype=np.uint16 if u16 else np.uint8)
        got = uva.convert_pix(bgr, h, w, bgr_fmt, fmt, **kw)
        assert np.array_equal(got, p422.bgr_to_pix(bgr, fmt, m, full, *mode, u16)), (h, w, m, rn, mode, "forward")
        p = p422.random_frame(rng, fmt, h, w)
        got = uva.convert_pix(p, h, w, fmt, bgr_fmt, **kw)
        assert np.array_equal(got, p422.pix_to_bgr(p, fmt, h, w, m, full, *mode, u16)), (h, w, m, rn, mode, "inverse")
        assert np.array_equal(uva.convert_pix(p, h, w, fmt, fmt, **kw), p)          # equal formats: a copy


@pytest.mark.parametrize("bit_depth", [8, 16])
@pytest.mark.parametrize("fmt", p422.FORMATS422)
def test_422_to_and_from_every_420_format(uva, fmt, bit_depth):
    h, w = 7, 40
    rng = np.random.default_rng(7 + bit_depth)
    for k, other in enumerate(cr.YUV + tuple(f for f in p422.FORMATS422 if f != fmt)):
        (m, rn), mode = COLOURS[k % 4], cr.MODES[(k + (bit_depth == 16)) % 4]
        kw = _kw(m, rn, mode, bit_depth)
        for a, b in ((fmt, other), (other, fmt)):
            p = p422.random_frame(rng, a, h, w)
            got = uva.convert_pix(p, h, w, a, b, **kw)
            assert np.array_equal(got, p422.convert(p, a, b, h, w, m, rn == "pc", *mode, bit_depth)), (a, b, m, rn, mode)


@pytest.mark.parametrize("fmt,bit_depth", [("yuv422p", 8), ("yuv422p10le", 16)])
def test_the_wide_path_at_1080p(uva, fmt, bit_depth):
    h, w = 1080, 1920
    u16 = bit_depth == 16
    bgr_fmt = "bgr48le" if u16 else "bgr24"
    rng = np.random.default_rng(1080 + bit_depth)
    bgr = rng.integers(0, 65536 if u16 else 256, (h, w, 3), dtype=np.uint16 if u16 else np.uint8)
    p = p422.random_frame(rng, fmt, h, w)
    for (m, rn), mode in ((("bt709", "tv"), ("bilinear", "left")), (("bt601", "pc"), ("bilinear", "center"))):
        kw = _kw(m, rn, mode, bit_depth)
        assert np.array_equal(uva.convert_pix(bgr, h, w, bgr_fmt, fmt, **kw), p422.bgr_to_pix(bgr, fmt, m, rn == "pc", *mode, u16)), (mode, "forward")
        assert np.array_equal(uva.convert_pix(p, h, w, fmt, bgr_fmt, **kw), p422.pix_to_bgr(p, fmt, h, w, m, rn == "pc", *mode, u16)), (mode, "inverse")
    assert np.array_equal(uva.convert_pix(p, h, w, fmt, bgr_fmt, bit_depth=bit_depth), p422.pix_to_bgr(p, fmt, h, w, u16=u16))
    assert np.array_equal(uva.convert_pix(bgr, h, w, bgr_fmt, fmt, bit_depth=bit_depth), p422.bgr_to_pix(bgr, fmt, u16=u16))


@pytest.mark.parametrize("fmt,off", [("yuv422p", 1), ("yuv422p10le", 2)])
def test_an_unaligned_base_takes_the_byte_path(uva, fmt, off):
    """a frame whose width would take the wide path, from a buffer `off` bytes past an aligned address: the same bytes"""
    import torch
    h, w = 7, 40
    net = load_net(uva, "2x")
    rng = np.random.default_rng(off)
    n = p422.frame_bytes(fmt, h, w)
    p = p422.random_frame(rng, fmt, h, w)
    bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for mode in cr.MODES:
        kw = dict(chroma_filter=mode[0], chroma_loc=mode[1])
        d_pack = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
        d_bgr = torch.zeros(3 * h * w + 64, dtype=torch.uint8, device="cuda")
        assert d_pack.data_ptr() % 16 == 0 and d_bgr.data_ptr() % 16 == 0
        for o in (0, off):
            # inverse: packed frame at the offset -> aligned BGR
            d_pack[o:o + n] = torch.from_numpy(p).cuda()
            d_bgr.zero_()
            torch.cuda.synchronize()
            net.convert_pix_device(d_pack.data_ptr() + o, h, w, fmt, d_bgr.data_ptr(), "bgr24", "bt709", "tv", **kw)
            net.synchronize()
            got = d_bgr.cpu().numpy()
            assert np.array_equal(got[:3 * h * w].reshape(h, w, 3), p422.pix_to_bgr(p, fmt, h, w, "bt709", False, *mode)), (mode, o, "inverse")
            assert not got[3 * h * w:].any()
            # forward: aligned BGR -> packed frame at the offset, nothing written beside it
            d_bgr[:3 * h * w] = torch.from_numpy(bgr.reshape(-1)).cuda()
            d_pack.zero_()
            torch.cuda.synchronize()
            net.convert_pix_device(d_bgr.data_ptr(), h, w, "bgr24", d_pack.data_ptr() + o, fmt, "bt709", "tv", **kw)
            net.synchronize()
            got = d_pack.cpu().numpy()
            assert np.array_equal(got[o:o + n], p422.bgr_to_pix(bgr, fmt, "bt709", False, *mode)), (mode, o, "forward")
            assert not got[:o].any() and not got[o + n:].any()


@pytest.mark.parametrize("in_fmt,out_fmt,bit_depth,mode", [
    ("yuv422p", "yuv422p", 8, ("replicate", "left")), ("yuv422p10le", "yuv422p10le", 16, ("replicate", "left")),
    ("yuv422p", "yuv422p", 8, ("bilinear", "center")), ("yuv422p10le", "p010le", 16, ("bilinear", "left"))])
def test_submit_pix_is_the_restatement_around_the_net(uva, in_fmt, out_fmt, bit_depth, mode):
    """inverse restatement -> process_u8 / process_u16 -> forward restatement; three frames in flight, pageable and pinned results"""
    net = load_net(uva, "2x")
    u16 = bit_depth == 16
    h, w, tile, border = 66, 90, 32, 10
    rng = np.random.default_rng(13 + bit_depth)
    m, rn = ("bt709", "tv") if u16 else ("bt601", "pc")
    run = net.process_u16 if u16 else net.process_u8
    frames = [p422.random_frame(rng, in_fmt, h, w) for _ in range(5)]
    wants = [p422.bgr_to_pix(run(p422.pix_to_bgr(f, in_fmt, h, w, m, rn == "pc", *mode, u16), tile_size=tile, border=border),
                             out_fmt, m, rn == "pc", *mode, u16) for f in frames]
    outs = [uva.pix_empty(out_fmt, 2 * h, 2 * w, uva.pinned_empty if k % 2 else None) for k in range(len(frames))]
    tickets, got = [], []
    for f, o in zip(frames, outs):
        if len(tickets) == 3:
            got.append(net.collect_u8(tickets.pop(0)))
        tickets.append(net.submit_pix(f, h, w, in_fmt, out=o, out_fmt=out_fmt, tile_size=tile, border=border, **_kw(m, rn, mode, bit_depth)))
    got += [net.collect_u8(t) for t in tickets]
    for k in range(len(frames)):
        assert np.array_equal(np.asarray(got[k]).reshape(-1).view(np.uint8), wants[k]), k


def test_submit_pix_sized(uva):
    net = load_net(uva, "2x")
    h, w, size = 66, 90, (100, 150)
    f = p422.random_frame(np.random.default_rng(17), "yuv422p", h, w)
    big = net.process_u8(p422.pix_to_bgr(f, "yuv422p", h, w, "bt709", False, "bilinear", "left"), tile_size=32, border=10)
    want = p422.bgr_to_pix(uva.resize(big, size), "yuv422p", "bt709", False, "bilinear", "left")
    got = net.collect_u8(net.submit_pix(f, h, w, "yuv422p", out_fmt="yuv422p", colour="bt709", tile_size=32, border=10,
                                        chroma_filter="bilinear", chroma_loc="left", out_size=size))
    assert got.nbytes == p422.frame_bytes("yuv422p", *size) and np.array_equal(got, want)


def test_rawvideo_end_to_end(uva, tmp_path):
    from upscale_video_amd import rawvideo
    net = load_net(uva, "2x")
    h, w, n, tile = 40, 58, 5, 32
    rng = np.random.default_rng(11)
    frames = [p422.random_frame(rng, "yuv422p10le", h, w) for _ in range(n)]
    src = tmp_path / "in.yuv"
    src.write_bytes(b"".join(f.tobytes() for f in frames))
    want = b"".join(net.collect_u8(net.submit_pix(f, h, w, "yuv422p10le", out_fmt="yuv422p10le", tile_size=tile, border=10,
                                                   bit_depth=16)).tobytes() for f in frames)
    assert len(want) == n * p422.frame_bytes("yuv422p10le", 2 * h, 2 * w)
    # (and those are the restatement's bytes around process_u16)
    first = p422.bgr_to_pix(net.process_u16(p422.pix_to_bgr(frames[0], "yuv422p10le", h, w, u16=True), tile_size=tile, border=10),
                            "yuv422p10le", u16=True)
    assert want[:first.size] == first.tobytes()
    geo = ["-W", str(w), "-H", str(h), "-s", "2", "--tile", str(tile), "--in-pix-fmt", "yuv422p10le", "--out-pix-fmt", "yuv422p10le",
           "--bit-depth", "16"]
    for gpus in ("0", "0,0"):
        dst = tmp_path / ("out_%s.yuv" % gpus.replace(",", "_"))
        assert rawvideo.main(["-i", str(src), "-o", str(dst), "-g", gpus] + geo) == 0
        assert dst.read_bytes() == want, gpus
    r = subprocess.run([sys.executable, "-m", "upscale_video_amd.rawvideo", "-g", "0"] + geo, input=src.read_bytes(),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout == want


def test_a_422_source_is_closer_to_the_truth_through_the_net(uva):
    """The 2x result of the ground-truth edges frame is the target.  The frame as a 4:2:2 source (the co-sited forward filter),
    fed (a) as yuv422p and (b) reduced to yuv420p by the project's own forward filter on the vertical axis, both bilinear/left,
    bgr24 out: (a) is strictly closer.  The size of the gap is recorded, not barred."""
    net = load_net(uva, "2x")
    truth = cr.edges_frame()
    h, w, _ = truth.shape
    target = net.process_u8(truth, tile_size=960, border=10)
    src = p422.bgr_to_pix(truth, "yuv422p", "bt601", False, "bilinear", "left")
    res = {}
    for fmt, f in (("yuv422p", src), ("yuv420p", p422.squeeze_to_420(src, "yuv422p", h, w, "left"))):
        got = net.collect_u8(net.submit_pix(f, h, w, fmt, out_fmt="bgr24", tile_size=960, border=10, chroma_filter="bilinear", chroma_loc="left"))
        d = np.abs(got.astype(np.int16) - target.astype(np.int16))
        res[fmt] = psnr_u8(got, target)
        record("2x edges 480x270, 4:2:2 source fed as %s, chroma bilinear/left" % fmt, kind="u8",
               vs="2x result of the ground-truth bgr24 frame", model=None, route=None, samples=int(d.size), max_lsb=int(d.max()),
               psnr_db=res[fmt], differ_share=float((d > 0).mean()), bar_max_lsb=None, bar_min_psnr_db=None, bar_max_share=None,
               structure=None, bar_structure_z=None)
    print("through the 2x net: fed as yuv422p %.2f dB, squeezed to yuv420p %.2f dB" % (res["yuv422p"], res["yuv420p"]))
    assert res["yuv422p"] > res["yuv420p"], res
