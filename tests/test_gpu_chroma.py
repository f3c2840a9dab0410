"""The sited, interpolating 4:2:0 chroma modes on the MI355X (-m gpu): the kernels bit for bit against
the numpy restatement (tests/chroma_ref.py), Net.submit_pix with three frames in flight, the quality gain through the 2x net,
the streamer as a subprocess, and the refusal of bad colour words by every entry that takes one."""
import itertools
import subprocess
import sys

import numpy as np
import pytest

import chroma_ref as cr
from conftest import ROOT, load_net
from parity_report import psnr_u8, record

pytestmark = pytest.mark.gpu

COLOURS = [(m, r) for m in ("bt601", "bt709") for r in ("tv", "pc")]
SIZES = [(1, 1), (3, 5), (7, 40), (970, 965), (1080, 1920)]       # (h, w): the last takes the vector path, the others the byte path


def _random_packed(fmt, h, w, rng):
    n = cr.ref16.frame_bytes(fmt, h, w)
    if cr.ref16.depth_of(fmt) == 10:       # any 16-bit word: the bits beside the 10-bit value must be ignored
        return rng.integers(0, 1 << 16, n // 2, dtype=np.uint16).astype("<u2").view(np.uint8)
    return rng.integers(0, 256, n, dtype=np.uint8)


@pytest.mark.parametrize("bit_depth", [8, 16])
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("fmt", cr.YUV)
def test_conversion_kernels_are_bit_exact(uva, fmt, h, w, bit_depth):
    """small frames: every siting x matrix x range; the two large ones: every siting, the matrix and range rotating with it"""
    u16 = bit_depth == 16
    bgr_fmt = "bgr48le" if u16 else "bgr24"
    rng = np.random.default_rng(h * 7 + w + bit_depth)
    combos = list(itertools.product(cr.SITINGS, COLOURS))
    if h * w > 10000:
        k0 = cr.YUV.index(fmt) + (h > 1000) + u16
        combos = [(loc, COLOURS[(k0 + i) % 4]) for i, loc in enumerate(cr.SITINGS)]
    for loc, (m, cr_range) in combos:
        full = cr_range == "pc"
        kw = dict(colour=m, color_range=cr_range, bit_depth=bit_depth, chroma_filter="bilinear", chroma_loc=loc)
        bgr = rng.integers(0, 65536 if u16 else 256, (h, w, 3), dtype=np.uint16 if u16 else np.uint8)
        got = uva.convert_pix(bgr, h, w, bgr_fmt, fmt, **kw)
        assert np.array_equal(got, cr.bgr_to_pix(bgr, fmt, m, full, "bilinear", loc, u16)), (fmt, loc, m, cr_range, "forward")
        p = _random_packed(fmt, h, w, rng)
        got = uva.convert_pix(p, h, w, fmt, bgr_fmt, **kw)
        assert np.array_equal(got, cr.pix_to_bgr(p, fmt, h, w, m, full, "bilinear", loc, u16)), (fmt, loc, m, cr_range, "inverse")
        if h * w <= 10000:      # packed to packed goes through u8 / u16 BGR; equal formats are a copy
            other = cr.YUV[(cr.YUV.index(fmt) + 1) % 4]
            assert np.array_equal(uva.convert_pix(p, h, w, fmt, other, **kw), cr.convert(p, fmt, other, h, w, m, full, "bilinear", loc, bit_depth))
            assert np.array_equal(uva.convert_pix(p, h, w, fmt, fmt, **kw), p)
    # the replicate path with the new keywords spelt out is the earlier releases' path
    p = _random_packed(fmt, h, w, rng)
    got = uva.convert_pix(p, h, w, fmt, bgr_fmt, bit_depth=bit_depth, chroma_filter="replicate", chroma_loc="left")
    assert np.array_equal(got, uva.convert_pix(p, h, w, fmt, bgr_fmt, bit_depth=bit_depth))
    assert np.array_equal(got, cr.pix_to_bgr(p, fmt, h, w, u16=u16))


def test_device_conversion_takes_the_mode(uva):
    import torch
    h, w = 37, 66
    net = load_net(uva, "2x")
    p = _random_packed("nv12", h, w, np.random.default_rng(5))
    d_in = torch.from_numpy(p.copy()).cuda()
    d_bgr = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    net.convert_pix_device(d_in.data_ptr(), h, w, "nv12", d_bgr.data_ptr(), "bgr24", "bt709", "tv", chroma_filter="bilinear", chroma_loc="topleft")
    net.synchronize()
    assert np.array_equal(d_bgr.cpu().numpy(), cr.pix_to_bgr(p, "nv12", h, w, "bt709", False, "bilinear", "topleft"))


@pytest.mark.parametrize("bit_depth", [8, 16])
@pytest.mark.parametrize("key,tile", [("2x", 64), ("2x", 0), ("4x", 64), ("4x", 0)])
def test_submit_pix_is_the_restatement_around_the_net(uva, key, tile, bit_depth):
    """inverse restatement -> process_u8 / process_u16 -> forward restatement, three frames in flight (buffer reuse shows)"""
    net = load_net(uva, key)
    s = net.scale
    u16 = bit_depth == 16
    h, w = 66, 90
    border = 10 if tile else 0
    rng = np.random.default_rng(13)
    fmt_in, fmt_out = ("yuv420p10le", "p010le") if u16 else ("yuv420p", "nv12")
    run = net.process_u16 if u16 else net.process_u8
    for i, loc in enumerate(cr.SITINGS):
        m, cr_range = COLOURS[(i + (s == 4) + u16) % 4]
        full = cr_range == "pc"
        frames = [_random_packed(fmt_in, h, w, rng) for _ in range(5)]
        wants = [cr.bgr_to_pix(run(cr.pix_to_bgr(f, fmt_in, h, w, m, full, "bilinear", loc, u16), tile_size=tile, border=border),
                               fmt_out, m, full, "bilinear", loc, u16) for f in frames]
        outs = [uva.pix_empty(fmt_out, h * s, w * s, uva.pinned_empty if k % 2 else None) for k in range(len(frames))]
        tickets, got = [], []
        for f, o in zip(frames, outs):
            if len(tickets) == 3:
                got.append(net.collect_u8(tickets.pop(0)))
            tickets.append(net.submit_pix(f, h, w, fmt_in, out=o, out_fmt=fmt_out, colour=m, color_range=cr_range, tile_size=tile, border=border,
                                          bit_depth=bit_depth, chroma_filter="bilinear", chroma_loc=loc))
        got += [net.collect_u8(t) for t in tickets]
        for k in range(len(frames)):
            assert np.array_equal(np.asarray(got[k]).reshape(-1).view(np.uint8), wants[k]), (loc, k)


def test_matched_bilinear_is_closer_to_the_truth_through_the_net(uva):
    """The 2x result of the ground-truth edges frame is the target.  That frame's 4:2:0 version of each siting (made with the
    siting's forward restatement), brought in with replicate and with the matched bilinear mode, bgr24 out: the matched mode's
    2x result is strictly closer.  (fp32 oracle, left: 29.39 against 27.53 dB; the fp16 kernels sit >= 55 dB from the oracle.)"""
    net = load_net(uva, "2x")
    truth = cr.edges_frame()
    h, w, _ = truth.shape
    target = net.process_u8(truth, tile_size=960, border=10)
    for src in cr.SITINGS:
        f = cr.bgr_to_pix(truth, "yuv420p", "bt601", False, "bilinear", src)
        res = {}
        for filt, loc in (("replicate", "left"), ("bilinear", src)):
            got = net.collect_u8(net.submit_pix(f, h, w, "yuv420p", out_fmt="bgr24", tile_size=960, border=10, chroma_filter=filt, chroma_loc=loc))
            d = np.abs(got.astype(np.int16) - target.astype(np.int16))
            res[filt] = psnr_u8(got, target)
            record("2x edges 480x270, %s-sited yuv420p in, chroma %s%s" % (src, filt, "/" + loc if filt == "bilinear" else ""), kind="u8",
                   vs="2x result of the ground-truth bgr24 frame", model=None, route=None, samples=int(d.size), max_lsb=int(d.max()),
                   psnr_db=res[filt], differ_share=float((d > 0).mean()), bar_max_lsb=None, bar_min_psnr_db=None, bar_max_share=None,
                   structure=None, bar_structure_z=None)
        print("source %-7s replicate %.2f dB, bilinear/%s %.2f dB" % (src, res["replicate"], src, res["bilinear"]))
        assert res["bilinear"] > res["replicate"], (src, res)


@pytest.mark.parametrize("bit_depth", [8, 16])
def test_streamer_subprocess(uva, tmp_path, bit_depth):
    net = load_net(uva, "2x")
    h, w, n, tile = 40, 58, 5, 32
    rng = np.random.default_rng(11)
    frames = [_random_packed("yuv420p", h, w, rng) for _ in range(n)]
    kw = dict(chroma_filter="bilinear", chroma_loc="left", bit_depth=bit_depth)
    want = b"".join(net.collect_u8(net.submit_pix(f, h, w, "yuv420p", out_fmt="p010le", tile_size=tile, border=10, **kw)).tobytes()
                    for f in frames)
    plain = b"".join(net.collect_u8(net.submit_pix(f, h, w, "yuv420p", out_fmt="p010le", tile_size=tile, border=10,
                                                    bit_depth=bit_depth)).tobytes() for f in frames)
    assert want != plain
    argv = ["-W", str(w), "-H", str(h), "-s", "2", "--tile", str(tile), "--in-pix-fmt", "yuv420p", "--out-pix-fmt", "p010le",
            "--bit-depth", str(bit_depth), "--chroma-filter", "bilinear", "--chroma-loc", "left", "-g", "0,0"]
    r = subprocess.run([sys.executable, "-m", "upscale_video_amd.rawvideo"] + argv, input=b"".join(f.tobytes() for f in frames),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout == want


def test_bad_colour_words_are_refused_by_every_entry(uva):
    import torch
    from upscale_video_amd import _lib
    L = _lib.load()
    net = load_net(uva, "2x")
    h, w = 8, 8
    src = np.zeros(cr.ref16.frame_bytes("yuv420p", h, w), np.uint8)
    out = np.zeros(6 * 4 * h * w, np.uint8)
    d_src, d_out = torch.zeros(src.size, dtype=torch.uint8, device="cuda"), torch.zeros(out.size, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    YUV420P, BGR24, BGR48 = 1, 0, 6
    for word in (8, 16, 8 | 1, 16 | 2, 4 | 8 | 16, 32, 64 | 4, 1 << 20, -1):       # siting without the filter bit, both sitings, unknown bits
        entries = {
            "uva_net_submit_pix": lambda: L.uva_net_submit_pix(net._h, src.ctypes.data, YUV420P, h, w, out.ctypes.data, BGR24, word, 0, 0) < 0,
            "uva_net_submit_pix16": lambda: L.uva_net_submit_pix16(net._h, src.ctypes.data, YUV420P, h, w, out.ctypes.data, BGR48, word, 0, 0) < 0,
            "uva_pix_convert": lambda: L.uva_pix_convert(0, src.ctypes.data, YUV420P, out.ctypes.data, BGR24, h, w, word) != 0,
            "uva_pix_convert16": lambda: L.uva_pix_convert16(0, src.ctypes.data, YUV420P, out.ctypes.data, BGR48, h, w, word) != 0,
            "uva_pix_convert_device": lambda: L.uva_pix_convert_device(0, d_src.data_ptr(), YUV420P, d_out.data_ptr(), BGR24, h, w, word,
                                                                       None, net._h) != 0,
        }
        for name, refused in entries.items():
            assert refused(), (name, word)
            assert b"colour" in L.uva_last_error(), (name, word, L.uva_last_error())
    # and the good ones pass
    for word in (0, 3, 4, 4 | 8 | 1, 4 | 16 | 2):
        assert L.uva_pix_convert(0, src.ctypes.data, YUV420P, out.ctypes.data, BGR24, h, w, word) == 0, word
