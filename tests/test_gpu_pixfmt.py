"""Raw-video pixel formats on the MI355X (-m gpu): the conversion kernels (csrc/uva_pixfmt.hip) bit for bit against the numpy
restatement (tests/pixfmt_ref.py), Net.submit_pix against submit_u8 with the restatement on either side, and the rawvideo
streamer end to end, file to file and pipe to pipe."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pixfmt_ref as ref
from conftest import ROOT, load_net

pytestmark = pytest.mark.gpu

YUV = ("yuv420p", "nv12", "p010le")
COLOURS = [(m, r) for m in ("bt601", "bt709") for r in ("tv", "pc")]
SIZES = [(1, 1), (3, 5), (7, 40), (970, 965), (1080, 1920)]


def _bgr_frames(h, w, seed):
    from oracle import uvoracle
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8), uvoracle.synthetic_frame(h, w, seed=seed)]


def _random_packed(fmt, h, w, seed):
    rng = np.random.default_rng(seed)
    n = ref.frame_bytes(fmt, h, w)
    if fmt == "p010le":          # any 16-bit word (the low six bits must be ignored)
        return rng.integers(0, 1 << 16, n // 2, dtype=np.uint16).astype("<u2").view(np.uint8)
    return rng.integers(0, 256, n, dtype=np.uint8)


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("fmt", YUV)
def test_conversion_kernels_are_bit_exact(uva, fmt, h, w):
    for k, (m, rng) in enumerate(COLOURS):
        full = rng == "pc"
        for i, f in enumerate(_bgr_frames(h, w, 10 * k + 1)):
            got = uva.convert_pix(f, h, w, "bgr24", fmt, m, rng)
            assert np.array_equal(got, ref.bgr_to_pix(f, fmt, m, full)), (fmt, m, rng, i, "forward")
        p = _random_packed(fmt, h, w, 10 * k + 2)
        got = uva.convert_pix(p, h, w, fmt, "bgr24", m, rng)
        assert np.array_equal(got, ref.pix_to_bgr(p, fmt, h, w, m, full)), (fmt, m, rng, "inverse")
        # packed to packed goes through u8 BGR; equal formats are a copy
        other = YUV[(YUV.index(fmt) + 1) % 3]
        assert np.array_equal(uva.convert_pix(p, h, w, fmt, other, m, rng), ref.convert(p, fmt, other, h, w, m, full))
        assert np.array_equal(uva.convert_pix(p, h, w, fmt, fmt, m, rng), p)


def test_device_conversion_in_front_of_a_net(uva):
    import torch
    h, w = 37, 66
    net = load_net(uva, "2x")
    p = _random_packed("nv12", h, w, 5)
    d_in = torch.from_numpy(p.copy()).cuda()
    d_bgr = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    d_out = torch.empty((2 * h, 2 * w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    net.convert_pix_device(d_in.data_ptr(), h, w, "nv12", d_bgr.data_ptr(), "bgr24", "bt709", "tv")
    net.process_u8_device(d_bgr.data_ptr(), h, w, d_out.data_ptr())
    net.synchronize()
    bgr = ref.pix_to_bgr(p, "nv12", h, w, "bt709")
    assert np.array_equal(d_bgr.cpu().numpy(), bgr)
    assert np.array_equal(d_out.cpu().numpy(), net.process_u8(bgr))


@pytest.mark.parametrize("key,h,w,tile", [("2x", 1080, 1920, 960), ("2x", 97, 131, 960), ("1x", 135, 241, 0), ("1x", 540, 960, 0)])
def test_submit_pix_equals_submit_u8_with_the_restatement(uva, key, h, w, tile):
    net = load_net(uva, key)
    s = net.scale
    border = 10 if tile else 0
    f = _bgr_frames(h, w, 7)[1]
    base = net.process_u8(f, tile_size=tile, border=border)
    for k, fmt in enumerate(YUV):
        m, rng = COLOURS[k % 4]
        full = rng == "pc"
        # yuv in -> bgr24 out: the net sees exactly the restatement's BGR
        p = _random_packed(fmt, h, w, 20 + k) if k == 1 else ref.bgr_to_pix(f, fmt, m, full)
        t = net.submit_pix(p, h, w, fmt, out_fmt="bgr24", colour=m, color_range=rng, tile_size=tile, border=border)
        got = net.collect_u8(t)
        assert np.array_equal(got, net.process_u8(ref.pix_to_bgr(p, fmt, h, w, m, full), tile_size=tile, border=border)), fmt
        # bgr24 in -> yuv out: the restatement of the net's u8 result
        got = net.collect_u8(net.submit_pix(f, h, w, "bgr24", out_fmt=fmt, colour=m, color_range=rng, tile_size=tile, border=border))
        assert np.array_equal(got, ref.bgr_to_pix(base, fmt, m, full)), fmt
    # both ends at once, three frames in flight, pinned and pageable buffers
    fmt_in, fmt_out = "yuv420p", "p010le"
    frames = [ref.bgr_to_pix(g, fmt_in) for g in _bgr_frames(h, w, 30) + [f]]
    outs = [uva.pix_empty(fmt_out, h * s, w * s, uva.pinned_empty if i % 2 else None) for i in range(3)]
    wants = [ref.bgr_to_pix(net.process_u8(ref.pix_to_bgr(p, fmt_in, h, w), tile_size=tile, border=border), fmt_out) for p in frames]
    tickets = [net.submit_pix(p, h, w, fmt_in, out=o, out_fmt=fmt_out, tile_size=tile, border=border) for p, o in zip(frames, outs)]
    for want, t in zip(wants, tickets):
        assert np.array_equal(net.collect_u8(t), want)
    # bgr24 at both ends: submit_u8's bytes
    assert np.array_equal(net.collect_u8(net.submit_pix(f, h, w, "bgr24", tile_size=tile, border=border)), base)


def _chain_want(nets, packed, h, w, models, fmt_in, fmt_out, tile):
    """the per-frame composition of the pieces: restated input conversion, the stages' synchronous calls, restated output"""
    from upscale_video_amd import upscale_processing as up
    x = ref.pix_to_bgr(packed, fmt_in, h, w)
    if "n=3" in models:
        x = up.denoise_u8(x, 3, device=0)
    if "a" in models.split(","):
        x = nets["1x"].process_u8(x)
    x = nets["2x"].process_u8(x, tile_size=tile, border=10)
    return ref.bgr_to_pix(x, fmt_out).tobytes()


def test_rawvideo_end_to_end(uva, tmp_path):
    nets = {"1x": load_net(uva, "1x"), "2x": load_net(uva, "2x")}
    h, w, n, tile = 72, 118, 6, 32
    frames = [ref.bgr_to_pix(f, "yuv420p") for i in range(n // 2) for f in _bgr_frames(h, w, 40 + i)]
    src = tmp_path / "in.yuv"
    src.write_bytes(b"".join(p.tobytes() for p in frames))
    geo = ["-W", str(w), "-H", str(h), "-s", "2", "--tile", str(tile), "--in-pix-fmt", "yuv420p", "--out-pix-fmt", "p010le"]
    from upscale_video_amd import rawvideo
    for models in ("a", "a,n=3"):
        want = b"".join(_chain_want(nets, p, h, w, models, "yuv420p", "p010le", tile) for p in frames)
        for gpus in ("0", "0,0"):
            dst = tmp_path / ("out_%s_%s.p010" % (models.replace(",", "_"), gpus.replace(",", "_")))     # (`-o a,b`: a list)
            assert rawvideo.main(["-i", str(src), "-o", str(dst)] + geo + ["-m", models, "-g", gpus]) == 0
            assert dst.read_bytes() == want, (models, gpus, "file")
        # pipe to pipe: a fresh interpreter between two pipes, as under ffmpeg
        r = subprocess.run([sys.executable, "-m", "upscale_video_amd.rawvideo"] + geo + ["-m", models, "-g", "0,0"],
                           input=src.read_bytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
        assert r.stdout == want, (models, "pipe")
    # default flags: today's bytes (bgr24 both ends)
    bgr = [ref.pix_to_bgr(p, "yuv420p", h, w) for p in frames]
    src2, dst2 = tmp_path / "in.bgr24", tmp_path / "out.bgr24"
    src2.write_bytes(b"".join(b.tobytes() for b in bgr))
    assert rawvideo.main(["-i", str(src2), "-o", str(dst2), "-W", str(w), "-H", str(h), "-s", "2", "--tile", str(tile), "-m", "a"]) == 0
    assert dst2.read_bytes() == b"".join(nets["2x"].process_u8(nets["1x"].process_u8(b), tile_size=tile, border=10).tobytes() for b in bgr)
    # `-s 1` without a net: one conversion per frame on the GPU
    dst3 = tmp_path / "out.nv12"
    assert rawvideo.main(["-i", str(src), "-o", str(dst3), "-W", str(w), "-H", str(h), "-s", "1", "--in-pix-fmt", "yuv420p",
                          "--out-pix-fmt", "nv12", "--colorspace", "bt709"]) == 0
    assert dst3.read_bytes() == b"".join(ref.convert(p, "yuv420p", "nv12", h, w, "bt709").tobytes() for p in frames)
    assert os.path.getsize(dst3) == n * ref.frame_bytes("nv12", h, w)
