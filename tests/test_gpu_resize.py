"""The resampler on the MI355X (-m gpu): ncnn.resize bit for bit against the numpy restatement
(tests/resize_ref.py, with the library's tap tables), padded strides and canaries, the device entry, cached tables across changing
geometries, Net.submit_pix(out_size=...) against the composition of the separate calls with three frames in flight, the streamer as
a subprocess (pipes, files, -m a, --bit-depth 16, -g 0,0), and the refusals of every entry."""
import os
import subprocess
import sys

import numpy as np
import pytest

import resize_ref as ref
from conftest import ROOT, load_net

pytestmark = pytest.mark.gpu

SMALL = [((1, 1), (1, 1)), ((3, 5), (7, 4)), ((7, 40), (5, 61)), ((64, 48), (16, 12)), ((9, 11), (36, 44)), ((5, 200), (20, 50))]
LARGE = [((970, 965), (647, 1287)), ((1080, 1920), (720, 1280)), ((2160, 3840), (1440, 2560)), ((2160, 3840), (1080, 3840)),
         ((1080, 1920), (1620, 2880)), ((1024, 772), (256, 193)), ((270, 193), (1080, 772))]


def _content(kind, shape, dtype, rng):
    mx = np.iinfo(dtype).max
    if kind == "random":
        return rng.integers(0, mx + 1, shape).astype(dtype)
    return (rng.integers(0, 2, shape) * mx).astype(dtype)


def _want(img, size, name):
    h, w, _ = img.shape
    return ref.resize(img, size, ref.library_tables(h, w, size[0], size[1], name))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("src,dst", SMALL)
def test_small_frames_bit_exact(uva, src, dst, dtype):
    rng = np.random.default_rng(src[0] * 31 + dst[1])
    for name in ref.FILTERS:
        for kind in ("random", "two-level"):
            img = _content(kind, src + (3,), dtype, rng)
            got = uva.resize(img, dst, name)
            assert got.dtype == dtype and got.shape == dst + (3,)
            assert np.array_equal(got, _want(img, dst, name)), (name, kind)
    flat = np.full(src + (3,), np.iinfo(dtype).max - 2, dtype)
    assert (uva.resize(flat, dst) == flat[0, 0, 0]).all()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("src,dst", LARGE)
def test_large_frames_bit_exact(uva, src, dst, dtype):
    """lanczos on random content, one other filter (rotating) on two-level content"""
    rng = np.random.default_rng(src[1] + dst[0])
    other = ("bicubic", "bilinear")[(src[0] + dst[1] + np.dtype(dtype).itemsize) % 2]
    for name, kind in (("lanczos", "random"), (other, "two-level")):
        img = _content(kind, src + (3,), dtype, rng)
        got = uva.resize(img, dst, name)
        want = _want(img, dst, name)
        assert np.array_equal(got, want), (name, kind, int(np.abs(got.astype(np.int64) - want).max()))


def test_identity_returns_the_input(uva):
    rng = np.random.default_rng(2)
    for dtype in (np.uint8, np.uint16):
        img = _content("random", (37, 53, 3), dtype, rng)
        for name in ref.FILTERS:
            assert np.array_equal(uva.resize(img, (37, 53), name), img)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("src,dst,pad_in,pad_out", [((7, 40), (5, 61), 5, 3), ((123, 211), (77, 300), 1, 7), ((270, 480), (405, 720), 16, 32),
                                                   ((540, 958), (360, 640), 2, 0), ((31, 33), (31, 50), 0, 9)])
def test_padded_strides_and_canaries(uva, src, dst, pad_in, pad_out, dtype):
    """rows padded on both sides (so that the aligned and the sample-by-sample load paths both run); the padding of the result
    buffer, and the sentinel rows around it, come back untouched"""
    rng = np.random.default_rng(pad_in * 10 + pad_out)
    (h, w), (oh, ow) = src, dst
    mx = np.iinfo(dtype).max
    big_in = rng.integers(0, mx + 1, (h, w + pad_in, 3)).astype(dtype)
    img = big_in[:, :w]
    canary = dtype(0xA5 if dtype == np.uint8 else 0xA55A)
    big_out = np.full((oh + 2, ow + pad_out, 3), canary, dtype)
    out = big_out[1:oh + 1, :ow]
    for name in ("lanczos", "bicubic"):
        big_out[...] = canary
        got = uva.resize(img, dst, name, out=out)
        assert got is out
        assert np.array_equal(out, _want(np.ascontiguousarray(img), dst, name)), name
        assert (big_out[0] == canary).all() and (big_out[-1] == canary).all() and (big_out[1:-1, ow:] == canary).all()


def test_device_entry_with_after_and_before(uva):
    import torch
    net = load_net(uva, "2x")
    rng = np.random.default_rng(8)
    h, w = 90, 130
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    up = net.process_u8(img)                                   # 180 x 260
    d_in = torch.from_numpy(img).cuda()
    d_up = torch.empty((2 * h, 2 * w, 3), dtype=torch.uint8, device="cuda")
    d_rs = torch.empty((135, 200, 3), dtype=torch.uint8, device="cuda")
    d_rs16 = torch.empty((77, 301, 3), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    # the net writes d_up; the resampler, on its own stream, comes after it (after=net) and the net's next work after the resampler
    net.process_u8_device(d_in.data_ptr(), h, w, d_up.data_ptr())
    net.resize_device(d_up.data_ptr(), 2 * h, 2 * w, d_rs.data_ptr(), 135, 200, "bicubic", after=net)
    net.synchronize()
    assert np.array_equal(d_up.cpu().numpy(), up)
    assert np.array_equal(d_rs.cpu().numpy(), _want(up, (135, 200), "bicubic"))
    img16 = rng.integers(0, 65536, (60, 150, 3), dtype=np.uint16)
    d_in16 = torch.from_numpy(img16.view(np.int16)).cuda()
    torch.cuda.synchronize()
    net.resize_device(d_in16.data_ptr(), 60, 150, d_rs16.data_ptr(), 77, 301, "lanczos", bit_depth=16)
    net.synchronize()
    assert np.array_equal(d_rs16.cpu().numpy().view(np.uint16), _want(img16, (77, 301), "lanczos"))


def test_cached_tables_across_geometries(uva):
    """repeated calls and geometries that come back; more geometries than the cache holds"""
    rng = np.random.default_rng(21)
    img = rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)
    sizes = [(20 + k, 30 + 2 * k) for k in range(40)]
    wants = {}
    for rnd in range(2):
        for k, size in enumerate(sizes):
            name = ref.FILTERS[k % 3]
            got = uva.resize(img, size, name)
            if rnd == 0:
                wants[size] = _want(img, size, name)
            assert np.array_equal(got, wants[size]), (rnd, size, name)
    # the same axis with another filter is another table
    a, b = uva.resize(img, (33, 47), "lanczos"), uva.resize(img, (33, 47), "bilinear")
    assert not np.array_equal(a, b) and np.array_equal(a, _want(img, (33, 47), "lanczos")) and np.array_equal(b, _want(img, (33, 47), "bilinear"))


# ---- behind the net ----------------------------------------------------------------------------------------------------
def _composition(uva, net, frame, h, w, in_fmt, out_fmt, size, tile, border, bit_depth, filt, **kw):
    """today's separate calls: -> BGR, the net, the resampler, -> out_fmt"""
    native = "bgr48le" if bit_depth == 16 else "bgr24"
    s = net.scale
    bgr = frame if in_fmt == native else uva.convert_pix(frame, h, w, in_fmt, native, bit_depth=bit_depth, **kw)
    up = (net.process_u16 if bit_depth == 16 else net.process_u8)(np.asarray(bgr).reshape(h, w, 3), tile_size=tile, border=border)
    rs = uva.resize(up, size, filt) if size != (h * s, w * s) else up
    return np.asarray(rs if out_fmt == native else uva.convert_pix(rs, size[0], size[1], native, out_fmt, bit_depth=bit_depth, **kw))


def _frame(fmt, h, w, rng):
    if fmt == "bgr24":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    n = (h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2))
    if fmt == "yuv420p":
        return rng.integers(16, 236, n, dtype=np.uint8)
    return rng.integers(64, 940, n, dtype=np.uint16).astype("<u2").view(np.uint8)        # yuv420p10le


@pytest.mark.parametrize("key,tile,border", [("2x", 0, 0), ("2x", 64, 10), ("4x", 0, 0), ("4x", 64, 10)])
@pytest.mark.parametrize("in_fmt,out_fmt,bit_depth,kw", [
    ("yuv420p", "p010le", 8, {}), ("bgr24", "bgr24", 8, {}),
    ("yuv420p10le", "p010le", 16, dict(chroma_filter="bilinear", chroma_loc="left", colour="bt709"))])
def test_submit_pix_out_size_is_the_composition(uva, key, tile, border, in_fmt, out_fmt, bit_depth, kw):
    net = load_net(uva, key)
    s = net.scale
    h, w = 66, 90
    rng = np.random.default_rng(17 + s + bit_depth)
    for size, filt in (((h * s * 3 // 4, w * s * 3 // 4 + 1), "lanczos"), ((h * s + 30, w * s // 2), "bicubic")):
        frames = [_frame(in_fmt, h, w, rng) for _ in range(5)]
        wants = [_composition(uva, net, f, h, w, in_fmt, out_fmt, size, tile, border, bit_depth, filt, **kw) for f in frames]
        outs = [uva.pix_empty(out_fmt, size[0], size[1], uva.pinned_empty if k % 2 else None) for k in range(len(frames))]
        tickets, got = [], []
        for f, o in zip(frames, outs):
            if len(tickets) == 3:
                got.append(net.collect_u8(tickets.pop(0)))
            tickets.append(net.submit_pix(f, h, w, in_fmt, out=o, out_fmt=out_fmt, tile_size=tile, border=border, bit_depth=bit_depth,
                                          out_size=size, resize_filter=filt, **kw))
        got += [net.collect_u8(t) for t in tickets]
        for k in range(len(frames)):
            assert got[k] is outs[k]
            assert np.array_equal(np.asarray(got[k]).reshape(-1).view(np.uint8), wants[k].reshape(-1).view(np.uint8)), (size, filt, k)
    # the net's own size: the resampler is skipped, the bytes are submit_pix's
    f = _frame(in_fmt, h, w, rng)
    plain = net.collect_u8(net.submit_pix(f, h, w, in_fmt, out_fmt=out_fmt, tile_size=tile, border=border, bit_depth=bit_depth, **kw))
    sized = net.collect_u8(net.submit_pix(f, h, w, in_fmt, out_fmt=out_fmt, tile_size=tile, border=border, bit_depth=bit_depth,
                                          out_size=(h * s, w * s), **kw))
    assert np.array_equal(np.asarray(plain).reshape(-1).view(np.uint8), np.asarray(sized).reshape(-1).view(np.uint8))


def test_submit_pix_out_size_reference_tiles_1080p(uva):
    """the route's own shape: 960/10 tiles, 540p -> 2x -> 1440 x 810, yuv420p both ways, against the composition"""
    net = load_net(uva, "2x")
    h, w, size = 540, 960, (810, 1440)
    rng = np.random.default_rng(4)
    f = _frame("yuv420p", h, w, rng)
    got = net.collect_u8(net.submit_pix(f, h, w, "yuv420p", out_fmt="yuv420p", tile_size=960, border=10, out_size=size))
    assert np.array_equal(got, _composition(uva, net, f, h, w, "yuv420p", "yuv420p", size, 960, 10, 8, "lanczos"))


# ---- the streamer ------------------------------------------------------------------------------------------------------
def _run(argv, data=None, timeout=600):
    r = subprocess.run([sys.executable, "-m", "upscale_video_amd.rawvideo"] + argv, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       cwd=ROOT, timeout=timeout)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r.stdout


@pytest.mark.parametrize("bit_depth,gpus,extra", [(8, "0", []), (16, "0", []), (8, "0,0", []), (8, "0,0", ["--round-robin"])])
def test_streamer_pipe_and_file(uva, tmp_path, bit_depth, gpus, extra):
    net = load_net(uva, "2x")
    h, w, n, tile, size = 40, 58, 7, 32, (61, 87)
    in_fmt, out_fmt = ("yuv420p10le", "p010le") if bit_depth == 16 else ("yuv420p", "yuv420p")
    rng = np.random.default_rng(11 + bit_depth)
    frames = [_frame(in_fmt, h, w, rng) for _ in range(n)]
    want = b"".join(_composition(uva, net, f, h, w, in_fmt, out_fmt, size, tile, 10, bit_depth, "bicubic").tobytes() for f in frames)
    assert len(want) == n * uva.pix_frame_bytes(out_fmt, *size)
    argv = ["-W", str(w), "-H", str(h), "-s", "2", "--tile", str(tile), "--in-pix-fmt", in_fmt, "--out-pix-fmt", out_fmt, "--bit-depth", str(bit_depth),
            "--out-size", "%dx%d" % (size[1], size[0]), "--resize-filter", "bicubic", "-g", gpus] + extra
    data = b"".join(f.tobytes() for f in frames)
    assert _run(argv, data) == want                                                  # pipe -> pipe
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(data)
    _run(argv + ["-i", str(src), "-o", str(dst)])                                    # file -> file (segments with -g 0,0)
    assert os.path.getsize(dst) == len(want) and dst.read_bytes() == want


def test_streamer_anime_pass_and_out_scale(uva):
    one, two = load_net(uva, "1x"), load_net(uva, "2x")
    h, w, n = 40, 58, 4
    size = ref.out_scale_size(h, w, 1.5)             # (60, 88)
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
    want = b"".join(uva.resize(two.process_u8(one.process_u8(f), tile_size=32, border=10), size, "lanczos").tobytes() for f in frames)
    got = _run(["-W", str(w), "-H", str(h), "-s", "2", "-m", "a", "--tile", "32", "--out-scale", "1.5"], b"".join(f.tobytes() for f in frames))
    assert got == want


@pytest.mark.parametrize("bit_depth", [8, 16])
def test_streamer_scale_1_without_a_net(uva, bit_depth):
    h, w, n, size = 30, 44, 3, (45, 50)
    in_fmt, out_fmt = ("yuv420p10le", "p010le") if bit_depth == 16 else ("yuv420p", "bgr24")
    native = "bgr48le" if bit_depth == 16 else "bgr24"
    rng = np.random.default_rng(6)
    frames = [_frame(in_fmt, h, w, rng) for _ in range(n)]
    want = b""
    for f in frames:
        x = uva.resize(uva.convert_pix(f, h, w, in_fmt, native, bit_depth=bit_depth), size, "bilinear")
        want += np.asarray(x if out_fmt == native else uva.convert_pix(x, size[0], size[1], native, out_fmt, bit_depth=bit_depth)).tobytes()
    got = _run(["-W", str(w), "-H", str(h), "-s", "1", "--in-pix-fmt", in_fmt, "--out-pix-fmt", out_fmt, "--bit-depth", str(bit_depth),
                "--out-size", "50x45", "--resize-filter", "bilinear"], b"".join(f.tobytes() for f in frames))
    assert got == want


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_through_every_entry(uva):
    import torch
    from upscale_video_amd import _lib
    L = _lib.load()
    net = load_net(uva, "2x")
    h, w = 16, 16
    src = np.zeros((h, w + 1, 3), np.uint16)
    out = np.zeros(6 * 64 * 64 + 64, np.uint8)
    d_src = torch.zeros(src.nbytes, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(out.size, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sp, op, dsp, dop = src.ctypes.data, out.ctypes.data, d_src.data_ptr(), d_out.data_ptr()
    LZ = 0
    # (oh, ow, filter, bits, in_stride, out_stride) -> a word of the message
    bad = [((3, 16, LZ, 8, 48, 48), b"[1/4, 4]"), ((16, 65, LZ, 8, 48, 195), b"[1/4, 4]"), ((0, 16, LZ, 8, 48, 48), b"at least 1"),
           ((16, -2, LZ, 8, 48, 48), b"at least 1"), ((16, 16, 3, 8, 48, 48), b"filter"), ((16, 16, -1, 8, 48, 48), b"filter"),
           ((16, 16, LZ, 12, 48, 48), b"bits"), ((16, 16, LZ, 16, 97, 96), b"2-byte"), ((16, 16, LZ, 16, 96, 99), b"2-byte"),
           ((16, 16, LZ, 8, 47, 48), b"stride"), ((16, 20, LZ, 8, 48, 59), b"stride")]
    for (oh, ow, f, bits, si, so), word in bad:
        assert L.uva_resize(0, sp, h, w, si, op, oh, ow, so, f, bits) != 0, (oh, ow, f, bits, si, so)
        assert word in L.uva_last_error(), (word, L.uva_last_error())
        assert L.uva_resize_device(0, dsp, h, w, si, dop, oh, ow, so, f, bits, None, net._h) != 0, (oh, ow, f, bits, si, so)
        assert word in L.uva_last_error(), (word, L.uva_last_error())
    assert L.uva_resize(0, None, h, w, 48, op, 16, 16, 48, LZ, 8) != 0 and b"null" in L.uva_last_error()
    frame = np.zeros(h * w * 3 // 2, np.uint8)
    for (oh, ow, f, bits), word in [((7, 32, LZ, 8), b"[1/4, 4]"), ((32, 129, LZ, 8), b"[1/4, 4]"), ((0, 32, LZ, 8), b"at least 1"),
                                    ((32, 32, 5, 8), b"filter"), ((32, 32, LZ, 10), b"bits")]:
        assert L.uva_net_submit_pix_sized(net._h, frame.ctypes.data, 1, h, w, op, 1, 0, 0, 0, oh, ow, f, bits) < 0, (oh, ow, f, bits)
        assert word in L.uva_last_error(), (word, L.uva_last_error())
    assert L.uva_net_submit_pix_sized(net._h, frame.ctypes.data, 1, h, w, op, 6, 0, 0, 0, 32, 32, LZ, 8) < 0 and b"16-bit" in L.uva_last_error()
    assert L.uva_net_submit_pix_sized(net._h, frame.ctypes.data, 1, h, w, op, 1, 32, 0, 0, 32, 32, LZ, 8) < 0 and b"colour" in L.uva_last_error()
    with pytest.raises(ValueError):
        net.submit_pix(frame, h, w, "yuv420p", out_fmt="yuv420p", out_size=(7, 32))
    with pytest.raises(ValueError):
        net.submit_pix(frame, h, w, "yuv420p", out_fmt="yuv420p", out_size=(32, 32), resize_filter="area")
    # ... and the net is as usable as before
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = net.collect_u8(net.submit_pix(img, h, w, "bgr24", out_fmt="bgr24", out_size=(24, 40)))
    assert np.array_equal(got, _want(net.process_u8(img), (24, 40), "lanczos"))
