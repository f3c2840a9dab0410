"""The 16-bit route on the MI355X (-m gpu): the u16 conversion kernels bit for bit against the numpy
restatement (tests/pixfmt16_ref.py), Net.process_u16 against the fp32 oracle, bgr24 through the 16-bit route against the u8
route, what the route is for (a 10-bit ramp keeps its depth), submit_pix16 and the rawvideo streamer with --bit-depth 16."""
import subprocess
import sys

import numpy as np
import pytest

import pixfmt16_ref as ref
from conftest import ROOT, load_net
from parity_report import check_f32, check_u8, slack

pytestmark = pytest.mark.gpu

YUV = ("yuv420p", "nv12", "p010le", "yuv420p10le")
COLOURS = [(m, r) for m in ("bt601", "bt709") for r in ("tv", "pc")]
SIZES = [(1, 1), (3, 5), (7, 40), (970, 965), (1080, 1920)]


def _random_packed(fmt, h, w, rng):
    n = ref.frame_bytes(fmt, h, w)
    if fmt == "p010le":
        return rng.integers(0, 65536, n // 2, dtype=np.uint16).astype("<u2").view(np.uint8)
    if fmt == "yuv420p10le":          # any 16-bit word: the high six bits must be ignored
        return rng.integers(0, 65536, n // 2, dtype=np.uint16).astype("<u2").view(np.uint8)
    return rng.integers(0, 256, n, dtype=np.uint8)


@pytest.mark.parametrize("h,w", SIZES)
def test_conversions_bit_exact(uva, h, w):
    rng = np.random.default_rng(h * 7 + w)
    big = h * w > 100000
    for m, r in (COLOURS[:1] + COLOURS[-1:] if big else COLOURS):
        full = r == "pc"
        bgr16 = rng.integers(0, 65536, (h, w, 3), dtype=np.uint16)
        for fmt in YUV + ("bgr24",):
            got = uva.convert_pix(bgr16, h, w, "bgr48le", fmt, m, r, bit_depth=16)
            assert np.array_equal(got.reshape(-1).view(np.uint8), ref.bgr16_to_pix(bgr16, fmt, m, full)), (fmt, m, r, "from u16")
            p = _random_packed(fmt, h, w, rng)
            got = uva.convert_pix(p, h, w, fmt, "bgr48le", m, r, bit_depth=16)
            assert np.array_equal(got, ref.pix_to_bgr16(p, fmt, h, w, m, full)), (fmt, m, r, "to u16")
        # Y'CbCr -> Y'CbCr through u16 BGR, and the 8-bit route's yuv420p10le
        p = _random_packed("yuv420p10le", h, w, rng)
        got = uva.convert_pix(p, h, w, "yuv420p10le", "p010le", m, r, bit_depth=16)
        assert np.array_equal(got.reshape(-1), ref.convert16(p, "yuv420p10le", "p010le", h, w, m, full))
        bgr8 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        got = uva.convert_pix(bgr8, h, w, "bgr24", "yuv420p10le", m, r)
        assert np.array_equal(got.reshape(-1), ref.bgr_to_pix8(bgr8, "yuv420p10le", m, full))
        got = uva.convert_pix(p, h, w, "yuv420p10le", "bgr24", m, r)
        assert np.array_equal(got, ref.pix_to_bgr8(p, "yuv420p10le", h, w, m, full))


def test_refusals(uva):
    from upscale_video_amd import _lib
    L = _lib.load()
    img = np.zeros((8, 8, 3), np.uint16)
    with pytest.raises(_lib.UvaError, match="2x and 4x Compact"):
        load_net(uva, "1x").process_u16(img)
    out = np.zeros(6 * 64, np.uint8)
    assert L.uva_pix_convert(0, img.ctypes.data, 6, out.ctypes.data, 1, 8, 8, 0) != 0
    assert b"16-bit" in L.uva_last_error()


def _head_input(x16):
    """what headp_kernel<64, 2> feeds the net: fp16(v * (1/257)) in fp32, the 1/255 on the accumulator"""
    return np.float16(x16.astype(np.float32) * np.float32(1 / 257.0)).astype(np.float32) / np.float32(255.0)


def _oracle_u16(om, x16, flags, tile, border=10, head=False):
    """fp32 oracle on x16 / 65535 (head=True: on the head's rounded operand, for the product-mode comparison), tiles composed
    as upscale_image does (tile <= 0: whole frame) -> float [h*s][w*s][3], clamped to [0, 1] as the u16 output is"""
    from upscale_video_amd import upscale_processing as up
    h, w, _ = x16.shape
    s = om.scale
    x = np.ascontiguousarray((_head_input(x16) if head else x16.astype(np.float32) / 65535.0).transpose(2, 0, 1))
    if tile <= 0:
        return np.clip(om.forward(x, flags=flags).transpose(1, 2, 0), 0, 1)
    out = np.zeros((h * s, w * s, 3), np.float32)
    for ty in range((h + tile - 1) // tile):
        for tx in range((w + tile - 1) // tile):
            (y0, y1, x0, x1), (t, b, lft, rgt) = up.tile_window(tile, ty, tx, h, w, border)
            o = om.forward(np.ascontiguousarray(x[:, y0 - t:y1 + b, x0 - lft:x1 + rgt]), flags=flags).transpose(1, 2, 0)
            out[y0 * s:y1 * s, x0 * s:x1 * s] = o[t * s:(t + y1 - y0) * s, lft * s:(lft + x1 - x0) * s]
    return np.clip(out, 0, 1)


def _smooth16(h, w, seed=0):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    rng = np.random.default_rng(seed)
    ch = [0.5 + 0.45 * np.sin(xx / (7 + 5 * k) + yy / (11 + 3 * k) + rng.uniform(0, 6)) for k in range(3)]
    return np.rint(np.stack(ch, -1) * 65535).astype(np.uint16)


@pytest.mark.parametrize("key,h,w,tile", [("2x", 70, 75, 0), ("2x", 70, 75, 64), ("2x", 150, 170, 960), ("4x", 45, 60, 0),
                                          ("4x", 45, 60, 64), ("2x", 1080, 1920, 0)])
def test_process_u16_matches_oracle(uva, oracle, oracle_models, key, h, w, tile):
    net, om = load_net(uva, key), oracle_models[key]
    golden = oracle.synthetic_frame(h, w, kind="random", seed=h + w)
    for name, x16 in (("golden*257", golden.astype(np.uint16) * 257), ("smooth16", _smooth16(h, w))):
        if h * w > 100000 and name == "golden*257":
            continue                     # (the 1080p frame: the genuinely 16-bit one only, the oracle takes a while)
        got = net.process_u16(x16, tile_size=tile, border=10).astype(np.float64) / 65535.0
        want32 = _oracle_u16(om, x16, 0, tile)
        tag = f"u16 {key} {w}x{h} t{tile} {name}"
        check_f32(tag, got, want32, vs="fp32 oracle", max_abs=6e-3, model=key, route="u16")
        if h * w <= 100000:
            want16 = _oracle_u16(om, x16, oracle.product_flags(), tile, head=True)
            check_f32(tag, got, want16, vs="product-mode oracle", model=key, route="u16",
                      max_abs=slack(key, "float", "f32_abs", 4e-3))


@pytest.mark.parametrize("key,tile", [("2x", 64), ("4x", 0), ("2x", 960)])
def test_bgr24_through_u16_matches_u8_route(uva, oracle, key, tile):
    net = load_net(uva, key)
    h, w = 96, 130
    img = oracle.synthetic_frame(h, w, kind="random", seed=5)
    u8 = net.process_u8(img, tile_size=tile, border=10)
    via16 = ref.narrow(net.process_u16(ref.widen(img), tile_size=tile, border=10))
    check_u8(f"u16 route as bgr24 {key} t{tile}", via16, u8, vs="u8 route", max_lsb=1, model=key, route="u16",
             max_share=slack(key, "tiled", "u8_differ_share", 5e-2))


def _ramp10(h, w):
    """a slow full-range 10-bit luma ramp plus a soft radial gradient, neutral chroma: p010le at 1080p, limited range"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    rad = np.hypot(yy - h / 2, xx - w / 2) / np.hypot(h / 2, w / 2)
    y = np.rint(64 + 876 * (0.8 * xx / (w - 1) + 0.2 * (1 - rad))).astype(np.int64)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return ref.pack("p010le", y, np.full((ch, cw), 512), np.full((ch, cw), 512))


def test_ten_bit_ramp_keeps_its_depth(uva, oracle_models):
    """THE POINT: p010le -> 2x -> p010le.  The 16-bit route's Y' error against the ideal (fp32 oracle on the exact 10-bit
    input, converted in float64) is at most half the 8-bit route's, and it fills at least twice as many Y' levels.  A level is
    filled when it holds at least a quarter of an even share of the pixels over the ideal's span: the 8-bit route's output
    also REACHES most codes, where the net's B, G, R differ by one 8-bit step (a few pixels each), but a band-free ramp puts
    comparable counts on every code and a banded one on every third or fourth."""
    h, w = 1080, 1920
    net, om = load_net(uva, "2x"), oracle_models["2x"]
    p = _ramp10(h, w)
    outs = {}
    for bd in (8, 16):
        outs[bd] = net.collect_u8(net.submit_pix(p, h, w, "p010le", out_fmt="p010le", tile_size=960, border=10, bit_depth=bd))
    y, u, v = ref.planes(p, "p010le", h, w)
    up2 = lambda a: np.repeat(np.repeat(a, 2, 0), 2, 1)[:h, :w]   # noqa: E731
    b, g, r = ref.float_inv(y, up2(u), up2(v), "bt601", False, 10)
    x16 = np.clip(np.stack([b, g, r], -1) / 65535.0, 0, 1)
    o = np.clip(om.forward(np.ascontiguousarray(x16.astype(np.float32).transpose(2, 0, 1))).transpose(1, 2, 0).astype(np.float64), 0, 1)
    ideal_y, _, _ = ref.float_fwd(o[..., 2] * 65535, o[..., 1] * 65535, o[..., 0] * 65535, "bt601", False, 10)
    share = ideal_y.size / (np.rint(ideal_y.max()) - np.rint(ideal_y.min()) + 1)
    rms, levels = {}, {}
    for bd, out in outs.items():
        gy = ref.planes(out, "p010le", 2 * h, 2 * w)[0].astype(np.float64)
        rms[bd] = float(np.sqrt(((gy - ideal_y) ** 2).mean()))
        _, counts = np.unique(gy, return_counts=True)
        levels[bd] = int((counts >= share / 4).sum())
    check_f32("p010le ramp 2x 1080p: Y' RMS in codes, 16-bit route", np.array([rms[16]]), np.array([0.0]), vs="float64 ideal",
              max_abs=0.5 * rms[8])
    assert levels[16] >= 2 * levels[8], (levels, rms)


def test_submit_pix16_in_flight(uva):
    from upscale_video_amd import ncnn
    net = load_net(uva, "2x")
    h, w, tile = 66, 90, 32
    rng = np.random.default_rng(9)
    frames = [_random_packed("yuv420p10le", h, w, rng) for _ in range(4)]
    want = [ref.bgr16_to_pix(net.process_u16(ref.pix_to_bgr16(f, "yuv420p10le", h, w), tile_size=tile, border=10), "p010le")
            for f in frames]
    for pinned in (False, True):
        outs = [ncnn.pix_empty("p010le", 2 * h, 2 * w, ncnn.pinned_empty if pinned else None) for _ in frames]
        tickets, got = [], []
        for f, o in zip(frames, outs):
            if len(tickets) == 3:
                got.append(net.collect_u8(tickets.pop(0)))
            tickets.append(net.submit_pix(f, h, w, "yuv420p10le", out=o, out_fmt="p010le", tile_size=tile, border=10, bit_depth=16))
        got += [net.collect_u8(t) for t in tickets]
        for k in range(len(frames)):
            assert np.array_equal(got[k].reshape(-1), want[k]), (pinned, k)


def test_rawvideo_bit_depth_16(uva, tmp_path):
    from upscale_video_amd import rawvideo
    net = load_net(uva, "2x")
    h, w, n, tile = 40, 58, 5, 32
    rng = np.random.default_rng(11)
    frames = [_random_packed("yuv420p10le", h, w, rng) for _ in range(n)]
    src = tmp_path / "in.yuv"
    src.write_bytes(b"".join(f.tobytes() for f in frames))
    want = b"".join(net.collect_u8(net.submit_pix(f, h, w, "yuv420p10le", out_fmt="p010le", tile_size=tile, border=10,
                                                   bit_depth=16)).tobytes() for f in frames)
    geo = ["-W", str(w), "-H", str(h), "-s", "2", "--tile", str(tile), "--in-pix-fmt", "yuv420p10le", "--out-pix-fmt", "p010le",
           "--bit-depth", "16"]
    for gpus in ("0", "0,0"):
        dst = tmp_path / ("out_%s.p010" % gpus.replace(",", "_"))
        assert rawvideo.main(["-i", str(src), "-o", str(dst), "-g", gpus] + geo) == 0
        assert dst.read_bytes() == want, gpus
    r = subprocess.run([sys.executable, "-m", "upscale_video_amd.rawvideo", "-g", "0,0"] + geo, input=src.read_bytes(),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout == want
