"""The 16-bit route on the MI355X (-m gpu): the u16 conversion kernels bit for bit against the numpy
restatement (tests/pixfmt16_ref.py), Net.process_u16 against the fp32 and product-mode oracles (in u16 codes: check_u16),
its depth against the 8-bit counterfactual, its edge shapes and inputs, row strides, the device entry and workspace reuse,
bgr24 through the 16-bit route against the u8 route, a 10-bit ramp through p010le, submit_pix16 and the rawvideo streamer
with --bit-depth 16."""
import subprocess
import sys

import numpy as np
import pytest

import pixfmt16_ref as ref
from conftest import ROOT, load_net
from parity_report import U16_PRODUCT, check_f32, check_u16, check_u8, slack

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


def _oracle_raw(om, x, flags, tile, border=10):
    """fp32 oracle on the float HWC frame x, tiles composed as upscale_image does (tile <= 0: whole frame) -> float
    [h*s][w*s][3], unclamped"""
    from upscale_video_amd import upscale_processing as up
    h, w, _ = x.shape
    s = om.scale
    x = np.ascontiguousarray(x.transpose(2, 0, 1))
    if tile <= 0:
        return om.forward(x, flags=flags).transpose(1, 2, 0)
    out = np.zeros((h * s, w * s, 3), np.float32)
    for ty in range((h + tile - 1) // tile):
        for tx in range((w + tile - 1) // tile):
            (y0, y1, x0, x1), (t, b, lft, rgt) = up.tile_window(tile, ty, tx, h, w, border)
            o = om.forward(np.ascontiguousarray(x[:, y0 - t:y1 + b, x0 - lft:x1 + rgt]), flags=flags).transpose(1, 2, 0)
            out[y0 * s:y1 * s, x0 * s:x1 * s] = o[t * s:(t + y1 - y0) * s, lft * s:(lft + x1 - x0) * s]
    return out


def _oracle_u16(om, x16, flags, tile, border=10, head=False):
    """fp32 oracle on x16 / 65535 (head=True: on the head's rounded operand, for the product-mode comparison), tiles composed
    as upscale_image does (tile <= 0: whole frame) -> float [h*s][w*s][3], clamped to [0, 1] as the u16 output is"""
    x = _head_input(x16) if head else x16.astype(np.float32) / 65535.0
    return np.clip(_oracle_raw(om, x, flags, tile, border), 0, 1)


def _smooth16(h, w, seed=0):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    rng = np.random.default_rng(seed)
    ch = [0.5 + 0.45 * np.sin(xx / (7 + 5 * k) + yy / (11 + 3 * k) + rng.uniform(0, 6)) for k in range(3)]
    return np.rint(np.stack(ch, -1) * 65535).astype(np.uint16)


def _up(a, s):
    return np.repeat(np.repeat(a, s, 0), s, 1)


def _tail_round(y):
    """clamp(rint(y * 65535), 0, 65535): what the tail stores (rint: half to even)"""
    return np.clip(np.rint(y * 65535), 0, 65535).astype(np.uint16)


def _fp32_u16(om, x16, tile, border=10):
    """the fp32 oracle on x16 / 65535, rounded as the tail rounds -> u16 [h*s][w*s][3]"""
    return _tail_round(_oracle_raw(om, x16.astype(np.float32) / 65535.0, 0, tile, border))


def _product_u16(om, oracle, x16, tile, border=10):
    """the product-mode oracle as the 16-bit route computes the frame -> u16 [h*s][w*s][3]: the net on the head's operand
    (_head_input), then the tail's own sum ((conv + bias) + residual) * 65535 in fp32 with the residual as the tail reads it,
    fp32 (v / 257) * (1/255) -- the fp16 rounding of the head's operand is not in it (up to 16 codes near full scale) -- and
    the tail's rounding.  The net ends in conv + nearest-upsampled input, so the oracle's own residual comes off exactly
    enough (fp32 rounding, ~1e-7)"""
    s = om.scale
    xh = _head_input(x16)
    body = _oracle_raw(om, xh, oracle.product_flags(), tile, border).astype(np.float64) - _up(xh, s)
    res = (x16.astype(np.float32) / np.float32(257.0)) * np.float32(1 / 255.0)
    y = (body.astype(np.float32) + _up(res, s)) * np.float32(65535.0)
    return np.clip(np.rint(y), 0, 65535).astype(np.uint16)


def _product_bars(key):
    """the 16-bit route's product-mode bars in codes (tests/golden/parity_slack.json "{key}/u16/...", tools/parity_slack.py):
    RMS; max |diff|, whose fallback is the float route's max bar the route borrowed before it had its own"""
    return {"max_rms": slack(key, "u16", "rms_codes", U16_RMS_CAP),
            "max_codes": slack(key, "u16", "max_codes", 65535 * slack(key, "float", "f32_abs", 4e-3))}


U16_RMS_CAP = 37.0      # half the RMS of an 8-bit hop on content spread over the codes (257 / sqrt(12) / 2)
FP32_MAX_CODES = 6e-3 * 65535
# RMS against the fp32 oracle, in codes: measured maximum (2x 17.3, 4x 44.2: the depth test's ramp) + 2
FP32_RMS = {"2x": 19.5, "4x": 46.5}


@pytest.mark.parametrize("key,h,w,tile", [("2x", 70, 75, 0), ("2x", 70, 75, 64), ("2x", 150, 170, 960), ("4x", 45, 60, 0),
                                          ("4x", 45, 60, 64), ("2x", 1080, 1920, 0)])
def test_process_u16_matches_oracle(uva, oracle, oracle_models, key, h, w, tile):
    net, om = load_net(uva, key), oracle_models[key]
    golden = oracle.synthetic_frame(h, w, kind="random", seed=h + w)
    for name, x16 in (("golden*257", golden.astype(np.uint16) * 257), ("smooth16", _smooth16(h, w))):
        if h * w > 100000 and name == "golden*257":
            continue                     # (the 1080p frame: the genuinely 16-bit one only, the oracle takes a while)
        got16 = net.process_u16(x16, tile_size=tile, border=10)
        got = got16.astype(np.float64) / 65535.0
        raw32 = _oracle_raw(om, x16.astype(np.float32) / 65535.0, 0, tile)
        want32 = np.clip(raw32, 0, 1)
        tag = f"u16 {key} {w}x{h} t{tile} {name}"
        check_f32(tag, got, want32, vs="fp32 oracle", max_abs=6e-3, model=key, route="u16")
        check_u16(tag, got16, _tail_round(raw32), vs="fp32 oracle", max_codes=FP32_MAX_CODES, max_rms=FP32_RMS[key], model=key,
                  route="u16", structure=False)
        if h * w <= 100000:
            want16 = _oracle_u16(om, x16, oracle.product_flags(), tile, head=True)
            check_f32(tag, got, want16, vs="product-mode oracle", model=key, route="u16",
                      max_abs=slack(key, "float", "f32_abs", 4e-3))
            check_u16(tag, got16, _product_u16(om, oracle, x16, tile), vs=U16_PRODUCT, model=key, route="u16",
                      **_product_bars(key))


def test_process_u16_4x_1080p_matches_fp32_oracle(uva, oracle_models):
    """4x at 1080p against the fp32 oracle on every one of its 99.5 M samples (the 2x frame: test_process_u16_matches_oracle).
    The product-mode oracle itself -- the 4x net's fp16 arithmetic -- is 437 codes (6.7e-3) from the fp32 oracle at worst on
    this frame, so the frame is held to the u8 route's fp32 bar, 2 u8 steps (514 codes), and to FP32_RMS"""
    net, om = load_net(uva, "4x"), oracle_models["4x"]
    x16 = _smooth16(1080, 1920)
    got16 = net.process_u16(x16, tile_size=0, border=10)
    raw32 = _oracle_raw(om, x16.astype(np.float32) / np.float32(65535.0), 0, 0)
    tag = "u16 4x 1920x1080 t0 smooth16"
    check_f32(tag, got16.astype(np.float32) / np.float32(65535.0), np.clip(raw32, 0, 1), vs="fp32 oracle", max_abs=2 / 255,
              model="4x", route="u16")
    check_u16(tag, got16, _tail_round(raw32), vs="fp32 oracle", max_codes=2 * 257, max_rms=FP32_RMS["4x"], model="4x",
              route="u16", structure=False)


def _smooth_full(h, w, seed=0):
    """smooth 16-bit content over the whole range, 0 .. 65535 (_smooth16 keeps to 0.05 .. 0.95)"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    rng = np.random.default_rng(seed)
    ch = [0.5 + 0.5 * np.sin(xx / (9 + 4 * k) + yy / (13 + 3 * k) + rng.uniform(0, 6)) for k in range(3)]
    return np.rint(np.stack(ch, -1) * 65535).astype(np.uint16)


def _ramp16(h, w):
    """_ramp10's slow ramp plus soft radial gradient in BGR48 (full range, 0 .. 65535, a slight tint per channel): about 110
    codes per pixel across 480 columns, so an 8-bit step spans two to three input pixels"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    rad = np.hypot(yy - h / 2, xx - w / 2) / np.hypot(h / 2, w / 2)
    v = 0.8 * xx / (w - 1) + 0.2 * (1 - rad)
    return np.rint(np.stack([v, 0.02 + 0.96 * v, 1 - 0.97 * (1 - v)], -1).clip(0, 1) * 65535).astype(np.uint16)


X257_BAR = 2 / 257      # share of unclamped samples that may be multiples of 257 (a 16-bit route: ~1/257; an 8-bit hop: all)


@pytest.mark.parametrize("content", ["smooth", "ramp"])
@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("key", ["2x", "4x"])
def test_process_u16_keeps_its_depth(uva, oracle, oracle_models, key, tile, content):
    """THE POINT of the route, on Net.process_u16 itself.  y = the product-mode oracle rounded as the tail rounds, q8 =
    widen(narrow(y)): what the route would give with an 8-bit hop anywhere in it (the counterfactual, computed here, no
    fault injected).  The route's RMS error against y is at most half of q8's, and hardly any unclamped sample is a multiple
    of 257 (q8: every one).  Against the fp32 oracle: RMS within FP32_RMS (measured: the fp16 trunk's own error, which at 4x
    is more than half an 8-bit hop's on a ramp).  q8 is recorded next to each comparison and must fail its RMS and
    multiple-of-257 bars.  The row / column statistic applies to the product-mode comparison of the smooth frame only: the
    ramp's error follows the frame's edges (UNIFORM), and against the fp32 oracle the fp16 trunk's own error follows the
    content by design."""
    net, om = load_net(uva, key), oracle_models[key]
    x16 = _smooth_full(96, 128, seed=3) if content == "smooth" else _ramp16(120, 480)
    h, w, _ = x16.shape
    got = net.process_u16(x16, tile_size=tile, border=10)
    y = _product_u16(om, oracle, x16, tile)
    q8 = ref.widen(ref.narrow(y))
    rms8 = float(np.sqrt(((q8.astype(np.float64) - y) ** 2).mean()))
    tag = f"u16 depth {key} {w}x{h} t{tile} {content}"
    bars16 = dict(_product_bars(key), max_x257=X257_BAR)
    bars16["max_rms"] = min(bars16["max_rms"], 0.5 * rms8)
    bars32 = {"max_rms": FP32_RMS[key], "max_x257": X257_BAR}
    for vs, want, bars in ((U16_PRODUCT, y, bars16), ("fp32 oracle", _fp32_u16(om, x16, tile), bars32)):
        check_u16(tag, got, want, vs=vs, model=key, route="u16", structure=vs == U16_PRODUCT and content != "ramp", **bars)
        check_u16(tag + " 8-bit hop", q8, want, vs=vs + " (counterfactual)", model=key, route="u16", counterfactual=True, **bars)


def _edge_input(kind, h, w, rng):
    if kind == "noise":
        return rng.integers(0, 65536, (h, w, 3), dtype=np.uint16)
    if kind == "zero":
        return np.zeros((h, w, 3), np.uint16)
    if kind == "max":
        return np.full((h, w, 3), 65535, np.uint16)
    if kind == "top":                   # the codes that would be inf in fp16 without the head's 1/257
        return rng.integers(65520, 65536, (h, w, 3), dtype=np.uint16)
    if kind == "bottom":
        return rng.integers(0, 16, (h, w, 3), dtype=np.uint16)
    # "gradient": 0 .. 65535 along the diagonal, channels in different directions: both clamp ends are reached
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    t = (yy + xx) / max(h + w - 2, 1)
    return np.rint(np.stack([t, 1 - t, (yy / max(h - 1, 1) + (1 - t)) / 2], -1) * 65535).astype(np.uint16)


EDGE_INPUTS = ("noise", "zero", "max", "top", "bottom", "gradient")
# Inputs whose error against the product-mode oracle follows the frame's and the tiles' edges rather than the content, so
# that the row / column statistic (parity_report.structure_codes) would flag the net's zero padding: constant frames here
# ("top" too: every code of 65520 .. 65535 is fp16(v / 257) = 255, the head's operand of 65535), the ramp of the depth test.
# Measured on the 4x ramp: the last ten output rows at up to twice the frame's mean |diff| of 0.48 codes, no bias; a row of
# 1920 x 3 samples tells 1.7x its neighbours' rate at 30 standard errors.
UNIFORM = ("zero", "max", "top")


@pytest.mark.parametrize("h,w,tile", [(1, 1, 0), (1, 17, 0), (2, 16, 0), (3, 15, 0), (5, 33, 0), (17, 31, 0), (16, 64, 0),
                                      (33, 47, 0), (65, 65, 64)])
@pytest.mark.parametrize("key", ["2x", "4x"])
def test_process_u16_edges(uva, oracle, oracle_models, key, h, w, tile):
    """Shapes where the tails' u16 residual staging (lane < 32 * SB, lane >> 5, partial 16-pixel row segments) and the head's
    clamped fetches meet their edges -- the last one a tiled frame whose last tile row and column are one pixel wide -- on
    inputs at both ends of the range, against both oracles: product mode (the route's RMS and max bars, and the row / column
    statistic) and fp32 (6e-3)"""
    net, om = load_net(uva, key), oracle_models[key]
    rng = np.random.default_rng(h * 131 + w)
    for kind in EDGE_INPUTS:
        x16 = _edge_input(kind, h, w, rng)
        got = net.process_u16(x16, tile_size=tile, border=10)
        tag = f"u16 edge {key} {w}x{h} t{tile} {kind}"
        check_u16(tag, got, _product_u16(om, oracle, x16, tile), vs=U16_PRODUCT, model=key, route="u16",
                  structure=kind not in UNIFORM, **_product_bars(key))
        check_u16(tag, got, _fp32_u16(om, x16, tile), vs="fp32 oracle", model=key, route="u16", max_codes=FP32_MAX_CODES,
                  structure=False)


def _strides(row):
    """two row strides past a row of `row` bytes: the first = 2 mod 4 (every other row only 2-byte aligned), the second a
    multiple of 16"""
    return row + 1 + (2 - (row + 1)) % 4, (row // 16 + 1) * 16


@pytest.mark.parametrize("tile", [0, 16])
@pytest.mark.parametrize("key", ["2x", "4x"])
def test_u16_row_strides_device_entry_and_repeatability(uva, key, tile):
    """uva_net_process_u16 with padded rows (a stride = 2 mod 4: every other row only 2-byte aligned; a multiple of 16) is
    bit for bit the tight call and leaves the padding alone; an odd stride is refused; uva_net_process_u16_device on torch
    tensors gives the host call's bytes; the same frame twice gives the same bytes"""
    import ctypes
    import torch
    from upscale_video_amd import _lib
    if not torch.cuda.is_available():
        pytest.fail("torch cannot see the GPU in this process")
    L = _lib.load()
    net = load_net(uva, key)
    s = net.scale
    h, w = 21, 37
    x16 = _edge_input("noise", h, w, np.random.default_rng(4))
    want = net.process_u16(x16, tile_size=tile, border=4)
    assert np.array_equal(want, net.process_u16(x16, tile_size=tile, border=4))
    in_row, out_row = w * 6, w * s * 6
    si, so = _strides(in_row), _strides(out_row)
    assert si[0] % 4 == 2 and so[0] % 4 == 2 and si[1] % 16 == 0 and so[1] % 16 == 0 and min(si) > in_row and min(so) > out_row
    for in_stride, out_stride in ((si[0], so[0]), (si[1], so[1]), (si[0], so[1]), (si[1], so[0])):
        src = np.full((h, in_stride), 0xA5, np.uint8)
        src[:, :in_row] = x16.reshape(h, in_row // 2).view(np.uint8)
        dst = np.full((h * s, out_stride), 0x5A, np.uint8)
        _lib.check(L.uva_net_process_u16(net._h, src.ctypes.data, h, w, in_stride, dst.ctypes.data, out_stride, tile, 4))
        assert np.array_equal(dst[:, :out_row].copy().view(np.uint16).reshape(h * s, w * s, 3), want), (in_stride, out_stride)
        assert (dst[:, out_row:] == 0x5A).all(), (in_stride, out_stride, "the padding was written")
        d_src = torch.from_numpy(src).cuda()
        d_dst = torch.full((h * s, out_stride), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _lib.check(L.uva_net_process_u16_device(net._h, ctypes.c_void_p(d_src.data_ptr()), h, w, in_stride,
                                                ctypes.c_void_p(d_dst.data_ptr()), out_stride, tile, 4))
        net.synchronize()
        assert np.array_equal(d_dst.cpu().numpy(), dst), (in_stride, out_stride, "device entry")
    src = np.zeros((h, in_row + 1), np.uint8)
    dst = np.zeros((h * s, out_row + 2), np.uint8)
    for in_stride, out_stride in ((in_row + 1, out_row), (in_row, out_row + 1)):
        assert L.uva_net_process_u16(net._h, src.ctypes.data, h, w, in_stride, dst.ctypes.data, out_stride, tile, 4) != 0
        assert b"2-byte aligned" in L.uva_last_error()
    assert not dst.any(), "a refused call wrote its output"


@pytest.mark.parametrize("key", ["2x", "4x"])
def test_u16_workspace_reuse(uva, key):
    """Frame sizes and tilings in turn on ONE net -- a u8 frame among them, on the same workspace cache -- give exactly the
    bytes a fresh net gives for each: nothing stale is reused"""
    net = load_net(uva, key)
    rng = np.random.default_rng(17)
    seq = [(70, 75, 64, 16), (1, 17, 0, 16), (33, 47, 0, 16), (70, 75, 0, 16), (70, 75, 64, 8), (16, 64, 16, 16), (33, 47, 0, 16)]
    frames = [(_edge_input("noise", h, w, rng), t, bits) for h, w, t, bits in seq]
    got = [net.process_u16(x, tile_size=t, border=10) if bits == 16 else net.process_u8(ref.narrow(x), tile_size=t, border=10)
           for x, t, bits in frames]
    for (x, t, bits), g in zip(frames, got):
        fresh = load_net(uva, key)
        want = fresh.process_u16(x, tile_size=t, border=10) if bits == 16 else fresh.process_u8(ref.narrow(x), tile_size=t, border=10)
        assert np.array_equal(g, want), (x.shape, t, bits)


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
