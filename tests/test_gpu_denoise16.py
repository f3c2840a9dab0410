"""`-m n=K` at --bit-depth 16 on the MI355X (csrc/uva_denoise16.hip.h): every kernel bit for bit against
the definition (tests/nlm16_ref.py), the host and device calls, and the raw-video route against the composition of its stages'
own calls."""
import ctypes

import numpy as np
import pytest

import nlm16_ref as ref
from conftest import load_net
from upscale_video_amd import _lib, rawvideo

pytestmark = pytest.mark.gpu


def _stage(stage, arr, strength=0.0):
    a = np.ascontiguousarray(arr, np.uint16)
    h, w = a.shape[:2]
    out = np.empty(a.shape, np.uint16)
    _lib.check(_lib.load().uva_debug_denoise16_stage(0, stage, a.ctypes.data, h, w, ctypes.c_float(strength), out.ctypes.data))
    return out


def _denoise16(img, K, pad_in=0, pad_out=0):
    """uva_denoise_u16 on a frame whose rows are pad_in / pad_out samples apart from dense"""
    h, w = img.shape[:2]
    src = np.full((h, w * 3 + pad_in), 0xABCD, np.uint16)
    src[:, :w * 3] = img.reshape(h, w * 3)
    dst = np.full((h, w * 3 + pad_out), 0x1234, np.uint16)
    _lib.check(_lib.load().uva_denoise_u16(0, src.ctypes.data, h, w, src.strides[0], dst.ctypes.data, dst.strides[0], float(K), float(K)))
    assert (dst[:, w * 3:] == 0x1234).all()                                              # nothing written between the rows
    return np.ascontiguousarray(dst[:, :w * 3]).reshape(h, w, 3)


def _noisy16(h, w):
    """the planes of tests/test_denoise.py test_nlm_stage_is_bit_exact, widened, low bits filled"""
    rng = np.random.default_rng(h * 100 + w)
    base = np.clip(rng.normal(120, 30, (h, w, 2)), 0, 255)
    noisy = np.clip(base + rng.normal(0, 6, (h, w, 2)), 0, 255)
    return np.clip(np.rint(noisy * 257.0) + rng.integers(-128, 129, (h, w, 2)), 0, 65535).astype(np.uint16)


def _grainy16(h, w, seed):
    """a frame with structure (8 x 8 blocks of colour) and grain of sigma 600 codes = 2.3 eight-bit levels: K = 3 has patches
    to average, so the stage changes a sample by about the grain's mean size (0.8 sigma) and not by a rounding's"""
    rng = np.random.default_rng(seed)
    base = np.clip(rng.normal(30000, 9000, (-(-h // 8), -(-w // 8), 3)), 0, 65535).repeat(8, 0).repeat(8, 1)[:h, :w]
    return np.clip(base + rng.normal(0, 600, (h, w, 3)), 0, 65535).astype(np.uint16)


@pytest.mark.parametrize("strength", [1.0, 3.0, 10.0, 30.0])
@pytest.mark.parametrize("h,w", [(33, 47), (16, 16), (5, 3), (1, 1), (40, 18), (17, 70)])
def test_nlm16_stage_is_bit_exact(uva, h, w, strength):
    noisy = _noisy16(h, w)
    one = np.ascontiguousarray(noisy[..., 0])
    assert np.array_equal(_stage(2, one, strength), ref.nlm_plane16(one, strength))
    assert np.array_equal(_stage(3, noisy, strength), ref.nlm_plane16(noisy, strength))


@pytest.mark.parametrize("strength", [3.0, 30.0])
def test_nlm16_on_a_full_range_checkerboard(uva, strength):
    """0 / 65535 checkerboard plus noise: squared differences at the top of 32 bits, patch distances far past the table's end
    (the index clamp), weighted sums past 32 bits"""
    h, w = 37, 45
    rng = np.random.default_rng(65535)
    cb = ((np.add.outer(np.arange(h), np.arange(w)) & 1) * 65535)[..., None].repeat(2, 2)
    cb[..., 1] = 65535 - cb[..., 1]
    noise = rng.integers(0, 700, (h, w, 2))
    plane = np.where(cb > 0, cb - noise, cb + noise).astype(np.uint16)
    plane[:4, :4] = np.array([0, 65535], np.uint16)                                    # exact extremes as well
    one = np.ascontiguousarray(plane[..., 0])
    want1, want2 = ref.nlm_plane16(one, strength), ref.nlm_plane16(plane, strength)
    assert not np.array_equal(want1, one)                                              # (the noise is averaged: not an identity)
    assert np.array_equal(_stage(2, one, strength), want1)
    assert np.array_equal(_stage(3, plane, strength), want2)


def test_lab16_stages_are_bit_exact_on_the_fixed_colour_set(uva):
    """the 64-level cube x 257, 2^20 seeded random 16-bit colours, the eight corners: forward on them as BGR, inverse on them
    as Lab triples (every L16 / a16 / b16 combination class, out-of-gamut ones included) and on the forward results"""
    c = ref.colour_set()
    n = len(c)
    w = 1024
    img = np.zeros((-(-n // w) * w, 3), np.uint16)
    img[:n] = c
    img = img.reshape(-1, w, 3)
    lab = ref.bgr2lab16(img)
    assert np.array_equal(_stage(0, img), lab)
    assert np.array_equal(_stage(1, img), ref.lab2bgr16(img))
    assert np.array_equal(_stage(1, lab), ref.lab2bgr16(lab))


@pytest.mark.parametrize("h,w", [(33, 47), (16, 16)])
def test_denoise_u16_end_to_end_with_strided_rows(uva, h, w):
    img = _grainy16(h, w, h + w)
    want = ref.denoise16(img, 3)
    assert np.array_equal(_denoise16(img, 3, pad_in=5, pad_out=9), want)
    assert np.array_equal(_denoise16(img, 3), want)
    assert np.abs(want.astype(float) - img).mean() > 100                                # something was removed


def test_denoise_u16_device_gives_the_host_calls_bytes(uva):
    import torch
    h, w = 33, 47
    img = _grainy16(h, w, 9)
    want = _denoise16(img, 5)
    net = load_net(uva, "2x")
    d_in = torch.from_numpy(img.view(np.int16)).cuda()
    d_out = torch.zeros((h, w + 2, 3), dtype=torch.int16, device="cuda")               # rows 12 bytes longer than dense
    torch.cuda.synchronize()
    net.denoise_u16_device(d_in.data_ptr(), h, w, d_out.data_ptr(), 5, out_stride=(w + 2) * 6)
    _lib.check(_lib.load().uva_denoise_synchronize(0))
    got = d_out.cpu().numpy().view(np.uint16)
    assert np.array_equal(got[:, :w], want) and not got[:, w:].any()
    with pytest.raises(_lib.UvaError, match="aligned"):
        net.denoise_u16_device(d_in.data_ptr() + 1, h, w, d_out.data_ptr(), 5)


def _p010_frames(n, h, w, seed, fmt):
    """frames with structure and grain (random 16-bit words would leave the stage nothing to average)"""
    import pixfmt16_ref as pref
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        base = np.clip(rng.normal(30000, 6000, (h // 4, w // 4, 3)), 0, 65535).repeat(4, 0).repeat(4, 1)
        bgr = np.clip(base + rng.normal(0, 900, (h, w, 3)), 0, 65535).astype(np.uint16)
        out.append(np.ascontiguousarray(pref.bgr16_to_pix(bgr, fmt, "bt601", False)).reshape(-1).view(np.uint8))
    return out


@pytest.mark.parametrize("in_fmt,scale,models", [("p010le", 1, "n=3"), ("yuv420p10le", 2, "n=3"), ("p010le", 2, "n=3,a")])
def test_route_is_the_composition_of_its_stages(uva, tmp_path, in_fmt, scale, models):
    """rawvideo.main on 4 frames of 32 x 24, byte for byte: convert_pix(bit_depth=16) to bgr48le, uva_denoise_u16, the nets' own
    16-bit calls, the last one producing p010le"""
    h, w, n, tile = 24, 32, 4, 32
    frames = _p010_frames(n, h, w, scale * 10 + len(models), in_fmt)
    src, dst = tmp_path / "in.raw", tmp_path / "out.p010"
    src.write_bytes(b"".join(f.tobytes() for f in frames))
    nets = []
    if "a" in models:
        nets.append((load_net(uva, "1x"), 0, 0))
        nets[-1][0].enable_u16_1x()
    if scale != 1:
        nets.append((load_net(uva, "%dx" % scale), tile, 10))
    want = []
    for f in frames:
        x = _denoise16(uva.convert_pix(f, h, w, in_fmt, "bgr48le", bit_depth=16), 3)
        if not nets:
            want.append(uva.convert_pix(x, h, w, "bgr48le", "p010le", bit_depth=16).tobytes())
            continue
        for net, t, border in nets[:-1]:
            x = net.process_u16(x, tile_size=t, border=border)
        net, t, border = nets[-1]
        want.append(net.collect_u8(net.submit_pix(x, x.shape[0], x.shape[1], "bgr48le", out_fmt="p010le", tile_size=t, border=border,
                                                  bit_depth=16)).tobytes())
    assert rawvideo.main(["-i", str(src), "-o", str(dst), "-W", str(w), "-H", str(h), "-s", str(scale), "-m", models, "--tile", str(tile),
                          "--in-pix-fmt", in_fmt, "--out-pix-fmt", "p010le", "--bit-depth", "16"]) == 0
    got = dst.read_bytes()
    assert len(got) == sum(len(b) for b in want) and got == b"".join(want)
