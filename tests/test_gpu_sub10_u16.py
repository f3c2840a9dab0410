"""16 bits through the 1x net on the MI355X (-m gpu): sub10_kernel16 behind Net.enable_u16_1x() --
equal to the u8 kernel on widened frames, against the product-mode and fp32 oracles in u16 codes on the geometries where the
strips, segments and lane groups meet their edges, its depth against the 8-bit counterfactual, strides, the device entry,
repeatability, workspace reuse and every refusal, submit_pix(bit_depth=16) with frames in flight, and the streamer's
`-m a --bit-depth 16` chain byte for byte against the two nets called stage by stage."""
import io
import subprocess
import sys

import numpy as np
import pytest

import pixfmt16_ref as ref
import repeat_ref
import sub10_u16_ref as s10
from conftest import ROOT, load_net
from parity_report import U16_PRODUCT, check_f32, check_u16, check_u8, slack
from test_gpu_bitdepth16 import U16_RMS_CAP, X257_BAR, _ramp16, _smooth16, _smooth_full

pytestmark = pytest.mark.gpu

KEY = "1x"
# the project's existing caps, not new numbers: the 16-bit route's RMS cap, and the float route's max bar of this net in codes
PRODUCT_BARS = {"max_rms": slack(KEY, "u16", "rms_codes", U16_RMS_CAP), "max_codes": 65535 * 3e-3}
FP32_MAX_CODES = 2 * 257
FP32_MAX_ABS = 3e-3


def _net(uva):
    net = load_net(uva, KEY)
    net.enable_u16_1x()
    return net


def _against_oracles(tag, net, om, oracle, x16, structure=True):
    got16 = net.process_u16(x16)
    assert got16.shape == x16.shape and got16.dtype == np.uint16
    sc = check_u16(tag, got16, s10.product_u16(om, oracle, x16), vs=U16_PRODUCT, model=KEY, route="u16", structure=structure, **PRODUCT_BARS)
    raw32 = s10.fp32_raw(om, x16)
    check_u16(tag, got16, s10.tail_round_u16(raw32), vs="fp32 oracle", max_codes=FP32_MAX_CODES, model=KEY, route="u16", structure=False)
    check_f32(tag, got16.astype(np.float64) / 65535.0, np.clip(raw32, 0, 1), vs="fp32 oracle", max_abs=FP32_MAX_ABS, model=KEY, route="u16")
    return got16, sc


# ---- 1. equal to the u8 kernel on widened frames ----------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(50, 33), (96, 130), (300, 700)])
def test_widened_frames_give_the_u8_kernels_result(uva, oracle, h, w):
    """Operand, body and residual are bit-identical by construction for v = 257 k, and rint(rint(257 z) / 257) = rint(z) away
    from exact ties: at most 1 LSB apart, at most 1 sample in 10 000 differing.  A condition, not a measurement."""
    net = _net(uva)
    img = oracle.synthetic_frame(h, w, kind="random", seed=h + w)
    u8 = net.process_u8(img)
    via16 = ref.narrow(net.process_u16(ref.widen(img)))
    check_u8(f"1x u16 route on widened frames {w}x{h}", via16, u8, vs="u8 route (sub10_kernel)", max_lsb=1, max_share=1e-4, model=KEY,
             route="u16")


# ---- 2. against the oracles ---------------------------------------------------------------------------------------------------
GEOMETRIES = [(1, 1), (3, 2), (1, 61), (2, 60), (17, 59), (5, 121), (50, 33), (64, 600)]


@pytest.mark.parametrize("h,w", GEOMETRIES)
def test_process_u16_matches_the_oracles(uva, oracle, oracle_models, h, w):
    """(1, 61), (2, 60), (17, 59): either side of the 60-column strip; (5, 121): three strips, the last one column wide;
    (64, 600): strips cut into segments across the 256 workgroups.
    The row / column statistic (parity_report.structure_codes; it applies to the 64 x 600 frame alone) is taken on the random
    frame, where the error follows the content.  On the smooth frame the sub-code error follows the frame's edges, as on the
    frames test_gpu_bitdepth16.py leaves out for that reason (UNIFORM, the ramp): the net's zero padding is the strongest edge
    of such a frame, activations and with them fp16's steps are largest beside it.  Measured on 64 x 600, mean |diff| per row
    in codes: 0.56, 0.65, 0.61, 0.50 on rows 0-3, 0.51 on rows 60-62, 0.34-0.43 everywhere between, no step at a segment's
    start (the 2x net's u16 route on the same frame: 1.08-1.22 on its first rows, 1.15 on its last, ~1.0 between); a row of
    1 800 samples tells 1.6x its neighbours' rate at 18 standard errors.  RMS and max hold on both frames."""
    net, om = _net(uva), oracle_models[KEY]
    golden = oracle.synthetic_frame(h, w, kind="random", seed=h + w)
    for name, x16 in (("golden*257", golden.astype(np.uint16) * 257), ("smooth16", _smooth16(h, w))):
        _against_oracles(f"u16 1x {w}x{h} {name}", net, om, oracle, x16, structure=name != "smooth16")


# ---- 3. edge inputs -----------------------------------------------------------------------------------------------------------
def _edge(kind, h, w, rng):
    if kind == "zero":
        return np.zeros((h, w, 3), np.uint16)
    if kind == "max":                      # the operand is 255.0 in fp16, not inf (an inf would leave NaN: the oracles would tell)
        return np.full((h, w, 3), 65535, np.uint16)
    x = rng.integers(0, 65536, (h, w, 3), dtype=np.uint16)
    if kind == "toprow":
        x[1:] = 0
    return x


@pytest.mark.parametrize("h,w", [(1, 17), (16, 64), (33, 121)])
def test_process_u16_edge_inputs(uva, oracle, oracle_models, h, w):
    net, om = _net(uva), oracle_models[KEY]
    rng = np.random.default_rng(h * 131 + w)
    for kind in ("zero", "max", "toprow", "noise"):
        x16 = _edge(kind, h, w, rng)
        got16, _ = _against_oracles(f"u16 1x edge {w}x{h} {kind}", net, om, oracle, x16, structure=False)
        if kind == "max":
            assert np.isfinite(s10.head_operand_u16(x16).astype(np.float32)).all()


# ---- 4. depth, the point of the change ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", ["ramp", "smooth"])
def test_process_u16_keeps_its_depth(uva, oracle, oracle_models, content):
    """y = the product-mode result, q8 = widen(narrow(y)): what the route would give with an 8-bit hop in it (computed here,
    no fault injected).  The route's RMS against y is at most half of q8's and hardly any unclamped sample is a multiple of 257;
    q8 is recorded next to it and must fail both bars."""
    net, om = _net(uva), oracle_models[KEY]
    x16 = _ramp16(120, 480) if content == "ramp" else _smooth_full(96, 128)
    h, w, _ = x16.shape
    got = net.process_u16(x16)
    y = s10.product_u16(om, oracle, x16)
    q8 = ref.widen(ref.narrow(y))
    rms8 = float(np.sqrt(((q8.astype(np.float64) - y) ** 2).mean()))
    bars = dict(PRODUCT_BARS, max_x257=X257_BAR)
    bars["max_rms"] = min(bars["max_rms"], 0.5 * rms8)
    tag = f"u16 1x depth {w}x{h} {content}"
    check_u16(tag, got, y, vs=U16_PRODUCT, model=KEY, route="u16", structure=content != "ramp", **bars)
    check_u16(tag + " 8-bit hop", q8, y, vs=U16_PRODUCT + " (counterfactual)", model=KEY, route="u16", counterfactual=True, **bars)


# ---- 5. entries and strides ---------------------------------------------------------------------------------------------------
def _strides(row):
    """two row strides past a row of `row` bytes: the first = 2 mod 4 (every other row only 2-byte aligned), the second a
    multiple of 16"""
    return row + 1 + (2 - (row + 1)) % 4, (row // 16 + 1) * 16


def test_row_strides_device_entry_repeatability_and_reuse(uva):
    import ctypes
    import torch
    from upscale_video_amd import _lib
    if not torch.cuda.is_available():
        pytest.fail("torch cannot see the GPU in this process")
    L = _lib.load()
    net = _net(uva)
    h, w = 21, 137                                  # three strips
    rng = np.random.default_rng(4)
    x16 = rng.integers(0, 65536, (h, w, 3), dtype=np.uint16)
    want = net.process_u16(x16)
    assert np.array_equal(want, net.process_u16(x16)), "two runs, two results"
    row = w * 6
    s = _strides(row)
    assert s[0] % 4 == 2 and s[1] % 16 == 0 and min(s) > row
    for in_stride, out_stride in ((s[0], s[0]), (s[1], s[1]), (s[0], s[1]), (s[1], s[0])):
        src = np.full((h, in_stride), 0xA5, np.uint8)
        src[:, :row] = x16.reshape(h, row // 2).view(np.uint8)
        dst = np.full((h, out_stride), 0x5A, np.uint8)
        _lib.check(L.uva_net_process_u16(net._h, src.ctypes.data, h, w, in_stride, dst.ctypes.data, out_stride, 0, 0))
        assert np.array_equal(dst[:, :row].copy().view(np.uint16).reshape(h, w, 3), want), (in_stride, out_stride)
        assert (dst[:, row:] == 0x5A).all(), (in_stride, out_stride, "the padding was written")
        d_src = torch.from_numpy(src).cuda()
        d_dst = torch.full((h, out_stride), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _lib.check(L.uva_net_process_u16_device(net._h, ctypes.c_void_p(d_src.data_ptr()), h, w, in_stride,
                                                ctypes.c_void_p(d_dst.data_ptr()), out_stride, 0, 0))
        net.synchronize()
        assert np.array_equal(d_dst.cpu().numpy(), dst), (in_stride, out_stride, "device entry")
    # a second geometry on the same net, a u8 frame in between, then the first again: what a fresh net gives
    y16 = rng.integers(0, 65536, (33, 47, 3), dtype=np.uint16)
    fresh = _net(uva)
    assert np.array_equal(net.process_u16(y16), fresh.process_u16(y16))
    assert np.array_equal(net.process_u8(ref.narrow(y16)), fresh.process_u8(ref.narrow(y16)))
    assert np.array_equal(net.process_u16(x16), want)


def test_refusals(uva):
    import ctypes
    import torch
    from upscale_video_amd import _lib
    L = _lib.load()
    img = np.zeros((8, 8, 3), np.uint16)
    # the switch off: the earlier message; on, then off again: the same
    net = load_net(uva, KEY)
    with pytest.raises(_lib.UvaError, match="2x and 4x Compact"):
        net.process_u16(img)
    net.enable_u16_1x()
    assert net.process_u16(img).shape == img.shape
    net.enable_u16_1x(False)
    with pytest.raises(_lib.UvaError, match="2x and 4x Compact"):
        net.process_u16(img)
    with pytest.raises(_lib.UvaError, match="2x and 4x Compact"):
        net.submit_pix(np.zeros(ref.frame_bytes("p010le", 8, 8), np.uint8), 8, 8, "p010le", out_fmt="p010le", bit_depth=16)
    # the switch on a 2x net
    with pytest.raises(_lib.UvaError, match="not the 1x SubCompact net"):
        load_net(uva, "2x").enable_u16_1x()
    net = _net(uva)
    # tiles
    with pytest.raises(_lib.UvaError, match="whole frames only"):
        net.process_u16(np.zeros((40, 40, 3), np.uint16), tile_size=32, border=4)
    # an odd stride
    h, w = 8, 8
    src, dst = np.zeros((h, w * 6 + 2), np.uint8), np.zeros((h, w * 6 + 2), np.uint8)
    for in_stride, out_stride in ((w * 6 + 1, w * 6), (w * 6, w * 6 + 1)):
        assert L.uva_net_process_u16(net._h, src.ctypes.data, h, w, in_stride, dst.ctypes.data, out_stride, 0, 0) != 0
        assert b"2-byte aligned" in L.uva_last_error()
    # overlapping frames (device entry: the host entry stages both): the same buffer, and a result that starts inside the input
    buf = torch.zeros(2 * h * w * 6, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for off in (0, (h - 1) * w * 6):
        assert L.uva_net_process_u16_device(net._h, ctypes.c_void_p(buf.data_ptr()), h, w, w * 6,
                                            ctypes.c_void_p(buf.data_ptr() + off), w * 6, 0, 0) != 0
        assert b"do not overlap" in L.uva_last_error()
    assert L.uva_net_process_u16_device(net._h, ctypes.c_void_p(buf.data_ptr()), h, w, w * 6,
                                        ctypes.c_void_p(buf.data_ptr() + h * w * 6), w * 6, 0, 0) == 0      # side by side: fine
    net.synchronize()
    assert not buf.cpu().numpy()[:h * w * 6].any()
    # a frame too tall for the row table: refused, not run at 8 bits
    with pytest.raises(_lib.UvaError, match="does not fit the fused kernel's row table"):
        net.process_u16(np.zeros((65505, 1, 3), np.uint16))
    # the u16 kernel's launches have their own slot in the statistics
    net.set_profiling(True)
    net.process_u16(img)
    net.process_u8(ref.narrow(img))
    net.synchronize()
    assert net.kernel_stats(3)[0] == 1 and net.kernel_stats(1)[0] == 1
    net.set_profiling(False)


# ---- 6. the route ---------------------------------------------------------------------------------------------------------------
def _packed(fmt, h, w, rng):
    return rng.integers(0, 65536, repeat_ref.frame_bytes(fmt, h, w) // 2, dtype=np.uint16).astype("<u2").view(np.uint8)


def test_submit_pix16_in_flight(uva):
    net = _net(uva)
    h, w = 66, 90
    rng = np.random.default_rng(9)
    frames = [_packed("yuv420p10le", h, w, rng) for _ in range(4)]
    want = [net.process_u16(ref.pix_to_bgr16(f, "yuv420p10le", h, w)) for f in frames]
    for pinned in (False, True):
        outs = [uva.pix_empty("bgr48le", h, w, uva.pinned_empty if pinned else None) for _ in frames]
        tickets, got = [], []
        for f, o in zip(frames, outs):
            if len(tickets) == 3:
                got.append(net.collect_u8(tickets.pop(0)))
            tickets.append(net.submit_pix(f, h, w, "yuv420p10le", out=o, out_fmt="bgr48le", bit_depth=16))
        got += [net.collect_u8(t) for t in tickets]
        for k in range(len(frames)):
            assert np.array_equal(np.asarray(got[k]).reshape(h, w, 3), want[k]), (pinned, k)


@pytest.mark.parametrize("case", ["out_size", "bilinear", "yuv422p10le"])
def test_submit_pix16_is_the_composition(uva, case):
    """the resampler behind the net, the interpolating chroma mode and a 4:2:2 format, each against the separate calls"""
    net = _net(uva)
    h, w = 66, 90
    rng = np.random.default_rng(21)
    in_fmt = "yuv422p10le" if case == "yuv422p10le" else "yuv420p10le"
    kw = dict(chroma_filter="bilinear", chroma_loc="left", colour="bt709") if case == "bilinear" else {}
    size = (h * 3 // 4, w + 11) if case == "out_size" else (h, w)
    f = _packed(in_fmt, h, w, rng)
    bgr = uva.convert_pix(f, h, w, in_fmt, "bgr48le", bit_depth=16, **kw)
    up = net.process_u16(np.asarray(bgr).reshape(h, w, 3))
    rs = uva.resize(up, size, "bicubic") if case == "out_size" else up
    want = np.asarray(uva.convert_pix(rs, size[0], size[1], "bgr48le", "p010le", bit_depth=16, **kw))
    extra = dict(out_size=size, resize_filter="bicubic") if case == "out_size" else {}
    got = net.collect_u8(net.submit_pix(f, h, w, in_fmt, out_fmt="p010le", bit_depth=16, **kw, **extra))
    assert np.array_equal(np.asarray(got).reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8))


# ---- 7. the streamer ------------------------------------------------------------------------------------------------------------
def _stage_by_stage(uva, frames, h, w, scale, tile):
    """the two nets called one after the other on every frame -> the bytes the streamer must write, and the frames between them"""
    from upscale_video_amd import rawvideo
    net1 = _net(uva)
    net2 = load_net(uva, "%dx" % scale) if scale != 1 else None
    out, mids = [], []
    for f in frames:
        if net2 is None:
            out.append(net1.collect_u8(net1.submit_pix(f, h, w, "yuv420p10le", out_fmt="p010le", bit_depth=16)).tobytes())
            continue
        mid = net1.collect_u8(net1.submit_pix(f, h, w, "yuv420p10le", out_fmt="bgr48le", bit_depth=16)).copy()
        mids.append(mid)
        out.append(net2.collect_u8(net2.submit_pix(mid, h, w, "bgr48le", out_fmt="p010le", tile_size=tile, border=rawvideo.TILE_BORDER,
                                                   bit_depth=16)).tobytes())
    return b"".join(out), mids


@pytest.mark.parametrize("scale", [2, 1])
def test_rawvideo_m_a_bit_depth_16(uva, tmp_path, scale):
    from upscale_video_amd import rawvideo
    h, w, n, tile = 40, 58, 5, 32
    rng = np.random.default_rng(11 + scale)
    frames = [_packed("yuv420p10le", h, w, rng) for _ in range(n)]
    src = tmp_path / "in.yuv"
    src.write_bytes(b"".join(f.tobytes() for f in frames))
    want, _ = _stage_by_stage(uva, frames, h, w, scale, tile)
    assert len(want) == n * ref.frame_bytes("p010le", h * scale, w * scale)
    geo = ["-W", str(w), "-H", str(h), "-s", str(scale), "-m", "a", "--tile", str(tile), "--in-pix-fmt", "yuv420p10le",
           "--out-pix-fmt", "p010le", "--bit-depth", "16"]
    for gpus in ("0", "0,0"):
        dst = tmp_path / ("out_%s.p010" % gpus.replace(",", "_"))
        assert rawvideo.main(["-i", str(src), "-o", str(dst), "-g", gpus] + geo) == 0
        assert dst.read_bytes() == want, gpus
    r = subprocess.run([sys.executable, "-m", "upscale_video_amd.rawvideo", "-g", "0"] + geo, input=src.read_bytes(),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout == want


def test_rawvideo_m_a_bit_depth_16_skip_repeats(uva, tmp_path, capsys):
    """a stream that shows each frame twice: the same bytes with --skip-repeats 0, and the count tests/repeat_ref.py predicts for
    both nets (the second one finds the repeats itself, in the first one's bgr48le results)"""
    from upscale_video_amd import rawvideo
    h, w, tile = 40, 58, 32
    rng = np.random.default_rng(13)
    distinct = [_packed("yuv420p10le", h, w, rng) for _ in range(5)]
    frames = [f for f in distinct for _ in range(2)]
    src, dst = tmp_path / "in.yuv", tmp_path / "out.p010"
    src.write_bytes(b"".join(f.tobytes() for f in frames))
    want, mids = _stage_by_stage(uva, frames, h, w, 2, tile)
    k = repeat_ref.skipped(repeat_ref.kept_indices(frames, "yuv420p10le", h, w, 0))
    k += repeat_ref.skipped(repeat_ref.kept_indices(mids, "bgr48le", h, w, 0))
    assert k >= 10
    argv = ["-i", str(src), "-o", str(dst), "-W", str(w), "-H", str(h), "-s", "2", "-m", "a", "--tile", str(tile),
            "--in-pix-fmt", "yuv420p10le", "--out-pix-fmt", "p010le", "--bit-depth", "16", "--skip-repeats", "0"]
    capsys.readouterr()
    assert rawvideo.main(argv) == 0
    assert "10 frames, skipped %d of 20" % k in capsys.readouterr().err
    assert dst.read_bytes() == want


# ---- 8. the chain keeps its depth -----------------------------------------------------------------------------------------------
def _ramp10(h, w):
    """a slow full-range 10-bit luma ramp plus a soft radial gradient, neutral chroma, as p010le (limited range)"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    rad = np.hypot(yy - h / 2, xx - w / 2) / np.hypot(h / 2, w / 2)
    y = np.rint(64 + 876 * (0.8 * xx / (w - 1) + 0.2 * (1 - rad))).astype(np.int64)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return ref.pack("p010le", y, np.full((ch, cw), 512), np.full((ch, cw), 512))


def test_the_chain_keeps_its_depth(uva, oracle_models):
    """p010le -> 1x -> 2x -> p010le (`-s 2 -m a`) at 16 and at 8 bits against the ideal: the fp32 oracles of both nets on the
    exact 10-bit input, float in between, converted in float64.  The 16-bit chain's Y' RMS is at most half the 8-bit chain's."""
    from upscale_video_amd import rawvideo
    h, w = 120, 480
    p = _ramp10(h, w)
    rms = {}
    y, u, v = ref.planes(p, "p010le", h, w)
    up2 = lambda a: np.repeat(np.repeat(a, 2, 0), 2, 1)[:h, :w]   # noqa: E731
    b, g, r = ref.float_inv(y, up2(u), up2(v), "bt601", False, 10)
    x = np.clip(np.stack([b, g, r], -1) / 65535.0, 0, 1).astype(np.float32)
    fwd = lambda om, a: om.forward(np.ascontiguousarray(a.transpose(2, 0, 1))).transpose(1, 2, 0)   # noqa: E731
    o = np.clip(fwd(oracle_models["2x"], np.clip(fwd(oracle_models[KEY], x), 0, 1)).astype(np.float64), 0, 1)
    ideal_y, _, _ = ref.float_fwd(o[..., 2] * 65535, o[..., 1] * 65535, o[..., 0] * 65535, "bt601", False, 10)
    for bd in (8, 16):
        net1 = load_net(uva, KEY)
        if bd == 16:
            net1.enable_u16_1x()
        chain = [(net1, 0), (load_net(uva, "2x"), 0)]
        fout = io.BytesIO()
        assert rawvideo.stream(io.BytesIO(p.tobytes()), fout, h, w, chain, pix=rawvideo.PixFormats("p010le", "p010le", bit_depth=bd)) == 1
        out = np.frombuffer(fout.getvalue(), np.uint8)
        gy = ref.planes(out, "p010le", 2 * h, 2 * w)[0].astype(np.float64)
        rms[bd] = float(np.sqrt(((gy - ideal_y) ** 2).mean()))
    check_f32("p010le ramp -m a -s 2: Y' RMS in codes, 16-bit chain (8-bit chain: %.3f)" % rms[8], np.array([rms[16]]), np.array([0.0]),
              vs="float64 ideal", max_abs=0.5 * rms[8])
