"""`--bit-depth 16 -m a` without a GPU: the command line takes the pair where an end of the stream has
more than 8 bits and still refuses the -m options that run at 8 bits only; a lane passes bgr48le between its nets; and the head and residual formulas of
sub10_kernel16 (tests/sub10_u16_ref.py) give, on v = 257 k, the u8 kernel's operand and residual bit for bit."""
import numpy as np
import pytest

import sub10_u16_ref as ref
from upscale_video_amd import rawvideo


class _Parsed(Exception):
    pass


@pytest.mark.parametrize("scale", ["1", "2", "4"])
def test_bit_depth_16_with_m_a_parses(monkeypatch, scale):
    """the arguments are accepted (the run is cut short where the first net would be loaded), and the 1x net of the lane is
    the one that gets enable_u16_1x()"""
    calls = []

    class Net:
        scale = 1

        def __init__(self, stem):
            self.stem = stem

        def enable_u16_1x(self, on=True):
            calls.append((self.stem, on))

    def load_net(stem, gpu, model_path):
        net = Net(stem)
        if stem != rawvideo.MODEL_FILES[1]:
            raise _Parsed()                     # the 2x / 4x net: the chain is built as far as this test looks
        return net

    monkeypatch.setattr(rawvideo, "load_net", load_net)
    monkeypatch.setattr(rawvideo, "stream", lambda *a, **k: (_ for _ in ()).throw(_Parsed()))
    with pytest.raises(_Parsed):
        rawvideo.main(["-W", "8", "-H", "8", "-s", scale, "-m", "a", "--bit-depth", "16", "--in-pix-fmt", "yuv420p10le",
                       "--out-pix-fmt", "p010le"])
    assert calls == [(rawvideo.MODEL_FILES[1], True)]


def test_m_a_at_8_bits_enables_nothing(monkeypatch):
    calls = []

    class Net:
        scale = 1

        def enable_u16_1x(self, on=True):
            calls.append(on)

    monkeypatch.setattr(rawvideo, "load_net", lambda stem, gpu, model_path: Net())
    monkeypatch.setattr(rawvideo, "stream", lambda *a, **k: (_ for _ in ()).throw(_Parsed()))
    with pytest.raises(_Parsed):
        rawvideo.main(["-W", "8", "-H", "8", "-s", "1", "-m", "a"])
    assert calls == []


@pytest.mark.parametrize("argv", [["-m", "n=3"], ["-m", "r", "-s", "4"], ["-m", "a,n=3"]])
def test_other_model_options_stay_refused_at_16_bits(capsys, argv):
    with pytest.raises(SystemExit) as e:
        rawvideo.main(["-W", "8", "-H", "8", "--bit-depth", "16"] + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--bit-depth 16 takes the 2x and 4x Compact nets only: -m n=K and -m r run at 8 bits" in err, argv
    assert "-m a," not in err.split("only:")[1].split("(")[0]


@pytest.mark.parametrize("fmts", [[], ["--in-pix-fmt", "yuv420p", "--out-pix-fmt", "nv12"], ["--in-pix-fmt", "yuv422p"]])
def test_m_a_at_16_bits_wants_a_format_of_more_than_8_bits(capsys, fmts):
    """8-bit frames in and out (the default bgr24 among them): the pair is refused as before this route existed, which
    tests/test_pixfmt16.py pins for the plain command; one 10- or 16-bit end is enough (test_bit_depth_16_with_m_a_parses,
    and below)"""
    with pytest.raises(SystemExit) as e:
        rawvideo.main(["-W", "8", "-H", "8", "-m", "a", "--bit-depth", "16"] + fmts)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--bit-depth 16 -m a is for frames of more than 8 bits" in err and "p010le, yuv420p10le, bgr48le, yuv422p10le" in err


@pytest.mark.parametrize("fmts", [["--out-pix-fmt", "p010le"], ["--in-pix-fmt", "yuv422p10le"], ["--in-pix-fmt", "bgr48le", "--out-pix-fmt", "yuv420p"]])
def test_one_deep_end_is_enough(monkeypatch, fmts):
    class Net:
        scale = 1

        def enable_u16_1x(self, on=True):
            pass

    monkeypatch.setattr(rawvideo, "load_net", lambda stem, gpu, model_path: Net())
    monkeypatch.setattr(rawvideo, "stream", lambda *a, **k: (_ for _ in ()).throw(_Parsed()))
    with pytest.raises(_Parsed):
        rawvideo.main(["-W", "8", "-H", "8", "-s", "1", "-m", "a", "--bit-depth", "16"] + fmts)


@pytest.mark.parametrize("bit_depth,mid", [(8, "bgr24"), (16, "bgr48le")])
def test_lane_passes_native_bgr_between_its_nets(bit_depth, mid):
    class Net:
        def __init__(self, scale):
            self.scale = scale

    pix = rawvideo.PixFormats("yuv420p10le" if bit_depth == 16 else "yuv420p", "p010le", bit_depth=bit_depth)
    lane = rawvideo.Lane([(Net(1), 0), (Net(2), 32)], 8, 10, None, pix=pix)
    a, b = lane.stages
    assert (a.in_fmt, a.out_fmt, a.tile) == (pix.in_fmt, mid, 0)          # the 1x stage: whole frame
    assert (b.in_fmt, b.out_fmt, b.tile) == (mid, "p010le", 32)
    assert a.outs[0].dtype == (np.uint16 if bit_depth == 16 else np.uint8) and a.outs[0].shape == (8, 10, 3)
    assert (b.h, b.w) == (8, 10)


def test_widened_u8_codes_give_the_u8_operand_and_residual_bit_for_bit():
    k = np.arange(256)
    v = k * 257
    assert v.max() == 65535
    op16, op8 = ref.head_operand_u16(v), ref.head_operand_u8(k)
    assert op16.dtype == np.float16 and np.array_equal(op16.view(np.uint16), op8.view(np.uint16))
    r16, r8 = ref.residual_u16(v), ref.residual_u8(k)
    assert r16.dtype == np.float32 and np.array_equal(r16.view(np.uint32), r8.view(np.uint32))
    # every u16 code has a finite operand of at most 255 (65535 is 255.0, not inf)
    allv = np.arange(65536)
    op = ref.head_operand_u16(allv).astype(np.float32)
    assert np.isfinite(op).all() and op.max() == 255.0 and op.min() == 0.0
    assert np.abs(op - allv / 257.0).max() <= 255.0 * 2.0 ** -11         # fp16's relative precision


def test_tail_rounding_of_widened_results():
    """rint(rint(257 z) / 257) = rint(z) away from exact ties: the u16 route narrowed is the u8 route (the GPU test's 1 LSB bar
    is this identity with fp32 products)"""
    rng = np.random.default_rng(0)
    y = rng.uniform(-0.01, 1.01, 300000).astype(np.float32)
    a = ref.tail_round_u8(y).astype(int)
    b = ref.tail_round_u16(y).astype(np.float64)
    narrowed = np.clip(np.rint(b / 257.0), 0, 255).astype(int)
    assert np.abs(a - narrowed).max() <= 1 and (a != narrowed).mean() <= 1e-4
