"""`-m n=K` at --bit-depth 16 on the CPU: properties of the definition (tests/nlm16_ref.py: integer numpy,
what the kernels of csrc/uva_denoise16.hip.h are held to bit for bit in tests/test_gpu_denoise16.py), its Lab conversions against
the float64 CIE values, the stage against the 8-bit one, what the feature is for (a shallow 10-bit ramp), the host-built tables
of the library against the definition's, the command line, and the streamer with a stand-in 16-bit denoise call."""
import io
import os
import subprocess

import numpy as np
import pytest

import nlm16_ref as ref
import pixfmt16_ref as pref
from oracle import nlm_oracle as no
from upscale_video_amd import _lib, ncnn, rawvideo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- non-local means ------------------------------------------------------------------------------------------------------
def test_weight_table_facts():
    for h, cn in ((1, 1), (3, 1), (3, 2), (10, 2), (30, 2)):
        t = ref.weight_table16(h, cn)
        assert t[0] == ref.FIXED == 103969
        assert (np.diff(t) <= 0).all() and t[-1] == 0 and (t[:-1] > 0).all()            # monotone, cut at its first zero
        assert t[:-1].min() >= 0.001 * 103969                                           # smaller weights are dropped entirely
    # the 8-bit stage's function of the mean squared patch difference: entry 16 i of the 16-bit table is entry i of the 8-bit
    # one up to the 257^2 / 2^16 = 1.0078 between `x 257` and `<< 8` (a bin of 2^9 * 2^8 / 257^2 = 1.984 eight-bit units^2, not 2)
    t8, t16 = no.weight_table(3, 1), ref.weight_table16(3, 1)
    i = np.arange(1, 40)
    want = np.rint(103969 * np.exp(-(16 * i) * (512.0 * 256.0 / (257.0 * 257.0 * 25.0)) / 9.0))
    assert np.array_equal(t16[16 * i], want)
    assert abs(16 * (512.0 * 256.0 / (257.0 * 257.0 * 25.0)) / 1.28 - 65536.0 / 66049.0) < 1e-15
    assert (t16[16 * i] >= t8[i]).all() and t16[16] - t8[1] == 99        # (the same exponent but for that factor)
    assert len(ref.weight_table16(30, 2)) == 156745                                     # "of the order of 10^5" (the issue)
    assert len(t16) == 785


def test_definition_properties():
    flat = np.full((12, 15), 77 * 257 + 5, np.uint16)
    assert np.array_equal(ref.nlm_plane16(flat, 5), flat)                               # a constant plane is a fixed point
    flat2 = np.empty((9, 11, 2), np.uint16)
    flat2[..., 0], flat2[..., 1] = 40000, 123
    assert np.array_equal(ref.nlm_plane16(flat2, 5), flat2)
    rng = np.random.default_rng(1)
    rng.integers(0, 256, (20, 23, 3), dtype=np.uint8)                                   # (tests/test_denoise.py draws these first:
    rng.integers(0, 256, (9, 9, 1), dtype=np.uint8)                                     #  the same noisy plane as its line 46)
    noisy8 = np.clip(128 + rng.normal(0, 12, (40, 40)), 0, 255).astype(np.uint8)
    noisy = noisy8.astype(np.uint16) * 257
    den = ref.nlm_plane16(noisy, 20)
    assert den.std() < 0.5 * noisy.std()                                                # test_denoise.py:48's bar, widened x 257
    assert np.array_equal(ref.nlm_plane16(noisy, 0.5), noisy)                           # tiny h: only exact matches weigh
    # the top of the 32-bit square, the index clamp and the 64-bit sums: 0 / 65535 checkerboard, every weight but the
    # equal-parity ones zero, the result the plane itself
    cb = ((np.add.outer(np.arange(9), np.arange(10)) & 1) * 65535).astype(np.uint16)
    assert np.array_equal(ref.nlm_plane16(cb, 30), cb)
    assert 25 * 2 * ((65535 * 65535) >> 8) < 2 ** 31 and 81 * 103969 * 65535 > 2 ** 32


# ---- Lab at 16 bits --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def colours():
    c = ref.colour_set()
    assert c.shape == (64 ** 3 + (1 << 20) + 8, 3) and c.dtype == np.uint16
    return c, ref.bgr2lab16(c)


def test_forward_lab_against_the_float64_cie_values(colours):
    """In 16-bit codes per plane, on the fixed set (the 64-level cube x 257, 2^20 seeded random colours, the eight corners).
    Measured: L 4, a 13, b 6 against the rounded float64 value (means 0.37, 0.84, 0.33), pinned.  The error is the 16-bit
    argument of the cube-root table: below t = 1000 of 65535 the cube root moves eight table units per step of t."""
    c, lab = colours
    f = np.clip(np.rint(ref.bgr2lab16_float(c)), 0, 65535)
    d = np.abs(lab.astype(np.float64) - f)
    print("forward Lab16 vs float64: max", d.max(0), "mean", d.mean(0))
    assert tuple(d.max(0)) == (4, 13, 6)
    assert (d.mean(0) < (0.4, 0.9, 0.4)).all()
    assert tuple(lab[-8]) == (0, 32896, 32896) and tuple(lab[-1]) == (65535, 32896, 32896)     # black and white


def test_lab_round_trip_is_far_inside_half_an_8_bit_level(colours):
    """BGR16 -> Lab16 -> BGR16 on the fixed set: the condition is a maximum under 128 codes (half an 8-bit level; the 8-bit
    stage loses up to 5 levels = 1285 codes there, tests/test_denoise.py:42).  Measured: 12 codes (B 6, G 10, R 12; mean 1.69),
    pinned."""
    c, lab = colours
    rt = np.abs(ref.lab2bgr16(lab).astype(int) - c.astype(int))
    print("round trip: max per channel", rt.max(0), "mean", rt.mean())
    assert rt.max() < 128
    assert tuple(rt.max(0)) == (6, 10, 12) and rt.mean() < 1.7


def _noisy_frame8():
    rng = np.random.default_rng(40)
    base = np.clip(rng.normal(120, 30, (40, 40, 3)), 0, 255)
    return np.clip(base + rng.normal(0, 5, (40, 40, 3)), 0, 255).astype(np.uint8)


def test_against_the_8_bit_stage_on_a_widened_frame():
    """denoise16(img8 * 257, K) >> 8 against the 8-bit stage's restatement on a seeded 40 x 40 noisy frame.  No bar was set in
    advance; measured at K = 3 and K = 10 alike: at most 4 levels, differences -3 ... +4, mean +0.28 / +0.24 (upward: the
    8-bit Lab2BGR truncates, test_denoise.py:66), pinned."""
    f8 = _noisy_frame8()
    for K, mean in ((3, 0.282), (10, 0.237)):
        d = (ref.denoise16(f8.astype(np.uint16) * 257, K) >> 8).astype(int) - no.denoise_colored(f8, K, K).astype(int)
        print("K", K, "min", d.min(), "max", d.max(), "mean", d.mean())
        assert (d.min(), d.max()) == (-3, 4)
        assert abs(d.mean() - mean) < 0.001


def test_a_shallow_ramp_keeps_its_depth():
    """The point of the feature.  A 48 x 64 ramp over 12 eight-bit levels at 10-bit precision plus grain of sigma = 1 eight-bit
    level: RMS against the clean ramp, in 16-bit codes, of denoise16 at K = 3 strictly below that of the 8-bit path (quantise to
    8 bits, nlm_oracle, widen).  Measured: 42.5 against 148.6 codes (the noisy input: 257.6)."""
    rng = np.random.default_rng(48)
    h, w = 48, 64
    clean10 = np.rint(np.tile(100.0 + 12.0 * np.arange(w) / (w - 1), (h, 1)) * 4.0)              # 10-bit codes of 1020
    clean = np.repeat(np.rint(clean10 * 65535.0 / 1020.0)[..., None], 3, 2)
    noisy = np.clip(np.rint(clean + rng.normal(0, 257.0, (h, w, 3))), 0, 65535).astype(np.uint16)
    rms = lambda x: float(np.sqrt(((x.astype(np.float64) - clean) ** 2).mean()))                  # noqa: E731
    r16 = rms(ref.denoise16(noisy, 3))
    q8 = ((noisy.astype(np.int64) * 255 + 32767) // 65535).astype(np.uint8)
    r8 = rms(no.denoise_colored(q8, 3, 3).astype(np.uint16) * 257)
    print("ramp: rms 16-bit stage", r16, "8-bit path", r8, "input", rms(noisy))
    assert r16 < r8
    assert abs(r16 - 42.47) < 0.01 and abs(r8 - 148.62) < 0.01


# ---- the library's host-built tables, in a program of their own ------------------------------------------------------------
def test_host_tables_are_the_definitions(tmp_path):
    """csrc/uva_denoise16_tables.h compiled by the host compiler alone (no HIP, no GPU; tests/host/denoise16_tables_check.cpp)
    under AddressSanitizer and UndefinedBehaviorSanitizer: every integer of the Lab tables and of four weight tables is the
    numpy definition's."""
    from test_plan_sanitized import FLAGS, host_compilers
    compilers = host_compilers()
    if not compilers:
        pytest.skip("no host C++ compiler (g++ or ROCm's clang++)")
    exe, out = str(tmp_path / "denoise16_tables_check"), str(tmp_path / "tables.bin")
    flags = [f for f in FLAGS if not f.startswith("-I") and not f.startswith("-D")]
    for cc in compilers:
        r = subprocess.run(cc + flags + [os.path.join(ROOT, "tests", "host", "denoise16_tables_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr[-4000:]
    cases = [(1, 1), (3, 2), (10, 1), (30, 2)]
    r = subprocess.run([exe, out] + [str(v) for c in cases for v in c], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    got = np.fromfile(out, dtype="<i8")
    t = ref.lab16_tables()
    want = [t["ftab"], t["fwd"].reshape(-1), t["inv"].reshape(-1),
            np.array([t[k] for k in ("l_mul", "l_sub", "a_mul", "b_mul", "il_mul", "il_add", "ia_mul", "ib_mul", "f_thr", "f_bias", "lin_mul")])]
    for h, cn in cases:
        w = ref.weight_table16(h, cn)
        want += [np.array([len(w)]), w]
    want = np.concatenate(want)
    assert got.shape == want.shape and np.array_equal(got, want)


# ---- the command line -------------------------------------------------------------------------------------------------------
class _Stop(Exception):
    pass


@pytest.mark.parametrize("argv,chain", [
    (["-s", "1", "-m", "n=3", "--in-pix-fmt", "p010le", "--out-pix-fmt", "p010le"], ["denoise"]),
    (["-s", "2", "-m", "n=3", "--in-pix-fmt", "yuv420p10le", "--out-pix-fmt", "p010le"], ["denoise", 2]),
    (["-s", "4", "-m", "n=30", "--in-pix-fmt", "bgr24", "--out-pix-fmt", "bgr48le"], ["denoise", 4]),
    (["-s", "2", "-m", "n=3,a", "--in-pix-fmt", "p010le", "--out-pix-fmt", "p010le"], ["denoise", 1, 2]),
    (["-s", "1", "-m", "a,n=7", "--in-pix-fmt", "yuv422p10le", "--out-pix-fmt", "bgr24"], ["denoise", 1]),
    (["-s", "2", "-m", "n=3", "--in-pix-fmt", "p010le", "--out-pix-fmt", "p010le", "--out-size", "40x30"], ["denoise", 2]),
])
def test_cli_accepts_denoise_at_bit_depth_16(monkeypatch, argv, chain):
    """the accepted combinations parse and build the reference's order: denoise, anime pass, upscale"""
    class Net:
        def __init__(self, scale):
            self.scale, self.u16 = scale, False

        def enable_u16_1x(self):
            self.u16 = True

    seen = {}

    def fake_stream(fin, fout, h, w, nets, **kw):
        seen["nets"], seen["pix"] = nets, kw["pix"]
        raise _Stop()

    monkeypatch.setattr(rawvideo, "load_net", lambda stem, gpu, path: Net(int(stem[0])))
    monkeypatch.setattr(rawvideo, "stream", fake_stream)
    monkeypatch.setattr(rawvideo, "grow_pipe", lambda f: None)
    monkeypatch.setattr(rawvideo.sys, "stdin", io.TextIOWrapper(io.BytesIO()))
    monkeypatch.setattr(rawvideo.sys, "stdout", io.TextIOWrapper(io.BytesIO()))
    with pytest.raises(_Stop):
        rawvideo.main(["-W", "16", "-H", "12", "--bit-depth", "16"] + argv)
    (lane,) = seen["nets"]
    assert ["denoise" if isinstance(n, tuple) else n.scale for n, _ in lane] == chain
    assert lane[0][0][0] == "denoise" and seen["pix"].bit_depth == 16
    assert all(n.u16 for n, _ in lane if not isinstance(n, tuple) and n.scale == 1)


@pytest.mark.parametrize("argv,msgs", [
    (["-m", "r", "-s", "4", "--in-pix-fmt", "p010le"], ("--bit-depth 16", "-m r")),
    (["-m", "n=3,r", "-s", "4", "--in-pix-fmt", "p010le"], ("--bit-depth 16", "-m r")),
    (["-m", "n=4"], ("--bit-depth 16",)),                                               # bgr24 at both ends
    (["-m", "n=4,a", "--in-pix-fmt", "yuv420p", "--out-pix-fmt", "nv12"], ("--bit-depth 16",)),
    (["-m", "n=4", "-s", "1", "--in-pix-fmt", "p010le", "--out-size", "24x20"], ("--out-size", "denoise stage")),
    (["-m", "n=31", "--in-pix-fmt", "p010le"], ("between 1 and 30",)),
])
def test_cli_refusals_at_bit_depth_16(capsys, argv, msgs):
    with pytest.raises(SystemExit) as e:
        rawvideo.main(["-W", "16", "-H", "12", "--bit-depth", "16"] + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert all(m in err for m in msgs), err


def test_lane_that_ends_in_the_16_bit_denoise_stage_refuses_a_resampler():
    pix = rawvideo.PixFormats("p010le", "p010le", bit_depth=16, out_size=(10, 12))
    with pytest.raises(ValueError, match="denoise"):
        rawvideo.Lane([(("denoise", 0, 4), 0)], 6, 8, lambda s: np.zeros(s, np.uint8), pix)


# ---- the streamer -----------------------------------------------------------------------------------------------------------
class Denoise16FakeLib:
    """_lib.load() stand-in: uva_denoise_u16 (65535 - x on a strided u16 frame) and uva_pix_convert16 (the restated conversions)
    on host pointers; the 8-bit entries fail the test"""

    def __init__(self):
        self.denoised, self.converted = [], []

    def uva_denoise_u8(self, *a):
        raise AssertionError("--bit-depth 16 must not take the 8-bit denoise stage")

    def uva_pix_convert(self, *a):
        raise AssertionError("--bit-depth 16 must not take the 8-bit conversions")

    @staticmethod
    def _arr(ptr, nbytes):
        import ctypes
        return np.frombuffer((ctypes.c_ubyte * nbytes).from_address(ptr), np.uint8)

    def uva_denoise_u16(self, gpu, src, h, w, ss, dst, ds, hl, hc):
        assert ss == ds == w * 6 and hl == hc
        a = self._arr(src, h * w * 6).view(np.uint16)
        self._arr(dst, h * w * 6).view(np.uint16)[...] = 65535 - a
        self.denoised.append((gpu, hl))
        return 0

    def uva_pix_convert16(self, gpu, src, in_code, dst, out_code, h, w, cw):
        names = {v: k for k, v in ncnn.PIX_FORMATS_ALL.items()}
        fi, fo = names[in_code], names[out_code]
        assert cw == ncnn.colour_word("bt709", "tv")
        a = self._arr(src, pref.frame_bytes(fi, h, w))
        x = pref.pix_to_bgr16(a, fi, h, w, "bt709", False)
        self._arr(dst, pref.frame_bytes(fo, h, w))[...] = np.ascontiguousarray(pref.bgr16_to_pix(x, fo, "bt709", False)).reshape(-1).view(np.uint8)
        self.converted.append((fi, fo))
        return 0


class Bgr48FakeNet:
    """Net.submit_pix(bit_depth=16) stand-in (tests/test_pixfmt16.py Pix16FakeNet) that records the formats it is handed"""

    def __init__(self, scale):
        self.scale, self.calls = scale, []

    def submit_u8(self, *a, **k):
        raise AssertionError("--bit-depth 16 must not take the 8-bit route")

    def submit_pix(self, buf, h, w, in_fmt, out=None, out_fmt="bgr24", colour="bt601", color_range="tv", tile_size=0, border=0,
                   bit_depth=8):
        assert bit_depth == 16 and np.asarray(buf).nbytes == pref.frame_bytes(in_fmt, h, w)
        self.calls.append((in_fmt, out_fmt))
        x = pref.pix_to_bgr16(np.asarray(buf).reshape(-1).view(np.uint8).copy(), in_fmt, h, w, colour, False)
        return (self.apply(x, self.scale), out, out_fmt, colour)

    def collect_u8(self, t):
        x, out, out_fmt, colour = t
        out.reshape(-1).view(np.uint8)[...] = np.ascontiguousarray(pref.bgr16_to_pix(x, out_fmt, colour, False)).reshape(-1).view(np.uint8)
        return out

    @staticmethod
    def apply(bgr16, scale):
        return np.minimum(np.repeat(np.repeat(bgr16.astype(np.int64), scale, 0), scale, 1) + 3, 65535).astype(np.uint16)


@pytest.mark.parametrize("in_fmt,out_fmt,scales", [("p010le", "p010le", []), ("yuv420p10le", "p010le", [2]), ("p010le", "bgr48le", [1, 2]),
                                                   ("bgr48le", "yuv420p10le", [2]), ("bgr48le", "bgr48le", [])])
def test_stream_hands_bgr48le_between_the_stages(monkeypatch, in_fmt, out_fmt, scales):
    """the formats handed between stages: in_fmt -> bgr48le in front of the 16-bit denoise call, bgr48le mid-chain (the nets
    behind it are submitted bgr48le frames), out_fmt from the last stage -- and the bytes are the per-frame composition"""
    h, w = 6, 8
    lib = Denoise16FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    pix = rawvideo.PixFormats(in_fmt, out_fmt, "bt709", "tv", bit_depth=16)
    rng = np.random.default_rng(7)
    frames = [np.ascontiguousarray(pref.bgr16_to_pix(rng.integers(0, 65536, (h, w, 3), dtype=np.uint16), in_fmt, "bt709")) for _ in range(9)]
    want = []
    for f in frames:
        x = 65535 - pref.pix_to_bgr16(f.reshape(-1).view(np.uint8), in_fmt, h, w, "bt709", False)
        for s in scales:
            x = Bgr48FakeNet.apply(x, s)
        want.append(np.ascontiguousarray(pref.bgr16_to_pix(x, out_fmt, "bt709", False)).tobytes())
    nets = [Bgr48FakeNet(s) for s in scales]
    chain = [(("denoise", 2, 5), 0)] + [(n, 32) for n in nets]
    fout = io.BytesIO()
    n = rawvideo.stream(io.BytesIO(b"".join(f.tobytes() for f in frames)), fout, h, w, chain, alloc=lambda s: np.zeros(s, np.uint8), pix=pix)
    assert n == len(frames) and fout.getvalue() == b"".join(want)
    assert lib.denoised == [(2, 5.0)] * len(frames)
    want_conv = ([(in_fmt, "bgr48le")] if in_fmt != "bgr48le" else []) + ([("bgr48le", out_fmt)] if not scales and out_fmt != "bgr48le" else [])
    assert lib.converted == want_conv * len(frames)
    for k, net in enumerate(nets):
        assert set(net.calls) == {("bgr48le", out_fmt if k == len(nets) - 1 else "bgr48le")}


def test_the_8_bit_denoise_stage_keeps_its_calls(monkeypatch):
    """at 8 bits nothing moved: bgr24 is the stage's native format and uva_denoise_u8 the call"""
    calls = []

    class Lib:
        def uva_denoise_u8(self, gpu, src, h, w, ss, dst, ds, hl, hc):
            calls.append((h, w, ss, ds, hl))
            return 0

    monkeypatch.setattr(_lib, "load", lambda: Lib())
    st = rawvideo.DenoiseStage(0, 4, 5, 7, lambda s: np.zeros(s, np.uint8))
    assert st.native == "bgr24" and st._bgr_in is None and st._bgr_out is None
    st.submit(np.zeros((5, 7, 3), np.uint8))
    assert calls == [(5, 7, 21, 21, 4.0)] and st.collect().shape == (5, 7, 3)


def test_symbols_are_declared_and_optional():
    for n in ("uva_denoise_u16", "uva_denoise_u16_device", "uva_debug_denoise16_stage"):
        assert n in _lib.SYMBOLS and n in _lib.OPTIONAL_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "uva.h")).read()
    for n in ("uva_denoise_u16(", "uva_denoise_u16_device(", "uva_debug_denoise16_stage("):
        assert n in hdr
    assert "#define UVA_ABI_VERSION 15" in hdr
