"""Stress nets (tests/stress_net.py): the kernel paths that the VALUES of a .bin choose, which the three shipped files leave untaken.

A PReLU channel whose slope exceeds 1 is computed negated on packed halves and the next layer's weights take the sign back
(trunkw_kernel TW_ACT_F16 / TW_ACT_F16_FLIP; uva_api.hip flip_w, wpk_wn, carry_out; the 1x net's pack_sub16 sin / sout; the f32
kernels' `sl <= 1 ? +inf : -inf` med3 selector).  Which of these run, on which layers and on how many channels, the .bin decides,
and the shipped ones (tests/golden/shipped_slope_census.json, test_the_census_of_the_shipped_files) never put a slope above 1 on
the last PReLU, never negate more than 8 channels of a layer, touch the `<= 1` boundary on two channels of one net, and carry
last-convolution biases of at most 1.3 u8 levels, so that a bias on the wrong pixel-shuffle channel sits inside every bar.
stress_net rewrites slopes or the last bias of a shipped .bin -- shapes and convolution weights untouched, activations in range --
and oracle.Model(param, bin) is the reference of any such file.

Frames: test_parity_bars.py's, synthetic_frame(seed=5), 270 x 480 for 2x / 4x and 540 x 960 for 1x (the "large" class).

MEASURED ON THE CPU (every figure below is asserted: PRODUCT_PSNR to +/- 0.3 dB; REACH as `max_lsb >= 3`)

  product-mode oracle against the fp32 oracle, both on the stress net itself (every one at most 1 LSB apart):

    kind            2x                    4x                    1x
    (shipped)       71.29 dB, 0.48 %      69.90 dB, 0.67 %      72.68 dB, 0.35 %
    head_up         --                    67.36 dB, 1.19 %      --
    last_up         67.24 dB, 1.23 %      67.08 dB, 1.28 %      66.79 dB, 1.36 %
    pair_all_up     68.74 dB, 0.87 %      66.31 dB, 1.52 %      67.40 dB, 1.18 %
    specials        70.03 dB, 0.65 %      --                    68.63 dB, 0.89 %
    bias_ramp       71.33 dB, 0.48 %      69.91 dB, 0.66 %      72.68 dB, 0.35 %
    tiled 64 / 10   last_up 67.20 dB, 1.24 %   pair_all_up 66.31 dB, 1.52 %

  The 1x column is the product mode WITH sub10_kernel's PReLU on packed halves in it (oracle SUB_PRELU_F16, product_flags()).
  Without it the oracle stood at 73.23 (shipped), 67.82, 67.89, 69.03 and 73.24 dB, and the kernel on 1x last_up -- 66.84 dB,
  1.345 % on the GPU -- left the window around 67.82 dB, 1.074 % that the shipped net (72.77 against 73.23 dB) stayed inside: the
  stress nets' finding.  The kernel rounds the sum to fp16, multiplies by the fp16 slope and rounds again (csrc/uva_sub10.hip.h
  sub10_store, as trunkw_kernel's TW_ACT_F16); the oracle restated that for the 64-feature nets only.  With it the stand-in is
  at 66.79 dB, 1.362 % there and at 72.68 dB, 0.351 % on the shipped net.

  the stress net's fp32 result against the shipped net's fp32 result (the rewrite reaches the output):

    kind            2x                          4x                          1x
    head_up         --                          33 LSB, 36.41 dB            --
    last_up         41 LSB, 29.34 dB            50 LSB, 26.17 dB            57 LSB, 27.47 dB
    pair_all_up     21 LSB, 37.60 dB            34 LSB, 32.35 dB            75 LSB, 28.14 dB
    specials        13 LSB, 41.04 dB            --                          70 LSB, 27.28 dB
    bias_ramp        6 LSB, 37.28 dB            12 LSB, 31.30 dB             3 LSB, 43.87 dB   (no sample at a clamp end)

PROOFS THAT THE BARS BITE, the product-mode oracle standing in for the kernel; pass / fail is _side_by_side's window (PSNR within
1.0 dB, share within a factor 1.25) around the product-mode figure of the stress net above.

  bias_ramp with the biases of the two channels whose offsets are nearest exchanged (stress_net variant "swap"), its product-mode
  result against the UNSWAPPED net's fp32 result -- outside the window:

    net   step (levels)   swapped                        the window's centre (unswapped)
    2x    1.0             56.84 dB, 13.45 %, max 1 LSB   71.33 dB, 0.48 %
    4x    0.5             62.80 dB,  3.41 %, max 1 LSB   69.91 dB, 0.66 %
    1x    2.0             42.76 dB, 66.77 %, max 3 LSB   72.68 dB, 0.35 %

  each slope kind with the rewritten slopes clamped to 1.0 (variant "clamp": what a kernel that kept max(x, s * x) without the
  sign trick leaves) -- outside the window, except `specials`:

    kind            2x                            4x                            1x
    head_up         --                            46.37 dB, 60.80 %, 13 LSB     --
    last_up         42.98 dB, 76.88 %,  8 LSB     39.87 dB, 84.26 %, 10 LSB     40.90 dB, 82.00 %, 12 LSB
    pair_all_up     42.76 dB, 72.43 %, 13 LSB     41.13 dB, 80.88 %, 17 LSB     34.47 dB, 90.74 %, 37 LSB
    specials        70.03 dB,  0.65 %,  1 LSB     --                            68.63 dB,  0.89 %,  1 LSB    (INSIDE: see below)
    specials, ones  38.10 dB, 86.97 %, 18 LSB     --                            27.16 dB, 95.43 %, 72 LSB

  `specials` probes the `<= 1` boundary itself, where max and min semantics coincide: its only slope above 1 is 1 + 2^-23, so the
  clamped net differs from it by one part in 10^7 on every eighth channel and the figures are the stress net's own.  That is the
  property the kind holds a kernel to -- nothing may depend on which side of the selector a slope of 1.0 or 1.0000001 falls --
  and it is asserted as such (test_specials_clamped_is_the_same_net).  That the specials' channels reach the bars is shown with
  every rewritten slope REPLACED by 1.0 (variant "ones", the same net as "clamp" for the other kinds): outside the window.

-m gpu: the kernels themselves on every stress net -- process_u8 whole and tiled against the oracle on the same net (product
mode: 1 LSB, 5 % / 8 % of the samples; fp32: 2 LSB, 50 dB; and the window around the product-mode oracle's distance), byte-exact
carry / sub5 / batch properties, the float route and the 16-bit route on bias_ramp.  Every record carries no model and no route,
so tools/parity_slack.py never harvests a stress net into the shipped bars."""
import functools
import json
import os

import numpy as np
import pytest

import mutant_net
import parity_report as pr
import stress_net
import test_parity_bars as bars
from conftest import ROOT
from oracle import uvoracle

FP32 = "fp32 oracle"
PRODUCT = "oracle, product rounding mode"
MATRIX = stress_net.MATRIX
IDS = [f"{k}-{kind}" for k, kind in MATRIX]
SLOPE_NETS = [(k, kind) for k, kind in MATRIX if kind != "bias_ramp"]
UP_NETS = [(k, kind) for k, kind in SLOPE_NETS if kind != "specials"]
TILED = [("2x", "last_up"), ("4x", "pair_all_up")]
# product-mode oracle against the fp32 oracle on the stress net, dB (the table above); asserted to +/- 0.3 dB
PRODUCT_PSNR = {("2x", "last_up"): 67.24, ("2x", "pair_all_up"): 68.74, ("2x", "specials"): 70.03, ("2x", "bias_ramp"): 71.33,
                ("4x", "head_up"): 67.36, ("4x", "last_up"): 67.08, ("4x", "pair_all_up"): 66.31, ("4x", "bias_ramp"): 69.91,
                ("1x", "last_up"): 66.79, ("1x", "pair_all_up"): 67.40, ("1x", "specials"): 68.63, ("1x", "bias_ramp"): 72.68}
PRODUCT_PSNR_TILED = {("2x", "last_up"): 67.20, ("4x", "pair_all_up"): 66.31}
FLOAT_STEP = 4.0                   # levels: the float result is not clamped, so saturation does not limit the float route's ramp


frame = bars.frame

_DIR = None


@pytest.fixture(scope="session")
def stress(tmp_path_factory):
    """the directory the stress .bin files of this session are written to (stress_bin); every test that uses one asks for it"""
    global _DIR
    _DIR = str(tmp_path_factory.mktemp("stress"))
    return _DIR


@functools.lru_cache(maxsize=None)
def stress_bin(key, kind, step=None, variant=None):
    """path of the stress .bin, written once per session"""
    dst = os.path.join(_DIR, f"{key}_{kind}_{step}_{variant}.bin")
    stress_net.write_stress_bin(key, dst, kind, step=step, variant=variant)
    return dst


@functools.lru_cache(maxsize=None)
def oracle_model(key, kind, step=None, variant=None):
    return uvoracle.Model(mutant_net.model_paths(key)[0], stress_bin(key, kind, step, variant))


@functools.lru_cache(maxsize=None)
def oracle_u8(key, kind, product=False, tile=0, variant=None):
    """the oracle's u8 result on frame(key) for a stress net: fp32 or product mode, whole frame or tiled"""
    uvoracle.build()
    flags = uvoracle.product_flags() if product else 0
    m = oracle_model(key, kind, None, variant)
    out = m.upscale_image(frame(key), tile_size=tile, border=10, flags=flags) if tile else m.apply_model(frame(key), flags=flags)
    out.setflags(write=False)
    return out


def _tag(key, kind, tile=0):
    return f"{key} stress {kind} {bars.FRAMES[key][1]}x{bars.FRAMES[key][0]} t{tile}"


# ------------------------------------------------------------------------------------------------------------------
# the writer and the census
# ------------------------------------------------------------------------------------------------------------------
def test_the_stress_writer_changes_the_named_arrays_only(tmp_path):
    """(write_stress_bin checks itself through the oracle's loader; here: the file differs from the shipped one only inside the
    bytes of the named arrays, every one of them changed; the arrays hold what the issue's table says; a kind on a net outside
    the matrix is refused)"""
    for key, kind in MATRIX:
        param, src = mutant_net.model_paths(key)
        dst = str(tmp_path / f"{key}_{kind}.bin")
        named = stress_net.write_stress_bin(key, dst, kind)
        layout, n_conv, n_prelu = mutant_net.bin_layout(param, src)
        last = n_prelu - 1
        assert named == {"head_up": [("slopes", 0)], "last_up": [("slopes", last)], "bias_ramp": [("bias", n_conv - 1)],
                         "pair_all_up": [("slopes", 4), ("slopes", 5)] if key == "1x" else [("slopes", 7), ("slopes", 8)],
                         "specials": [("slopes", 4 if key == "1x" else 7)]}[kind]
        a, b = np.fromfile(src, np.uint8), np.fromfile(dst, np.uint8)
        assert a.size == b.size
        inside = np.zeros(a.size, bool)
        m = uvoracle.Model(param, dst)
        for what, idx, off, n in layout:
            if (what, idx) not in named:
                continue
            inside[off:off + 4 * n] = True
            assert (a[off:off + 4 * n] != b[off:off + 4 * n]).any(), (key, kind, what, idx)
            c = np.arange(n)
            if kind in ("head_up", "last_up"):
                s0 = uvoracle.load_model(key).prelu(idx)
                assert np.array_equal(m.prelu(idx), np.where(c % 3 == 0, np.float32(1.25), s0))
            elif kind == "pair_all_up":
                s = m.prelu(idx)
                assert np.array_equal(s, (1.0 + 0.125 * (c % 4)).astype(np.float32)) and (s == 1).sum() == n // 4 and (s > 1).sum() == 3 * n // 4
            elif kind == "specials":
                s = m.prelu(idx)
                assert s[:6].tobytes() == np.array([0.0, -0.0, 1.0, 6e-8, -1.5, 1.0000001], np.float32).tobytes() and s[5] > 1
                assert 0 < np.float16(s[3]) < np.float16(6.2e-5), "6e-8 is to be subnormal, not zero, in fp16"
                assert np.array_equal(s[c % 8 >= 6], uvoracle.load_model(key).prelu(idx)[c % 8 >= 6])
            else:
                off_lv = (m.conv(idx)[1].astype(np.float64) - uvoracle.load_model(key).conv(idx)[1]) * 255 / stress_net.RAMP_STEP[key]
                want = stress_net.ramp_pi(n) - (n - 1) / 2
                assert np.allclose(off_lv, want, atol=1e-4) and len(set(np.rint(off_lv * 2).astype(int))) == n
                if n > 3:            # neighbouring channels far apart: at least a quarter of the ramp
                    assert np.abs(np.diff(want)).min() >= n // 4
                i, j = stress_net.swapped_channels(n)
                assert abs(want[i] - want[j]) == 1
        assert not (a != b)[~inside].any(), (key, kind, "bytes outside the named arrays changed")
    for key, kind in (("2x", "head_up"), ("1x", "head_up"), ("4x", "specials")):
        with pytest.raises(AssertionError):
            stress_net.write_stress_bin(key, str(tmp_path / "x.bin"), kind)
    with pytest.raises(AssertionError):
        stress_net.write_stress_bin("2x", str(tmp_path / "x.bin"), "weights")


def test_the_census_of_the_shipped_files():
    """tests/golden/shipped_slope_census.json is what models/ holds -- and it holds the gaps the stress kinds exist for.  If a
    shipped file changes, the first assertion says so, and the ones below say which kind has become redundant (the shipped net
    now takes that path itself) or insufficient."""
    committed = json.load(open(os.path.join(ROOT, "tests", "golden", "shipped_slope_census.json")))
    now = stress_net.census()
    assert now == committed["census"], "models/ changed: regenerate the census (stress_net.census) and re-read the kinds"
    for key in ("2x", "4x", "1x"):
        s = now[key]["slopes"]
        assert s[-1]["gt1"] == 0, (key, "the last PReLU has a slope above 1: last_up is redundant on this net")
        assert max(e["gt1"] for e in s) <= (5 if key == "1x" else 8), (key, "more channels of a layer negated than before: re-read pair_all_up")
        assert now[key]["bias"][-1]["abs_max"] * 255 < 1.5, (key, "the last bias exceeds 1.5 levels: bias_ramp's step may be too small")
    assert now["4x"]["slopes"][0]["gt1"] == 0, "the 4x head has a slope above 1: head_up is redundant"
    assert [e["gt1"] for e in now["2x"]["slopes"][15:]] == [0, 0] and [e["gt1"] for e in now["4x"]["slopes"][14:]] == [0, 0, 0]
    assert sum(e["eq1"] for k in now for e in now[k]["slopes"]) == 2, "slopes of exactly 1.0: specials / pair_all_up put them on every net"


# ------------------------------------------------------------------------------------------------------------------
# without a GPU: the stress nets are usable references, and the bars tell a wrong kernel on them
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,kind", MATRIX, ids=IDS)
def test_stress_net_is_usable_as_a_reference(stress, key, kind):
    """product mode at most 1 LSB from fp32 and inside the fixed fp32 bars, at the measured distance (PRODUCT_PSNR)"""
    got, want = oracle_u8(key, kind, product=True), oracle_u8(key, kind)
    worst, psnr, share = pr.check_u8(_tag(key, kind) + ": product-mode oracle", got, want, vs=FP32, model=None, route=None, max_lsb=2, min_psnr=50)
    print(f"{key} {kind}: product mode against fp32 {psnr:.2f} dB, {100 * share:.2f} %, max {worst} LSB")
    assert worst <= 1
    assert psnr == pytest.approx(PRODUCT_PSNR[key, kind], abs=0.3), (key, kind, psnr, share)


@pytest.mark.parametrize("key,kind", TILED)
def test_tiled_stress_net_is_usable_as_a_reference(stress, key, kind):
    got, want = oracle_u8(key, kind, product=True, tile=64), oracle_u8(key, kind, tile=64)
    worst, psnr, share = pr.check_u8(_tag(key, kind, 64) + ": product-mode oracle", got, want, vs=FP32, model=None, route=None, max_lsb=2, min_psnr=50)
    print(f"{key} {kind} tiled 64 / 10: product mode against fp32 {psnr:.2f} dB, {100 * share:.2f} %, max {worst} LSB")
    assert worst <= 1
    assert psnr == pytest.approx(PRODUCT_PSNR_TILED[key, kind], abs=0.3), (key, kind, psnr, share)


@pytest.mark.parametrize("key,kind", MATRIX, ids=IDS)
def test_the_rewrite_reaches_the_output(stress, key, kind):
    worst, psnr, share = mutant_net.distance_u8(oracle_u8(key, kind), bars.oracle_u8(key))
    print(f"{key} {kind}: stress fp32 against shipped fp32 max {worst} LSB, {psnr:.2f} dB, {100 * share:.2f} %")
    assert worst >= 3, (key, kind, worst, psnr, share)
    if kind == "bias_ramp":          # no sample at a clamp end: every channel's offset is in the result in full
        for product in (False, True):
            out = oracle_u8(key, kind, product=product)
            assert int(((out == 0) | (out == 255)).sum()) == 0, (key, product)


def _window(key, kind, got_variant, name):
    """-> (the KNOWN BAD variant's distance, the stress net's own), both product mode against the stress net's fp32 result, and
    whether _side_by_side's window tells them apart (it raises if it does)"""
    got, product, want = oracle_u8(key, kind, product=True, variant=got_variant), oracle_u8(key, kind, product=True), oracle_u8(key, kind)
    g, p = mutant_net.distance_u8(got, want), mutant_net.distance_u8(product, want)
    try:
        bars._side_by_side(name, got, product, want)
    except AssertionError:
        return g, p, True
    return g, p, False


@pytest.mark.parametrize("key", bars.KEYS)
def test_a_swapped_tail_bias_leaves_the_window(stress, key):
    """bias_ramp with two channels' biases exchanged -- the two whose offsets are nearest, one step apart: the smallest
    misplacement there is -- is told from the stress net by the window the GPU tests hold the kernels to"""
    g, p, outside = _window(key, "bias_ramp", "swap", f"{key} stress bias_ramp, two channels swapped (KNOWN BAD) as the kernel's stand-in")
    print(f"{key} bias_ramp swapped: {g[1]:.2f} dB, {100 * g[2]:.2f} %, max {g[0]} LSB | unswapped {p[1]:.2f} dB, {100 * p[2]:.2f} %")
    assert p[1] == pytest.approx(PRODUCT_PSNR[key, "bias_ramp"], abs=0.3)
    assert outside, (key, g, p)
    assert g[1] < p[1] - 1.0 and g[2] > 1.25 * p[2], (key, g, p)            # ... on both of its figures


@pytest.mark.parametrize("key,kind", UP_NETS, ids=[f"{k}-{kind}" for k, kind in UP_NETS])
def test_slopes_clamped_to_one_leave_the_window(stress, key, kind):
    """max(x, s * x) without the sign trick is PReLU with min(s, 1): on every kind that puts slopes above 1 the window tells it"""
    g, p, outside = _window(key, kind, "clamp", f"{key} stress {kind}, slopes clamped to 1.0 (KNOWN BAD) as the kernel's stand-in")
    print(f"{key} {kind} clamped: {g[1]:.2f} dB, {100 * g[2]:.2f} %, max {g[0]} LSB | the stress net {p[1]:.2f} dB, {100 * p[2]:.2f} %")
    assert outside, (key, kind, g, p)
    assert g[1] < p[1] - 1.0 and g[2] > 1.25 * p[2], (key, kind, g, p)


@pytest.mark.parametrize("key", ["2x", "1x"])
def test_specials_clamped_is_the_same_net(stress, key):
    """specials' only slope above 1 is 1 + 2^-23 (module docstring): clamping moves one channel in eight by one part in 10^7,
    and no sample of either oracle mode may notice -- which side of the selector the boundary slopes fall on decides nothing"""
    (idx,) = [i for what, i in stress_net.targets(key, "specials", 0, 0)]
    a, b = oracle_model(key, "specials").prelu(idx), oracle_model(key, "specials", None, "clamp").prelu(idx)
    c = np.arange(a.size)
    assert np.array_equal(a[c % 8 != 5], b[c % 8 != 5]) and (b[c % 8 == 5] == 1).all() and (a[c % 8 == 5] == np.float32(1.0000001)).all()
    for product in (False, True):
        d = mutant_net.distance_u8(oracle_u8(key, "specials", product=product, variant="clamp"), oracle_u8(key, "specials", product=product))
        print(f"{key} specials clamped against itself, product={product}: max {d[0]} LSB, {100 * d[2]:.4f} %")
        # (a slope moved by 2^-23: even a channel that moved the output by the 75 levels of test_the_rewrite_reaches_the_output
        # at a slope change of order 1 moves it by 1e-5 level here, which flips the rounding of 2e-5 of the samples: measured
        # 5e-6 and 7e-6.  In product mode the slope is rounded to fp16, 1.0 either way, wherever the PReLU is on halves; where
        # it is not, a moved value's own rounding to fp16 may flip by a whole ulp: held to 1 LSB here and to the window below)
        assert d[0] <= 1 and (product or d[2] <= 1e-4), (key, product, d)
    g, p, outside = _window(key, "specials", "clamp", f"{key} stress specials, slopes clamped to 1.0 as the kernel's stand-in")
    assert not outside, (key, g, p)


@pytest.mark.parametrize("key", ["2x", "1x"])
def test_specials_replaced_by_one_leave_the_window(stress, key):
    g, p, outside = _window(key, "specials", "ones", f"{key} stress specials, rewritten slopes replaced by 1.0 (KNOWN BAD) as the kernel's stand-in")
    print(f"{key} specials replaced by 1.0: {g[1]:.2f} dB, {100 * g[2]:.2f} %, max {g[0]} LSB | the stress net {p[1]:.2f} dB, {100 * p[2]:.2f} %")
    assert outside, (key, g, p)
    assert g[1] < p[1] - 1.0 and g[2] > 1.25 * p[2], (key, g, p)


# ------------------------------------------------------------------------------------------------------------------
# -m gpu: the kernels themselves on the stress nets
# ------------------------------------------------------------------------------------------------------------------
def _load(uva, path, key):
    """(test_parity_bars._load, for a .bin given by its path)"""
    net = uva.Net()
    net.opt.use_vulkan_compute = True
    net.set_vulkan_device(0)
    assert net.load_param(mutant_net.model_paths(key)[0]) == 0, getattr(net, "last_error", "")
    assert net.load_model(path) == 0, getattr(net, "last_error", "")
    return net


def _product_share(key):
    """share of u8 samples that may differ, by one level, from the product-mode oracle: the round numbers of test_gpu_parity.py's
    U8_DIFFER (5 %; 8 % where the trunk runs as Winograd F(2,3)) -- the shipped nets' measured bars are not a stress net's"""
    return 8e-2 if (uvoracle.product_flags() & uvoracle.WINOGRAD_F23) and key != "1x" else 5e-2


def _hold_to_the_oracle(name, got, product, want, key):
    pr.check_u8(name, got, product, vs=PRODUCT, max_lsb=1, max_share=_product_share(key), model=None, route=None)
    pr.check_u8(name, got, want, vs=FP32, max_lsb=2, min_psnr=50, model=None, route=None, input_class="smooth")
    return bars._side_by_side(name, got, product, want)


@pytest.mark.gpu
@pytest.mark.parametrize("key,kind", MATRIX, ids=IDS)
def test_gpu_whole_frame_on_the_stress_net(uva, stress, key, kind):
    assert uva.get_gpu_count() > 0
    net = _load(uva, stress_bin(key, kind), key)
    got = net.process_u8(frame(key), tile_size=0)
    _hold_to_the_oracle(_tag(key, kind), got, oracle_u8(key, kind, product=True), oracle_u8(key, kind), key)


@pytest.mark.gpu
@pytest.mark.parametrize("key,kind", TILED)
def test_gpu_tiled_frame_on_the_stress_net(uva, stress, key, kind):
    assert uva.get_gpu_count() > 0
    net = _load(uva, stress_bin(key, kind), key)
    got = net.process_u8(frame(key), tile_size=64, border=10)
    _hold_to_the_oracle(_tag(key, kind, 64), got, oracle_u8(key, kind, product=True, tile=64), oracle_u8(key, kind, tile=64), key)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["pair_all_up", "last_up"])
@pytest.mark.parametrize("key", ["2x", "4x"])
def test_gpu_sign_carry_changes_no_bit_on_the_stress_net(uva, stress, key, kind, monkeypatch):
    """test_gpu_parity.py's test_sign_carry_between_launches_changes_no_bit where it matters: every channel of both layers of a
    launch negated and carried into the next (pair_all_up), and the last pair restoring its signs in front of the tail (last_up)"""
    assert uva.get_gpu_count() > 0
    img = uvoracle.synthetic_frame(131, 94, seed=77)
    monkeypatch.setenv("UVA_TW_CARRY", "0")
    plain = _load(uva, stress_bin(key, kind), key)            # (the switches are read when a net's device side is built)
    a = plain.process_u8(img, tile_size=64, border=10)
    b = plain.process_u8(img, tile_size=0)
    monkeypatch.delenv("UVA_TW_CARRY")
    net = _load(uva, stress_bin(key, kind), key)
    assert np.array_equal(net.process_u8(img, tile_size=64, border=10), a)
    assert np.array_equal(net.process_u8(img, tile_size=0), b)


KINDS_1X = [kind for k, kind in MATRIX if k == "1x"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS_1X)
def test_gpu_sub5_gives_the_bytes_of_sub10_on_the_stress_net(uva, stress, kind):
    """(loaded as test_gpu_sub5.py's `both`)"""
    assert uva.get_gpu_count() > 0
    os.environ["UVA_SUB5"] = "1"          # (the switches are read when a net's device side is built)
    try:
        split = _load(uva, stress_bin("1x", kind), "1x")
        split.process_u8(np.zeros((8, 8, 3), np.uint8), tile_size=0)
    finally:
        del os.environ["UVA_SUB5"]
    whole = _load(uva, stress_bin("1x", kind), "1x")
    for h, w in ((50, 33), (37, 54), (130, 216)):
        img = uvoracle.synthetic_frame(h, w, kind="random", seed=31 * h + w)
        a, b = split.process_u8(img, tile_size=0), whole.process_u8(img, tile_size=0)
        assert np.array_equal(a, b), (kind, h, w, int(np.abs(a.astype(int) - b.astype(int)).max()), float((a != b).mean()))


@pytest.mark.gpu
def test_gpu_batch_gives_the_bytes_of_single_calls_on_the_stress_net(uva, stress):
    from test_gpu_batch import run_batch
    assert uva.get_gpu_count() > 0
    net = _load(uva, stress_bin("1x", "last_up"), "1x")
    h, w, count = 37, 121, 3
    frames = [uvoracle.synthetic_frame(h, w, kind="random" if k & 1 else "smooth", seed=77 * count + k) for k in range(count)]
    want = [net.process_u8(f, tile_size=0) for f in frames]
    got = run_batch(net, frames)
    for k in range(count):
        assert np.array_equal(got[k], want[k]), (k, float((got[k] != want[k]).mean()))


@pytest.mark.gpu
@pytest.mark.parametrize("key,h,w", [("2x", 37, 70), ("4x", 21, 45), ("1x", 50, 33)])
def test_gpu_float_route_puts_every_tail_bias_on_its_channel(uva, stress, key, h, w):
    """bias_ramp with a step of 4 levels: neighbouring offsets are 4 / 255 = 1.57e-2 apart, the float bar is 6e-3 -- no two
    channels can be exchanged inside it"""
    assert uva.get_gpu_count() > 0
    n = 3 * oracle_model(key, "bias_ramp", FLOAT_STEP).scale ** 2
    assert np.abs(np.diff(np.sort(stress_net.ramp_offsets(n, FLOAT_STEP)))).min() > 2 * 6e-3
    net = _load(uva, stress_bin(key, "bias_ramp", FLOAT_STEP), key)
    x = uvoracle.from_pixels_normalize(uvoracle.synthetic_frame(h, w, kind="random", seed=h * 1000 + w))
    got = net._extract(x)
    want = oracle_model(key, "bias_ramp", FLOAT_STEP).forward(x)
    assert got.shape == want.shape
    pr.check_f32(f"{key} stress bias_ramp step {FLOAT_STEP} extract {w}x{h}", got, want, vs=FP32, max_abs=6e-3, model=None, route=None)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["2x", "4x"])
def test_gpu_u16_route_puts_every_tail_bias_on_its_channel(uva, stress, key):
    from test_gpu_bitdepth16 import _product_bars, _product_u16, _smooth16
    assert uva.get_gpu_count() > 0
    net = _load(uva, stress_bin(key, "bias_ramp"), key)
    x16 = _smooth16(64, 96)
    got = net.process_u16(x16, tile_size=0, border=10)
    want = _product_u16(oracle_model(key, "bias_ramp"), uvoracle, x16, 0)
    pr.check_u16(f"u16 {key} stress bias_ramp 96x64 t0 smooth16", got, want, vs=pr.U16_PRODUCT, model=None, route=None, **_product_bars(key))
