"""Stress nets for tests/test_stress_nets.py: a shipped .bin with PReLU slopes or the last convolution's bias rewritten in place,
every shape and every convolution weight untouched.  Several kernel paths are chosen by the VALUES of a .bin, not by its shapes
-- a PReLU channel whose slope exceeds 1 is computed negated and the next layer's weights take the sign back -- and the three
shipped files leave most of those choices untaken (tests/golden/shipped_slope_census.json).  The kinds (c: the channel's index):

    head_up      PReLU 0: c % 3 == 0 -> 1.25                                                    (4x: its head has no slope above 1)
    last_up      the last PReLU: c % 3 == 0 -> 1.25                                             (no shipped net has one there)
    pair_all_up  PReLU 7 and 8 (2x, 4x: both layers of one trunkw launch, carried into the next), PReLU 4 and 5 (1x: either side
                 of the sub5 split): every channel -> 1.0 + 0.125 * (c % 4), a quarter of them exactly 1.0
    specials     PReLU 7 (2x), PReLU 4 (1x): c % 8 = 0..5 -> 0.0, -0.0, 1.0, 6e-8 (subnormal in fp16), -1.5, 1.0000001
    bias_ramp    the last convolution's bias + (pi(c) - (n - 1) / 2) * step / 255, pi(c) = c * k mod n with k = 5, 19, 2 for
                 n = 12, 48, 3: every channel its own offset, neighbouring channels far apart -- a bias that lands on the wrong
                 pixel-shuffle channel shows, which the same constant on every channel (mutant_net's tail_bias) cannot

and two KNOWN BAD variants of them, for the proofs that the bars bite:

    swap         bias_ramp with the biases of the two channels whose offsets are nearest (pi = n / 2 and n / 2 - 1) exchanged
    clamp        a slope kind with the rewritten slopes clamped to 1.0: what max(x, s * x) without the sign trick leaves
    ones         a slope kind with every rewritten slope replaced by 1.0 (the same net as clamp wherever all of them exceed 1)

write_stress_bin checks itself through the oracle's loader as mutant_net.write_mutant_bin does: every array but the named ones
equals the shipped one."""
import shutil

import numpy as np

from mutant_net import bin_layout, model_paths
from oracle import uvoracle

SLOPE_KINDS = ("head_up", "last_up", "pair_all_up", "specials")
KINDS = SLOPE_KINDS + ("bias_ramp",)
VARIANTS = (None, "swap", "clamp", "ones")
MATRIX = [("2x", "last_up"), ("2x", "pair_all_up"), ("2x", "specials"), ("2x", "bias_ramp"),
          ("4x", "head_up"), ("4x", "last_up"), ("4x", "pair_all_up"), ("4x", "bias_ramp"),
          ("1x", "last_up"), ("1x", "pair_all_up"), ("1x", "specials"), ("1x", "bias_ramp")]
SPECIALS = (0.0, -0.0, 1.0, 6e-8, -1.5, 1.0000001)
RAMP_K = {12: 5, 48: 19, 3: 2}
RAMP_STEP = {"2x": 1.0, "4x": 0.5, "1x": 2.0}      # levels between two neighbouring offsets of bias_ramp


def targets(key, kind, n_conv, n_prelu):
    """-> [(what, index)] of the arrays `kind` rewrites on net `key`"""
    assert (key, kind) in MATRIX, (key, kind, "is not a stress net")
    if kind == "bias_ramp":
        return [("bias", n_conv - 1)]
    if kind == "head_up":
        return [("slopes", 0)]
    if kind == "last_up":
        return [("slopes", n_prelu - 1)]
    first = 4 if key == "1x" else 7
    return [("slopes", first), ("slopes", first + 1)] if kind == "pair_all_up" else [("slopes", first)]


def ramp_pi(n):
    c = np.arange(n)
    pi = c * RAMP_K[n] % n
    assert sorted(pi) == list(c), (n, "k and n share a factor")
    return pi


def ramp_offsets(n, step):
    """bias_ramp's offset of every channel, in units of the output (one u8 level = 1 / 255)"""
    return ((ramp_pi(n) - (n - 1) / 2) * step / 255.0).astype(np.float32)


def swapped_channels(n):
    """the two channels whose bias_ramp offsets are nearest"""
    pi = list(ramp_pi(n))
    return pi.index(n // 2), pi.index(n // 2 - 1)


def rewrite(kind, a, step=None, variant=None):
    """shipped array a -> the stress net's (f32)"""
    c = np.arange(a.size)
    b = a.copy()
    if kind == "bias_ramp":
        b = a + ramp_offsets(a.size, step)
        if variant == "swap":
            i, j = swapped_channels(a.size)
            b[[i, j]] = b[[j, i]]
        else:
            assert variant is None, (kind, variant)
        return b.astype("<f4")
    if kind in ("head_up", "last_up"):
        new = c % 3 == 0
        b[new] = 1.25
    elif kind == "pair_all_up":
        new = np.ones(a.size, bool)
        b = 1.0 + 0.125 * (c % 4)
    elif kind == "specials":
        new = c % 8 < len(SPECIALS)
        b[new] = np.array(SPECIALS, np.float32)[c[new] % 8]
    b = b.astype(np.float32)
    if variant == "clamp":
        b[new] = np.minimum(b[new], np.float32(1.0))
    elif variant == "ones":
        b[new] = 1.0
    else:
        assert variant is None, (kind, variant)
    return b.astype("<f4")


def write_stress_bin(key, dst, kind, step=None, variant=None):
    """shipped .bin of `key` -> dst with the arrays of `kind` rewritten (module docstring); returns [(what, index)] of them"""
    assert kind in KINDS and variant in VARIANTS, (kind, variant)
    if kind == "bias_ramp" and step is None:
        step = RAMP_STEP[key]
    param, src = model_paths(key)
    layout, n_conv, n_prelu = bin_layout(param, src)
    want = targets(key, kind, n_conv, n_prelu)
    where = {(what, idx): (off, n) for what, idx, off, n in layout}
    shutil.copyfile(src, dst)
    written = {}
    with open(dst, "r+b") as f:
        for t in want:
            off, n = where[t]
            f.seek(off)
            a = np.frombuffer(f.read(4 * n), "<f4")
            b = rewrite(kind, a, step, variant)
            assert b.shape == a.shape and a.tobytes() != b.tobytes(), (key, kind, t, "changes nothing")
            f.seek(off)
            f.write(b.tobytes())
            written[t] = b
    # the self-check: through the oracle's own loader, every array is the shipped one except the targets
    shipped, stress = uvoracle.Model(param, src), uvoracle.Model(param, dst)
    assert stress.bin_consumed == stress.bin_size == shipped.bin_size
    for i in range(n_conv):
        (w0, b0, t0), (w1, b1, t1) = shipped.conv(i), stress.conv(i)
        assert t0 == t1 and np.array_equal(w0, w1), (key, kind, "weights of convolution", i)
        if ("bias", i) in written:
            assert b1.tobytes() == written[("bias", i)].tobytes(), (key, kind, "the bias was not rewritten")
        else:
            assert b0.tobytes() == b1.tobytes(), (key, kind, "bias of convolution", i)
    for i in range(n_prelu):
        s0, s1 = shipped.prelu(i), stress.prelu(i)
        if ("slopes", i) in written:
            assert s1.tobytes() == written[("slopes", i)].tobytes(), (key, kind, "the slopes were not rewritten")     # (bytes: -0.0)
        else:
            assert s0.tobytes() == s1.tobytes(), (key, kind, "slopes of PReLU", i)
    return want


def census():
    """-> {net: {"slopes": [{"prelu", "n", "gt1", "eq1", "lt0"}], "bias": [{"conv", "n", "abs_max"}]}} of the shipped files:
    what tests/golden/shipped_slope_census.json records (how many slopes of each PReLU exceed 1, equal 1, are negative; the
    absolute maximum of each convolution's bias)"""
    out = {}
    for key in ("2x", "4x", "1x"):
        param, src = model_paths(key)
        layout, _, _ = bin_layout(param, src)
        raw = open(src, "rb").read()
        slopes, bias = [], []
        for what, idx, off, n in layout:
            a = np.frombuffer(raw, "<f4", n, off)
            if what == "slopes":
                slopes.append({"prelu": idx, "n": n, "gt1": int((a > 1).sum()), "eq1": int((a == 1).sum()), "lt0": int((a < 0).sum())})
            else:
                bias.append({"conv": idx, "n": n, "abs_max": float(np.abs(a).max())})
        out[key] = {"slopes": slopes, "bias": bias}
    return out
