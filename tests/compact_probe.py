"""Probe nets for tests/test_compact_probes.py: the shipped .param of the 2x / 4x / 1x Compact nets with a .bin whose arithmetic is
EXACT, so that the kernels the product ships on (headp_kernel / head_kernel, trunkw_kernel<64>, trunk2_kernel, trunk_kernel,
tail_kernel, tail4_kernel, sub10_kernel, sub10_kernel16, sub5_kernel, pair24_kernel) and the host code that packs their weights
(the Winograd transform, flip_w / wpk_wn / carry_out, pack_sub16, the tails' pixel-shuffle order) can be held to a float64
reference bit for bit -- tests/generic_probe.py's idea on the nets whose constants are compile-time.

Every weight, bias, slope and input is a small dyadic number.  Every stored activation is then a value fp16 holds exactly, every
Winograd-transformed input and weight too, and every fp32 accumulation adds multiples of one power of two whose absolute sum stays
below 2^24 of them: exact in ANY order.  A correct kernel of any flavour returns the reference's bits; Ref.forward(audit=...)
proves the premise per (net, weight set, frame).

    design(key, wset)    the arrays of weight set `wset` (NSETS[key] of them), every non-zero placed by construction:
        base family      every output channel of a convolution has one +1 and one -1 (the last convolution: TAIL_NZ[key] weights of
                         +-0.25, signs alternating), biases k/8 with |k| <= 2, PReLU slopes 0 or -1 (activations stay >= 0, a
                         difference of two of them cannot outgrow them), inputs k/8 in [0, 1] or 0 / 1.  The non-zeros of a
                         convolution walk its (input channel, tap) positions: position q is channel q % cin at tap
                         (q // cin + q % cin) % 9, output channel o of set s takes q0(s) + 2 o and the next one, so that channel
                         and tap move together, a set reads every input channel of every layer (nothing is cut off from the
                         output) and the sets' windows of positions tile all of them: coverage()
        excursions       a window of two or three consecutive PReLUs (WINDOWS[key][wset]; over the sets every PReLU is in one:
                         the head's, both layers of every trunkw launch, the last one, either side of the 1x net's sub5 split)
                         carries slopes of 2, 1.25, exactly 1.0 and 0.5 on a pattern of channels (as far as the lattice budget
                         of the set allows: design, lattice_min), the convolution in front of
                         the window a third weight of +-0.5 on up to every other output channel; 2x / 4x
                         set 4 has EVERY channel of PReLU 9 and 10 above 1 (all 64 channels negated in both layers of one launch
                         and carried into the next).
                         A weight that reads a channel whose slope is 2 is +-0.5: the range comes back behind the window
        tail             the last convolution's biases are odd multiples of 2^-4 (4x: 2^-6, see tail_bias), a different one on
                         each channel, neighbouring channels far apart (stress_net.ramp_pi): a weight or a bias on the wrong
                         pixel-shuffle channel shows
    write_probe_bin      the .bin of a design for the shipped .param, each convolution's storage flag as shipped; checks itself
                         through the oracle's loader
    Ref                  float64 forward of (param, bin): its own reader of the .bin, convolution with zero padding as a loop
                         over the non-zero weights, PReLU, PixelShuffle, nearest Interp, Add; per-layer taps; the u8 / u16 frame
                         routes whole and tiled; the audit; and MUTANTS, one plausible slip each, restated in numpy
"""
import struct

import numpy as np

from generic_probe import _conv64, _f16_exact, _low_bit, wino_audit
from mutant_net import model_paths
from oracle.generic_oracle import FP16_FLAG, conv_shapes, parse_param
from stress_net import ramp_pi

KEYS = ("2x", "4x", "1x")
NSETS = {"2x": 8, "4x": 8, "1x": 9}        # 1x: nine, so that eight weights per channel of its last convolution cover its 216 positions
TAIL_NZ = {"2x": 6, "4x": 2, "1x": 8}           # non-zeros per output channel of the last convolution (12 / 48 / 3 channels)
# the PReLUs inside set s's excursion window.  2x / 4x: PReLU 2k - 1 and 2k are the two layers of one trunkw launch
WINDOWS = {"2x": ((0, 1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16)),
           "1x": ((0, 1), (2, 3), (4, 5), (6, 7), (8,), (3, 4), (5, 6), (7, 8), (1, 2))}
WINDOWS["4x"] = WINDOWS["2x"]
ALL_UP_SET = 4                                  # 2x / 4x: every channel of PReLU 9 and 10 (one launch) above 1
STRIP = 30                                      # trunkw_kernel's strips own 30 columns (csrc/uva_wino.hip.h)
# slopes of an excursion layer by channel % 8.  One layer of a window is RICH (1.25 and 0.5 refine the lattice the values lie on by
# 4 and 2), the others PLAIN (2 and 1.0 leave it alone): refinements on different channels of one layer do not multiply, those of
# consecutive layers do, and a window spends 3 bits of lattice that way (1/8 -> 1/64 behind it), whichever of its layers is RICH.
# The three-layer window of set 0 (the head's PReLU and the first launch) is PLAIN_HEAD, PLAIN, PLAIN for the same budget.
RICH = (2.0, 1.25, 1.0, 0.5, 0.0, -1.0, 1.25, 2.0)
PLAIN = (2.0, 1.0, 0.0, -1.0, 2.0, -1.0, 1.0, 0.0)
PLAIN_HEAD = (2.0, 1.0, 0.5, 0.0, -1.0, 2.0, 1.0, -1.0)


def net_shape(key):
    """-> (layers of the shipped .param, [(cout, cin)] of its convolutions, scale)"""
    layers = parse_param(model_paths(key)[0])
    convs = [(co, ci) for _, co, ci, k, b in conv_shapes(layers) if k == 3 and b]
    assert len(convs) == sum(L["type"] == "Convolution" for L in layers)
    return layers, convs, {"2x": 2, "4x": 4, "1x": 1}[key]


# ---------------------------------------------------------------------------------------------------------------- the design
def position(q, cin):
    """position q of a convolution's cin * 9 (input channel, tap) positions: channel and tap move together"""
    q %= cin * 9
    ci = q % cin
    return ci, (q // cin + ci) % 9


def tail_bias(key, n):
    """odd multiples of 2^-4, a different one on each of the n channels, stress_net.ramp_pi's order.  4x: 2^-6 -- 48 different
    odd multiples of 2^-4 span 47 / 8 = 5.9, six times the output's range, and with the bias of a channel uniform over that span
    at most 9 channels in 48 can be inside [0, 1] for any one pixel: a clamp share of 81 % at least, and channels that never
    leave a clamp end.  Odd multiples of 2^-6 span 1.47 as the 12 channels of 2x do with 2^-4 (1.38)."""
    pi = ramp_pi(n).astype(np.float64)
    step = 2.0 ** -6 if key == "4x" else 2.0 ** -4
    b = (2 * pi - (n - 1) - (n % 2)) * step
    assert len(set(b)) == n and (np.abs(b / step) % 2 == 1).all()
    return b


# no activation of set s lies on a lattice finer than 2^lattice_min(s): 2^-6 leaves room for every excursion of a window in a row
# (1.25 costs two bits, 0.5 and a halved weight one each); the SHALLOW sets stop at 2^-5, which puts the output on 2^-7 behind
# the last convolution's 0.25 -- what the 16-bit route needs (epilogue_audit) -- and drop the excursions that do not fit
SHALLOW = (1, 5)          # (odd sets: the PLAIN layer of their window comes first, and both layers keep slopes above 1)


def lattice_min(wset):
    return -5 if wset in SHALLOW else -6


def wanted_slopes(key, wset, i, n):
    """the slopes PReLU i of set wset is to take, the lattice permitting (design)"""
    c = np.arange(n)
    win = WINDOWS[key][wset]
    if i not in win:
        return np.where((c + i + wset) % 2 == 0, 0.0, -1.0)
    k = win.index(i)
    if key != "1x" and wset == ALL_UP_SET:
        return np.where(c % 2 == 0, 2.0, 1.25) if k == 0 else np.full(n, 2.0)
    if len(win) == 3:
        pat = np.array(PLAIN if k else PLAIN_HEAD)
    else:
        pat = np.array(RICH if len(win) == 1 or (k + wset) % 2 == 0 else PLAIN)
    return pat[(c + wset + i) % 8]


def design(key, wset):
    """-> W [(w [cout][cin][3][3], bias [cout])] per convolution, S [slopes] per PReLU: float64, every value exact in fp16.

    The lattice every channel's values lie on (2^e, e per channel) is followed layer by layer, and an excursion that would
    take a channel below 2^lattice_min(wset) gives way: a slope of 1.25 there becomes 2, one of 0.5 becomes 1.0, one of 2 whose channel
    could not be read with +-0.5 becomes 1.0 (in the all-up set it stays, the weights that read it stay +-1 and the range
    stays doubled), a third weight is left out.  The budget is
    what keeps 65535 y clear of the one rounding the tails' fp32 epilogue cannot promise (epilogue_audit)."""
    _, convs, _ = net_shape(key)
    n_conv = len(convs)
    win = WINDOWS[key][wset]
    LATTICE_MIN = lattice_min(wset)
    W, S = [], []
    e_in = np.full(3, -3)                       # inputs k / 8 (the frames' 0 and 1 are coarser)
    up = np.zeros(3, bool)                      # input channels the PReLU in front doubled
    for i, (cout, cin) in enumerate(convs):
        last = i == n_conv - 1
        per = TAIL_NZ[key] if last else 2
        w = np.zeros((cout, cin, 9))
        q0 = wset * per * cout + 7 * i
        halve = up & (e_in - (2 if last else 0) - 1 >= (LATTICE_MIN - 2 if last else LATTICE_MIN))
        want = wanted_slopes(key, wset, i, cout) if not last else None
        for o in range(cout):
            for j in range(per):
                ci, tap = position(q0 + per * o + j, cin)
                assert w[o, ci, tap] == 0
                w[o, ci, tap] = (0.25 if last else 1.0) * (0.5 if halve[ci] else 1.0) * (1 if (j + o + wset) % 2 == 0 else -1)
            # the third weight, in front of the window: every other output channel, those with a slope of 1.25 or 0.5 left out
            # (its bit and theirs would add up on the one channel)
            if not last and i == win[0] and o % 2 == wset % 2 and want[o] not in (1.25, 0.5):
                ci, tap = position(q0 + per * o + 2 + 9 * (cin // 3) + 5, cin)
                if w[o, ci, tap] == 0 and not up[ci] and e_in[ci] - 1 >= LATTICE_MIN:
                    w[o, ci, tap] = 0.5 if o % 4 < 2 else -0.5
        if last:
            b = tail_bias(key, cout)
        else:
            b = ((3 * np.arange(cout) + i + wset) % 5 - 2) / 8.0
            e_pre = np.full(cout, -3)
            for o, ci, tap in np.argwhere(w != 0):
                e_pre[o] = min(e_pre[o], e_in[ci] + int(np.log2(abs(w[o, ci, tap]))))
            sl = want.copy()
            sl[(sl == 1.25) & (e_pre - 2 < LATTICE_MIN)] = 2.0
            sl[(sl == 0.5) & (e_pre - 1 < LATTICE_MIN)] = 1.0
            if key == "1x" or wset != ALL_UP_SET:           # (the all-up set keeps every 2: its range stays doubled where need be)
                sl[(sl == 2.0) & (e_pre - 1 < LATTICE_MIN)] = 1.0
            S.append(sl)
            e_in = e_pre - 2 * (sl == 1.25) - (sl == 0.5)
            up = sl == 2.0
            assert e_in.min() >= LATTICE_MIN
        W.append((w.reshape(cout, cin, 3, 3), b))
    return W, S


def coverage(key):
    """-> (positions (convolution, input channel, tap) in all, those read in some set by a non-zero weight whose output channel
    reaches the net's output through non-zero weights of that set, output channels left empty in some set).  Reachability is
    computed on the graph of non-zeros, backwards from the last convolution (whose every channel is an output)."""
    _, convs, _ = net_shape(key)
    seen = [np.zeros((ci, 9), bool) for _, ci in convs]
    empty = 0
    for s in range(NSETS[key]):
        W, _ = design(key, s)
        live = np.ones(convs[-1][0], bool)
        for i in range(len(convs) - 1, -1, -1):
            nz = W[i][0].reshape(convs[i][0], convs[i][1], 9) != 0
            empty += int((~nz.any(axis=(1, 2))).sum())
            seen[i] |= nz[live].any(axis=0)
            live = nz[live].any(axis=(0, 2))             # the input channels a live output channel reads
    return sum(a.size for a in seen), sum(int(a.sum()) for a in seen), empty


# ---------------------------------------------------------------------------------------------------------------- the writer
def bin_walk(key, raw):
    """mutant_net.bin_layout's walk of the shipped .bin, extended to the weights: -> [(what, index, offset, count, flag)] with
    what = "weights" / "bias" (index: the convolution's) / "slopes" (the PReLU's)"""
    layers, convs, _ = net_shape(key)
    off, conv, prelu, out = 0, 0, 0, []
    for L in layers:
        if L["type"] == "Convolution":
            co, ci = convs[conv]
            n = co * ci * 9
            flag, = struct.unpack_from("<I", raw, off)
            assert flag in (FP16_FLAG, 0), (L["name"], hex(flag))
            out.append(("weights", conv, off + 4, n, flag))
            off += 4 + ((2 * n + 3) // 4 * 4 if flag == FP16_FLAG else 4 * n)
            out.append(("bias", conv, off, co, 0))
            off += 4 * co
            conv += 1
        elif L["type"] == "PReLU":
            n = int(L["kv"][0])
            out.append(("slopes", prelu, off, n, 0))
            off += 4 * n
            prelu += 1
    assert off == len(raw), ("the walk and the .bin disagree", off, len(raw))
    return out


def _arrays(key, raw):
    """the arrays of a .bin by the walk -> W, S as design() gives them"""
    W, S, w = [], [], None
    _, convs, _ = net_shape(key)
    for what, idx, off, n, flag in bin_walk(key, raw):
        if what == "weights":
            w = np.frombuffer(raw, "<f2" if flag == FP16_FLAG else "<f4", n, off).astype(np.float64).reshape(convs[idx][0], convs[idx][1], 3, 3)
        elif what == "bias":
            W.append((w, np.frombuffer(raw, "<f4", n, off).astype(np.float64)))
        else:
            S.append(np.frombuffer(raw, "<f4", n, off).astype(np.float64))
    return W, S


def write_probe_bin(key, dst, wset):
    """the complete .bin of design(key, wset) for the shipped .param of `key`; every array read back through the oracle's loader
    equals what was written, and the loader consumes the whole file"""
    from oracle import uvoracle
    param, src = model_paths(key)
    raw = bytearray(open(src, "rb").read())
    W, S = design(key, wset)
    for what, idx, off, n, flag in bin_walk(key, bytes(raw)):
        if what == "weights":
            a = W[idx][0].ravel().astype("<f2" if flag == FP16_FLAG else "<f4")
            assert np.array_equal(a.astype(np.float64), W[idx][0].ravel()) and _f16_exact(W[idx][0])
        else:
            a = (W[idx][1] if what == "bias" else S[idx]).astype("<f4")
            assert np.array_equal(a.astype(np.float64), W[idx][1] if what == "bias" else S[idx])
        assert a.size == n
        raw[off:off + a.nbytes] = a.tobytes()
    with open(dst, "wb") as f:
        f.write(bytes(raw))
    m = uvoracle.Model(param, dst)
    assert m.bin_consumed == m.bin_size == len(raw)
    assert m.num_conv == len(W)
    for i, (w, b) in enumerate(W):
        w1, b1, _ = m.conv(i)
        assert np.array_equal(w1.astype(np.float64), w) and np.array_equal(b1.astype(np.float64), b), (key, wset, "convolution", i)
    for i, s in enumerate(S):
        assert np.array_equal(m.prelu(i).astype(np.float64), s), (key, wset, "PReLU", i)
    return dst


# ---------------------------------------------------------------------------------------------------------------- inputs
def probe_input(h, w, seed):
    """float route: f32 [3][h][w] of k / 8, k = 0 .. 8"""
    return (np.random.default_rng(seed).integers(0, 9, (3, h, w)) / 8.0).astype(np.float32)


def probe_frame(h, w, seed, dtype=np.uint8):
    """a frame of samples 0 and 255 (u8) / 0 and 65535 (u16): exactly 0.0 and 1.0 on every route"""
    top = 255 if dtype == np.uint8 else 65535
    return (np.random.default_rng(seed).integers(0, 2, (h, w, 3)) * top).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------- the audit
F32 = np.float32
IN_SCALE = float(F32(1 / 255.0))                 # HeadArgs::in_scale: the double 1 / 255 rounded to fp32


def _f32_exact(a):
    return np.asarray(a, np.float64).astype(F32).astype(np.float64) == a


def head_scale_audit(a0, w, b, slopes, top):
    """csrc/uva_kernels.hip.h head_kernel / headp_kernel on a u8 / u16 frame: the MFMA's operand is the sample itself (u16:
    fp16(v / 257)), i.e. 0 or 255, and the fp32 accumulator takes `* in_scale + bias` -- contracted to one fma (headp_kernel:
    __builtin_elementwise_fma) or not (head_kernel: the compiler's choice) --, then the PReLU on floats (x, x * slope, med3) and
    one rounding to fp16.  255 * fl(1 / 255) is 1 + 5.9e-8, a hair below fp32's tie at 1 + 2^-24; 765 * fl(1 / 255) rounds to
    3 + 2^-22.  True if both forms round to the fp16 of the exact value everywhere."""
    acc = _conv64(a0 * 255.0, w, np.zeros_like(b), 3)                         # exact: integers below 2^24
    exact = _conv64(a0, w, b, 3)
    s3 = slopes[:, None, None]
    want = np.where(exact < 0, exact * s3, exact)
    b3 = b[:, None, None]
    ok = True
    for x in ((acc * IN_SCALE).astype(F32).astype(np.float64) + b3, acc * IN_SCALE + b3):      # two roundings / one
        x = x.astype(F32)
        t = (x.astype(np.float64) * s3).astype(F32)
        v = np.where(x < 0, t, x)
        with np.errstate(over="ignore"):
            ok = ok and bool(np.array_equal(v.astype(np.float16).astype(np.float64), want))
    return ok and _f16_exact(want)


def epilogue_audit(conv, bias, res, top):
    """the tails' `((acc + b) + res) * 255` (tail_kernel, tail4_kernel, sub10_kernel; `* 65535` on the 16-bit route) in fp32,
    with res = sample * norm (u16: (v / 257) * norm), norm = fl(1 / 255), on frames of samples 0 and top.  The sample's factor
    is 0 or 255, and 255 * norm is 1 + 5.9e-8: rounded on its own it is 1.0, contracted into the sum -- fma(255, norm, acc + b),
    what hipcc's default -ffp-contract makes of tail_kernel's and tail4_kernel's line -- it moves a sum in [0.25, 1) up by
    2^-24, 0.0039 code at 16 bits.  Both forms are evaluated here in fp32.
    -> (samples, samples whose exact value lies within 0.05 of a half-integer where rounding decides the result, samples for
    which either form's code differs from the exact value's, exact ties).

    The bound: each of the three operations rounds at most once, relative error 2^-24 each, so the fp32 product is off by at
    most 3 * 2^-24 * top * |y| = 0.0117 code at y = 1 on the 16-bit route (top = 65535) and 4.6e-5 on the 8-bit one -- below
    0.025, half of 0.05: a sample further than 0.05 from a half-integer rounds as its exact value does whatever fp32 did.  That
    margin cannot be had for every sample -- with 255 y = 256 y - y a value on a lattice of 2^-7 is within 0.05 of a
    half-integer whenever y is within 0.05 of 0.5, a tenth of the range, and no linear last layer takes activations of 8 bits
    to a coarser lattice inside [0, 1] --, so the audit asks for what the margin was to guarantee, sample by sample: the code
    of BOTH fp32 forms equals the exact value's.  On the 8-bit routes that holds on any of the probes' lattices: every fp32
    operation of the uncontracted form is exact, ties included (the only tie in range is y = 0.5, the even code is the one
    above: both forms round up), and the contracted form's 2^-24 is 1.5e-5 code.  On the 16-bit route it holds where y is a
    multiple of 2^-7 (the SHALLOW sets): the values nearest a half-integer are 1 / 128 code away and 0.0039 moves none across.
    At 2^-8 it does not: y = 129 / 256 is 65535 y = 33023.496, the contracted sum gives 33023.5 and the even code 33024 --
    what tail_kernel and tail4_kernel returned on 0.1 % of the samples of such a set."""
    s1 = (conv + bias).astype(F32)
    assert np.array_equal(s1.astype(np.float64), conv + bias)                # (acc + b: the accumulation's own lattice)
    src = res * 255.0
    r1 = (src * IN_SCALE).astype(F32).astype(np.float64)
    plain = ((s1.astype(np.float64) + r1).astype(F32).astype(np.float64) * top).astype(F32)
    fused = ((s1.astype(np.float64) + src * IN_SCALE).astype(F32).astype(np.float64) * top).astype(F32)
    v = (conv + bias + res) * top
    code = lambda a: np.clip(np.rint(a), 0, top)                             # noqa: E731
    wrong = (code(plain) != code(v)) | (code(fused) != code(v))
    decides = (v > -0.45) & (v < top + 0.45)           # outside, every value within the error bound clamps to the same end
    near = (np.abs(v - np.floor(v) - 0.5) < 0.05) & decides
    return int(v.size), int(near.sum()), int(wrong.sum()), int(((v - np.floor(v) == 0.5) & decides).sum())


# ---------------------------------------------------------------------------------------------------------------- reference
MUTANTS = ("mirror_x", "swap_cin", "wino_row", "clamp_slope", "tail_swap", "seam_col", "border_row", "lost_carry_rows")


def tail_swap_channels(n):
    """the two tail channels whose biases are nearest (stress_net.swapped_channels)"""
    pi = list(ramp_pi(n))
    return pi.index(n // 2), pi.index(n // 2 - 1)


class Ref:
    """float64 forward of (shipped .param of key, bin).  mutant: dict(kind=one of MUTANTS, layer=convolution index, ...):
        mirror_x     convolution `layer` has its taps mirrored in x
        swap_cin     ... reads input channel c ^ 1 where it should read c
        wino_row     ... evaluated as F(2,3) with filter row `row`'s third transformed weight (g0 + g1 + g2) / 2 for
                     (g0 - g1 + g2) / 2; output pairs start at column -1 (odd layers, the first of a launch) or 0
        clamp_slope  the PReLU behind convolution `layer` has its slopes above 1 clamped to 1
        tail_swap    two output channels of the last convolution exchanged (the two whose biases are nearest)
        seam_col     convolution `layer` computes output column `col` with input column col - 1 read from col - 2
        border_row   (tiled route) plane `plane`'s innermost top border row is zero: the padding instead of the neighbour
        lost_carry_rows  (tiled route) in plane `plane`, convolution `layer` (the first of a trunkw launch: its result is the
                     launch's intermediate) has rows r0 - 1 and r0 zero over columns x0 .. x0 + width - 1: the two
                     intermediate rows a segment whose first output row is r0 needs from above its first full block, i.e.
                     what its first step must bring (a fill step's two valid rows, a six-row start's first two) -- lost
                     where a segment starts on the state the previous one left in the rings.  tests/schedule_census.py
                     carry_starts() gives (plane, x0, r0, width)"""

    def __init__(self, key, bin_path):
        self.key = key
        self.layers, self.convs, self.scale = net_shape(key)
        self.W, self.S = _arrays(key, open(bin_path, "rb").read())
        self.wino = key != "1x"                 # the 64 -> 64 layers run as Winograd F(2,3) in trunkw_kernel

    def forward(self, x, taps=None, audit=None, mutant=None, frame_top=None):
        """x [3][h][w] -> float64 [3][h s][w s]; taps: a list that receives every convolution's result (behind its PReLU);
        frame_top 255 / 65535: x came from a u8 / u16 frame (the head's and the tails' frame arithmetic is audited as well)"""
        mu = mutant or {}
        blobs = {}
        conv = 0
        last = len(self.convs) - 1
        for k, L in enumerate(self.layers):
            t, ins, outs, kv = L["type"], L["ins"], L["outs"], L["kv"]
            if t == "Input":
                y = np.asarray(x, np.float64)
                if audit is not None:
                    audit.blob("input", y)
            elif t == "Split":
                for o in outs:
                    blobs[o] = blobs[ins[0]]
                continue
            elif t == "Convolution":
                a, (w, b) = blobs[ins[0]], self.W[conv]
                at = mu.get("layer") == conv
                if at and mu["kind"] == "mirror_x":
                    w = w[:, :, :, ::-1]
                if at and mu["kind"] == "swap_cin":
                    w = w[:, np.arange(w.shape[1]) ^ 1]
                y = _conv64(a, w, b, 3)
                if at and mu["kind"] == "seam_col" and 2 <= mu["col"] < a.shape[2]:
                    a2 = a.copy()
                    a2[:, :, mu["col"] - 1] = a[:, :, mu["col"] - 2]
                    y[:, :, mu["col"]] = _conv64(a2, w, b, 3)[:, :, mu["col"]]
                if at and mu["kind"] == "wino_row":
                    # U2 = U1 adds sum g1 (d2 - d1) to a pair's first column and takes it from the second
                    g1 = np.zeros_like(w)
                    g1[:, :, mu["row"], 1] = w[:, :, mu["row"], 1]
                    e = _conv64(a, g1, np.zeros_like(b), 3)                   # e[x] = sum g1 * in[row, x]
                    ep = np.zeros(e.shape[:2] + (e.shape[2] + 3,))
                    ep[:, :, 1:-2] = e                                        # ep[x + 1] = e[x]
                    for xa in range(-1 if conv % 2 else 0, e.shape[2], 2):
                        d = ep[:, :, xa + 2] - ep[:, :, xa + 1]
                        if xa >= 0:
                            y[:, :, xa] += d
                        if xa + 1 < e.shape[2]:
                            y[:, :, xa + 1] -= d
                if at and mu["kind"] == "tail_swap":
                    i, j = tail_swap_channels(y.shape[0])
                    y[[i, j]] = y[[j, i]]
                if audit is not None:
                    name = "conv %d" % conv
                    gw, ga, gb = _low_bit(w), _low_bit(a), _low_bit(b)
                    gexp = None if gw is None or ga is None else gw + ga
                    if gb is not None:
                        gexp = gb if gexp is None else min(gexp, gb)
                    audit.terms(name, gexp, float(_conv64(np.abs(a), np.abs(w), np.abs(b), 3).max()))
                    if self.wino and 1 <= conv < last:
                        audit.winograd(name, wino_audit(a, w, b))
                    if conv < last:
                        audit.blob(name + " sum", y)                # (sub10_store and TW_ACT_F16 round the sum to fp16 first)
                    if conv == 0 and frame_top:
                        audit.head = getattr(audit, "head", True) and head_scale_audit(a, w, b, self.S[0], frame_top)
                if conv < last:
                    s = self.S[conv]
                    if at and mu["kind"] == "clamp_slope":
                        s = np.minimum(s, 1.0)
                    y = np.where(y < 0, y * s[:, None, None], y)
                    if at and mu["kind"] == "lost_carry_rows":
                        y[:, max(mu["r0"] - 1, 0):mu["r0"] + 1, mu["x0"]:mu["x0"] + mu["width"]] = 0
                    if audit is not None:
                        audit.blob("conv %d" % conv, y)
                        audit.slopes = getattr(audit, "slopes", True) and _f16_exact(s)
                elif audit is not None and frame_top:
                    res = np.repeat(np.repeat(blobs["input"], self.scale, 1), self.scale, 2)
                    f = self.scale
                    sh = np.zeros_like(res)
                    for ch in range(y.shape[0]):
                        sh[ch // (f * f), (ch // f) % f::f, ch % f::f] = y[ch] - b[ch]
                    bb = np.zeros_like(res)
                    for ch in range(y.shape[0]):
                        bb[ch // (f * f), (ch // f) % f::f, ch % f::f] = b[ch]
                    e = epilogue_audit(sh, bb, res, float(frame_top))
                    audit.epilogue = tuple(p + q for p, q in zip(getattr(audit, "epilogue", (0, 0, 0, 0)), e))
                if taps is not None:
                    taps.append(y)
                conv += 1
            elif t == "PReLU":
                blobs[outs[0]] = blobs[ins[0]]            # (applied with its convolution above: the kernels' fusion, and the taps')
                continue
            elif t == "PixelShuffle":
                f = int(kv.get(0, 1))
                a = blobs[ins[0]]
                c, h, w_ = a.shape
                y = np.zeros((c // (f * f), h * f, w_ * f))
                for ch in range(c):                       # input channel (o f + i) f + j -> output o at (y f + i, x f + j)
                    y[ch // (f * f), (ch // f) % f::f, ch % f::f] = a[ch]
            elif t == "Interp":
                f = int(float(kv.get(1, 1.0)))
                assert int(kv.get(0, 1)) == 1
                y = np.repeat(np.repeat(blobs[ins[0]], f, axis=1), f, axis=2)
            elif t == "BinaryOp":
                y = blobs[ins[0]] + blobs[ins[1]]
            else:
                raise ValueError("layer type " + t)
            blobs[outs[0]] = y
        return blobs["output"]

    def frame_values(self, img, **kw):
        """u8 / u16 HWC frame -> float64 HWC top * result (before rounding): normalise, forward, scale"""
        top = 255 if img.dtype == np.uint8 else 65535
        x = img.transpose(2, 0, 1).astype(np.float64) / top
        return self.forward(x, frame_top=top, **kw).transpose(1, 2, 0) * top

    def tiled_values(self, img, ts, border=10, mutant=None, **kw):
        """upscale_image's windows (upscale_processing.tile_window), every tile a plane of its own, cores pasted"""
        from upscale_video_amd import upscale_processing as up
        h, w, _ = img.shape
        s = self.scale
        out = np.zeros((s * h, s * w, 3))
        mu = mutant or {}
        k = 0
        for ty in range(-(-h // ts)):
            for tx in range(-(-w // ts)):
                (y0, y1, x0, x1), (top, bottom, left, right) = up.tile_window(ts, ty, tx, h, w, border)
                tile = np.ascontiguousarray(img[y0 - top:y1 + bottom, x0 - left:x1 + right])
                if mu.get("kind") == "border_row" and mu["plane"] == k and top:
                    tile = tile.copy()
                    tile[top - 1] = 0
                here = mu.get("kind") != "border_row" and (mu.get("kind") != "lost_carry_rows" or mu["plane"] == k)
                v = self.frame_values(tile, mutant=mutant if here else None, **kw)
                out[s * y0:s * y1, s * x0:s * x1] = v[s * top:s * (top + y1 - y0), s * left:s * (left + x1 - x0)]
                k += 1
        return out


def to_codes(v, dtype=np.uint8):
    """clamp(rint_half_even(v)) -> u8 / u16"""
    return np.clip(np.rint(v), 0, 255 if dtype == np.uint8 else 65535).astype(dtype)


def first_difference(got, want):
    """-> (index of the first differing element, got there, want there) or None"""
    d = np.argwhere(np.asarray(got) != np.asarray(want))
    if not len(d):
        return None
    i = tuple(int(v) for v in d[0])
    return i, float(np.asarray(got)[i]), float(np.asarray(want)[i])
