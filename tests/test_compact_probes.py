"""The kernels the product ships on -- headp_kernel / head_kernel, trunkw_kernel<64>, trunk2_kernel, trunk_kernel, tail_kernel,
tail4_kernel, sub10_kernel, sub10_kernel16, sub5_kernel, pair24_kernel -- and the host code that packs their weights, against a
float64 reference BIT FOR BIT, on the shipped .param files with probe .bin files whose arithmetic is exact
(tests/compact_probe.py).  Every other comparison of these kernels with an independent reference is statistical (1 LSB on 5-8 %
of the samples, 2 LSB and 50 dB), every byte-exact one compares a kernel with another build of itself, and every net they have
run on carries the shipped convolution weights: two taps exchanged in one trunk layer, a wrong sign in one Winograd weight row,
a tail weight on the neighbouring pixel-shuffle channel or a seam column read one to the side sit inside all of that.

CPU (unmarked): the writer's self-check; the coverage (every (convolution, input channel, tap) read by a weight that reaches the
output: 100 %); the audit that licenses array_equal for every (net, weight set, frame) the GPU part uses; Ref == the oracle in fp32
== the oracle's product modes, bit for bit, on the float route (output and every tap) and on the u8 route whole and tiled, for every
probe; every mutant of the reference (one plausible slip each) differing from it; the clamp share of the u8 frames.

GPU (-m gpu): every route and switch against Ref with np.array_equal.  CASES lists them; kernel_table() says which kernel each
reaches and how many of the shipped workloads' schedule classes (tests/schedule_census.py) its cases visit."""
import os

import numpy as np
import pytest

import compact_probe as cp
import parity_report as pr
import schedule_census as sc
from generic_probe import Audit
from mutant_net import model_paths
from oracle import uvoracle

REF = "float64 reference (compact_probe.Ref)"
SETS = tuple(range(8))                           # the 2x / 4x sets
SETS_1X = tuple(range(cp.NSETS["1x"]))
# 2x / 4x.  37 x 70: 5 tile rows, 3 tile columns, ragged both ways, three trunkw strips; the small ones: one pixel, one tile, two
FLOAT_SHAPES = {0: (37, 70), 1: (1, 1), 2: (37, 70), 3: (37, 70), 4: (8, 32), 5: (37, 70), 6: (16, 64), 7: (37, 70)}
WHOLE = (37, 70)
# frames of 2T x 2T with tile T and border 10: four planes of (T + 10)^2 -- T = 32: a folded last strip of 12 columns, 34: an
# unfolded one of 14, 33: one of 13
TILES = {0: 32, 1: 33, 2: 34, 3: 32, 4: 33, 5: 34, 6: 32, 7: 34}
SWITCHES = (("UVA_TRUNK_WINO", (4, 0, 6)), ("UVA_TRUNK_FUSION", (4, 5)), ("UVA_TW_ACT16", (4, 1, 7)), ("UVA_TW_FOLD", (0, 6)),
            ("UVA_TW_CARRY", (4, 0, 2)), ("UVA_HEAD_PERSIST", (0, 3)))
U16_SETS = {0: cp.SHALLOW, 64: cp.SHALLOW}              # tile -> sets; whole 37 x 70, tiled 70 x 75 with tile 64
U16_TILED = (70, 75)
# 1x.  50 x 33 and 3 x 2: one strip; 37 x 121 and 130 x 216: more than one strip pair
SHAPES_1X = {0: (50, 33), 1: (37, 121), 2: (130, 216), 3: (3, 2), 4: (50, 33), 5: (37, 121), 6: (50, 33), 7: (130, 216)}
SWITCHES_1X = (("UVA_SUB5", "1", (2, 5, 6)), ("UVA_SUB10", "0", (2, 4, 8)))
BATCH_1X = (1, 37, 121)                          # set, h, w: three different frames in one call
U16_1X = cp.SHALLOW                             # (the 16-bit route takes the sets whose output lies on 2^-7: epilogue_audit)
# The frames above give a workgroup a list of at most 4 steps (1x: 24 rows) -- no lap of a ring, no second segment in a list.
# CENSUS_* are the frames that visit the states the shipped workloads' lists reach (schedule_census: the coverage test below),
# chosen by greedy cover over the census for the fewest pixels -- the float64 audit costs ~145 us a pixel on the 64-feature
# nets --, which is why they are NARROW: a strip costs a step whatever its width, a 256-workgroup launch needs ~3000 steps
# for lists of 12, and 61 columns are a first, an interior and a one-column last strip.  (h, w, tile), border 10:
#   3841 x 61 / 120   33 planes of 61 columns: lists of >= 12 steps, three segments per list, six-row and fill starts in the middle
#                     of a plane at every phase of the rings, folded one-column last strips, no idle workgroup
#   4508 x 31 / 300   lists of 8 steps on full and on folded strips: the phases of fill starts and of stores that the first
#                     leaves open, above all for the kernels that only run its default lists (UVA_TW_CARRY=0, UVA_TW_ACT16=0)
#   1696 x 45 / 100   a last strip of 15 columns, too wide to fold and (trunk2_kernel) to be narrow: ragged single stores at
#                     every phase
#   760 x 12 / 250    planes of ONE folded strip (lists of 4 steps): folded starts at a plane's top, a folded store phase
CENSUS_TILED = ((3841, 61, 120), (4508, 31, 300), (1696, 45, 100), (760, 12, 250))
CENSUS_SETS = (cp.ALL_UP_SET, 6)                # u8; the all-up set's sign carry between launches meets long lists here
CENSUS_U16 = 1                                  # a cp.SHALLOW set
# The float route is whole-frame (one plane, its own lists): the two smallest census frames with every layer's tap -- 1696 x 45
# whole has 242 segments that start in the middle of the plane; the 17 float64 taps of 64 channels are 0.66 GB for it and
# would be 1.2 / 2 GB for the two larger frames
CENSUS_F32 = {"2x": 2, "4x": 3}
CENSUS_SWITCHES = ("UVA_TW_CARRY", "UVA_TW_ACT16", "UVA_TRUNK_WINO", "UVA_TRUNK_FUSION")      # other kernels: every census frame
PLANNER_SWITCHES = (("UVA_TW_FOLD", "0"), ("UVA_TW_SIX", "1"), ("UVA_TW_SIX", "0"))             # other lists, the same kernel
SMALL_SWITCH_FRAMES = (("UVA_TRUNK_WINO", 38, 50), ("UVA_TRUNK_FUSION", 16, 64))   # a wide ragged last strip; full tile columns
# 1x.  4328 x 120: two full 60-column strips, lists of ~90 rows with two segments, segments of more than S10_RES_ROWS = 32 written
# rows, no idle workgroup; 40 x 230: a first, an interior and a last strip pair for sub5_kernel; 16 x 64: pair24_kernel's full
# tiles; four frames of 4500 x 61 in one call: lists of >= 160 rows that cross from one frame into the next (--batch 4: 560)
CENSUS_1X = (4328, 120)
CENSUS_1X_SMALL = ((40, 230), (16, 64))
CENSUS_1X_SETS = {"u8": 2, "UVA_SUB5": 5, "UVA_SUB10": 4}
LONG_BATCH_1X = (1, 4500, 61, 4)                # set, h, w, frames


class Case:
    """one GPU run and its reference: net, weight set, route ("f32", "u8", "u16", "batch", "batch4"), frame, tile, switch"""

    def __init__(self, key, wset, route, h, w, tile=0, env=None):
        self.key, self.wset, self.route, self.h, self.w, self.tile, self.env = key, wset, route, h, w, tile, env
        self.frames = {"batch": 3, "batch4": 4}.get(route, 1)
        self.id = "%s-w%d-%s-%dx%d-t%d%s" % (key, wset, route, h, w, tile, "-%s=%s" % env if env else "")
        self.frame_key = (key, wset, route, h, w, tile)              # (what the reference depends on: a switch changes nothing)


def _cases():
    out = []
    for key in ("2x", "4x"):
        out += [Case(key, s, "f32", *FLOAT_SHAPES[s]) for s in SETS]
        out += [Case(key, s, "u8", *WHOLE) for s in SETS]
        out += [Case(key, s, "u8", 2 * TILES[s], 2 * TILES[s], TILES[s]) for s in SETS]
        out += [Case(key, 2 * k + 1, "u8", h, w) for k, (h, w) in enumerate(((1, 1), (8, 32), (16, 64)))]
        for name, sets in SWITCHES:
            for s in sets:
                out += [Case(key, s, "u8", *WHOLE, env=(name, "0")), Case(key, s, "u8", 2 * TILES[s], 2 * TILES[s], TILES[s], env=(name, "0"))]
        out += [Case(key, s, "u16", *(WHOLE if t == 0 else U16_TILED), tile=t) for t, sets in U16_SETS.items() for s in sets]
    out += [Case("1x", s, "f32", *SHAPES_1X[(s + 3) % 8]) for s in SETS_1X]
    out += [Case("1x", s, "u8", *SHAPES_1X[s % 8]) for s in SETS_1X]
    out += [Case("1x", s, "u8", *hw, env=(name, val)) for name, val, sets in SWITCHES_1X for s in sets for hw in ((50, 33), (130, 216))]
    out += [Case("1x", BATCH_1X[0], "batch", *BATCH_1X[1:])]
    out += [Case("1x", s, "u16", *hw) for s in U16_1X for hw in ((50, 33), (37, 121))]
    return out + _census_cases()


def _census_cases():
    out = []
    for key in ("2x", "4x"):
        for h, w, t in CENSUS_TILED:
            out += [Case(key, s, "u8", h, w, t) for s in CENSUS_SETS] + [Case(key, CENSUS_U16, "u16", h, w, t)]
            out += [Case(key, cp.ALL_UP_SET, "u8", h, w, t, env=(name, "0")) for name in CENSUS_SWITCHES]
        h, w, t = CENSUS_TILED[0]
        out += [Case(key, cp.ALL_UP_SET, "u8", h, w, t, env=env) for env in PLANNER_SWITCHES]
        out += [Case(key, CENSUS_F32[key], "f32", h, w) for h, w, _ in CENSUS_TILED[-2:]]
        out += [Case(key, 5 if (h, w) == (16, 64) else 0, "u8", h, w, env=(name, "0")) for name, h, w in SMALL_SWITCH_FRAMES]
    out += [Case("1x", CENSUS_1X_SETS["u8"], "u8", *CENSUS_1X), Case("1x", U16_1X[0], "u16", *CENSUS_1X)]
    for hw in (CENSUS_1X,) + CENSUS_1X_SMALL:
        out += [Case("1x", CENSUS_1X_SETS[name], "u8", *hw, env=(name, val)) for name, val, _ in SWITCHES_1X]
    out += [Case("1x", LONG_BATCH_1X[0], "batch4", *LONG_BATCH_1X[1:3])]
    return out


CASES = _cases()


def kernel_table(uva):
    """which case reaches which kernel, from the census (it cannot go stale): 2x tail_kernel / 4x tail4_kernel and headp_kernel
    on every frame case of that net (head_kernel: UVA_HEAD_PERSIST=0), pair24_kernel also on the 1x float route; per trunk /
    1x kernel group the cases that run it and the classes of the workloads' lists they visit
    -> [(kernel, cases, classes reached, {workload: its classes}, text)]"""
    rows = []
    for kernel in sc.TRUNK_KERNELS + sc.ROW_KERNELS:
        cases = [c for c in CASES if c.route != "f32" and sc.kernel_of(c.key, c.route, c.env)[0] == kernel]
        have = _reached(uva, cases)
        want = {name: w for name, w in ((name, sc.workload_census(uva, name, kernel)) for name in sc.WORKLOADS) if w is not None}
        every = set().union(*want.values())
        rows.append((kernel, cases, have, want, "%-30s %3d cases, %3d classes visited, %3d of the workloads' %3d" %
                     (kernel, len(cases), len(have), len(have & every), len(every))))
    return rows


def _reached(uva, cases):
    """the union of the census over the geometries (and planner switches) of `cases`, which all run one kernel group"""
    out = set()
    for kernel, planner, h, w, tile, frames in sorted({sc.kernel_of(c.key, c.route, c.env) + (c.h, c.w, c.tile, c.frames) for c in cases}):
        out |= sc.census(uva, kernel, h, w, tile, 10 if tile else 0, frames, planner)
    return out


class Probes:
    """the probes' files, references, values and audits, made on first use and shared by every test of the module"""

    def __init__(self, directory):
        self.dir, self.refs, self.done = str(directory), {}, {}

    def bin(self, key, wset):
        self.ref(key, wset)
        return os.path.join(self.dir, "%s_w%d.bin" % (key, wset))

    def ref(self, key, wset):
        if (key, wset) not in self.refs:
            self.refs[key, wset] = cp.Ref(key, cp.write_probe_bin(key, os.path.join(self.dir, "%s_w%d.bin" % (key, wset)), wset))
        return self.refs[key, wset]

    def input(self, c, k=0):
        seed = 1000 * c.h + c.w + 7 * c.wset + 100003 * k
        if c.route == "f32":
            return cp.probe_input(c.h, c.w, seed)
        return cp.probe_frame(c.h, c.w, seed, np.uint16 if c.route == "u16" else np.uint8)

    def want(self, c, k=0):
        """-> (reference, taps, audit).  f32: float64 [3][sh][sw] and every convolution's activation; frames: float64 [sh][sw][3],
        top * result before rounding.  Shared, never written to."""
        key = c.frame_key + (k,)
        if key not in self.done:
            r, x, a, taps = self.ref(c.key, c.wset), self.input(c, k), Audit(), []
            if c.route == "f32":
                v = r.forward(x, taps=taps, audit=a)
            elif c.tile:
                v = r.tiled_values(x, c.tile, audit=a)
            else:
                v = r.frame_values(x, audit=a)
            v.setflags(write=False)
            self.done[key] = (v, taps, a)
        return self.done[key]


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    return Probes(tmp_path_factory.mktemp("compact_probes"))


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if c.frame_key not in seen:
            seen.add(c.frame_key)
            out.append(c)
    return out


# ------------------------------------------------------------------------------------------------------------------- CPU
def test_the_writer_checks_itself_and_keeps_the_shipped_layout(probes):
    """write_probe_bin reads every array back through the oracle's loader (bin_consumed == bin_size, every array equal to what
    was written); here: every set of every net is written, the file has the shipped one's length and storage flags, and no two
    sets of a net are the same file"""
    for key in cp.KEYS:
        shipped = open(model_paths(key)[1], "rb").read()
        files = [open(probes.bin(key, s), "rb").read() for s in range(cp.NSETS[key])]
        assert len(set(files)) == cp.NSETS[key] and all(len(f) == len(shipped) for f in files)
        for f in files:
            assert [(e[0], e[1], e[2], e[4]) for e in cp.bin_walk(key, f)] == [(e[0], e[1], e[2], e[4]) for e in cp.bin_walk(key, shipped)]


@pytest.mark.parametrize("key", cp.KEYS)
def test_every_position_is_read_by_a_weight_that_reaches_the_output(key):
    total, reached, empty = cp.coverage(key)
    print(f"{key}: {reached} of {total} (convolution, input channel, tap) read and reaching = {100.0 * reached / total:.1f} %, "
          f"{empty} empty output channels, {cp.NSETS[key]} sets")
    assert reached == total and empty == 0
    # the excursions land where they must: over the sets every PReLU is inside a window, with a slope above 1 on it
    _, convs, _ = cp.net_shape(key)
    up = [set() for _ in range(len(convs) - 1)]
    for s in range(cp.NSETS[key]):
        _, S = cp.design(key, s)
        assert sum((a > 1).any() or (a == 1).any() or (a == 0.5).any() for a in S) == len(cp.WINDOWS[key][s]) <= 3
        for i in cp.WINDOWS[key][s]:
            up[i] |= set(S[i][S[i] > 0])
    assert all(u & {2.0, 1.25} for u in up), up
    for i in ([0, len(up) - 1] + ([4, 5] if key == "1x" else [7, 8])):
        assert 1.0 in up[i] and 2.0 in up[i], (key, i, up[i])
    if key != "1x":
        _, S = cp.design(key, cp.ALL_UP_SET)
        assert cp.WINDOWS[key][cp.ALL_UP_SET] == (9, 10)                  # (one trunkw launch: layers 2k - 1 and 2k)
        assert (S[9] > 1).all() and (S[10] > 1).all() and {1.25, 2.0} <= set(S[9])
    _, S = cp.design(key, 7 if key != "1x" else 4)
    assert (S[-1] > 1).any()                                   # the last PReLU in front of the tail


@pytest.mark.parametrize("key", cp.KEYS)
def test_exactness_audit(probes, key):
    """What licenses array_equal on the GPU, for every (net, weight set, frame) the GPU part uses: every stored activation (and
    every sum in front of its PReLU: sub10_store and TW_ACT_F16 round it first) an fp16 value, every Winograd-transformed input
    and weight too, every accumulation order-independent, the head's in_scale harmless, the tails' epilogue exact or clear of a
    tie (compact_probe.epilogue_audit), the clamp share of the u8 frames at most 60 % with unclamped samples on every tail
    channel."""
    n_layers = len(cp.net_shape(key)[1]) - 1
    worst = np.zeros(n_layers)
    cases = _unique([c for c in CASES if c.key == key])
    clamp_worst, near_all, ties_all = 0.0, 0, 0
    for c in cases:
        for k in range(c.frames):
            v, _, a = probes.want(c, k)
            assert a.bad() == [], (c.id, a.bad())
            assert a.slopes is True
            bits = [a.blobs["conv %d" % i][1] for i in range(n_layers)]
            sums = [a.blobs["conv %d sum" % i][1] for i in range(n_layers)]
            # (generic_probe.Audit's figure is log2(max |v| / lattice) + 1: the largest value's bit count is its floor)
            worst = np.maximum(worst, np.floor(np.maximum(bits, sums)))
            if key != "1x":
                assert all(a.wino["conv %d" % i] for i in range(1, n_layers)), c.id
            if c.route != "f32":
                assert a.head is True, c.id
                n, near, wrong, ties = a.epilogue
                # the bound is epilogue_audit's: the fp32 epilogue is off by < 0.025 code, half the margin of 0.05 -- which
                # cannot be had for every sample (there: why), so every sample is asked directly: the fp32 epilogue's code,
                # with the residual's product contracted into the sum or not, is the exact value's
                assert wrong == 0, (c.id, a.epilogue)
                near_all, ties_all = near_all + near, ties_all + ties
                top = 65535 if c.route == "u16" else 255
                f = cp.net_shape(key)[2]
                clamp = float(((v <= 0) | (v >= top)).mean())
                if c.h * c.w >= 256:                   # (a frame of one or six pixels has no share to speak of)
                    clamp_worst = max(clamp_worst, clamp)
                    assert clamp <= 0.60, (c.id, clamp)
                    for i in range(f):
                        for j in range(f):
                            sub = v[i::f, j::f]
                            assert (((sub > 0) & (sub < top)).sum(axis=(0, 1)) > 0).all(), (c.id, "a tail channel without an unclamped sample", i, j)
                    assert len(np.unique(cp.to_codes(v, np.uint16 if top > 255 else np.uint8))) >= 16
    print(f"{key}: {len(cases)} frames audited; worst significant bits per layer " + " ".join("%d" % b for b in worst) +
          f"; worst clamp share {100 * clamp_worst:.1f} %; {near_all} samples within 0.05 of a half-integer, {ties_all} exact ties, "
          "every one with the exact value's code in fp32 either way")
    assert worst.max() <= 11 and (key == "1x" or worst[:-1].max() <= 10)          # (in front of a Winograd layer: 10)


def test_bit_exact_cases_reach_every_schedule_class_of_the_workloads(uva):
    """Every state of a strip-walking kernel that a shipped workload's lists reach (tests/schedule_census.py: ring phase of a
    segment start and of a store, kind of start, rows stored, list length, segments per list, ...) is reached by a case that is
    held to the float64 reference bit for bit -- per kernel group, because a switch that selects another kernel (or another
    instantiation of one) has lists and states of its own; UVA_TW_FOLD / UVA_TW_SIX only give the default kernel other lists.
    The classes are the issue's: a segment start is (kind, top of plane or not, list index mod 5, folded or not, rmask), a store
    (list index mod 5, folded or not, rows, full or ragged columns); the union is taken over every case of the group.
    There is no allow-list.  One bucket is wider than a first count would make it, because the class cannot be reached below a
    frame size whose float64 audit takes minutes (a 256-workgroup launch, ~145 us of audit per pixel): trunk_kernel's turns
    per workgroup are 1 and >= 2, not "a lap of its 5 slots" -- 6 turns are 3072 tiles of 4 x 32 pixels, 0.39 M pixels."""
    missing = []
    for kernel, cases, have, want, text in kernel_table(uva):
        print(text)
        assert cases, kernel
        for name, classes in want.items():
            missing += [(kernel, name, cls) for cls in sorted(classes - have, key=str)]
    assert not missing, "%d schedule classes of the workloads reached by no bit-exact case:\n%s" % (
        len(missing), "\n".join("  %-32s %-20s %s" % m for m in missing))


TAP_SHAPE = (9, 35)


@pytest.mark.parametrize("key", cp.KEYS)
def test_the_reference_is_the_oracle_in_every_mode(probes, key):
    """Ref (float64, a loop over the non-zero weights, its own reader of the .bin) == uvoracle.Model in fp32 == the oracle's
    product modes (fp16 storage, Winograd F(2,3) with fp16 transforms, PReLU on halves), bit for bit: the float route's output
    and every tap, the u8 route whole and tiled, for every probe"""
    uvoracle.build()
    modes = (0, uvoracle.product_flags("f32"), uvoracle.product_flags())
    assert modes[2] & uvoracle.WINOGRAD_F23 and modes[2] & uvoracle.PRELU_F16
    param = model_paths(key)[0]
    for s in range(cp.NSETS[key]):
        om = uvoracle.Model(param, probes.bin(key, s))
        r = probes.ref(key, s)
        cs = [c for c in _unique(CASES) if c.key == key and c.wset == s]
        c = [c for c in cs if c.route == "f32"][0]
        want, _, _ = probes.want(c)
        x = probes.input(c)
        for flags in modes:
            got = om.forward(x, flags=flags).astype(np.float64)
            assert np.array_equal(got, want), (key, s, flags, cp.first_difference(got, want))
        xt = cp.probe_input(*TAP_SHAPE, seed=50 + s)
        taps = []
        r.forward(xt, taps=taps)
        for flags in modes:
            for idx in range(om.num_conv - 1):
                got = om.tap(xt, idx, flags=flags).astype(np.float64)
                assert np.array_equal(got, taps[idx]), (key, s, flags, "conv", idx, cp.first_difference(got, taps[idx]))
        whole = max((c for c in cs if c.route == "u8" and c.tile == 0), key=lambda c: c.h * c.w)
        img = probes.input(whole)
        for flags in (0, modes[2]):
            got, w8 = om.apply_model(img, flags=flags), cp.to_codes(probes.want(whole)[0])
            assert np.array_equal(got, w8), (key, s, flags, "whole", cp.first_difference(got, w8))
        if key != "1x":
            tiled = [c for c in cs if c.route == "u8" and c.tile][0]
            img = probes.input(tiled)
            for flags in (0, modes[2]):
                got, w8 = om.upscale_image(img, tile_size=tiled.tile, border=10, flags=flags), cp.to_codes(probes.want(tiled)[0])
                assert np.array_equal(got, w8), (key, s, flags, "tiled", cp.first_difference(got, w8))


def _mutants(key):
    n_conv = len(cp.net_shape(key)[1])
    out = [dict(kind="mirror_x", layer=5), dict(kind="swap_cin", layer=6), dict(kind="swap_cin", layer=n_conv - 1),
           dict(kind="clamp_slope", layer=None), dict(kind="tail_swap", layer=n_conv - 1), dict(kind="border_row", plane=2)]
    if key != "1x":
        out += [dict(kind="wino_row", layer=7, row=1), dict(kind="wino_row", layer=8, row=0), dict(kind="wino_row", layer=8, row=2),
                dict(kind="seam_col", layer=8, col=cp.STRIP), dict(kind="seam_col", layer=3, col=2 * cp.STRIP),
                dict(kind="lost_carry_rows", layer=7)]
    return out


def _old_geometries():
    """the 2x / 4x frame cases from before the census frames, each with the planner switch it runs under"""
    new = {(h, w, t) for h, w, t in CENSUS_TILED}
    return sorted({(c.h, c.w, c.tile, sc.kernel_of(c.key, c.route, c.env)[1]) for c in CASES
                   if c.key != "1x" and c.route in ("u8", "u16") and (c.h, c.w, c.tile) not in new})


@pytest.mark.parametrize("key", cp.KEYS)
def test_mutants_bite(probes, uva, key):
    """one plausible slip each, restated in numpy on the reference: the probes see every one, with every weight set it is tried
    on (the float route's 37 x 70 / 50 x 33 frame and the tiled u8 frame of that set).  lost_carry_rows sits where the census
    puts a segment that needs rows from above it -- a later segment of a list, or a six-row start in the middle of a plane --
    on a census frame (4508 x 31 at tile 300) with the weight sets the GPU runs there; NO frame from before the census has such a place (carry_starts is empty for every one of
    them, under the planner switch it runs with): that is why they could not have seen this slip."""
    assert {m["kind"] for k in cp.KEYS for m in _mutants(k)} == set(cp.MUTANTS)
    for mu in _mutants(key):
        for s in (0, 4, 6) if key != "1x" else (0, 2, 5):
            if mu["kind"] == "lost_carry_rows" and s not in CENSUS_SETS:
                continue
            m = dict(mu)
            r = probes.ref(key, s)
            if m["kind"] == "clamp_slope":
                m["layer"] = max(cp.WINDOWS[key][s], key=lambda i: int((r.S[i] > 1).sum()))
            if m["kind"] == "lost_carry_rows":
                for h, w, t, planner in _old_geometries():
                    assert sc.carry_starts(uva, h, w, t, 10 if t else 0, planner) == [], (h, w, t, planner)
                h, w, t = CENSUS_TILED[1]
                starts = sc.carry_starts(uva, h, w, t, 10)
                assert starts
                plane, x0, r0, width = starts[len(starts) // 2]
                m.update(plane=plane, x0=x0, r0=r0, width=width)
                c = Case(key, s, "u8", h, w, t)
                img = probes.input(c)
                want = cp.to_codes(r.tiled_values(img, t))
                got = cp.to_codes(r.tiled_values(img, t, mutant=m))
            elif m["kind"] == "border_row":
                c = Case(key, s, "u8", 64, 64, 32)
                img = probes.input(c)
                want = cp.to_codes(r.tiled_values(img, 32))
                got = cp.to_codes(r.tiled_values(img, 32, mutant=m))
            else:
                h, w = (37, 70) if key != "1x" else (50, 33)
                x = cp.probe_input(h, w, seed=77 + s)
                want, got = r.forward(x), r.forward(x, mutant=m)
            differ = int((got != want).sum())
            print(f"{key} set {s} mutant {m}: {differ} of {want.size} samples differ")
            assert differ > 0, (key, s, m)


# ------------------------------------------------------------------------------------------------------------------- GPU
def _load(uva, path, key):
    net = uva.Net()
    net.opt.use_vulkan_compute = True
    net.set_vulkan_device(0)
    assert net.load_param(model_paths(key)[0]) == 0, getattr(net, "last_error", "")
    assert net.load_model(path) == 0, getattr(net, "last_error", "")
    return net


def _hold(name, got, want, layer="output"):
    """record through parity_report (no model, no route: tools/parity_slack.py never harvests a probe), then equality; the
    message names the first differing (layer, channel, y, x) -- frames: (layer, y, x, channel)"""
    try:
        if got.dtype == np.uint8:
            pr.check_u8(name, got, want, vs=REF, max_lsb=0, model=None, route=None)
        elif got.dtype == np.uint16:
            pr.check_u16(name, got, want, vs=REF, max_codes=0, model=None, route=None)
        else:
            pr.check_f32(name, got.astype(np.float64), want, vs=REF, max_abs=0, model=None, route=None)
    except AssertionError as e:
        raise AssertionError((name, "first difference (index, got, want) at layer", layer, cp.first_difference(got, want),
                              "differing samples", int((got != want).sum()), "of", got.size, str(e)[:300])) from None
    assert got.shape == want.shape and np.array_equal(got, want), (name, layer, cp.first_difference(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("c", [c for c in CASES if c.route == "f32"], ids=lambda c: c.id)
def test_gpu_float_route_and_every_layer(uva, probes, c):
    """_extract against Ref.forward, and debug_read_activation(idx) against the reference's tap for every idx"""
    assert uva.get_gpu_count() > 0
    net = _load(uva, probes.bin(c.key, c.wset), c.key)
    want, taps, _ = probes.want(c)
    got = net._extract(probes.input(c))
    for idx in range(net.num_convs - 1):
        _hold(f"probe {c.id} conv {idx}", net.debug_read_activation(idx, c.h, c.w), taps[idx], layer="conv %d" % idx)
    _hold(f"probe {c.id} extract", got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [c for c in CASES if c.route in ("u8", "u16")], ids=lambda c: c.id)
def test_gpu_frame_routes(uva, probes, c, monkeypatch):
    """process_u8 / process_u16, whole and tiled, by default and under every switch, against Ref -- not against each other"""
    assert uva.get_gpu_count() > 0
    if c.env:
        monkeypatch.setenv(*c.env)             # (the switches are read when a net's device side is built)
    net = _load(uva, probes.bin(c.key, c.wset), c.key)
    img = probes.input(c)
    if c.route == "u16":
        if c.key == "1x":
            net.enable_u16_1x()
        got = net.process_u16(img, tile_size=c.tile, border=10 if c.tile else 0)
    else:
        got = net.process_u8(img, tile_size=c.tile, border=10 if c.tile else 0)
    _hold(f"probe {c.id}", got, cp.to_codes(probes.want(c)[0], got.dtype))


@pytest.mark.gpu
def test_gpu_batch_of_three_frames(uva, probes):
    """process_u8_device_batch: three different frames in one sub10_kernel launch, each against Ref"""
    from test_gpu_batch import run_batch
    assert uva.get_gpu_count() > 0
    (c,) = [c for c in CASES if c.route == "batch"]
    net = _load(uva, probes.bin(c.key, c.wset), c.key)
    frames = [probes.input(c, k) for k in range(3)]
    got = run_batch(net, frames)
    for k in range(3):
        _hold(f"probe {c.id} frame {k}", got[k], cp.to_codes(probes.want(c, k)[0]))


@pytest.mark.gpu
def test_gpu_long_batch_of_four_frames(uva, probes):
    """process_u8_device_batch with four frames whose row lists are >= 160 rows long and run on from one frame into the next
    (the workload's --batch 4 runs lists of 560 rows; the batch of three above: 24), each frame against Ref"""
    from test_gpu_batch import run_batch
    assert uva.get_gpu_count() > 0
    (c,) = [c for c in CASES if c.route == "batch4"]
    net = _load(uva, probes.bin(c.key, c.wset), c.key)
    got = run_batch(net, [probes.input(c, k) for k in range(c.frames)])
    for k in range(c.frames):
        _hold(f"probe {c.id} frame {k}", got[k], cp.to_codes(probes.want(c, k)[0]))
