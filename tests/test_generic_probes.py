"""The generic executor's kernels (rdb4_kernel, g_conv3_sw / _sww / _sk, g_conv3_lds, the element-wise kernels; what runs
4x_Valar_v1) against a float64 reference BIT FOR BIT, on probe graphs whose arithmetic is exact (tests/generic_probe.py).

CPU (unmarked): the audit that licenses array_equal -- every blob exact in fp16, every fp32 accumulation order-independent,
g_conv3_sww's transforms exact -- for every probe x weight set x shape the GPU tests use; the float64 forward against
oracle/generic_oracle.py (another route: float32 im2col + tensordot) and against the independent torch fixture; the plan the host
loader derives for every probe; and every MUTANT of the reference (one plausible kernel slip each) differing from the reference
on the shapes its probe runs at.

GPU (-m gpu): every executor switch is read once per process, so every setting is a child process that runs all probes of its
group and leaves one .npz; the parent compares with the reference and checks the launch census (uva_net_debug_generic_launches):
the kernel a probe is named after ran, the one a switch takes away did not."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import generic_probe as gp
from conftest import ROOT

# launch-census indices (include/uva.h uva_net_debug_generic_launches)
LDS1, LDS2, LDS3, LDS4, LDS4_T8 = 11, 12, 13, 14, 15
LDS1_K1, LDS2_K1, LDS3_K1, LDS4_K1 = 16, 17, 18, 19
LDS2_WG, LDS4_WG, LDS2_T8 = 21, 22, 23
SW_SUM, SW_SUM2, SW64_SUM, SW64_ACT, RDB4, SW_PLAIN, SW64_PLAIN, SW64_UP = 24, 25, 26, 27, 28, 29, 30, 31
SK_SUM, SK_SUM2, SK_PLAIN = 32, 33, 34
CONV1, CONV3, SWW, SWW_SUM, SWW_SUM2, AXPBY, AXPBY_STRIDED, CONCAT_PART, INTERP, PRELU, PIXELSHUFFLE = range(40, 51)
INPUT_F32, INPUT_U8, OUTPUT_F32, OUTPUT_U8 = 51, 52, 53, 54
ALL_LDS = (LDS1, LDS2, LDS3, LDS4, LDS4_T8, LDS1_K1, LDS2_K1, LDS3_K1, LDS4_K1, LDS2_WG, LDS4_WG, LDS2_T8)

# ---------------------------------------------------------------------------------------------------------------- the cases
# rdb4_kernel: 48-column strips of which 42 are owned, rings of depth 10 / 8 / 6 / 4, partial sums one step late (RA_LAG),
# g_conv3_sw's four-row blocks (SW_R) -- every width and every height of the list occurs, the cross is pruned
DENSE_W = (16, 17, 41, 42, 43, 47, 48, 49, 84, 85, 90, 97)
DENSE_H = (1, 2, 3, 4, 7, 9, 10, 11, 23)
DENSE_SHAPES = sorted({(DENSE_H[i % 9], w) for i, w in enumerate(DENSE_W)} | {(DENSE_H[(2 * i + 4) % 9], w) for i, w in enumerate(DENSE_W)} |
                      {(23, 97), (23, 85), (11, 90), (10, 48), (9, 43), (23, 17)})
NARROW_SHAPES = [(9, 15), (23, 15)]                      # below the wmin >= 16 gate: the same graph layer by layer
SUM2_SHAPES = [(23, 97), (9, 84), (11, 49), (4, 64), (7, 31), (10, 17)]
TWO_SHAPES = [(23, 97), (9, 85), (10, 48), (3, 43), (7, 17)]
# g_conv3_lds: GC_TW = 32 columns, 8-row tiles; g_conv3_sw: 32- / 64-column strips
SINGLE_SHAPES = [(1, 1), (17, 1), (7, 31), (8, 32), (9, 33), (17, 63), (1, 64), (8, 64), (7, 65), (9, 96), (17, 96)]
TALL_SHAPE = (512, 1024)                                 # tiles >= 4 x CUs: g_conv3_lds's 16-row, 8-wave forms (UVA_GENERIC_NW=8)
# (h, w, tile): nine ragged planes; three wide ones; 14 and 27 small ones (the last: 21 of one class, more than one batch of 16)
FRAMES = [(70, 75, 32), (40, 150, 64), (20, 100, 16), (40, 132, 16)]
WHOLE = (37, 45)                                         # process_u8(tile_size=0) against _extract
SMALL_BATCH_PIXELS = 6000                                # splits the nine planes of 70x75 / 32 into several batches

SINGLES = {
    "conv3_48to16": lambda: gp.g_conv(48, 16),
    "conv3_64to32_act": lambda: gp.g_conv(64, 32, act=True),
    "conv3_32to32_sumba": lambda: gp.g_conv(32, 32, sum_order="ba"),
    "conv3_64to64": lambda: gp.g_conv(64, 64),
    "conv3_64to64_act": lambda: gp.g_conv(64, 64, act=True),
    "conv3_64to64_sumba": lambda: gp.g_conv(64, 64, sum_order="ba"),
    "conv3_64to64_sumab": lambda: gp.g_conv(64, 64, sum_order="ab"),
    "conv1_64to16": lambda: gp.g_conv(64, 16, k=1),
    "conv1_48to32_act": lambda: gp.g_conv(48, 32, k=1, act=True),
    "conv1_64to64_sumba": lambda: gp.g_conv(64, 64, k=1, sum_order="ba"),
    "interp": gp.g_interp,
    "prelu_axpby": gp.g_prelu_axpby,
    "concat": gp.g_concat,
}
WINO_CONVS = ("b0c5", "b1c5")


class Case:
    """one run: graph x weight set x input; `want` (float64, the reference) and `audit` are made once and shared"""

    def __init__(self, group, graph, wset, h, w, route="f32", tile=0):
        self.group, self.graph, self.wset, self.h, self.w, self.route, self.tile = group, graph, wset, h, w, route, tile
        self.net = "%s_w%d" % (graph.name, wset)
        self.key = "%dx%d_t%d_%s" % (h, w, tile, route)


def _cases():
    out = []
    d1, d15, ds, d2 = gp.g_dense(), gp.g_dense(), gp.g_dense(double_sum=True), gp.g_dense(2)
    for ws in gp.WSETS:
        out += [Case("dense", d1, ws, h, w) for h, w in DENSE_SHAPES + NARROW_SHAPES]
        out += [Case("sum2", ds, ws, h, w) for h, w in SUM2_SHAPES]
        out += [Case("two", d2, ws, h, w) for h, w in TWO_SHAPES]
    for k, (name, make) in enumerate(SINGLES.items()):
        g = make()
        assert g.name == name, (g.name, name)
        # (every shape and every weight set occur with every probe; the full cross is the dense block's)
        out += [Case("single", g, (i + k) % 3, h, w) for i, (h, w) in enumerate(SINGLE_SHAPES)]
    out.append(Case("tall", gp.g_tall(), 1, *TALL_SHAPE))
    for g in (gp.g_dense(u8=True), gp.g_scale2_u8()):
        out += [Case("u8", g, i % 3, h, w, "u8", t) for i, (h, w, t) in enumerate(FRAMES)]
        out += [Case("u8", g, 2, WHOLE[0], WHOLE[1], r, 0) for r in ("u8", "f32of_u8")]
    return out


CASES = _cases()


class Probes:
    """the probes' files, references and audits, made on first use and shared by every test of the module"""

    def __init__(self, directory):
        self.dir, self.files, self.refs, self.done = directory, {}, {}, {}

    def paths(self, c):
        if c.net not in self.files:
            self.files[c.net] = gp.write_probe(c.graph, c.wset, self.dir)
            self.refs[c.net] = gp.Ref(*self.files[c.net])
        return self.files[c.net]

    def ref(self, c):
        self.paths(c)
        return self.refs[c.net]

    def input(self, c):
        return gp.probe_input(c.h, c.w, seed=1000 * c.h + c.w + 7 * c.wset, u8=c.route != "f32")

    def want(self, c, mutant=None):
        """-> (reference, audit): f32 route float64 [3][sh][sw]; u8 route float64 [sh][sw][3] = 255 * result before rounding"""
        k = (c.net, c.key)
        if mutant is None and k in self.done:
            return self.done[k]
        r, x, a = self.ref(c), self.input(c), gp.Audit() if mutant is None else None
        if c.route == "f32":
            res = r.forward(x, audit=a, wino=WINO_CONVS, mutant=mutant)
        elif c.route == "f32of_u8":
            res = r.forward(gp.q16(x.transpose(2, 0, 1).astype(np.float32) * np.float32(1 / 255.0)), audit=a, wino=WINO_CONVS, mutant=mutant)
        elif c.tile == 0:
            res = r.u8_values(x, audit=a, wino=WINO_CONVS, mutant=mutant)
        else:
            res = gp.tiled_u8(r, x, c.tile, swap_border_of=(mutant or {}).get("plane"), audit=a, wino=WINO_CONVS)
        if mutant is None:
            self.done[k] = (res, a)
        return res, a


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    return Probes(tmp_path_factory.mktemp("probes"))


def _tie_mask(v):
    """u8 route: samples whose reference value 255 y ends in exactly .5"""
    return np.abs(v - np.floor(v) - 0.5) == 0


# ------------------------------------------------------------------------------------------------------------ CPU: the audit
@pytest.mark.parametrize("group", ["dense", "sum2", "two", "single", "tall", "u8"])
def test_exactness_audit(probes, group):
    """What licenses array_equal on the GPU.  The two-block probe's SECOND block is the one exception the design has: its
    accumulations are order-independent like all others, its blobs need fp16's rounding -- the same rounding on both sides, which
    is why no Winograd claim is made there."""
    n = 0
    for c in CASES:
        if c.group != group:
            continue
        v, a = probes.want(c)
        skip = {k for k in a.blobs if k.startswith("b1") or k == "tail_o"} if group == "two" else ()
        bad = [b for b in a.bad(skip) if not (group == "two" and b == ("wino", "b1c5"))]      # (no Winograd claim for block 2)
        assert bad == [], (c.net, c.key, bad)
        if group in ("dense", "sum2", "two"):
            assert a.wino.get("b0c5") is True
        if c.route == "u8":
            tie, inside = float(_tie_mask(v).mean()), float(((v >= 0) & (v <= 255)).mean())
            assert tie <= 0.01 and inside >= 0.90, (c.net, c.key, tie, inside)
            assert len(np.unique(gp.to_u8(v))) >= 16            # (not a flat frame)
        n += 1
    assert n > 0


def test_weight_sets_fill_every_k_step():
    """every convolution of every weight set has a non-zero at every k-step (tap x 32-channel chunk: rdb4_kernel splits a
    convolution's k-steps between waves) and in every output channel; at least three sets, all different"""
    assert len(gp.WSETS) >= 3
    for g in (gp.g_dense(2, double_sum=True), gp.g_dense(u8=True), gp.g_concat()):
        sets = [gp.weights(g, ws)[0] for ws in gp.WSETS]
        for name, (w, b) in sets[0].items():
            for s in sets:
                w = s[name][0]
                cout, cin, k, _ = w.shape
                hit = {(dy * k + dx, ci // 32) for _, ci, dy, dx in np.argwhere(w != 0)}
                assert len(hit) == k * k * -(-cin // 32), name
                assert (np.abs(w).reshape(cout, -1).sum(axis=1) > 0).all(), name
            assert not np.array_equal(sets[0][name][0], sets[1][name][0]) and not np.array_equal(sets[1][name][0], sets[2][name][0])


def test_float64_forward_agrees_with_the_restatement_and_the_fixture(probes, tmp_path):
    """Two evaluations by different routes: generic_probe.Ref (float64, a loop over the non-zero weights) and
    generic_oracle.Model.forward (float32, im2col + tensordot) agree bit for bit on the probes; on dense Gaussian weights Ref
    meets the independent torch evaluation of all 1206 layers of 4x_Valar_v1 at that fixture's bar."""
    from oracle import generic_oracle as go
    from upscale_video_amd import upscale_processing as up
    by_net, kinds = {}, set()
    for c in CASES:
        if c.group != "tall":
            by_net.setdefault(c.net, []).append(c)
    assert len(by_net) == 3 * 3 + 3 * len(SINGLES) + 2 * 3
    for net, cs in by_net.items():
        # float route: the net's first shape and a taller one (rows above and below every tap); u8 route: the whole-frame
        # call both ways and the smallest tiled frame
        tall = [c for c in cs if c.h >= 7 and c.w >= 7]
        pick = {cs[0].key: cs[0]}
        if tall:
            c = min(tall, key=lambda c: abs(c.h * c.w - 800))
            pick[c.key] = c
        if cs[0].route != "f32":
            tiled = [c for c in cs if c.tile > 0]
            pick = {c.key: c for c in [c for c in cs if c.tile == 0] + ([min(tiled, key=lambda c: c.h * c.w)] if tiled else [])}
        om = go.Model(*probes.paths(cs[0]))
        compared = 0
        for c in pick.values():
            want, _ = probes.want(c)
            x = probes.input(c)
            if c.route == "f32":
                got = om.forward(x, f16_storage=True).astype(np.float64)
            elif c.route == "f32of_u8":
                got = om.forward(x.transpose(2, 0, 1).astype(np.float32) * np.float32(1 / 255.0), f16_storage=True).astype(np.float64)
            elif c.tile == 0:
                got, want = om.apply_u8(x, f16_storage=True), gp.to_u8(want)
            else:                               # the reference's tile loop over generic_oracle, as test_generic_graph.py builds it
                s_ = c.graph.scale["output"]
                got, want = np.zeros((s_ * c.h, s_ * c.w, 3), np.uint8), gp.to_u8(want)
                for ty in range(-(-c.h // c.tile)):
                    for tx in range(-(-c.w // c.tile)):
                        (y0, y1, x0, x1), (top, bottom, left, right) = up.tile_window(c.tile, ty, tx, c.h, c.w)
                        t = om.apply_u8(np.ascontiguousarray(x[y0 - top:y1 + bottom, x0 - left:x1 + right]), f16_storage=True)
                        got[s_ * y0:s_ * y1, s_ * x0:s_ * x1] = t[s_ * top:s_ * (top + y1 - y0), s_ * left:s_ * (left + x1 - x0)]
            assert got.shape == want.shape and np.array_equal(got, want), (c.net, c.key)
            compared += 1
            kinds.add((c.graph.name, c.route, c.tile > 0))
        assert compared == len(pick) >= (1 if cs[0].route != "f32" or not tall else 2), (net, compared)
    for g in ("dense1_u8", "scale2_u8"):        # (a u8 graph's whole-frame cases sit with one weight set, its tiled frames with all)
        assert {(g, "u8", False), (g, "f32of_u8", False), (g, "u8", True)} <= kinds, (g, sorted(kinds))
    from upscale_video_amd import synth
    g = np.load(os.path.join(ROOT, "tests", "golden", "valar_synthetic.npz"))
    seed, gain = g["valar_seed_gain"]
    valar = os.path.join(ROOT, "models", "4x_Valar_v1.param")
    b = str(tmp_path / "4x_Valar_v1.bin")
    synth.synthetic_weights(valar, b, seed=int(seed), gain=float(gain))
    x = g["valar_12x20_in"].transpose(2, 0, 1).astype(np.float32) * np.float32(1 / 255.0)
    f = gp.Ref(valar, b).forward(x, f16_storage=False)
    want = g["valar_12x20_f32"]
    assert f.shape == want.shape and float(np.abs(f - want).max()) <= 2e-5 * float(np.abs(want).max()) + 1e-6


def test_probe_plans(uva, probes):
    """every probe through the library's host loader: dense blocks recognised (info[6]), their chains' Concats free, the
    three-input Concat of the `concat` probe a copying one outside any chain"""
    from upscale_video_amd import _lib
    L = _lib.load()
    want = {"dense1": (1, 1, 4, 4, 0), "dense1_sum2": (1, 1, 4, 4, 0), "dense2": (2, 2, 8, 8, 0), "dense1_u8": (1, 1, 4, 4, 0),
            "concat": (0, 0, 1, 0, 0)}
    seen = set()
    for c in CASES:
        if c.net in seen:
            continue
        seen.add(c.net)
        p, b = probes.paths(c)
        net = uva.Net()
        assert net.load_param(p) == 0 and net.load_model(b) == 0, (c.net, getattr(net, "last_error", ""))
        info = (ctypes.c_int * 8)()
        assert L.uva_net_debug_generic_plan(net._h, info) == 0, L.uva_last_error()
        rdbs, groups, concats, free, first = info[6], info[0], info[1], info[2], info[3]
        assert (rdbs, groups, concats, free, first) == want.get(c.graph.name, (0, 0, 0, 0, 0)), (c.net, list(info))
        assert net.scale == c.graph.scale["output"]
        n = ctypes.c_int(0)
        assert L.uva_net_debug_generic_launches(net._h, None, 0, ctypes.byref(n)) == 0 and n.value == OUTPUT_U8 + 1
        assert sum(net.debug_generic_launches()) == 0          # (nothing has run)


# ------------------------------------------------------------------------------------------------------ CPU: the mutants bite
def _mutants():
    out = []
    for conv, nchunk in (("head", 1), ("b0c1", 2), ("b0c2", 3), ("b0c3", 4), ("b0c4", 5), ("b0c5", 6)):
        out += [("dense", dict(kind="kstep", layer=conv, tap=t, chunk=ch)) for t, ch in ((4, nchunk - 1), (8, 0), (0, nchunk // 2))]
    out += [("dense", dict(kind="kstep", layer="b0c2s", tap=0, chunk=1)), ("two", dict(kind="kstep", layer="b1c2", tap=2, chunk=2))]
    # strips: rdb4_kernel's second 48-column strip starts at column 42 and owns from 45; g_conv3_sw's at 32 (192 inputs) / 64
    out += [("dense", dict(kind="halo_col", layer=conv, col=col)) for conv, col in (("b0c1", 41), ("b0c4", 44), ("b0c4", 83), ("b0c5", 31), ("b0c5", 63))]
    out += [("single", dict(kind="halo_col", layer="mid", col=col, probe=p)) for p, col in (("conv3_64to64", 63), ("conv3_64to64_act", 63),
                                                                                          ("conv3_64to64_sumba", 63), ("conv3_48to16", 31), ("interp", 63))]
    out += [("dense", dict(kind="seg_row", layer=conv, row=row)) for conv in ("b0c1", "b0c2", "b0c3", "b0c4", "b0c5") for row in (0, 3, 8)]
    out += [("single", dict(kind="seg_row", layer="mid", row=7, probe="conv3_64to64")), ("single", dict(kind="seg_row", layer="mid", row=3, probe="conv3_64to64_act"))]
    out += [("dense", dict(kind="last_row", layer=ly)) for ly in ("b0c1", "b0add2", "b0c3", "b0add4", "b0sum")]
    out += [("single", dict(kind="last_row", layer="mid", probe=p)) for p in SINGLES if p != "prelu_axpby"]
    out += [("dense", dict(kind="preact", layer="b0add4")), ("two", dict(kind="preact", layer="b1add4"))]
    out += [("dense", dict(kind="swap_sum", layer="b0sum")), ("sum2", dict(kind="swap_sum", layer="sum2")), ("sum2", dict(kind="swap_sum", layer="b0sum")),
            ("two", dict(kind="swap_sum", layer="b1sum"))]
    out += [("single", dict(kind="swap_sum", layer="sum", probe=p)) for p in SINGLES if "sum" in p or p == "prelu_axpby"]
    out += [("u8", dict(kind="border", plane=k, probe=p)) for p in ("dense1_u8", "scale2_u8") for k in (1, 4)]
    return out


@pytest.mark.parametrize("group,mutant", _mutants(), ids=lambda v: v if isinstance(v, str) else "-".join(str(x) for x in v.values()))
def test_mutants_bite(probes, group, mutant):
    """one plausible kernel slip, restated in numpy (generic_probe.Ref.forward): its result differs from the reference on at
    least one of the shapes the GPU test of that probe runs -- the shapes and the weights can see the slip -- with at least two of
    the three weight sets."""
    mu = {k: v for k, v in mutant.items() if k != "probe"}
    cs = [c for c in CASES if c.group == group and ("probe" not in mutant or c.graph.name == mutant["probe"])]
    if group == "u8":
        cs = [c for c in cs if c.tile > 0]
    # only where the slip can show at all: the column or row it touches lies inside the plane
    cs = [c for c in cs if c.w >= mu.get("col", 0) + 2 and c.h >= mu.get("row", 0) + 2]
    # Per weight set the mutant is evaluated until one shape shows it (one reference evaluation each: the order only saves
    # time).  Mid-sized planes first, smallest first among them -- they nearly always show the slip; planes of fewer than 300
    # pixels (a row or two: little for a slip to touch) come last, the larger of those first.
    mid = sorted((c for c in cs if c.h * c.w >= 300), key=lambda c: c.h * c.w)
    tiny = sorted((c for c in cs if c.h * c.w < 300), key=lambda c: -c.h * c.w)
    caught = set()
    for c in mid + tiny:
        if c.wset in caught:
            continue
        want, _ = probes.want(c)
        got, _ = probes.want(c, mutant=mu)
        if c.route == "u8":
            m = ~_tie_mask(want)
            caught |= set() if np.array_equal(gp.to_u8(got)[m], gp.to_u8(want)[m]) else {c.wset}
        else:
            caught |= set() if np.array_equal(got, want) else {c.wset}
    # every weight set sees 48 of the 64 channels and reads most, not all, channels of x1 .. x4: a slip confined to ONE
    # output channel may hide from one set, never from two
    assert len(caught) >= min(2, len({c.wset for c in cs})) and caught, (sorted(caught), mutant)


# ---------------------------------------------------------------------------------------------------------------- GPU side
_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from upscale_video_amd import ncnn
job = json.load(open(sys.argv[2]))
inputs = np.load(job["inputs"])
out = {}
for nd in job["nets"]:
    net = ncnn.Net()
    net.set_vulkan_device(0)
    assert net.load_param(nd["param"]) == 0 and net.load_model(nd["bin"]) == 0, getattr(net, "last_error", "")
    for r in nd["runs"]:
        x = inputs[nd["key"] + "/" + r["key"]]
        if r["route"] == "u8":
            y = net.process_u8(x, tile_size=r["tile"], border=10)
        elif r["route"] == "f32of_u8":
            y = net._extract(x.transpose(2, 0, 1).astype(np.float32) * np.float32(1 / 255.0))
        else:
            y = net._extract(x)
        out[nd["key"] + "/" + r["key"]] = y
        out["census/" + nd["key"] + "/" + r["key"]] = np.array(net.debug_generic_launches(), np.int64)
    del net
np.savez(sys.argv[3], **out)
"""
_DIED = []          # a child that did not end with status 0, or hung: nothing more is started on the GPU by this module


def _run_child(probes, tmp_path, env, cases):
    """-> {(net, key): (result, launches of that run)}: one child process under `env` runs `cases` net by net"""
    if _DIED:
        pytest.fail("an earlier child process died (%s): nothing more is started" % _DIED[0])
    nets, inputs = {}, {}
    for c in cases:
        p, b = probes.paths(c)
        nets.setdefault(c.net, dict(key=c.net, param=p, bin=b, runs=[]))["runs"].append(dict(key=c.key, route=c.route, tile=c.tile))
        inputs[c.net + "/" + c.key] = probes.input(c)
    np.savez(str(tmp_path / "inputs.npz"), **inputs)
    with open(str(tmp_path / "job.json"), "w") as f:
        json.dump(dict(inputs=str(tmp_path / "inputs.npz"), nets=list(nets.values())), f)
    out = str(tmp_path / "out.npz")
    try:
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path / "job.json"), out], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        _DIED.append("timeout under %r" % (env,))
        raise
    if r.returncode != 0:       # a signal, an abort, or a HIP error raised through _lib.check (exit 1: a GPU fault reads like that)
        _DIED.append("exit %d under %r" % (r.returncode, env))
    assert r.returncode == 0, (env, r.returncode, r.stdout[-1500:] + r.stderr[-3000:])
    z = np.load(out)
    res, last = {}, {}
    for c in cases:
        cen = z["census/%s/%s" % (c.net, c.key)]
        res[(c.net, c.key)] = (z["%s/%s" % (c.net, c.key)], cen - last.get(c.net, 0))
        last[c.net] = cen
    return res


def _compare(probes, res, cases):
    """every result equals the reference's bits (u8 route: its bytes outside the tie mask); all differences are collected
    before the assertion, so that one failure names every shape that differs"""
    bad = []
    for c in cases:
        got, _ = res[(c.net, c.key)]
        want, _ = probes.want(c)
        if c.route == "u8":
            m = ~_tie_mask(want)
            ok = got.shape == want.shape and np.array_equal(got[m], gp.to_u8(want)[m])
        else:
            ok = got.shape == want.shape and np.array_equal(got.astype(np.float64), want)
        if not ok:
            d = np.argwhere(got.astype(np.float64) != (gp.to_u8(want) if c.route == "u8" else want)) if got.shape == want.shape else []
            bad.append((c.net, c.key, len(d), [tuple(int(v) for v in e) for e in d[:4]]))
    assert not bad, "%d of %d runs differ from the reference: %r" % (len(bad), len(cases), bad[:12])


def _census(res, cases, rule):
    """rule(case) -> {census index: how often that kernel must have been launched by this run}"""
    bad = []
    for c in cases:
        cen = res[(c.net, c.key)][1]
        bad += [(c.net, c.key, idx, int(cen[idx]), want) for idx, want in rule(c).items() if int(cen[idx]) != want]
    assert not bad, bad[:12]


DENSE_SETTINGS = {
    "default": {}, "wino0": {"UVA_GENERIC_WINO": "0"}, "sk1": {"UVA_GENERIC_SK": "1"}, "rdb0": {"UVA_GENERIC_RDB": "0"},
    "sw0": {"UVA_GENERIC_SW": "0"}, "fuse_add0": {"UVA_GENERIC_FUSE_ADD": "0"}, "lds0": {"UVA_GENERIC_LDS": "0"},
    "grid2": {"UVA_GENERIC_GRID": "2"}, "grid8": {"UVA_GENERIC_GRID": "8"},
}


def _on(env, name, default=True):
    return env.get(name, "1" if default else "0") != "0"


def _dense_rule(env, blocks=1, sum2=False):
    """how often a dense-block probe launches which kernel on an h x w plane under `env` (csrc/uva_generic_run.hip generic_run_planes):
    exact counts, so a probe that silently takes another kernel fails here"""
    def rule(c):
        lds = _on(env, "UVA_GENERIC_LDS")
        fused = lds and _on(env, "UVA_GENERIC_FUSE_ADD")
        rdb = lds and _on(env, "UVA_GENERIC_RDB") and c.w >= 16
        strips = lds and _on(env, "UVA_GENERIC_SW") and c.w >= 32     # the 192 -> 64 convolution on 32-column strips
        two = sum2 and fused and strips                               # the second sum goes into the strip kernels' epilogue
        e = {k: 0 for k in (SWW, SWW_SUM, SWW_SUM2, SW_PLAIN, SW_SUM, SW_SUM2, SK_PLAIN, SK_SUM, SK_SUM2)}
        if strips:
            family = (SK_PLAIN, SK_SUM, SK_SUM2) if _on(env, "UVA_GENERIC_SK", False) else \
                     (SWW, SWW_SUM, SWW_SUM2) if _on(env, "UVA_GENERIC_WINO") else (SW_PLAIN, SW_SUM, SW_SUM2)
            e[family[2 if two else 1 if fused else 0]] = blocks
        e.update({INPUT_F32: 1, OUTPUT_F32: 1, PIXELSHUFFLE: 1, RDB4: blocks if rdb else 0,
                  LDS2_WG: 0 if rdb or not lds else 4 * blocks, LDS2_K1: 0 if rdb or not lds else blocks,
                  LDS4_WG: 1 + (0 if strips else blocks) if lds else 0, LDS3_K1: 1 if lds else 0,
                  AXPBY_STRIDED: (0 if fused else blocks if rdb else 3 * blocks) + (1 if sum2 and not two else 0) if lds else 0,
                  AXPBY: 0 if lds else 3 * blocks + (1 if sum2 else 0),
                  CONV1: 0 if lds else blocks + 1, CONV3: 0 if lds else 1 + 5 * blocks, CONCAT_PART: 0 if lds else 14 * blocks})
        return e
    return rule


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(DENSE_SETTINGS))
def test_dense_block_probes_bit_for_bit(probes, tmp_path, setting):
    """rdb4_kernel, then the 192 -> 64 convolution with the block's sum in its epilogue -- as g_conv3_sww (Winograd F(2,3), the
    default), g_conv3_sw<6, 1> (UVA_GENERIC_WINO=0), g_conv3_sk (UVA_GENERIC_SK=1) -- and the same graph layer by layer
    (UVA_GENERIC_RDB=0, _SW=0, _FUSE_ADD=0, _LDS=0, and below the 16-column gate), on 2 and 8 workgroups (several segments and
    strips per workgroup): every setting, every shape, every weight set the reference's bits."""
    cases = [c for c in CASES if c.group == "dense"]
    res = _run_child(probes, tmp_path, DENSE_SETTINGS[setting], cases)
    _compare(probes, res, cases)
    _census(res, cases, _dense_rule(DENSE_SETTINGS[setting]))


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(DENSE_SETTINGS))
def test_double_sum_probes_bit_for_bit(probes, tmp_path, setting):
    """a second sum behind the block's (models/4x_Valar_v1.param:55-56): g_conv3_sw<6, 1, false, 2, 2>, g_conv3_sk<2, 2> and
    g_conv3_sww's double epilogue on planes of at least 32 columns, a launch of its own below"""
    cases = [c for c in CASES if c.group == "sum2"]
    res = _run_child(probes, tmp_path, DENSE_SETTINGS[setting], cases)
    _compare(probes, res, cases)
    _census(res, cases, _dense_rule(DENSE_SETTINGS[setting], sum2=True))


TWO_SETTINGS = {"wino0": {"UVA_GENERIC_WINO": "0"}, "sk1": {"UVA_GENERIC_SK": "1"}, "rdb0": {"UVA_GENERIC_RDB": "0", "UVA_GENERIC_WINO": "0"}}


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(TWO_SETTINGS))
def test_two_dense_blocks_bit_for_bit(probes, tmp_path, setting):
    """the sum that closes block 1 writes x into block 2's shared array.  Block 2's blobs need fp16's rounding (the same on
    both sides; its accumulations are still order-independent), so its Winograd transforms are not exact: the claim is made with
    the direct kernels only -- the layer-by-layer run (UVA_GENERIC_RDB=0) therefore with UVA_GENERIC_WINO=0 as well."""
    cases = [c for c in CASES if c.group == "two"]
    res = _run_child(probes, tmp_path, TWO_SETTINGS[setting], cases)
    _compare(probes, res, cases)
    _census(res, cases, _dense_rule(TWO_SETTINGS[setting], blocks=2))


SINGLE_SETTINGS = {"default": {}, "wg0": {"UVA_GENERIC_WG": "0"}, "fuse_interp0": {"UVA_GENERIC_FUSE_INTERP": "0"}, "sw0": {"UVA_GENERIC_SW": "0"},
                   "fuse_add0": {"UVA_GENERIC_FUSE_ADD": "0"}, "lds0": {"UVA_GENERIC_LDS": "0"}}


def _lds_slot(cout, k, wg):
    mbn = -(-cout // 16)
    if k == 1:
        return (LDS1_K1, LDS2_K1, LDS3_K1, LDS4_K1)[mbn - 1]
    if wg and mbn in (2, 4):
        return LDS2_WG if mbn == 2 else LDS4_WG
    return (LDS1, LDS2, LDS3, LDS4)[mbn - 1]


def _single_rule(env):
    """a walk over the probe's layers that restates which kernel generic_run_planes gives each (exact launch counts)"""
    lds, wg, fold = _on(env, "UVA_GENERIC_LDS"), _on(env, "UVA_GENERIC_WG"), _on(env, "UVA_GENERIC_FUSE_INTERP")
    sw, fused = lds and _on(env, "UVA_GENERIC_SW"), lds and _on(env, "UVA_GENERIC_FUSE_ADD")

    def rule(c):
        g = c.graph
        by_out = {op["out"]: op for op in g.ops}
        readers = {}
        for op in g.ops:
            for b in op["ins"]:
                readers.setdefault(b, []).append(op)
        e = {k: 0 for k in ALL_LDS + (RDB4, SW64_SUM, SW64_ACT, SW64_PLAIN, SW64_UP, CONV1, CONV3, AXPBY, AXPBY_STRIDED, CONCAT_PART, INTERP,
                                      PRELU, PIXELSHUFFLE, INPUT_F32, OUTPUT_F32)}
        absorbed = set()
        for op in g.ops:
            t = op["type"]
            if t == "Input":
                e[INPUT_F32] += 1
            elif t == "Convolution":
                cv, out = op["conv"], op["out"]
                if not lds:
                    e[CONV3 if cv["k"] == 3 else CONV1] += 1
                    continue
                pos = None              # the sum this convolution takes into its epilogue, and which operand the convolution is
                rd = readers.get(out, [])
                if fused and len(rd) == 1 and rd[0]["type"] == "Eltwise" and cv["cout"] % 8 == 0:
                    pos = rd[0]["ins"].index(out)
                    absorbed.add(rd[0]["name"])
                strips = sw and cv["k"] == 3 and -(-cv["cin"] // 32) * 32 == 64 and cv["cout"] == 64 and c.w * g.scale[out] >= 64
                slot = {(False, None): SW64_PLAIN, (True, None): SW64_ACT, (False, 1): SW64_SUM}.get((cv["act"], pos)) if strips else None
                src = by_out[op["ins"][0]]
                if slot == SW64_ACT and fold and src["type"] == "Interp" and len(readers[src["out"]]) == 1:
                    slot = SW64_UP
                    e[INTERP] -= 1                       # (counted when the walk passed it: never launched)
                e[slot if slot is not None else _lds_slot(cv["cout"], cv["k"], wg)] += 1
            elif t == "Eltwise":
                e[AXPBY] += op["name"] not in absorbed
            elif t == "Concat":
                e[CONCAT_PART] += len(op["ins"])
            else:
                e[{"Interp": INTERP, "PReLU": PRELU, "PixelShuffle": PIXELSHUFFLE}[t]] += 1
        e[OUTPUT_F32] = 1
        return e
    return rule


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(SINGLE_SETTINGS))
def test_single_layer_probes_bit_for_bit(probes, tmp_path, setting):
    """one layer between a 3 -> C head and the selecting tail: g_conv3_lds with 16 / 32 / 48 / 64 outputs, 3x3 and 1x1, weights
    in registers or through LDS (UVA_GENERIC_WG=0), 32 / 64 / 96 padded inputs, fused LeakyReLU, a fused sum in both operand
    orders with unequal coefficients; g_conv3_sw's 64 -> 64 forms (sum, activation, plain, the 2x Interp folded in and
    UVA_GENERIC_FUSE_INTERP=0); g_interp_nearest, g_prelu, g_pixelshuffle, g_axpby, g_concat_part; the plain g_conv
    (UVA_GENERIC_LDS=0)"""
    cases = [c for c in CASES if c.group == "single"]
    res = _run_child(probes, tmp_path, SINGLE_SETTINGS[setting], cases)
    _compare(probes, res, cases)
    _census(res, cases, _single_rule(SINGLE_SETTINGS[setting]))


@pytest.mark.gpu
def test_tall_plane_takes_the_16_row_tiles_bit_for_bit(probes, tmp_path):
    """g_conv3_lds<2, 3, true, 8> and <4, 3, true, 8>: 16-row tiles on 8 waves, taken under UVA_GENERIC_NW=8 where tiles >= 4 x CUs
    -- 3 -> 32, 32 -> 32 and 32 -> 64 on a 512 x 1024 plane"""
    cases = [c for c in CASES if c.group == "tall"]
    res = _run_child(probes, tmp_path, {"UVA_GENERIC_NW": "8"}, cases)
    _compare(probes, res, cases)
    _census(res, cases, lambda c: {LDS2_T8: 2, LDS4_T8: 1, LDS2_WG: 0, LDS4_WG: 0, LDS1_K1: 1, CONV3: 0})


U8_SETTINGS = {"default": {}, "batch0": {"UVA_GENERIC_BATCH": "0"}, "fuse_out0": {"UVA_GENERIC_FUSE_OUT": "0"},
               "small_batches": {"UVA_GENERIC_BATCH_PIXELS": str(SMALL_BATCH_PIXELS)}}


def _batches(h, w, tile, bound):
    """-> (planes, batches) of an h x w frame as the executor plans them (uva_debug_generic_batches)"""
    from upscale_video_amd import _lib
    L = _lib.load()
    need = ctypes.c_size_t(0)
    L.uva_debug_generic_batches(h, w, tile, 10, bound, None, 0, ctypes.byref(need))
    words = (ctypes.c_int32 * need.value)()
    assert L.uva_debug_generic_batches(h, w, tile, 10, bound, words, need.value, ctypes.byref(need)) == 0, L.uva_last_error()
    pl = np.frombuffer(words, np.int32).reshape(-1, 4)
    return pl, len(set(int(b) for b in pl[:, 2]))


def test_frames_give_the_batches_the_gpu_test_is_about():
    """20 x 100 with 16-pixel tiles is 14 planes; 40 x 132 is 27, 21 of them of one class: more than one batch of 16; the small
    bound splits 70 x 75"""
    assert len(_batches(20, 100, 16, 0)[0]) == 14 and len(_batches(40, 132, 16, 0)[0]) == 27
    assert _batches(40, 132, 16, 0)[1] > len(set(int(c) for c in _batches(40, 132, 16, 0)[0][:, 3]))     # a class split by the 16-plane bound
    assert _batches(70, 75, 32, SMALL_BATCH_PIXELS)[1] > _batches(70, 75, 32, 0)[1] > 1


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(U8_SETTINGS))
def test_tiled_u8_probes_byte_for_byte(probes, tmp_path, setting):
    """plane batches and the u8 epilogue: frames cut into the reference's tiles (nine ragged planes; three wide ones; 14 and 27
    small ones, more than one batch; a pixel bound that splits a batch) through the dense-block probe and a scale-2 probe, the
    frame's bytes against the reference's tile loop outside the tie mask; one plane after the other (UVA_GENERIC_BATCH=0), the
    bytes from g_output_u8 (UVA_GENERIC_FUSE_OUT=0); and process_u8(tile_size=0) = clip(rint(255 * _extract(img / 255)))"""
    cases = [c for c in CASES if c.group == "u8"]
    res = _run_child(probes, tmp_path, U8_SETTINGS[setting], cases)
    _compare(probes, res, cases)
    for g in {c.graph.name for c in cases}:
        u8, f32 = [next(c for c in cases if c.graph.name == g and c.route == r and c.tile == 0) for r in ("u8", "f32of_u8")]
        m = ~_tie_mask(probes.want(u8)[0])
        assert np.array_equal(res[(u8.net, u8.key)][0][m], gp.to_u8(res[(f32.net, f32.key)][0].transpose(1, 2, 0).astype(np.float64) * 255.0)[m])

    def rule(c):
        if c.route != "u8":
            return {INPUT_F32: 1, OUTPUT_F32: 1, INPUT_U8: 0, OUTPUT_U8: 0}
        planes, _ = _batches(c.h, c.w, c.tile, SMALL_BATCH_PIXELS if setting == "small_batches" else 0)
        groups = [planes[planes[:, 2] == b] for b in sorted(set(int(b) for b in planes[:, 2]))]
        if setting == "batch0":
            groups = [planes[k:k + 1] for k in range(len(planes))]
        e = {INPUT_U8: len(planes), OUTPUT_U8: len(planes) if setting == "fuse_out0" else 0, OUTPUT_F32: 0, INPUT_F32: 0}
        if c.graph.name == "dense1_u8":      # one rdb4 launch per batch of planes at least 16 columns wide, layer by layer below
            e[RDB4] = sum(1 for g in groups if int(g[:, 1].min()) >= 16)
        else:                                # the 2x Interp is folded into g_conv3_sw's row DMA from 32 columns on, a launch per plane below
            e[INTERP] = sum(len(g) for g in groups if int(g[:, 1].min()) < 32)
            e[SW64_UP] = sum(1 for g in groups if int(g[:, 1].min()) >= 32)
        return e
    _census(res, cases, rule)
