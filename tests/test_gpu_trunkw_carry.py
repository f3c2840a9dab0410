"""trunkw_kernel's producers carry the partial sums of the two rows a step shares with the next one across the step boundary
(csrc/uva_wino.hip.h kloop_carry: 32 fragment reads per k-loop instead of 48, a four-row A-ring) instead of reading the two
shared rows again.  Per output the MFMAs come in the order they always did, so nothing arithmetic changes and the bar is
equality: every frame must equal, BYTE FOR BYTE, the one a net built with UVA_TW_CARRY=0 gives -- that switch selects
trunkw_kernel<64, ACT, false>, the k-loop that reads all six rows of a step's window (and, as before, restores the signs of
negated channels in every launch: also exact).

Whole frames (tile 0) are one plane of their own size; plane heights 1, 2, 3, 4, 5, 7, 8, 9, 13 put a carried row at every
phase of a step and give the last step 1 to 4 valid rows, widths 1, 29, 30, 31, 61 are one, two and three strips with full and
partial last ones.  Two planes of one size come from a frame two tiles wide: 128 columns at tile 64 / border 10 are two planes of
74 (a last strip of 14 columns, the width the first folded schedule got wrong: walked alone), 124 at tile 62 two planes of 72,
whose 12-column last strips FOLD into one walk.
The same frames again with UVA_TW_SIX=1, where every workgroup's first step fetches all six input rows and the producers
make the carried sums from the two extra rows themselves (carry_in), and with UVA_TW_ACT16=0, the instantiation with the fp32
PReLU (its own register allocation: the one closest to the 256-register limit)."""
import numpy as np
import pytest

from conftest import load_net

HEIGHTS = (1, 2, 3, 4, 5, 7, 8, 9, 13)
WIDTHS = (1, 29, 30, 31, 61)


def frames(oracle):
    out = []
    for h in HEIGHTS:
        for w in WIDTHS:
            out.append((oracle.synthetic_frame(h, w, kind="random", seed=1000 * h + w), 0))
        out.append((oracle.synthetic_frame(h, 128, kind="random", seed=1000 * h + 74), 64))      # two planes of h x 74
        out.append((oracle.synthetic_frame(h, 124, kind="random", seed=1000 * h + 72), 62))      # two planes of h x 72, folded last strips
    # ranges cut the twelve strips of four planes into segments of at most three steps, one per workgroup
    out.append((oracle.synthetic_frame(96, 128, kind="random", seed=96128), 64))
    # 64 planes of up to 52 x 52: lists with a second segment, which starts on the sums the first one left behind
    out.append((oracle.synthetic_frame(256, 256, kind="random", seed=256256), 32))
    # fewer steps than workgroups: lists of a few steps, many workgroups without work
    out.append((oracle.synthetic_frame(200, 70, kind="random", seed=20070), 0))
    return out


def run(net, cases):
    return [net.process_u8(img, tile_size=t, border=10 if t else 0) for img, t in cases]


@pytest.fixture(scope="module")
def cases(oracle):
    return frames(oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("act16", [None, "0"])
@pytest.mark.parametrize("six", [None, "1"])
@pytest.mark.parametrize("key", ["2x", "4x"])
def test_carried_partial_sums_change_no_bit(uva, oracle, cases, key, six, act16, monkeypatch):
    if act16 is None:
        monkeypatch.delenv("UVA_TW_ACT16", raising=False)
    else:
        monkeypatch.setenv("UVA_TW_ACT16", act16)
    if six is None:
        monkeypatch.delenv("UVA_TW_SIX", raising=False)
    else:
        monkeypatch.setenv("UVA_TW_SIX", six)       # (read when a geometry's lists are built: both nets below are new)
    monkeypatch.setenv("UVA_TW_CARRY", "0")
    want = run(load_net(uva, key), cases)           # (the switches are read when a net's device side is built)
    monkeypatch.delenv("UVA_TW_CARRY")
    got = run(load_net(uva, key), cases)
    for (img, t), g, w in zip(cases, got, want):
        assert g.shape == w.shape
        assert np.array_equal(g, w), (key, six, act16, img.shape[:2], t, int(np.abs(g.astype(int) - w.astype(int)).max()), float((g != w).mean()))


def test_the_frames_are_the_planes_they_claim(uva, monkeypatch):
    """the geometry behind the cases above, from the schedule itself (host only)"""
    from test_trunkw_schedule import schedule
    monkeypatch.delenv("UVA_TW_SIX", raising=False)
    monkeypatch.delenv("UVA_TW_FOLD", raising=False)
    steps, nsteps, planes, _ = schedule(uva, 13, 128, 64, 10)
    assert [tuple(int(v) for v in p[:2]) for p in planes] == [(13, 74), (13, 74)]
    assert not ((steps[:, :, 1] >> 27) & 1).any()
    steps, nsteps, planes, _ = schedule(uva, 13, 124, 62, 10)
    assert [tuple(int(v) for v in p[:2]) for p in planes] == [(13, 72), (13, 72)]
    assert ((steps[:, :, 1] >> 27) & 1).any()
    # a segment's fill step: producers active, consumers idle
    def fills(steps, nsteps):
        return [sum(1 for g in range(int(nsteps[b])) if not (int(steps[b, g, 5]) >> 24) & 1) for b in range(steps.shape[0])]
    steps, nsteps, planes, _ = schedule(uva, 96, 128, 64, 10)
    assert sum(fills(steps, nsteps)) >= 4 * sum(-(-int(p[1]) // 30) for p in planes)      # every strip in four segments or more
    steps, nsteps, planes, _ = schedule(uva, 256, 256, 32, 10)
    assert max(fills(steps, nsteps)) >= 2                                               # two segments in one workgroup's list
    steps, nsteps, planes, _ = schedule(uva, 200, 70, 0, 0)
    assert 0 < int((nsteps > 0).sum()) < steps.shape[0]
