"""Which STATES of the strip-walking kernels a frame geometry visits: a census of the step lists of trunkw_kernel and
trunk2_kernel, the tile lists of trunk_kernel and the row lists of sub10_kernel / sub5_kernel, decoded on the host through the
debug hooks (the decoders of test_trunkw_schedule.py, test_trunk2_schedule.py, test_sub10_rows.py, test_sub5_rows.py) and
reduced to a set of coarse CLASSES.  A class says "this state of the kernel was visited", not "this exact frame": a ring
phase, the kind of a segment's first step, which rows a consumer step stores, a list's length bucket.

tests/test_compact_probes.py holds the union of the census over its bit-exact cases against the census of the shipped
workloads (WORKLOADS): a state a real frame reaches and no bit-exact case does is where a kernel can be wrong unseen.

Why list index mod 5 and mod 3 (mod 4, mod 3 for trunk2; row index mod 4 for the 1x kernels) are the phases.  The kernels
keep LDS rings whose write position advances by a fixed number of rows per step and never resets inside a workgroup's list:
  trunkw_kernel   the consumers' ring of intermediate rows has TW_BROWS = 10 rows (csrc/uva_wino.hip.h:59) and takes 4 new
                  rows per step: position (4 g) % 10, period 5 steps.  The producers' ring of transformed input rows has
                  AROWS = 6 with UVA_TW_CARRY=0 (csrc/uva_wino.hip.h:67; 4 new rows per step: period 3) and 4 with the
                  carry (period 1: no phase)
  trunk2_kernel   T2_SLOTS = 4 input halo tiles (csrc/uva_plan.h:54; one per step: period 4) and T2_RING_ROWS = 12
                  intermediate rows (csrc/uva_kernels.hip.h:1313; 4 per step: period 3)
  trunk_kernel    TRUNK_SLOTS = 5 tile slots (csrc/uva_kernels.hip.h:922), two tiles per turn of a workgroup
  sub10_kernel    every layer's activation ring has 4 rows (S10_RINGB = 4 * S10_ROWB, csrc/uva_sub10.hip.h:36; rows are addressed
                  (d & 3): csrc/uva_sub10.hip.h:204, :410), one row per step: period 4; the residual ring S10_RES_ROWS = 32
                  (csrc/uva_sub10.hip.h:40) bounds the middle bucket of a segment's written rows
  sub5_kernel     the same with RINGB = 4 * ROWB (csrc/uva_sub5.hip.h:40; (d & 3): csrc/uva_sub5.hip.h:183, :351)
So a segment start, a store or a warm-up row at list index g meets the ring at phase g mod period, whatever came before it in
the list -- and a list shorter than the period (every list of the small probe frames: at most 4 steps) never closes a lap."""
import contextlib
import os

import test_sub5_rows as s5
import test_sub10_rows as s10
import test_trunk2_schedule as t2
import test_trunkw_schedule as tw

GRID = 256                      # workgroups: one per CU of an MI355X (uva_api.hip: grid = ncu rounded down to a multiple of 8)
TW_BPERIOD, TW_APERIOD = 5, 3   # see above
T2_PERIODS = (4, 3)
TRUNK_SLOTS = 5
ROW_RING = 4                    # sub10 / sub5 activation ring rows
RES_ROWS = 32                   # S10_RES_ROWS

# the geometries BASELINE.md and bench.py run: (net group, h, w, tile, border, frames)
WORKLOADS = {
    "1080p at 960/10": ("2x4x", 1080, 1920, 960, 10, 1),
    "1080p whole": ("2x4x", 1080, 1920, 0, 0, 1),
    "2160p at 960/10": ("2x4x", 2160, 3840, 960, 10, 1),
    "1x 1080p, batch 1": ("1x", 1080, 1920, 0, 0, 1),
    "1x 1080p, batch 4": ("1x", 1080, 1920, 0, 0, 4),
}
# the kernel groups (kernel_of): each has a census of its own
TRUNK_KERNELS = ("trunkw_kernel", "trunkw_kernel, UVA_TW_CARRY=0", "trunkw_kernel, UVA_TW_ACT16=0", "trunk2_kernel", "trunk_kernel")
ROW_KERNELS = ("sub10_kernel", "sub10_kernel16", "sub5_kernel", "pair24_kernel")


@contextlib.contextmanager
def planner_env(group):
    """the planner's switches are read per call (uva_api.hip): set the one of `group` around a hook call, drop the others"""
    # (the library honours its switches only under this opt-in, tests/conftest.py sets it: without it every group would
    # silently get the default lists)
    assert os.environ.get("UVA_DEBUG_SWITCHES") == "1", "the planner's switches need UVA_DEBUG_SWITCHES=1"
    names = ("UVA_TW_SIX", "UVA_TW_FOLD", "UVA_T2_NARROW")
    old = {k: os.environ.get(k) for k in names}
    for k in names:
        os.environ.pop(k, None)
    if "=" in group and group.split("=")[0] in names:
        os.environ[group.split("=")[0]] = group.split("=")[1]
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def bucket(n, exact, *bounds):
    """1 .. exact as themselves, then "a-b" per bound and ">= last" """
    if n <= exact:
        return str(n)
    lo = exact + 1
    for b in bounds:
        if n <= b:
            return "%d-%d" % (lo, b)
        lo = b + 1
    return ">=%d" % lo


def _off(v):
    return int(v[0]) | ((int(v[1]) & 0xff) << 32)


# ------------------------------------------------------------------------------------------------------------------ trunkw
def trunkw_lists(uva, h, w, tile, border, group="default"):
    """-> [workgroup][segment] of dicts: plane, x0, r0 (first output row), g0 (list index of its first step), six, fold, rmask,
    steps [(g, rmask, c_lo, c_hi, stores or None)], stores = (v0, v1, vx)"""
    with planner_env(group):
        steps, nsteps, planes, guard = tw.schedule(uva, h, w, tile, border, GRID)
    out = []
    for b in range(GRID):
        segs, prev = [], None
        for g in range(int(nsteps[b])):
            a, bb = steps[b, g, :4], steps[b, g, 4:]
            fold, six = (int(a[1]) >> 27) & 1, (int(a[1]) >> 25) & 1
            pi = int(a[2]) >> 24 if fold else int(a[3])
            row, col = tw.locate(_off(a), planes, guard, pi)
            yA, x0 = row - 2, col + 1
            rmask, c_lo, c_hi = (int(a[1]) >> 8) & 15, (int(a[1]) >> 12) & 63, (int(a[1]) >> 18) & 63
            if prev != (pi, x0, yA - 4):
                segs.append(dict(plane=pi, x0=x0, r0=yA + (1 if six else 3), g0=g, six=six, fold=fold, rmask=rmask, steps=[],
                                 ph=int(planes[pi, 0]), pw=int(planes[pi, 1])))
            prev = (pi, x0, yA)
            st = None
            if (int(bb[1]) >> 24) & 1:
                st = ((int(bb[1]) >> 17) & 7, (int(bb[1]) >> 8) & 7, (int(bb[1]) >> 11) & 63)
            segs[-1]["steps"].append((g, rmask, c_lo, c_hi, st))
        out.append(segs)
    return out


def trunkw_census(uva, h, w, tile, border, group="default"):
    lists = trunkw_lists(uva, h, w, tile, border, group)
    a_ring = group == "UVA_TW_CARRY=0"
    out = set()
    for segs in lists:
        if not segs:
            continue
        out.add(("list length", bucket(sum(len(s["steps"]) for s in segs), 5, 11)))
        out.add(("segments per list", bucket(len(segs), 2)))
        for k, s in enumerate(segs):
            kind = "six-row" if s["six"] else "fill"
            where = "top of plane" if s["r0"] == 0 else "mid-plane"
            out.add(("segment start", kind, where, "index %% 5 = %d" % (s["g0"] % TW_BPERIOD), "folded" if s["fold"] else "single", "rmask %d" % s["rmask"]))
            if a_ring:
                out.add(("segment start, A-ring", kind, where, "index %% 3 = %d" % (s["g0"] % TW_APERIOD)))
            if k:
                p = segs[k - 1]
                out.add(("between segments", "next plane" if p["plane"] != s["plane"] else "next strip" if p["x0"] != s["x0"] else "same strip"))
            for g, rmask, c_lo, c_hi, st in s["steps"]:
                out.add(("c_lo", c_lo))
                out.add(("c_hi", "full" if c_hi == 32 else "ragged"))
                out.add(("rmask", rmask))
                if st:
                    v0, v1, vx = st
                    out.add(("store", "index %% 5 = %d" % (g % TW_BPERIOD), "folded" if s["fold"] else "single", "rows %d..%d" % (v0, v1),
                             "full" if vx == tw.SW else "ragged"))
                    if a_ring:
                        out.add(("store, A-ring", "index %% 3 = %d" % (g % TW_APERIOD), "rows %d..%d" % (v0, v1)))
    busy = sum(1 for s in lists if s)
    out.add(("launch", "every workgroup busy" if busy == GRID else "some workgroups idle"))
    return out


def carry_starts(uva, h, w, tile, border, planner="default"):
    """where a slip in the rows a segment needs from ABOVE it would show: the segments that start on the state another one
    left (a second or later segment of a list) or with six rows in the middle of a plane -> [(plane, x0, r0, strip width)]"""
    out = []
    for segs in trunkw_lists(uva, h, w, tile, border, planner):
        for k, s in enumerate(segs):
            if s["r0"] > 0 and (k > 0 or s["six"]):
                out.append((s["plane"], s["x0"], s["r0"], min(tw.SW, s["pw"] - s["x0"])))
    return sorted(out)


# ------------------------------------------------------------------------------------------------------------------ trunk2
def trunk2_census(uva, h, w, tile, border, group="UVA_TRUNK_WINO=0"):
    with planner_env(group):
        steps, nsteps, planes, guard = t2.schedule(uva, h, w, tile, border, GRID)
    out = set()
    for b in range(GRID):
        n = int(nsteps[b])
        if not n:
            continue
        out.add(("list length", bucket(n, 4, 11)))
        prev, nseg, first = None, 0, None
        for g in range(n):
            a, bb = steps[b, g, :4], steps[b, g, 4:]
            pi, row, col = t2.locate(_off(a), planes, guard, int(a[3]))
            if col == int(planes[pi, 2]) - 1:
                row, col = row + 1, -1
            yA, x0 = row, col + 1
            rmask, c_lo, c_hi, narrow = (int(a[1]) >> 8) & 15, (int(a[1]) >> 12) & 63, (int(a[1]) >> 18) & 63, (int(a[1]) >> 25) & 1
            # (the two rings turn independently: a class per ring, not per pair of phases)
            phase, phase3 = "index %% 4 = %d" % (g % T2_PERIODS[0]), "index %% 3 = %d" % (g % T2_PERIODS[1])
            if prev != (pi, x0, yA - 4):
                nseg += 1
                out.add(("segment start", "top of plane" if yA == -1 else "mid-plane", phase, "narrow" if narrow else "wide", "rmask %d" % rmask))
                out.add(("segment start, row ring", "top of plane" if yA == -1 else "mid-plane", phase3))
                if prev is not None:
                    out.add(("between segments", "next plane" if prev[0] != pi else "next strip" if prev[1] != x0 else "same strip"))
            prev = (pi, x0, yA)
            out.add(("c_lo", c_lo))
            out.add(("c_hi", "full" if c_hi == 32 else "ragged"))
            out.add(("rmask", rmask))
            if (int(bb[1]) >> 24) & 1:
                vy, vx = (int(bb[1]) >> 8) & 7, (int(bb[1]) >> 11) & 31
                out.add(("store", phase, "narrow" if narrow else "wide", "rows %d" % vy, "full" if vx == t2.SW else "ragged"))
                out.add(("store, row ring", phase3, "rows %d" % vy))
            else:
                out.add(("no store", phase))
                out.add(("no store, row ring", phase3))
        out.add(("segments per list", bucket(nseg, 2)))
    out.add(("launch", "every workgroup busy" if int((nsteps > 0).sum()) == GRID else "some workgroups idle"))
    return out


# ------------------------------------------------------------------------------------------------------------------ trunk_kernel
def trunk_census(uva, h, w, tile, border):
    """trunk_kernel (UVA_TRUNK_FUSION=0) walks 4-row work tiles of 32 columns, plane after plane, XCD x the x-th eighth of
    them and a workgroup two tiles per turn through TRUNK_SLOTS slots: no state but the slots"""
    _, _, planes, _ = tw.schedule(uva, h, w, tile, border, GRID)
    out, ntiles = set(), 0
    for ph, pw, pitch, _ in planes:
        ph, pw = int(ph), int(pw)
        ntiles += -(-ph // 4) * -(-pw // 32)
        out.add(("tile rows", "full" if ph % 4 == 0 else "ragged"))
        out.add(("tile columns", "full" if pw % 32 == 0 else "ragged"))
    per_xcd = -(-ntiles // 8)
    turns = -(-per_xcd // (2 * (GRID // 8)))
    out.add(("turns per workgroup", bucket(turns, 1)))          # (a lap of the TRUNK_SLOTS slots: 3072 tiles, see the coverage test)
    out.add(("planes", bucket(len(planes), 1)))
    return out


# ------------------------------------------------------------------------------------------------------------------ 1x rows
def rows_census(h, w, frames=1, kernel="sub10"):
    """sub10_kernel / sub10_kernel16 (one frame, or `frames` of them through the batch hook) and sub5_kernel"""
    if kernel == "sub5":
        rows, nrows, _ = s5.rows_for(h, w, GRID)
        nl, unit = s5.NL, s5.PAIRW
    else:
        rows, nrows, _ = s10.rows_for_batch(h, w, frames, GRID) if frames > 1 else s10.rows_for(h, w, GRID)
        nl, unit = s10.NL, s10.VALID
    nunits = -(-w // unit)
    out = set()
    for b in range(GRID):
        r = rows[b, :nrows[b]]
        if not len(r):
            continue
        out.add(("list length", bucket(len(r), 0, 24, 159)))
        i, nseg, frames_seen = 0, 0, set()
        while i < len(r):
            j = i
            while j + 1 < len(r) and r[j + 1, 0] == r[j, 0] + 1 and r[j + 1, 1] == r[i, 1] and (r[j + 1, 2] >> 8) == (r[i, 2] >> 8):
                j += 1
            seg = r[i:j + 1]
            nseg += 1
            frames_seen.add(int(seg[0, 2]) >> 8)
            written = int((seg[:, 2] & 1).sum())
            out.add(("written rows per segment", bucket(written, 0, ROW_RING, RES_ROWS)))
            u = (int(seg[0, 1]) + nl) // unit
            out.add(("strip", "only" if nunits == 1 else "first" if u == 0 else "last" if u == nunits - 1 else "interior"))
            if u == nunits - 1:
                out.add(("last strip", "ragged" if w % unit else "full"))
            y0, y1 = int(seg[nl, 0]), int(seg[len(seg) - 1 - nl, 0]) + 1
            out.add(("segment", "top of frame" if y0 == 0 else "below the top", "to the bottom" if y1 == h else "ends above the bottom"))
            for k in range(len(seg)):
                out.add(("row", "index %% 4 = %d" % ((i + k) % ROW_RING), "written" if seg[k, 2] & 1 else "warm-up above" if k < nl else "warm-up below"))
            out.add(("segment start", "index %% 4 = %d" % (i % ROW_RING), "first of list" if i == 0 else "later"))
            i = j + 1
        out.add(("segments per list", bucket(nseg, 2)))
        if frames > 1:
            out.add(("list", "crosses into the next frame" if len(frames_seen) > 1 else "inside one frame"))
    out.add(("launch", "every workgroup busy" if int((nrows > 0).sum()) == GRID else "some workgroups idle"))
    return out


# ------------------------------------------------------------------------------------------------------------------ per kernel
def kernel_of(key, route, env):
    """-> (kernel group, planner switch) of a frame-route case (key "2x" / "4x" / "1x", route "u8" / "u16" / "batch", env
    (name, value) or None).  A switch that selects another kernel or another instantiation of one has a census of its own;
    UVA_TW_SIX and UVA_TW_FOLD only change the lists the SAME trunkw_kernel walks, UVA_HEAD_PERSIST does not touch the trunk:
    their cases count for the default kernel, with their own lists."""
    name, val = env or (None, None)
    if key == "1x":
        if name == "UVA_SUB10":
            return "pair24_kernel", "default"
        if name == "UVA_SUB5":
            return "sub5_kernel", "default"
        return ("sub10_kernel16" if route == "u16" else "sub10_kernel"), "default"
    if name in ("UVA_TW_SIX", "UVA_TW_FOLD"):
        return "trunkw_kernel", "%s=%s" % (name, val)
    return {"UVA_TRUNK_WINO": "trunk2_kernel", "UVA_TRUNK_FUSION": "trunk_kernel", "UVA_TW_CARRY": "trunkw_kernel, UVA_TW_CARRY=0",
            "UVA_TW_ACT16": "trunkw_kernel, UVA_TW_ACT16=0"}.get(name, "trunkw_kernel"), "default"


def census(uva, kernel, h, w, tile=0, border=0, frames=1, planner="default"):
    """the classes kernel group `kernel` visits on a geometry, its lists built under the planner switch `planner`"""
    if kernel.startswith("trunkw_kernel"):
        return trunkw_census(uva, h, w, tile, border, "UVA_TW_CARRY=0" if "CARRY" in kernel else planner)
    if kernel == "trunk2_kernel":
        return trunk2_census(uva, h, w, tile, border)
    if kernel == "trunk_kernel":
        return trunk_census(uva, h, w, tile, border)
    if kernel == "pair24_kernel":       # 8-row work tiles of 32 columns, two per turn, no state between tiles
        return {("tile rows", "full" if h % 8 == 0 else "ragged"), ("tile columns", "full" if w % 32 == 0 else "ragged"),
                ("turns per workgroup", bucket(-(-(-(-h // 8) * -(-w // 32)) // (2 * GRID)), 1, 2))}
    return rows_census(h, w, frames, "sub5" if kernel == "sub5_kernel" else "sub10")


def workload_census(uva, name, kernel):
    """the census of workload `name` for `kernel`, or None where the workload never runs that kernel (the batch: u8 only)"""
    net, h, w, tile, border, frames = WORKLOADS[name]
    if (net == "1x") != (kernel in ROW_KERNELS) or (frames > 1 and kernel != "sub10_kernel"):
        return None
    return census(uva, kernel, h, w, tile, border, frames)
