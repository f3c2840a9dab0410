#!/usr/bin/env python3
"""One SHA-256 per case over everything the planner's debug hooks return (csrc/uva_plan.cpp through uva_debug_trunk2_schedule,
uva_debug_trunkw_schedule, uva_debug_sub10_rows_batch, uva_debug_sub5_rows) of the library UVA_LIB_PATH selects: a change of
one schedule word changes a digest.  tests/golden/plan_digests.json holds the digests of a known commit and
tests/test_plan_digests.py holds the tree's library to them; a change that alters a schedule on purpose regenerates the file
from its own build and shows the diff.
    python tools/plan_digests.py                      # JSON to stdout
    UVA_LIB_PATH=<lib of commit C> python tools/plan_digests.py --write --commit C"""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_digests.json")

# every (h, w, tile, border) of tests/test_trunkw_schedule.py and tests/test_trunk2_schedule.py, and three of tools/lib_identity.py
TRUNK_GEOMETRIES = [(1080, 1920, 960, 10), (2160, 3840, 960, 10), (1080, 1920, 0, 0), (256, 256, 960, 10), (24, 40, 0, 0),
                    (70, 75, 32, 10), (5, 3, 0, 0), (131, 61, 64, 10), (1, 1, 0, 0), (960, 960, 0, 0), (96, 128, 64, 10),
                    (540, 960, 240, 10), (33, 1000, 0, 0), (1000, 9, 0, 0)]
GRIDS = [8, 256]
SIX = [None, "0", "1"]          # UVA_TW_SIX
FOLD = [None, "0", "14"]        # UVA_TW_FOLD
SUB_GEOMETRIES = [(1080, 1920), (720, 1280), (61, 59), (1, 1), (9, 1000), (1000, 9), (2160, 3840)]
SUB10_FRAMES = [1, 2, 4, 8]


def _sha(*arrays):
    import numpy as np
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).astype(a.dtype.newbyteorder("<"), copy=False).tobytes())
    return h.hexdigest()


def trunk_digest(L, kind, h, w, tile, border, grid):
    """(plane_info, nplanes, guard, stride, nsteps, words) of one step-list hook, or the refusal"""
    import numpy as np
    fn = getattr(L, "uva_debug_%s_schedule" % kind)
    need = ctypes.c_size_t()
    stride, nplanes, guard = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
    pinfo = np.zeros(64 * 4, np.int64)
    nsteps = np.zeros(grid, np.int32)
    fn(h, w, tile, border, grid, None, 0, need, None, stride, pinfo.ctypes.data, 64, nplanes, guard)
    words = np.zeros(need.value, np.uint32)
    if fn(h, w, tile, border, grid, words.ctypes.data, words.size, need, nsteps.ctypes.data, stride, pinfo.ctypes.data, 64, nplanes, guard):
        return "refused: " + L.uva_last_error().decode()
    return _sha(pinfo[:4 * nplanes.value], np.array([nplanes.value, guard.value, stride.value], np.int64), nsteps, words)


def rows_digest(L, kind, h, w, frames, grid):
    """(stride, nrows, words) of one row-list hook, or the refusal"""
    import numpy as np
    if kind == "sub10":
        def fn(*a):
            return L.uva_debug_sub10_rows_batch(h, w, frames, grid, *a)
    else:
        def fn(*a):
            return L.uva_debug_sub5_rows(h, w, grid, *a)
    need, stride = ctypes.c_size_t(), ctypes.c_int()
    nrows = np.zeros(grid, np.int32)
    fn(None, 0, need, None, stride)
    words = np.zeros(need.value, np.uint32)
    if fn(words.ctypes.data, words.size, need, nrows.ctypes.data, stride):
        return "refused: " + L.uva_last_error().decode()
    return _sha(np.array([stride.value], np.int64), nrows, words)


def compute():
    """{case name: digest or refusal} of the loaded library; the planner's switches are set per case and put back"""
    os.environ["UVA_DEBUG_SWITCHES"] = "1"          # (the library honours its switches only under this opt-in, read once)
    sys.path.insert(0, ROOT)
    from upscale_video_amd import _lib
    L = _lib.load()
    switches = ("UVA_TW_SIX", "UVA_TW_FOLD", "UVA_T2_NARROW")
    saved = {k: os.environ.pop(k, None) for k in switches}
    out = {}
    try:
        for six in SIX:
            for fold in FOLD:
                for k, v in (("UVA_TW_SIX", six), ("UVA_TW_FOLD", fold)):
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
                for kind in ("trunk2", "trunkw"):
                    for (h, w, tile, border) in TRUNK_GEOMETRIES:
                        for grid in GRIDS:
                            name = "%s %dx%d tile %d border %d grid %d six %s fold %s" % (kind, h, w, tile, border, grid, six or "-", fold or "-")
                            out[name] = trunk_digest(L, kind, h, w, tile, border, grid)
        for k in switches:
            os.environ.pop(k, None)
        for (h, w) in SUB_GEOMETRIES:
            for grid in GRIDS:
                for frames in SUB10_FRAMES:
                    out["sub10 %dx%d frames %d grid %d" % (h, w, frames, grid)] = rows_digest(L, "sub10", h, w, frames, grid)
                out["sub5 %dx%d grid %d" % (h, w, grid)] = rows_digest(L, "sub5", h, w, 1, grid)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return out


if __name__ == "__main__":
    doc = {"commit": sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else None, "digests": compute()}
    if "--write" in sys.argv:
        if not doc["commit"]:
            sys.exit("--write needs --commit <id of the commit the library was built from>")
        with open(GOLDEN, "w") as f:
            json.dump(doc, f, indent=0, sort_keys=True)
            f.write("\n")
        print("%d digests of commit %s -> %s" % (len(doc["digests"]), doc["commit"], GOLDEN))
    else:
        print(json.dumps(doc, indent=0, sort_keys=True))
