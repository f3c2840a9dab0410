"""The planner's tables against the digests of a known commit: tests/golden/plan_digests.json holds one SHA-256 per case over
everything the schedule hooks return (tools/plan_digests.py: step lists of trunk2_kernel and trunkw_kernel over the schedule
tests' geometries, two grids and the UVA_TW_SIX / UVA_TW_FOLD settings; row lists of sub10_kernel and sub5_kernel), written
from a build of the commit the file names.  The library built from this tree must reproduce every entry, refusals included:
a change to csrc/uva_plan.cpp that moves one schedule word fails here, and one that means to regenerates the file."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_reproduces_every_recorded_digest(uva):
    spec = importlib.util.spec_from_file_location("plan_digests", os.path.join(ROOT, "tools", "plan_digests.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(tool.GOLDEN) as f:
        golden = json.load(f)
    assert len(golden["commit"]) == 40
    want = golden["digests"]
    assert len(want) == 2 * len(tool.TRUNK_GEOMETRIES) * len(tool.GRIDS) * len(tool.SIX) * len(tool.FOLD) \
        + len(tool.SUB_GEOMETRIES) * len(tool.GRIDS) * (len(tool.SUB10_FRAMES) + 1)
    got = tool.compute()
    assert sorted(got) == sorted(want)
    wrong = [k for k in sorted(want) if got[k] != want[k]]
    assert not wrong, "%d of %d cases differ from commit %s: %s" % (len(wrong), len(want), golden["commit"][:12], wrong[:8])
