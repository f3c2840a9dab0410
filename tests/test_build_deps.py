"""The build list against the sources: upscale_video_amd/build.py rebuilds an object only when its source or one of the
headers listed for it in SOURCES changed, so a header that a source reaches through `#include "..."` and that the list
lacks means a stale object after an edit of that header."""
import os
import re

import pytest

from upscale_video_amd import build

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)
ROOTS = [build.CSRC, os.path.normpath(os.path.join(build.CSRC, "..", "..", "include"))]


def reached(path, seen):
    """every project header `path` includes, directly or not -> seen (absolute paths)"""
    with open(path) as f:
        text = f.read()
    for name in INCLUDE.findall(text):
        dep = os.path.normpath(os.path.join(os.path.dirname(path), name))
        assert os.path.exists(dep), "%s includes %s, which does not exist" % (path, name)
        assert any(dep.startswith(r + os.sep) for r in ROOTS), "%s includes %s from outside csrc/ and include/" % (path, name)
        if dep not in seen:
            seen.add(dep)
            reached(dep, seen)
    return seen


@pytest.mark.parametrize("src", sorted(build.SOURCES))
def test_every_header_a_source_reaches_is_in_its_list(src):
    listed = {os.path.normpath(os.path.join(build.CSRC, d)) for d in build.SOURCES[src]}
    missing = reached(os.path.join(build.CSRC, src), set()) - listed
    assert not missing, "build.SOURCES[%r] lacks %s" % (src, sorted(os.path.relpath(m, build.CSRC) for m in missing))


def test_every_kernel_header_is_compiled_by_one_source():
    """A header that defines kernels (`__global__`) belongs to one translation unit.  Template kernels reached by two
    sources would still link -- and be compiled twice, minutes each, without anyone noticing."""
    users = {}
    for src in build.SOURCES:
        for dep in reached(os.path.join(build.CSRC, src), set()):
            users.setdefault(dep, []).append(src)
    kernel_headers = []
    for name in sorted(os.listdir(build.CSRC)):
        path = os.path.join(build.CSRC, name)
        if name.endswith(".h"):
            with open(path) as f:
                if "__global__" in f.read():
                    kernel_headers.append(path)
    assert kernel_headers, "no kernel header found under csrc/: the test looks in the wrong place"
    for path in kernel_headers:
        assert len(users.get(path, [])) == 1, "%s is reached by %s" % (os.path.relpath(path, build.CSRC), sorted(users.get(path, [])))


def test_every_source_file_is_built():
    on_disk = {f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".cpp"))}
    assert on_disk == set(build.SOURCES)
