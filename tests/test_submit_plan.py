"""The pipelined host route's plan alone: tests/host/submit_check.cpp, csrc/uva_submit.cpp and csrc/uva_crop_host.cpp compiled
by the host compiler -- no HIP runtime, no kernel object, no GPU -- and run as a child.  The program holds submit_plan to
known answers worked out from the frame layouts and to the relations between a plan's members over a seeded sweep
(formats x bits x scales x odd and even sizes x window or none x sized or not).  That it links from these two sources is also
the proof that the plan needs nothing of the device."""
import os
import subprocess

import pytest

from test_plan_sanitized import ROCM, ROOT, host_compilers

SOURCES = [os.path.join(ROOT, "tests", "host", "submit_check.cpp"),
           os.path.join(ROOT, "upscale_video_amd", "csrc", "uva_submit.cpp"),
           os.path.join(ROOT, "upscale_video_amd", "csrc", "uva_crop_host.cpp")]
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include")]


def build_and_run(tmp_path, flags, strip):
    """submit_check built with `flags` by the first host compiler that can (strip: the compilers' own sanitizer switches
    are dropped), run once -> the finished process"""
    compilers = host_compilers()
    if not compilers:
        pytest.skip("no host C++ compiler (g++ or ROCm's clang++)")
    exe = str(tmp_path / "submit_check")
    for cc in compilers:        # (the second only where the first cannot build it)
        if strip:
            cc = [a for a in cc if not a.startswith("-static-lib")]
        r = subprocess.run(cc + flags + SOURCES + ["-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.startswith("submit_check:") and r.stdout.rstrip().endswith(": ok")
    return r


def test_submit_plan_known_answers_and_relations(tmp_path):
    build_and_run(tmp_path, FLAGS, strip=True)
