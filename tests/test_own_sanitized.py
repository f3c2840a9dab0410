"""The handle types of csrc/uva_own.h under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own:
tests/host/own_check.cpp compiled by the host compiler -- the header's core includes no HIP header, nothing is loaded into
this process, no GPU -- and run as a child.  What the program shows is listed in it.  No ROCm include path is given: that it
builds is the proof that the core is free of HIP."""
import os
import subprocess

from test_plan_sanitized import ROOT, host_compilers

import pytest

FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_own_check_runs_clean_under_asan_and_ubsan(tmp_path):
    compilers = host_compilers()
    if not compilers:
        pytest.skip("no host C++ compiler (g++ or ROCm's clang++)")
    exe = str(tmp_path / "own_check")
    src = os.path.join(ROOT, "tests", "host", "own_check.cpp")
    for cc in compilers:        # (the second only where the first lacks its sanitizer runtimes)
        r = subprocess.run(cc + FLAGS + [src, "-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.startswith("own_check:") and r.stdout.rstrip().endswith(": ok")

