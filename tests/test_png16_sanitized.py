"""The PNG reader on 16-bit files under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own:
tests/host/png16_check.cpp and csrc/uva_pngread.cpp compiled by the host compiler -- no HIP runtime, nothing loaded into this
process, no GPU -- and run as a child (the manner of tests/test_plan_sanitized.py)."""
import os
import subprocess

import pytest

from test_plan_sanitized import FLAGS, ROOT, host_compilers


def test_png16_check_runs_clean_under_asan_and_ubsan(tmp_path):
    compilers = host_compilers()
    if not compilers:
        pytest.skip("no host C++ compiler (g++ or ROCm's clang++)")
    exe = str(tmp_path / "png16_check")
    srcs = [os.path.join(ROOT, "tests", "host", "png16_check.cpp"), os.path.join(ROOT, "upscale_video_amd", "csrc", "uva_pngread.cpp")]
    for cc in compilers:        # (the second only where the first lacks its sanitizer runtimes)
        r = subprocess.run(cc + FLAGS + srcs + ["-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.startswith("png16_check:") and r.stdout.rstrip().endswith(": ok")
