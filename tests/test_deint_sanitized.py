"""The deinterlacer's host half under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own:
tests/host/deint_check.cpp and csrc/uva_deint_host.cpp compiled by the host compiler -- no HIP runtime, nothing loaded into this
process, no GPU -- and run as a child.  That uva_deint_host.cpp builds this way is also the proof that the plane table, the
refusals and the scalar rule are host-only code."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
         "-I" + os.path.join(ROCM, "include")]


def host_compilers():
    out = []
    gxx = shutil.which("g++")
    if gxx:
        # (the runtimes linked into the program: it then runs whatever else the environment preloads into every process)
        out.append([gxx, "-static-libasan", "-static-libubsan"])
    clang = shutil.which("clang++") or os.path.join(ROCM, "llvm", "bin", "clang++")
    if os.path.exists(clang):
        out.append([clang, "-x", "c++"])
    return out


def test_deint_check_runs_clean_under_asan_and_ubsan(tmp_path):
    compilers = host_compilers()
    if not compilers:
        pytest.skip("no host C++ compiler (g++ or ROCm's clang++)")
    exe = str(tmp_path / "deint_check")
    srcs = [os.path.join(ROOT, "tests", "host", "deint_check.cpp"), os.path.join(ROOT, "upscale_video_amd", "csrc", "uva_deint_host.cpp")]
    for cc in compilers:        # (the second only where the first lacks its sanitizer runtimes)
        r = subprocess.run(cc + FLAGS + srcs + ["-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.startswith("deint_check:") and r.stdout.rstrip().endswith(": ok")
