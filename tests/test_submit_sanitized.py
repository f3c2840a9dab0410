"""The pipelined host route's plan under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own:
tests/host/submit_check.cpp, csrc/uva_submit.cpp and csrc/uva_crop_host.cpp compiled by the host compiler -- no HIP runtime,
nothing loaded into this process, no GPU -- and run as a child, as tests/test_plan_sanitized.py does with the frame planner."""
from test_plan_sanitized import FLAGS
from test_submit_plan import build_and_run


def test_submit_check_runs_clean_under_asan_and_ubsan(tmp_path):
    r = build_and_run(tmp_path, FLAGS, strip=False)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
