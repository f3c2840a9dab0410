"""`-m n=K` at --bit-depth 16 measured on the MI355X, every figure beside the 8-bit stage's taken in the
same call on the same box.  The yardstick is the 8-bit stage; the 16-bit form stages twice the LDS bytes and sums in 64 bits.

    host [reps]     uva_denoise_u16 against uva_denoise_u8 on a synthetic 1080p frame, K = 10 and K = 3, host to host and
                    synchronous (H2D, Lab, two NLM passes, Lab, D2H), alternating: median ms per frame.  The loop `kernel` profiles.
    kernel          `host` as a child under rocprofv3 --kernel-trace --stats: time per launch of nlm_plane16<1>, nlm_plane16<2>,
                    nlm_bgr2lab16 and nlm_lab2bgr16 against the 8-bit kernels' on those frames.
    route [frames]  p010le -> p010le -s 2 at 1080p, file to file in a RAM disk, -g 0: --bit-depth 16 -m n=3 against the same at 8
                    bits and against --bit-depth 16 without n=3, every run a child process of its own (frames/s over the frames a run of n has more than a run of n / 2).
    all [--out DIR] the three as child processes, each under a time limit of its own, stopping at the first that fails; their
                    output goes to DIR/{host,kernel,route}.txt (default profiles/denoise16).
"""
import argparse
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = {"host": 180, "kernel": 300, "route": 420}     # seconds per step of `all`


def frames_1080p():
    """-> (u8 frame, u16 frame): synth.synthetic_frame with grain; the 16-bit one is the same picture with 16-bit grain"""
    import numpy as np
    from upscale_video_amd.synth import synthetic_frame
    rng = np.random.default_rng(16)
    clean = synthetic_frame(1080, 1920, seed=2).astype(np.float64)
    grain = rng.normal(0, 3.0, clean.shape)
    return (np.clip(np.rint(clean + grain), 0, 255).astype(np.uint8),
            np.clip(np.rint((clean + grain) * 257.0), 0, 65535).astype(np.uint16))


def host(reps=20):
    import numpy as np
    from upscale_video_amd import _lib
    L = _lib.load()
    f8, f16 = frames_1080p()
    o8, o16 = np.empty_like(f8), np.empty_like(f16)
    h, w = f8.shape[:2]

    def run8(K):
        _lib.check(L.uva_denoise_u8(0, f8.ctypes.data, h, w, w * 3, o8.ctypes.data, w * 3, float(K), float(K)))

    def run16(K):
        _lib.check(L.uva_denoise_u16(0, f16.ctypes.data, h, w, w * 6, o16.ctypes.data, w * 6, float(K), float(K)))

    for K in (10, 3):
        for _ in range(3):
            run8(K)
            run16(K)
        t8, t16 = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            run8(K)
            t1 = time.perf_counter()
            run16(K)
            t2 = time.perf_counter()
            t8.append(t1 - t0)
            t16.append(t2 - t1)
        m8, m16 = statistics.median(t8) * 1e3, statistics.median(t16) * 1e3
        print(f"1920x1080, K = {K:2d}, host to host, synchronous: uva_denoise_u8 median {m8:6.2f} ms (best {min(t8) * 1e3:6.2f}), "
              f"uva_denoise_u16 median {m16:6.2f} ms (best {min(t16) * 1e3:6.2f}); 16 / 8 = {m16 / m8:.2f}", flush=True)
        d = np.abs((o16 >> 8).astype(int) - o8.astype(int))
        print(f"    (results: 16-bit >> 8 against 8-bit, max {d.max()} levels, mean {d.mean():.3f})", flush=True)


def kernel():
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    with tempfile.TemporaryDirectory(prefix="uva_denoise16_") as d:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable,
                            os.path.abspath(__file__), "host", "20"], cwd=ROOT, capture_output=True, text=True, timeout=LIMITS["kernel"] - 20)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-2000:])
            sys.exit(r.returncode)
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                rows += [row for row in csv.DictReader(f) if "nlm_" in row.get("Name", "")]
    if not rows:
        sys.exit("no nlm_* kernels in the trace")
    print("rocprofv3 --kernel-trace --stats over 46 frames of each depth (1920x1080; K = 10 and K = 3 together):")
    avg = {}
    for row in sorted(rows, key=lambda r: r["Name"]):
        name = row["Name"].split("(")[0].replace("void ", "").replace("uva::", "")
        avg[name] = float(row["AverageNs"])
        print(f"  {name:24s} calls {row['Calls']:>4s}  average {float(row['AverageNs']) / 1e3:8.1f} us  min {float(row['MinNs']) / 1e3:8.1f}  "
              f"max {float(row['MaxNs']) / 1e3:8.1f}")
    for k16, k8 in (("nlm_plane16<1>", "nlm_plane<1>"), ("nlm_plane16<2>", "nlm_plane<2>"), ("nlm_bgr2lab16", "nlm_bgr2lab"),
                    ("nlm_lab2bgr16", "nlm_lab2bgr")):
        if k16 in avg and k8 in avg:
            print(f"  {k16} / {k8} = {avg[k16] / avg[k8]:.2f}")
    s8 = sum(v for k, v in avg.items() if "16" not in k)
    s16 = sum(v for k, v in avg.items() if "16" in k)
    if s8 and s16:
        print(f"  the four kernels of a frame: 8-bit {s8 / 1e3:.1f} us, 16-bit {s16 / 1e3:.1f} us; 16 / 8 = {s16 / s8:.2f}")


def route_one(depth, denoise, n):
    import numpy as np
    from upscale_video_amd import ncnn, rawvideo
    _, f16 = frames_1080p()
    h, w = f16.shape[:2]
    p010 = ncnn.convert_pix(f16, h, w, "bgr48le", "p010le", bit_depth=16)
    base = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        src, dst = os.path.join(base, "in.p010"), os.path.join(base, "out.p010")
        with open(src, "wb") as f:
            for _ in range(n):
                f.write(memoryview(np.ascontiguousarray(p010)).cast("B"))
        argv = ["-i", src, "-o", dst, "-W", str(w), "-H", str(h), "-s", "2", "--in-pix-fmt", "p010le", "--out-pix-fmt", "p010le"]
        argv += ["--bit-depth", "16"] if depth == 16 else []
        argv += ["-m", "n=3"] if denoise else []
        rawvideo.main(argv + ["--frames", "8"])                       # warm-up: code objects, page cache
        times = []
        for k in (n // 2, n):                                         # every run loads its nets anew: the rate is taken over the
            t = time.perf_counter()                                   # frames the second run has more than the first
            rawvideo.main(argv + ["--frames", str(k)])
            times.append(time.perf_counter() - t)
        rate = (n - n // 2) / (times[1] - times[0])
    finally:
        shutil.rmtree(base, ignore_errors=True)
    print(f"--bit-depth {depth:2d} {'-m n=3' if denoise else '      '}: p010le 1080p -> p010le 2160p, -s 2, -g 0: {rate:6.1f} frames/s ({n // 2} frames in {times[0]:.2f} s, {n} in {times[1]:.2f} s)",
          flush=True)


def route(n=128):
    for depth, denoise in ((16, 1), (8, 1), (16, 0), (16, 1), (8, 1), (16, 0)):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "route-one", str(depth), str(denoise), str(n)], cwd=ROOT, timeout=120)
        if r.returncode != 0:
            sys.exit(r.returncode)


def run_all(out):
    os.makedirs(out, exist_ok=True)
    for step in ("host", "kernel", "route"):
        path = os.path.join(out, step + ".txt")
        with open(path, "w") as f:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), step], stdout=f, stderr=subprocess.STDOUT, cwd=ROOT,
                                   timeout=LIMITS[step])
                rc = r.returncode
            except subprocess.TimeoutExpired:
                rc = 124
        print(open(path).read(), end="", flush=True)
        if rc != 0:                      # nothing more is started on the GPU after a step that failed or ran out of time
            print(f"{step}: exit status {rc}; stopping here", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["host", "kernel", "route", "route-one", "all"])
    ap.add_argument("args", nargs="*", type=int)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise16"))
    a = ap.parse_args()
    if a.what == "all":
        sys.exit(run_all(a.out))
    if a.what == "route-one":
        route_one(*a.args)
    else:
        {"host": host, "kernel": kernel, "route": route}[a.what](*a.args)
