"""16 bits through the 1x net measured: sub10_kernel16 beside sub10_kernel, and the `-m a` chain's rate.

    kernel          one 1080p frame resident in HBM through sub10_kernel (u8) and sub10_kernel16 (u16) in turn in ONE process,
                    timed by the library's own events (uva_net_kernel_stats kinds 1 and 3): ms per launch of each.
    launches [N]    N launches of each kernel on 1080p frames and nothing else: the child that `bytes` runs under the profiler.
    bytes           FETCH_SIZE and WRITE_SIZE of both kernels per 1080p launch: `launches` under rocprofv3, one counter pass
                    each with kernel tracing only.  From the byte counts alone the u16 kernel moves 12 B per pixel where the u8
                    kernel moves 6, plus whatever part of the tail's residual re-read misses L2 / MALL: this step says how much.
    route [frames]  python -m upscale_video_amd.rawvideo -m a -s 2, p010le in and out, 1080p -> 2160p, pipe -> pipe, at
                    --bit-depth 16 and at 8, twice each (frames held in /dev/shm; rate = (frames - 1) / (wall - wall of a
                    1-frame run)).
    all [--out DIR] kernel, bytes and route as child processes, each under a time limit of its own, stopping at the first that
                    fails; their output goes to DIR/{kernel,bytes,route}.txt (default profiles/sub10_u16).
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
from upscale_video_amd import ncnn                      # noqa: E402
from upscale_video_amd.synth import synthetic_frame      # noqa: E402

H, W = 1080, 1920
LIMITS = {"kernel": 180, "bytes": 400, "route": 600}     # seconds per step of `all`


def _net_and_frames():
    import ctypes
    import numpy as np
    import torch
    from upscale_video_amd import _lib
    from upscale_video_amd.rawvideo import MODEL_FILES, load_net
    net = load_net(MODEL_FILES[1], 0, os.path.join(ROOT, "models"))
    net.enable_u16_1x()
    img = synthetic_frame(H, W, seed=3)
    d8 = torch.from_numpy(img).cuda()
    x16 = (img.astype(np.uint16) << 8) | synthetic_frame(H, W, seed=4)        # (16 bits of content; torch takes it as int16 words)
    d16 = torch.from_numpy(x16.view(np.int16)).cuda()
    o8, o16 = torch.empty_like(d8), torch.empty_like(d16)
    torch.cuda.synchronize()
    L = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731

    def run8():
        _lib.check(L.uva_net_process_u8_device(net._h, p(d8), H, W, W * 3, p(o8), W * 3, 0, 0))

    def run16():
        _lib.check(L.uva_net_process_u16_device(net._h, p(d16), H, W, W * 6, p(o16), W * 6, 0, 0))
    return net, run8, run16


def kernel(reps=100):
    net, run8, run16 = _net_and_frames()
    for _ in range(10):
        run8(); run16()
    net.synchronize()
    for block in range(3):
        net.set_profiling(True)
        for _ in range(reps):
            run8(); run16()
        net.synchronize()
        (n8, ms8), (n16, ms16) = net.kernel_stats(1), net.kernel_stats(3)
        net.set_profiling(False)
        assert n8 == reps and n16 == reps, (n8, n16)
        print(f"block {block}: {W}x{H}  sub10_kernel (u8) {ms8 / n8 * 1e3:7.1f} us per launch   sub10_kernel16 (u16) {ms16 / n16 * 1e3:7.1f} us "
              f"per launch   u16 / u8 = {ms16 / ms8:.3f}   ({reps} launches each, alternating)", flush=True)


def launches(n=6):
    net, run8, run16 = _net_and_frames()
    for _ in range(n):
        run8()
    for _ in range(n):
        run16()
    net.synchronize()


def bytes_():
    prof = shutil.which("rocprofv3")
    if not prof:
        print("rocprofv3 not found: bytes per launch not measured", flush=True)
        return 1
    tmp = tempfile.mkdtemp(prefix="s10u16_")
    try:
        med = {}
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, counter)
            r = subprocess.run([prof, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", d, "-o", "p", "--",
                                sys.executable, os.path.abspath(__file__), "launches"], cwd=ROOT, stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, timeout=180)
            if r.returncode != 0:
                print(r.stdout.decode(errors="replace")[-2000:])
                return r.returncode
            v = {}
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if "sub10_kernel" in row["Kernel_Name"] and row["Counter_Name"] == counter:
                        k = ("sub10_kernel16" if "sub10_kernel16" in row["Kernel_Name"] else "sub10_kernel", row["Dispatch_Id"])
                        v[k] = v.get(k, 0.0) + float(row["Counter_Value"])
            for name in ("sub10_kernel", "sub10_kernel16"):
                vals = [x for (k, _), x in v.items() if k == name]
                med[(name, counter)] = (statistics.median(vals), len(vals)) if vals else (float("nan"), 0)
        px = H * W
        for name, bpp in (("sub10_kernel", 3), ("sub10_kernel16", 6)):
            (f, nf), (w, nw) = med[(name, "FETCH_SIZE")], med[(name, "WRITE_SIZE")]
            print(f"{name:15s} {W}x{H}: frame {px * bpp / 1e6:6.2f} MB in, the same out;  FETCH_SIZE {f:9.0f} KB = {f * 1024 / 1e6:6.2f} MB "
                  f"({f * 1024 / px:5.2f} B per pixel, median of {nf} launches);  WRITE_SIZE {w:9.0f} KB = {w * 1024 / 1e6:6.2f} MB "
                  f"({w * 1024 / px:5.2f} B per pixel, {nw} launches)", flush=True)
        print("(FETCH_SIZE counts what the L2 fetched from the fabric in KB; the u16 tail's residual re-read shows as fetch beyond "
              "6 B per pixel plus the strips' overlap)", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


def route(n=120):
    import numpy as np
    base = [sys.executable, "-m", "upscale_video_amd.rawvideo", "-W", str(W), "-H", str(H), "-s", "2", "-m", "a",
            "--in-pix-fmt", "p010le", "--out-pix-fmt", "p010le"]
    packed = [np.asarray(ncnn.convert_pix(synthetic_frame(H, W, seed=i), H, W, "bgr24", "p010le")).tobytes() for i in range(8)]
    src = "/dev/shm/uva_sub10_u16_in.p010"

    def wall(cmd, shell=False):
        t0 = time.perf_counter()
        subprocess.run(cmd, shell=shell, check=True, stderr=subprocess.DEVNULL, stdout=subprocess.DEVNULL if not shell else None, cwd=ROOT,
                       timeout=240)
        return time.perf_counter() - t0
    try:
        with open(src, "wb") as o:
            for i in range(n):
                o.write(packed[i % 8])
        rates = {8: [], 16: []}
        for bd in (8, 16, 8, 16):
            cmd = base + ["--bit-depth", str(bd)]
            t1 = wall(cmd + ["-i", src, "-o", "/dev/null", "--frames", "1"])
            tn = wall(f"cat {src} | {' '.join(cmd)} 2>/dev/null | cat > /dev/null", shell=True)
            rates[bd].append((n - 1) / (tn - t1))
            print(f"-m a -s 2 p010le {W}x{H} --bit-depth {bd:2d}: {n} frames in {tn:6.2f} s (start-up {t1:5.2f} s) = {rates[bd][-1]:7.1f} frames/s",
                  flush=True)
        r8, r16 = (sum(v) / len(v) for v in (rates[8], rates[16]))
        print(f"16 bits {r16:.1f} against 8 bits {r8:.1f} frames/s = {100 * (r16 / r8 - 1):+.1f} %", flush=True)
    finally:
        if os.path.exists(src):
            os.remove(src)


def run_all(out):
    os.makedirs(out, exist_ok=True)
    for step in ("kernel", "bytes", "route"):
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
    ap.add_argument("what", choices=["kernel", "launches", "bytes", "route", "all"])
    ap.add_argument("count", nargs="?", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sub10_u16"))
    a = ap.parse_args()
    if a.what == "all":
        sys.exit(run_all(a.out))
    if a.what == "bytes":
        sys.exit(bytes_())
    {"kernel": lambda: kernel(a.count or 100), "launches": lambda: launches(a.count or 6), "route": lambda: route(a.count or 120)}[a.what]()
