"""--skip-repeats measured: the frame-difference kernel alone, the host's wait in submit, and the route.

    kernel          uva_frame_diff_device at 1080p (bgr24, yuv420p, p010le) and 2160p (bgr24), equal frames (a repeat: two loads and
                    a test per 16 bytes) and unrelated ones (every sample differs).  A call is a memset, the kernel, a 32-byte
                    read-back and a wait; the same call on a 16 x 16 frame is that fixed part, the difference is the kernel's time
                    over the frame, set against the copy ceiling of DESIGN.md section 7.4 (6.29 TB/s) in bytes read per second.
    wait            Net.submit_pix yuv420p -> yuv420p, 1080p -> 2x, three frames in flight, no frame repeating its predecessor:
                    how long submit() takes with skipping off and with threshold 0 -- the difference is the one blocking point,
                    the comparison waiting its turn beside the net's persistent kernels -- as median and worst case.
    route [frames]  python -m upscale_video_amd.rawvideo pipe -> pipe, 1080p -> 2x, yuv420p both ways, on streams that show every
                    frame once, twice and three times, each with and without --skip-repeats, in this one process' children
                    (frames held in /dev/shm; rate = (frames - 1) / (wall - wall of a 1-frame run)).
    all [--out DIR] the three as child processes, each under a time limit of its own, stopping at the first that fails; their
                    output goes to DIR/{kernel,wait,route}.txt (default profiles/repeat).
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from upscale_video_amd import ncnn                      # noqa: E402
from upscale_video_amd.synth import synthetic_frame      # noqa: E402

COPY_CEILING = 6.29e12        # bytes per second: DESIGN.md section 7.4
LIMITS = {"kernel": 240, "wait": 240, "route": 600}     # seconds per step of `all`


def kernel():
    import numpy as np
    import torch
    rng = np.random.default_rng(1)

    def per_call(fmt, h, w, equal, reps=300):
        n = ncnn.pix_frame_bytes(fmt, h, w)
        a = torch.from_numpy(rng.integers(0, 256, n, dtype=np.uint8)).cuda()
        b = a.clone() if equal else torch.from_numpy(rng.integers(0, 256, n, dtype=np.uint8)).cuda()
        torch.cuda.synchronize()
        for _ in range(20):
            ncnn.frame_diff(a.data_ptr(), b.data_ptr(), fmt, h, w, device=True)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ncnn.frame_diff(a.data_ptr(), b.data_ptr(), fmt, h, w, device=True)
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), min(ts), n
    fixed, fixed_min, _ = per_call("bgr24", 16, 16, True)
    print(f"fixed part of a call (16 x 16 frame): median {fixed * 1e6:.1f} us, best {fixed_min * 1e6:.1f} us", flush=True)
    for fmt, h, w in (("bgr24", 1080, 1920), ("yuv420p", 1080, 1920), ("p010le", 1080, 1920), ("bgr24", 2160, 3840)):
        for equal in (True, False):
            med, best, n = per_call(fmt, h, w, equal)
            over = max(med - fixed, 1e-9)
            print(f"{fmt:8s} {w}x{h} {'equal    ' if equal else 'unrelated'}: call median {med * 1e6:7.1f} us (best {best * 1e6:7.1f}), over the "
                  f"fixed part {over * 1e6:7.1f} us = {2 * n / over / 1e12:5.2f} TB/s read, {100 * 2 * n / over / COPY_CEILING:5.1f} % of the "
                  f"copy ceiling", flush=True)


def wait(n=240):
    from upscale_video_amd.rawvideo import load_net
    h, w = 1080, 1920
    net = load_net("2x_Compact_Pretrain", 0, os.path.join(ROOT, "models"))
    frames = []
    for i in range(4):
        buf = ncnn.pix_empty("yuv420p", h, w, ncnn.pinned_empty)
        buf[...] = ncnn.convert_pix(synthetic_frame(h, w, seed=i), h, w, "bgr24", "yuv420p")
        frames.append(buf)
    outs = [ncnn.pix_empty("yuv420p", 2 * h, 2 * w, ncnn.pinned_empty) for _ in range(4)]
    for label, t in (("off", None), ("threshold 0", 0), ("off", None), ("threshold 0", 0)):
        net.set_skip_repeats(t)
        inflight, ts = [], []
        t_all = time.perf_counter()
        for i in range(n):
            if len(inflight) == 3:
                net.collect_u8(inflight.pop(0))
            t0 = time.perf_counter()
            inflight.append(net.submit_pix(frames[i % 4], h, w, "yuv420p", out=outs[i % 4], out_fmt="yuv420p", tile_size=960, border=10))
            ts.append(time.perf_counter() - t0)
        while inflight:
            net.collect_u8(inflight.pop(0))
        t_all = time.perf_counter() - t_all
        ts = ts[20:]
        print(f"submit() with skipping {label:11s}: median {statistics.median(ts) * 1e6:7.1f} us, worst {max(ts) * 1e6:8.1f} us, "
              f"{n / t_all:6.1f} frames/s, skip_stats {net.skip_stats()}", flush=True)


def route(n=240):
    h, w = 1080, 1920
    base = [sys.executable, "-m", "upscale_video_amd.rawvideo", "-W", str(w), "-H", str(h), "-s", "2",
            "--in-pix-fmt", "yuv420p", "--out-pix-fmt", "yuv420p"]
    packed = [ncnn.convert_pix(synthetic_frame(h, w, seed=i), h, w, "bgr24", "yuv420p").tobytes() for i in range(8)]
    src = "/dev/shm/uva_repeat_in.yuv"

    def wall(cmd, shell=False):
        t0 = time.perf_counter()
        subprocess.run(cmd, shell=shell, check=True, stderr=subprocess.DEVNULL, stdout=subprocess.DEVNULL if not shell else None, cwd=ROOT,
                       timeout=240)
        return time.perf_counter() - t0
    try:
        for shown in (1, 2, 3):
            with open(src, "wb") as o:
                for i in range(n):
                    o.write(packed[(i // shown) % 8])
            rates = {}
            for opt in ([], ["--skip-repeats"], [], ["--skip-repeats"]):
                cmd = base + opt
                t1 = wall(cmd + ["-i", src, "-o", "/dev/null", "--frames", "1"])
                tn = wall(f"cat {src} | {' '.join(cmd)} 2>/dev/null | cat > /dev/null", shell=True)
                rate = (n - 1) / (tn - t1)
                rates.setdefault(bool(opt), []).append(rate)
                print(f"every frame shown {shown}x, {'--skip-repeats' if opt else 'without      '}: {n} frames in {tn:6.2f} s (start-up {t1:5.2f} s) "
                      f"= {rate:7.1f} frames/s", flush=True)
            off, on = (sum(v) / len(v) for v in (rates[False], rates[True]))
            print(f"every frame shown {shown}x: {on:.1f} against {off:.1f} frames/s = {100 * (on / off - 1):+.1f} %", flush=True)
    finally:
        if os.path.exists(src):
            os.remove(src)


def run_all(out):
    os.makedirs(out, exist_ok=True)
    for step in ("kernel", "wait", "route"):
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
    ap.add_argument("what", choices=["kernel", "wait", "route", "all"])
    ap.add_argument("frames", nargs="?", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repeat"))
    a = ap.parse_args()
    if a.what == "all":
        sys.exit(run_all(a.out))
    {"kernel": kernel, "wait": lambda: wait(a.frames), "route": lambda: route(a.frames)}[a.what]()
