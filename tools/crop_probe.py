"""--crop measured: the two kernels alone, and the route with and without a letterbox crop.

    kernel          uva_crop_sums_device per 1080p yuv420p and p010le frame beside uva_frame_diff_device on the same frames in
                    the same process (unrelated frames, so the difference kernel works on every sample; the sums read the luma
                    plane once, the difference both frames whole: half to two thirds of the bytes), and uva_pix_window_device
                    for a 1440 x 1080 pillarbox of a 1920 x 1080 frame.  A call is its memsets or none, the kernel, a read-back
                    and a wait; the same call on a 16 x 16 frame is that fixed part, the difference the kernel's time over the
                    frame.
    trace           the `kernel` step again under rocprofv3 --kernel-trace: the three kernels' own times per dispatch, which the
                    calls above -- tens of microseconds of fixed cost each -- cannot resolve.
    route [frames]  rawvideo.stream() in this process from memory to nowhere (no start-up, no file system in the figure), the
                    route of `yuv420p -> yuv420p -s 2` at 1920 x 1080 with --crop 1920:800:0:140 and without, three runs each,
                    alternating; the pixel count says 1080 / 800 = 1.35.
    all [--out DIR] the three as child processes, each under a time limit of its own, stopping at the first that fails; their
                    output goes to DIR/{kernel,trace,route}.txt (default profiles/crop).
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from upscale_video_amd import _lib, ncnn                 # noqa: E402
from upscale_video_amd.synth import synthetic_frame      # noqa: E402

LIMITS = {"kernel": 240, "trace": 300, "route": 420}     # seconds per step of `all`


def timed(fn, reps=300):
    for _ in range(20):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts)


def kernel():
    import numpy as np
    import torch
    rng = np.random.default_rng(1)
    L = _lib.load()

    def frames(fmt, h, w):
        n = ncnn.pix_frame_bytes(fmt, h, w)
        a, b = (torch.from_numpy(rng.integers(0, 256, n, dtype=np.uint8)).cuda() for _ in range(2))
        torch.cuda.synchronize()
        return a, b, n

    def window_call(a, out, fmt, sh, sw, x, y, h, w):
        _lib.check(L.uva_pix_window_device(0, ctypes.c_void_p(a.data_ptr()), ncnn.PIX_FORMATS_ALL[fmt], sh, sw, x, y, h, w,
                                           ctypes.c_void_p(out.data_ptr())))
    a, b, _ = frames("yuv420p", 16, 16)
    fixed_sums = timed(lambda: ncnn.crop_sums(a.data_ptr(), "yuv420p", 16, 16, device=True))[0]
    fixed_diff = timed(lambda: ncnn.frame_diff(a.data_ptr(), b.data_ptr(), "yuv420p", 16, 16, device=True))[0]
    fixed_win = timed(lambda: window_call(a, b, "yuv420p", 16, 16, 2, 0, 16, 12))[0]
    print(f"fixed part of a call (16 x 16 frame): crop_sums {fixed_sums * 1e6:.1f} us, frame_diff {fixed_diff * 1e6:.1f} us, "
          f"pix_window {fixed_win * 1e6:.1f} us (medians)", flush=True)
    h, w = 1080, 1920
    for fmt in ("yuv420p", "p010le"):
        a, b, n = frames(fmt, h, w)
        luma = h * w * (2 if fmt == "p010le" else 1)
        s_med, s_best = timed(lambda: ncnn.crop_sums(a.data_ptr(), fmt, h, w, device=True))
        d_med, d_best = timed(lambda: ncnn.frame_diff(a.data_ptr(), b.data_ptr(), fmt, h, w, device=True))
        s_over, d_over = max(s_med - fixed_sums, 1e-9), max(d_med - fixed_diff, 1e-9)
        print(f"{fmt:8s} {w}x{h}: crop_sums call median {s_med * 1e6:7.1f} us (best {s_best * 1e6:7.1f}), over the fixed part "
              f"{s_over * 1e6:7.1f} us = {luma / s_over / 1e12:5.2f} TB/s read | frame_diff call median {d_med * 1e6:7.1f} us (best "
              f"{d_best * 1e6:7.1f}), over the fixed part {d_over * 1e6:7.1f} us = {2 * n / d_over / 1e12:5.2f} TB/s read", flush=True)
        cw, x = 1440, 240
        out = torch.zeros(ncnn.pix_frame_bytes(fmt, h, cw), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        w_med, w_best = timed(lambda: window_call(a, out, fmt, h, w, x, 0, h, cw))
        w_over = max(w_med - fixed_win, 1e-9)
        print(f"{fmt:8s} {w}x{h}: pix_window 1440x1080 pillarbox call median {w_med * 1e6:7.1f} us (best {w_best * 1e6:7.1f}), over the "
              f"fixed part {w_over * 1e6:7.1f} us = {2 * out.numel() / w_over / 1e12:5.2f} TB/s read + written", flush=True)


def trace(out):
    """the kernels' own times: the `kernel` step again under rocprofv3 --kernel-trace, every dispatch of the three kernels grouped
    by kernel and grid size (the 16 x 16 calls have grids of one workgroup) -> count, median, best, in microseconds"""
    import csv
    import glob
    d = os.path.join(out, "trace")
    subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "crop", "--", sys.executable,
                    os.path.abspath(__file__), "kernel"], check=True, cwd=ROOT, timeout=200, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        print("no kernel trace was written")
        return 1
    groups = {}
    for row in csv.DictReader(open(files[0])):
        name = row.get("Kernel_Name", "")
        for k in ("crop_sums_kernel", "frame_diff_kernel", "pix_window_kernel"):
            if k in name:
                key = (k + ("<2>" if "ILi2E" in name or "<2>" in name else "<1>"), int(row.get("Grid_Size_X", row.get("Grid_Size", 0))) // 256)
                groups.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for (name, wgs), ts in sorted(groups.items()):
        print(f"{name:22s} {wgs:5d} workgroups: {len(ts):4d} dispatches, median {statistics.median(ts):7.2f} us, best {min(ts):7.2f} us", flush=True)
    return 0


class _Cycle:
    """a reader that deals out `n` frames, cycling through a few held in memory"""

    def __init__(self, frames, n):
        self.frames, self.n, self.i = frames, n, 0

    def readinto(self, view):
        if self.i >= self.n:
            return 0
        f = self.frames[self.i % len(self.frames)]
        view[:len(f)] = f
        self.i += 1
        return len(f)


class _Null:
    def write(self, b):
        return len(b)

    def flush(self):
        pass


def route(n=600):
    """in one process, so that neither start-up nor a file system is in the figure: rawvideo.stream() from memory to nowhere"""
    from upscale_video_amd import rawvideo
    h, w = 1080, 1920
    packed = []
    for i in range(8):
        bgr = synthetic_frame(h, w, seed=i).copy()
        bgr[:140] = 0
        bgr[940:] = 0                                   # a 1920 x 800 picture in a 1920 x 1080 frame
        packed.append(memoryview(ncnn.convert_pix(bgr, h, w, "bgr24", "yuv420p").tobytes()))
    net = rawvideo.load_net(rawvideo.MODEL_FILES[2], 0, os.path.join(ROOT, "models"))
    chain = [(net, rawvideo.TILE_SIZE)]
    whole = rawvideo.PixFormats("yuv420p", "yuv420p")
    cropped = rawvideo.PixFormats("yuv420p", "yuv420p", crop=(1920, 800, 0, 140))

    def run(pix, frames):
        if pix.crop is None:
            net.set_input_window()
        t0 = time.perf_counter()
        assert rawvideo.stream(_Cycle(packed, frames), _Null(), h, w, chain, pix=pix) == frames
        return frames / (time.perf_counter() - t0)
    run(whole, 60)
    run(cropped, 60)                                    # (buffers allocated, clocks up)
    rates = {False: [], True: []}
    for k in range(6):
        crop = bool(k & 1)
        rate = run(cropped if crop else whole, n)
        rates[crop].append(rate)
        print(f"{'--crop 1920:800:0:140 ' if crop else 'whole 1920x1080 frames'}: {n} frames = {rate:7.1f} frames/s", flush=True)
    for crop in (False, True):
        v = rates[crop]
        print(f"{'cropped' if crop else 'whole  '}: mean {sum(v) / len(v):7.1f} frames/s, scatter {min(v):.1f} ... {max(v):.1f} over "
              f"{len(v)} runs", flush=True)
    off, on = (sum(v) / len(v) for v in (rates[False], rates[True]))
    print(f"cropped against whole: {on / off:.3f}x (1080 / 800 = 1.350 by the pixel count)", flush=True)


def run_all(out):
    os.makedirs(out, exist_ok=True)
    for step in ("kernel", "trace", "route"):
        path = os.path.join(out, step + ".txt")
        with open(path, "w") as f:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), step, "--out", out], stdout=f, stderr=subprocess.STDOUT, cwd=ROOT,
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
    ap.add_argument("what", choices=["kernel", "trace", "route", "all"])
    ap.add_argument("frames", nargs="?", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crop"))
    a = ap.parse_args()
    if a.what == "all":
        sys.exit(run_all(a.out))
    sys.exit({"kernel": kernel, "trace": lambda: trace(a.out), "route": lambda: route(a.frames)}[a.what]() or 0)
