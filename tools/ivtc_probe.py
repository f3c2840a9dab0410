"""--detelecine measured: the kernel alone beside its siblings, the stateful push host to host, and the
route.

    kernel          uva_ivtc_metrics_device on 1920 x 1080 frames of yuv420p, p010le and bgr24 resident in HBM, beside
                    uva_frame_diff_device and uva_deint_frames_device (mode frame) on the same frames: whole calls, launch and wait.
    trace           the `kernel` step again under rocprofv3 --kernel-trace: the time per dispatch of ivtc_metrics_kernel,
                    frame_diff_kernel and deint_kernel, grouped by instantiation and grid size.
    push            uva_ivtc_push host to host on page-locked frames of a 2:3 pulldown stream: upload, metric, read-back, weave,
                    frame difference, read-back, download, wait -- what the reader thread spends per input frame; median, worst.
    route [frames]  rawvideo.stream() in this process from memory to nowhere, `yuv420p -> yuv420p -s 2` at 1920 x 1080 on a
                    synthetic pulldown stream: without the option and with --detelecine, in INPUT frames per second, three runs
                    each, alternating.
    all [--out DIR] the four as child processes, each under a time limit of its own, stopping at the first that fails; their
                    output goes to DIR/{kernel,trace,push,route}.txt (default profiles/ivtc).
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from upscale_video_amd import ncnn                       # noqa: E402
from upscale_video_amd.synth import synthetic_frame      # noqa: E402

LIMITS = {"kernel": 240, "trace": 300, "push": 240, "route": 480}     # seconds per step of `all`
FORMATS = ("yuv420p", "p010le", "bgr24")
KERNELS = ("ivtc_metrics_kernel", "frame_diff_kernel", "deint_kernel")
H, W = 1080, 1920


def timed(fn, reps=200):
    for _ in range(20):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def weave(cur, x, fmt, h, w):
    """numpy: the even rows of every plane from cur, the odd rows from x (tff)"""
    import numpy as np
    out = np.array(cur, copy=True)
    nb = 2 if fmt in ("p010le",) else 1
    planes = [(0, h, w * 3)] if fmt == "bgr24" else ([(0, h, w), (h * w, (h + 1) // 2, 2 * ((w + 1) // 2))] if fmt == "p010le" else
                                                      [(0, h, w), (h * w, (h + 1) // 2, (w + 1) // 2),
                                                       (h * w + ((h + 1) // 2) * ((w + 1) // 2), (h + 1) // 2, (w + 1) // 2)])
    for off, ph, rs in planes:
        o = out[off * nb:(off + ph * rs) * nb].reshape(ph, rs * nb)
        o[1::2] = np.asarray(x)[off * nb:(off + ph * rs) * nb].reshape(ph, rs * nb)[1::2]
    return out


def pulldown_stream(fmt, n):
    """n video frames: film frames (the synthetic picture moved sideways) through 2:3 pulldown"""
    import numpy as np
    film = []
    for i in range(4 * (n // 5 + 2)):
        bgr = np.roll(synthetic_frame(H, W, seed=1), 7 * i, axis=1).copy()
        film.append(ncnn.convert_pix(bgr, H, W, "bgr24", fmt).reshape(-1).view(np.uint8) if fmt != "bgr24" else bgr.reshape(-1))
    pat = [(0, 0), (0, 1), (1, 2), (2, 2), (3, 3)]
    return [weave(film[4 * (j // 5) + pat[j % 5][0]], film[4 * (j // 5) + pat[j % 5][1]], fmt, H, W) for j in range(n)]


def kernel():
    import torch
    for fmt in FORMATS:
        n = ncnn.pix_frame_bytes(fmt, H, W)
        video = pulldown_stream(fmt, 3)
        d = [torch.from_numpy(v.copy()).cuda() for v in video] + [torch.zeros(n, dtype=torch.uint8).cuda()]
        torch.cuda.synchronize()
        p = [t.data_ptr() for t in d]
        calls = (("uva_ivtc_metrics_device", lambda: ncnn.ivtc_metrics(p[0], p[1], p[2], fmt, H, W, device=True)),
                 ("uva_frame_diff_device", lambda: ncnn.frame_diff(p[0], p[1], fmt, H, W, 0, device=True)),
                 ("uva_deint_frames_device", lambda: ncnn.deint_frames(p[0], p[1], p[2], fmt, H, W, "frame", device=True, out_a=p[3])))
        for name, fn in calls:
            med, best, _ = timed(fn)
            print(f"{fmt:8s} {W}x{H} {name:24s}: call median {med * 1e6:7.1f} us (best {best * 1e6:7.1f}), launch, read-back and wait included",
                  flush=True)
        print(f"{fmt:8s} stats {ncnn.ivtc_metrics(p[0], p[1], p[2], fmt, H, W, device=True)}", flush=True)


def trace(out):
    import csv
    import glob
    d = os.path.join(out, "trace")
    subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "ivtc", "--", sys.executable,
                    os.path.abspath(__file__), "kernel"], check=True, cwd=ROOT, timeout=200, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        print("no kernel trace was written")
        return 1
    groups = {}
    for row in csv.DictReader(open(files[0])):
        name = row.get("Kernel_Name", "")
        for k in KERNELS:
            if k in name:
                wgs = (int(row.get("Grid_Size_X", row.get("Grid_Size", 0))) // 256) * max(1, int(row.get("Grid_Size_Y", 1)))
                groups.setdefault((name[name.index(k):][:30], wgs), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for (name, wgs), ts in sorted(groups.items()):
        print(f"{name:32s} {wgs:5d} workgroups: {len(ts):4d} dispatches, median {statistics.median(ts):7.2f} us, best {min(ts):7.2f} us", flush=True)
    return 0


def push():
    for fmt in FORMATS:
        n = ncnn.pix_frame_bytes(fmt, H, W)
        video = pulldown_stream(fmt, 10)
        src = [ncnn.pinned_empty((n,)) for _ in video]
        for s, v in zip(src, video):
            s[:] = v
        out = ncnn.pinned_empty((n,))
        for keep_all in (False, True):
            with ncnn.Detelecine(fmt, H, W, keep_all=keep_all) as dt:
                k = [0]

                def one():
                    dt.push(src[k[0] % 10], out)
                    k[0] += 1
                med, best, worst = timed(one, 150)
                st = dt.stats()
            print(f"{fmt:8s} {W}x{H} {'keep-all' if keep_all else 'decimate'}: push median {med * 1e6:8.1f} us, best {best * 1e6:8.1f}, worst "
                  f"{worst * 1e6:8.1f} = {1 / med:7.1f} input frames/s on the reader thread; {st}", flush=True)


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


def route(n=300):
    """in one process, so that neither start-up nor a file system is in the figure: rawvideo.stream() from memory to nowhere"""
    from upscale_video_amd import rawvideo
    packed = [memoryview(v.tobytes()) for v in pulldown_stream("yuv420p", 10)]
    net = rawvideo.load_net(rawvideo.MODEL_FILES[2], 0, os.path.join(ROOT, "models"))
    chain = [(net, rawvideo.TILE_SIZE)]
    pix = rawvideo.PixFormats("yuv420p", "yuv420p")

    def run(on, frames):
        spec = rawvideo.DetelecineSpec() if on else None
        kw = {"deint": spec} if on else {}
        t0 = time.perf_counter()
        written = rawvideo.stream(_Cycle(packed, frames), _Null(), H, W, chain, pix=pix, **kw)
        dt = time.perf_counter() - t0
        assert written == (frames - frames // 5 if on else frames), (written, frames)
        return frames / dt, written / dt, (spec.summary() if on else "")
    for on in (False, True):
        run(on, 40)                                     # (buffers allocated, clocks up)
    rates = {False: [], True: []}
    for k in range(6):
        on = bool(k % 2)
        fin, fout, text = run(on, n)
        rates[on].append(fin)
        print(f"{'--detelecine   ' if on else 'no --detelecine'}: {n} input frames = {fin:7.1f} in/s, {fout:7.1f} out/s  {text}", flush=True)
    base = sum(rates[False]) / len(rates[False])
    for on in (False, True):
        v = rates[on]
        print(f"{'--detelecine' if on else 'without     '}: mean {sum(v) / len(v):7.1f} input frames/s, scatter {min(v):.1f} ... {max(v):.1f} over {len(v)} runs = "
              f"{sum(v) / len(v) / base:.3f} of the rate without the option", flush=True)


def run_all(out):
    os.makedirs(out, exist_ok=True)
    for step in ("kernel", "trace", "push", "route"):
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
    ap.add_argument("what", choices=["kernel", "trace", "push", "route", "all"])
    ap.add_argument("frames", nargs="?", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivtc"))
    a = ap.parse_args()
    if a.what == "all":
        sys.exit(run_all(a.out))
    sys.exit({"kernel": kernel, "trace": lambda: trace(a.out), "push": push, "route": lambda: route(a.frames)}[a.what]() or 0)
