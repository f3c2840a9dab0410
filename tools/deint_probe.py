"""--deinterlace measured: the kernel alone, the stateful push host to host, and the route.

    kernel          uva_deint_frames_device on 1920 x 1080 frames of yuv420p, p010le and bgr24 resident in HBM, modes frame and
                    field, beside the same call on a 16 x 16 frame (every slot a ragged one: the sample-by-sample path).
    trace           the `kernel` step again under rocprofv3 --kernel-trace: deint_kernel's own time per dispatch, grouped by
                    instantiation and grid size, set against the bytes the launch must move (frame: about 2.5 frames read and one
                    written; field: three read and two written) and section 7.4's 6.29 TB/s copy ceiling.
    push            uva_deint_push host to host on pageable and on page-locked frames: upload, kernel, download, wait -- what
                    the reader thread of the route spends per input frame; median and worst.
    route [frames]  rawvideo.stream() in this process from memory to nowhere, `yuv420p -> yuv420p -s 2` at 1920 x 1080: without
                    the option, with --deinterlace frame (input frames per second) and with --deinterlace field (output frames
                    per second against the same), three runs each, alternating.
    all [--out DIR] the four as child processes, each under a time limit of its own, stopping at the first that fails; their
                    output goes to DIR/{kernel,trace,push,route}.txt (default profiles/deint).
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
CEILING = 6.29e12                                         # bytes / s, DESIGN.md section 7.4


def timed(fn, reps=200):
    for _ in range(20):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def moved_bytes(n, mode):
    """what a launch must move: frame mode reads cur and half of prev and of next... about 2.5 frames, and writes one; field
    mode reads all three and writes two"""
    return (2.5 + 1) * n if mode == "frame" else (3 + 2) * n


def kernel():
    import numpy as np
    import torch
    rng = np.random.default_rng(1)

    def frames(fmt, h, w, k):
        n = ncnn.pix_frame_bytes(fmt, h, w)
        out = [torch.from_numpy(rng.integers(0, 256, n, dtype=np.uint8)).cuda() for _ in range(k)]
        torch.cuda.synchronize()
        return out, n

    def call(d, fmt, h, w, mode):
        ncnn.deint_frames(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), fmt, h, w, mode, device=True, out_a=d[3].data_ptr(),
                          out_b=d[4].data_ptr() if mode == "field" else None)
    # (a 16 x 16 frame is no measure of a call's fixed part here: all its slots are ragged ones, which go sample by sample, and
    # the first run of this probe found the call SLOWER than on a 1080p frame; it is the figure for that path)
    d, _ = frames("yuv420p", 16, 16, 5)
    small = timed(lambda: call(d, "yuv420p", 16, 16, "field"))[0]
    print(f"16 x 16 frame (every slot a ragged one, one workgroup): call median {small * 1e6:.1f} us", flush=True)
    h, w = 1080, 1920
    for fmt in FORMATS:
        d, n = frames(fmt, h, w, 5)
        for mode in ("frame", "field"):
            med, best, _ = timed(lambda: call(d, fmt, h, w, mode))
            print(f"{fmt:8s} {w}x{h} {mode:5s}: call median {med * 1e6:7.1f} us (best {best * 1e6:7.1f}) = "
                  f"{moved_bytes(n, mode) / med / 1e12:5.2f} TB/s moved, launch and wait included", flush=True)


def trace(out):
    import csv
    import glob
    d = os.path.join(out, "trace")
    subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "deint", "--", sys.executable,
                    os.path.abspath(__file__), "kernel"], check=True, cwd=ROOT, timeout=200, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        print("no kernel trace was written")
        return 1
    groups = {}
    for row in csv.DictReader(open(files[0])):
        name = row.get("Kernel_Name", "")
        if "deint_kernel" in name:
            key = (name[name.index("deint_kernel"):][:24], int(row.get("Grid_Size_X", row.get("Grid_Size", 0))) // 256)
            groups.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for (name, wgs), ts in sorted(groups.items()):
        print(f"{name:26s} {wgs:5d} workgroups: {len(ts):4d} dispatches, median {statistics.median(ts):7.2f} us, best {min(ts):7.2f} us", flush=True)
    for fmt in FORMATS:
        n = ncnn.pix_frame_bytes(fmt, 1080, 1920)
        print(f"{fmt:8s} 1920x1080 at the {CEILING / 1e12:.2f} TB/s copy ceiling: frame {moved_bytes(n, 'frame') / CEILING * 1e6:5.2f} us, "
              f"field {moved_bytes(n, 'field') / CEILING * 1e6:5.2f} us", flush=True)
    return 0


def push():
    import numpy as np
    rng = np.random.default_rng(2)
    h, w = 1080, 1920
    for fmt in FORMATS:
        n = ncnn.pix_frame_bytes(fmt, h, w)
        for pinned in (False, True):
            alloc = ncnn.pinned_empty if pinned else (lambda shape: np.empty(shape, np.uint8))
            src = [alloc((n,)) for _ in range(3)]
            for s in src:
                s[:] = rng.integers(0, 256, n, dtype=np.uint8)
            outs = [alloc((n,)) for _ in range(2)]
            for mode in ("frame", "field"):
                with ncnn.Deinterlacer(fmt, h, w, mode) as di:
                    k = [0]

                    def one():
                        di.push(src[k[0] % 3], outs)
                        k[0] += 1
                    med, best, worst = timed(one, 150)
                print(f"{fmt:8s} {w}x{h} {mode:5s} {'page-locked' if pinned else 'pageable   '}: push median {med * 1e6:8.1f} us, best "
                      f"{best * 1e6:8.1f}, worst {worst * 1e6:8.1f} = {1 / med:7.1f} input frames/s on the reader thread", flush=True)


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
    h, w = 1080, 1920
    packed = [memoryview(ncnn.convert_pix(synthetic_frame(h, w, seed=i).copy(), h, w, "bgr24", "yuv420p").tobytes()) for i in range(8)]
    net = rawvideo.load_net(rawvideo.MODEL_FILES[2], 0, os.path.join(ROOT, "models"))
    chain = [(net, rawvideo.TILE_SIZE)]
    pix = rawvideo.PixFormats("yuv420p", "yuv420p")

    def run(mode, frames):
        kw = {} if mode is None else {"deint": rawvideo.DeintSpec(mode)}
        t0 = time.perf_counter()
        written = rawvideo.stream(_Cycle(packed, frames), _Null(), h, w, chain, pix=pix, **kw)
        dt = time.perf_counter() - t0
        assert written == frames * (2 if mode == "field" else 1)
        return frames / dt, written / dt
    for mode in (None, "frame", "field"):
        run(mode, 40)                                   # (buffers allocated, clocks up)
    rates = {None: [], "frame": [], "field": []}
    for k in range(9):
        mode = (None, "frame", "field")[k % 3]
        fin, fout = run(mode, n)
        rates[mode].append((fin, fout))
        print(f"{'no --deinterlace     ' if mode is None else '--deinterlace ' + mode + '  '}: {n} input frames = {fin:7.1f} in/s, {fout:7.1f} out/s",
              flush=True)
    base = sum(r[1] for r in rates[None]) / len(rates[None])
    for mode in (None, "frame", "field"):
        v = [r[1] for r in rates[mode]]
        print(f"{str(mode):6s}: mean {sum(v) / len(v):7.1f} output frames/s, scatter {min(v):.1f} ... {max(v):.1f} over {len(v)} runs = "
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deint"))
    a = ap.parse_args()
    if a.what == "all":
        sys.exit(run_all(a.out))
    sys.exit({"kernel": kernel, "trace": lambda: trace(a.out), "push": push, "route": lambda: route(a.frames)}[a.what]() or 0)
