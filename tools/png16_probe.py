"""The PNG route at 16 bits measured on the MI355X, every figure beside the 8-bit one taken in the same
call on the same box.

    encode [reps]   Net results of a synthetic 1080p frame at 2x (3840 x 2160), u8 and u16, through ncnn.png_encode_u8 /
                    png_encode_u16 in turn: host clock per call (H2D copy + kernels + download + framing).  The loop `kernel`
                    profiles.
    kernel          `encode` as a child under rocprofv3 --kernel-trace --stats: time per launch of png_deflate_kernel16 against
                    png_deflate_kernel (and png_pack_kernel) on those frames.  The 16-bit kernel handles twice the bytes.
    sizes           packed bytes per frame on synth.synthetic_frame results (four seeds): the 8-bit file, the 16-bit file, and
                    zlib level 1 / Z_RLE on the 16-bit frame (what cv2.imwrite would write).
    route [frames]  PNG -> PNG frames/s through FramePool at 1080p -> 2x in a RAM disk, BIT_DEPTH 16 against 8, alternating, two
                    runs each, every run a child process of its own (rate over the frames after a warm-up batch).
    all [--out DIR] the four as child processes, each under a time limit of its own, stopping at the first that fails; their
                    output goes to DIR/{encode,kernel,sizes_gpu,route}.txt (default profiles/png16).
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

LIMITS = {"encode": 240, "kernel": 420, "sizes": 300, "route": 600}     # seconds per step of `all`


def results(seed=1):
    """-> (u8 result, u16 result) of the 2x net on a synthetic 1080p frame (the 16-bit input: the frame widened x257)"""
    import numpy as np
    from upscale_video_amd.rawvideo import load_net
    from upscale_video_amd.synth import synthetic_frame
    net = load_net("2x_Compact_Pretrain", 0, os.path.join(ROOT, "models"))
    small = synthetic_frame(1080, 1920, seed=seed)
    return net.process_u8(small, tile_size=960, border=10), net.process_u16(small.astype(np.uint16) * 257, tile_size=960, border=10)


def encode(reps=30):
    from upscale_video_amd import ncnn
    big8, big16 = results()
    ws8, ws16 = ncnn.PngWorkspace(2160, 3840), ncnn.PngWorkspace(2160, 3840, bit_depth=16)
    for _ in range(5):
        ncnn.png_encode_u8(big8, workspace=ws8)
        ncnn.png_encode_u16(big16, workspace=ws16)
    t8, t16 = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        p8 = ncnn.png_encode_u8(big8, workspace=ws8)
        t1 = time.perf_counter()
        p16 = ncnn.png_encode_u16(big16, workspace=ws16)
        t2 = time.perf_counter()
        t8.append(t1 - t0)
        t16.append(t2 - t1)
    for name, ts, png, raw in (("8-bit ", t8, p8, big8.nbytes), ("16-bit", t16, p16, big16.nbytes)):
        print(f"{name} 3840x2160 result, {raw / 1e6:.1f} MB raw: call (H2D + kernels + download + framing) median {statistics.median(ts) * 1e3:6.2f} ms, "
              f"best {min(ts) * 1e3:6.2f}, worst {max(ts) * 1e3:6.2f}; file {len(png) / 1e6:.2f} MB = {len(png) / raw:.3f} of raw", flush=True)


def kernel():
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    with tempfile.TemporaryDirectory(prefix="uva_png16_") as d:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable,
                            os.path.abspath(__file__), "encode", "30"], cwd=ROOT, capture_output=True, text=True, timeout=LIMITS["kernel"] - 20)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-2000:])
            sys.exit(r.returncode)
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                rows += [row for row in csv.DictReader(f) if "png_" in row.get("Name", "")]
    if not rows:
        sys.exit("no png_* kernels in the trace")
    print("rocprofv3 --kernel-trace --stats over 35 encodes of each kind (3840x2160 results of the 2x net):")
    avg = {}
    for row in rows:
        name = row["Name"].split("(")[0]
        avg[name] = float(row["AverageNs"])
        print(f"  {name:32s} calls {row['Calls']:>4s}  average {float(row['AverageNs']) / 1e3:8.1f} us  min {float(row['MinNs']) / 1e3:8.1f}  "
              f"max {float(row['MaxNs']) / 1e3:8.1f}")
    k8 = [v for k, v in avg.items() if k.endswith("png_deflate_kernel")]
    k16 = [v for k, v in avg.items() if k.endswith("png_deflate_kernel16")]
    if k8 and k16:
        print(f"  png_deflate_kernel16 / png_deflate_kernel = {k16[0] / k8[0]:.2f} (twice the bytes per frame)")


def sizes():
    from upscale_video_amd import _imageio, ncnn
    ws8, ws16 = ncnn.PngWorkspace(2160, 3840), ncnn.PngWorkspace(2160, 3840, bit_depth=16)
    print("packed bytes per 3840x2160 result frame (2x net on synth.synthetic_frame(1080, 1920, seed)):")
    for seed in (1, 2, 3, 4):
        big8, big16 = results(seed)
        n8 = len(ncnn.png_encode_u8(big8, workspace=ws8))
        n16 = len(ncnn.png_encode_u16(big16, workspace=ws16))
        z16 = len(_imageio.png_bytes16(big16))
        print(f"  seed {seed}: 8-bit file {n8:9d} B ({n8 / big8.nbytes:.3f} of raw)   16-bit file {n16:9d} B ({n16 / big16.nbytes:.3f} of raw)   "
              f"zlib level 1 / Z_RLE at 16 bits {z16:9d} B (ours / zlib {n16 / z16:.3f})", flush=True)


def route_one(depth, n):
    import numpy as np
    from upscale_video_amd import _imageio, upscale_processing as up
    from upscale_video_amd.synth import synthetic_frame
    base = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        os.chdir(base)
        frame = synthetic_frame(1080, 1920, seed=1)
        if depth == 16:          # a 10-bit source as ffmpeg extracts it to rgb48be: ten significant bits, replicated downwards
            v10 = (frame.astype(np.uint32) * 1023 + 127) // 255
            frame = ((v10 << 6) | (v10 >> 4)).astype(np.uint16)
        _imageio.imwrite("src.png", frame)
        for i in range(0, n + 1):
            shutil.copy("src.png", "%d.extract.png" % i)
        models = os.path.join(ROOT, "models")
        up.BIT_DEPTH = depth
        up.upscale_frames(0, 0, 0, "extract", 2, [0], 0, models, "x_Compact_Pretrain", "input", "output")     # warm-up: nets, rings
        t = time.perf_counter()
        up.upscale_frames(1, 1, n, "extract", 2, [0], 0, models, "x_Compact_Pretrain", "input", "output")
        dt = time.perf_counter() - t
        up.shutdown_workers()
        size = os.path.getsize("1.png")
    finally:
        os.chdir("/")
        shutil.rmtree(base, ignore_errors=True)
    print(f"BIT_DEPTH {depth:2d}: {n} frames 1080p -> 2x, PNG -> PNG, -g 0: {n / dt:6.1f} frames/s; result file {size / 1e6:.2f} MB", flush=True)


def route(n=120):
    for depth in (8, 16, 8, 16):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "route-one", str(depth), str(n)], cwd=ROOT, timeout=200)
        if r.returncode != 0:
            sys.exit(r.returncode)


def run_all(out):
    os.makedirs(out, exist_ok=True)
    for step in ("encode", "kernel", "sizes", "route"):
        path = os.path.join(out, ("sizes_gpu" if step == "sizes" else step) + ".txt")     # (sizes.txt there: the CPU test's ratios)
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
    ap.add_argument("what", choices=["encode", "kernel", "sizes", "route", "route-one", "all"])
    ap.add_argument("args", nargs="*", type=int)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png16"))
    a = ap.parse_args()
    if a.what == "all":
        sys.exit(run_all(a.out))
    if a.what == "route-one":
        route_one(*a.args)
    else:
        {"encode": encode, "kernel": kernel, "sizes": sizes, "route": route}[a.what](*a.args)
