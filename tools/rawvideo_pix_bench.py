"""Rate of the rawvideo streamer (python -m upscale_video_amd.rawvideo -s 2) at 1080p -> 2x per pair of pixel formats
(--in-pix-fmt / --out-pix-fmt), file -> /dev/null and pipe -> pipe, frames held in /dev/shm: whole process wall time minus
the wall time of a 1-frame run (interpreter start, model load, first-use allocations), as tools/rawvideo_bench.py.
Argument: frames (default 600).  --formats in:out[,in:out...] picks the rows; --chroma-filter / --chroma-loc / --bit-depth go to
the streamer (DESIGN.md sections 7.4, 7.5)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from upscale_video_amd import ncnn                      # noqa: E402
from upscale_video_amd.synth import synthetic_frame      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("frames", nargs="?", type=int, default=600)
ap.add_argument("--formats", default="bgr24:bgr24,yuv420p:yuv420p,yuv420p:p010le")
ap.add_argument("--chroma-filter", default="replicate", choices=list(ncnn.CHROMA_FILTERS))
ap.add_argument("--chroma-loc", default="left", choices=list(ncnn.CHROMA_LOCS))
ap.add_argument("--bit-depth", type=int, default=8, choices=[8, 16])
a = ap.parse_args()
N = a.frames
h, w = 1080, 1920
base = [sys.executable, "-m", "upscale_video_amd.rawvideo", "-W", str(w), "-H", str(h), "-s", "2"]
if a.chroma_filter != "replicate":
    base += ["--chroma-filter", a.chroma_filter, "--chroma-loc", a.chroma_loc]
    print("chroma %s/%s" % (a.chroma_filter, a.chroma_loc), flush=True)


def wall(cmd, shell=False):
    t0 = time.perf_counter()
    subprocess.run(cmd, shell=shell, check=True, stderr=subprocess.DEVNULL, stdout=subprocess.DEVNULL if not shell else None, cwd=ROOT)
    return time.perf_counter() - t0


if a.bit_depth == 16:
    base += ["--bit-depth", "16"]
    print("bit depth 16", flush=True)
fr = [synthetic_frame(h, w, seed=i) for i in range(4)]
for fin, fout in (tuple(x.split(":")) for x in a.formats.split(",")):
    src = "/dev/shm/uva_in.%s" % fin
    packed = [ncnn.convert_pix(f, h, w, "bgr24", fin).tobytes() if fin != "bgr24" else f.tobytes() for f in fr]
    with open(src, "wb") as o:
        for i in range(N):
            o.write(packed[i % 4])
    fmts = ["--in-pix-fmt", fin, "--out-pix-fmt", fout]
    t1 = wall(base + fmts + ["-i", src, "-o", "/dev/null", "--frames", "1"])
    tn = wall(base + fmts + ["-i", src, "-o", "/dev/null"])
    mb = (ncnn.pix_frame_bytes(fin, h, w) + ncnn.pix_frame_bytes(fout, 2 * h, 2 * w)) / 1e6
    print(f"{fin:11s} -> {fout:11s} ({mb:5.1f} MB/frame) file -> /dev/null : {N} frames in {tn:6.2f} s (start-up {t1:5.2f} s) = "
          f"{(N - 1) / (tn - t1):7.1f} frames/s", flush=True)
    tn = wall(f"cat {src} | {' '.join(base + fmts)} 2>/dev/null | cat > /dev/null", shell=True)
    print(f"{fin:11s} -> {fout:11s} ({mb:5.1f} MB/frame) pipe -> pipe      : {N} frames in {tn:6.2f} s = {(N - 1) / (tn - t1):7.1f} frames/s",
          flush=True)
    os.remove(src)
