"""The 16-bit route against the 8-bit one at 1080p -> 2x, 960/10 tiles.

    probe [frames]  Net.submit_pix p010le -> p010le with three frames in flight, bit_depth 8 and 16 alternated in blocks of
                    20 frames in ONE process: the run `rocprofv3 --kernel-trace --stats` profiles for the head, tail and
                    conversion kernels' times.  Prints each route's wall-clock rate.
    pipe [frames]   profiler off: python -m upscale_video_amd.rawvideo pipe -> pipe, p010le both ways, --bit-depth 8 and 16
                    (frames held in /dev/shm; rate = (frames - 1) / (wall - wall of a 1-frame run)).
    --chroma-filter bilinear [--chroma-loc left|center|topleft]: either run with the interpolating chroma kernels (section 7.5).
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from upscale_video_amd import ncnn                      # noqa: E402
from upscale_video_amd.synth import synthetic_frame      # noqa: E402

h, w = 1080, 1920


CHROMA = {}            # submit_pix's chroma keywords (main fills them in)


def probe(n):
    from upscale_video_amd.rawvideo import load_net
    net = load_net("2x_Compact_Pretrain", 0, os.path.join(ROOT, "models"))
    frames = []
    for i in range(4):
        buf = ncnn.pix_empty("p010le", h, w, ncnn.pinned_empty)
        buf[...] = ncnn.convert_pix(synthetic_frame(h, w, seed=i), h, w, "bgr24", "p010le")
        frames.append(buf)
    outs = [ncnn.pix_empty("p010le", 2 * h, 2 * w, ncnn.pinned_empty) for _ in range(3)]
    spent = {8: 0.0, 16: 0.0}
    done = {8: 0, 16: 0}
    k = 0
    while done[8] + done[16] < 2 * n:
        bd = 8 if (k // 20) % 2 == 0 else 16
        t0 = time.perf_counter()
        inflight = []
        for i in range(20):
            if len(inflight) == 3:
                net.collect_u8(inflight.pop(0))
            inflight.append(net.submit_pix(frames[i % 4], h, w, "p010le", out=outs[i % 3], out_fmt="p010le", tile_size=960, border=10,
                                           bit_depth=bd, **CHROMA))
        while inflight:
            net.collect_u8(inflight.pop(0))
        if k >= 40:                                   # (the first block of each route warms up)
            spent[bd] += time.perf_counter() - t0
            done[bd] += 20
        k += 20
    for bd in (8, 16):
        print(f"submit_pix p010le -> p010le, 1080p -> 2x, bit depth {bd}: {done[bd]} frames in {spent[bd]:.3f} s = "
              f"{done[bd] / spent[bd]:.1f} frames/s", flush=True)


def pipe(n):
    base = [sys.executable, "-m", "upscale_video_amd.rawvideo", "-W", str(w), "-H", str(h), "-s", "2",
            "--in-pix-fmt", "p010le", "--out-pix-fmt", "p010le"]
    for k, v in CHROMA.items():
        base += ["--" + k.replace("_", "-"), v]
    src = "/dev/shm/uva_bd16_in.p010"
    packed = [ncnn.convert_pix(synthetic_frame(h, w, seed=i), h, w, "bgr24", "p010le").tobytes() for i in range(4)]
    with open(src, "wb") as o:
        for i in range(n):
            o.write(packed[i % 4])

    def wall(cmd, shell=False):
        t0 = time.perf_counter()
        subprocess.run(cmd, shell=shell, check=True, stderr=subprocess.DEVNULL, stdout=subprocess.DEVNULL if not shell else None, cwd=ROOT)
        return time.perf_counter() - t0
    try:
        for bd in (8, 16):
            cmd = base + ["--bit-depth", str(bd)]
            t1 = wall(cmd + ["-i", src, "-o", "/dev/null", "--frames", "1"])
            tn = wall(f"cat {src} | {' '.join(cmd)} 2>/dev/null | cat > /dev/null", shell=True)
            print(f"p010le -> p010le --bit-depth {bd:2d} pipe -> pipe: {n} frames in {tn:6.2f} s (start-up {t1:5.2f} s) = "
                  f"{(n - 1) / (tn - t1):7.1f} frames/s", flush=True)
    finally:
        os.remove(src)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="probe", choices=["probe", "pipe"])
    ap.add_argument("frames", nargs="?", type=int, default=None)
    ap.add_argument("--chroma-filter", default="replicate", choices=list(ncnn.CHROMA_FILTERS))
    ap.add_argument("--chroma-loc", default="left", choices=list(ncnn.CHROMA_LOCS))
    a = ap.parse_args()
    if a.chroma_filter != "replicate":
        CHROMA.update(chroma_filter=a.chroma_filter, chroma_loc=a.chroma_loc)
    n = a.frames if a.frames is not None else (200 if a.what == "probe" else 600)
    probe(n) if a.what == "probe" else pipe(n)
