"""1080p -> 2x frames through Net.submit_pix (yuv420p in, p010le out; include/uva.h uva_net_submit_pix) with three frames in
flight: the run `rocprofv3 --kernel-trace --stats` profiles for the conversion kernels' times.
Prints the wall-clock rate; argument: frames (default 200).  --chroma-filter bilinear [--chroma-loc left|center|topleft]: the
interpolating chroma kernels instead."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from upscale_video_amd import ncnn                      # noqa: E402
from upscale_video_amd.rawvideo import load_net          # noqa: E402
from upscale_video_amd.synth import synthetic_frame      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("frames", nargs="?", type=int, default=200)
ap.add_argument("--chroma-filter", default="replicate", choices=list(ncnn.CHROMA_FILTERS))
ap.add_argument("--chroma-loc", default="left", choices=list(ncnn.CHROMA_LOCS))
a = ap.parse_args()
N = a.frames
chroma = {} if a.chroma_filter == "replicate" else {"chroma_filter": a.chroma_filter, "chroma_loc": a.chroma_loc}
h, w = 1080, 1920
net = load_net("2x_Compact_Pretrain", 0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "models"))
frames = []
for i in range(4):
    buf = ncnn.pix_empty("yuv420p", h, w, ncnn.pinned_empty)
    buf[...] = ncnn.convert_pix(synthetic_frame(h, w, seed=i), h, w, "bgr24", "yuv420p")
    frames.append(buf)
outs = [ncnn.pix_empty("p010le", 2 * h, 2 * w, ncnn.pinned_empty) for _ in range(3)]
inflight = []
t0 = None
for i in range(N + 10):
    if i == 10:
        while inflight:
            net.collect_u8(inflight.pop(0))
        t0 = time.perf_counter()
    if len(inflight) == 3:
        net.collect_u8(inflight.pop(0))
    inflight.append(net.submit_pix(frames[i % 4], h, w, "yuv420p", out=outs[i % 3], out_fmt="p010le", tile_size=960, border=10,
                                   **chroma))
while inflight:
    net.collect_u8(inflight.pop(0))
dt = time.perf_counter() - t0
print(f"submit_pix yuv420p -> p010le, 1080p -> 2x, chroma {a.chroma_filter}{'/' + a.chroma_loc if chroma else ''}: {N} frames in {dt:.3f} s = {N / dt:.1f} frames/s")
