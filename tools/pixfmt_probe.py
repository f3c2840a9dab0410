"""1080p -> 2x frames through Net.submit_pix (yuv420p in, p010le out; include/uva.h uva_net_submit_pix) with three frames in
flight: the run `rocprofv3 --kernel-trace --stats` profiles for the conversion kernels' times.
Prints the wall-clock rate; argument: frames (default 200).  --chroma-filter bilinear [--chroma-loc left|center|topleft]: the
interpolating chroma kernels instead.  --in-pix-fmt / --out-pix-fmt / --bit-depth: other formats and
the 16-bit route (DESIGN.md sections 7.4, 7.7).  --stats DIR: no run; reads the kernel_stats.csv rocprofv3 left under DIR for a
run with the same format options and prints each conversion kernel's time and its effective bandwidth over the compulsory bytes
(the packed frame and the BGR frame, each moved once), computed from the shapes.  --verdict FILE: no run; reads such lines of a
4:2:2 case, and of its 4:2:0 twin profiled twice, from FILE and says whether each 4:2:2 kernel's bandwidth is at least the lower of
its twin's two runs, i.e. not below the twin by more than the twin's own run-to-run difference."""
import argparse
import csv
import glob
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from upscale_video_amd import ncnn                      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("frames", nargs="?", type=int, default=200)
ap.add_argument("--chroma-filter", default="replicate", choices=list(ncnn.CHROMA_FILTERS))
ap.add_argument("--chroma-loc", default="left", choices=list(ncnn.CHROMA_LOCS))
ap.add_argument("--in-pix-fmt", default="yuv420p", choices=list(ncnn.PIX_FORMATS_ALL))
ap.add_argument("--out-pix-fmt", default="p010le", choices=list(ncnn.PIX_FORMATS_ALL))
ap.add_argument("--bit-depth", type=int, default=8, choices=[8, 16])
ap.add_argument("--stats", default=None, metavar="DIR")
ap.add_argument("--verdict", default=None, metavar="FILE")
a = ap.parse_args()
N = a.frames
chroma = {} if a.chroma_filter == "replicate" else {"chroma_filter": a.chroma_filter, "chroma_loc": a.chroma_loc}
depth = {} if a.bit_depth == 8 else {"bit_depth": 16}
fin, fout = a.in_pix_fmt, a.out_pix_fmt
h, w = 1080, 1920

if a.verdict:
    rows = {}       # (direction, words of 16 bits) -> {"422": [TB/s], "420": [TB/s]}
    for ln in open(a.verdict):
        m = re.match(r"\s+(yuv42[02]p(?:10le)?) +-> +\S+ +(to_bgr|from_bgr) .* ([0-9.]+) TB/s over", ln)
        if m:
            rows.setdefault((m.group(2), "10le" in m.group(1)), {"422": [], "420": []})[m.group(1)[3:6]].append(float(m.group(3)))
    ok = bool(rows)
    for (which, w16), r in sorted(rows.items()):
        if len(r["422"]) != 1 or len(r["420"]) != 2:
            print("%s %s: needs one 4:2:2 run and two runs of its twin, got %s" % (which, "10-bit" if w16 else "8-bit", r))
            ok = False
            continue
        lo, hi = min(r["420"]), max(r["420"])
        met = r["422"][0] >= lo
        ok = ok and met
        print("%-8s %-6s 4:2:2 %.3f TB/s; 4:2:0 twin %.3f and %.3f TB/s (its runs differ by %.1f %%): %+.1f %% against the twin's better run: bar %s"
              % (which, "10-bit" if w16 else "8-bit", r["422"][0], r["420"][0], r["420"][1], 100 * (hi - lo) / hi, 100 * (r["422"][0] / hi - 1),
                 "met" if met else "MISSED"))
    print("bandwidth bar met" if ok else "bandwidth bar NOT met")
    sys.exit(0)

if a.stats:
    bps = a.bit_depth // 8
    # the kernel in front of the net reads the packed h x w frame and writes BGR; the one behind reads BGR of 2h x 2w
    nbytes = {"to_bgr": ncnn.pix_frame_bytes(fin, h, w) + 3 * h * w * bps, "from_bgr": 3 * 4 * h * w * bps + ncnn.pix_frame_bytes(fout, 2 * h, 2 * w)}
    for path in sorted(glob.glob(os.path.join(a.stats, "**", "*kernel_stats.csv"), recursive=True)):
        for r in csv.DictReader(open(path)):
            for which, nb in nbytes.items():
                if which in r.get("Name", "") and "pix" in r["Name"]:
                    avg = float(r["AverageNs"])
                    print("    %-6s -> %-11s %-8s %-64s %4d launches  avg %8.1f us  (min %.1f, max %.1f)  %.3f TB/s over %.1f MB"
                          % (fin, fout, which, r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:64], int(r["Calls"]), avg / 1e3, float(r["MinNs"]) / 1e3,
                             float(r["MaxNs"]) / 1e3, nb / avg / 1e3, nb / 1e6))
    sys.exit(0)

from upscale_video_amd.rawvideo import load_net          # noqa: E402
from upscale_video_amd.synth import synthetic_frame      # noqa: E402

net = load_net("2x_Compact_Pretrain", 0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "models"))
frames = []
for i in range(4):
    buf = ncnn.pix_empty(fin, h, w, ncnn.pinned_empty)
    buf.reshape(-1).view("u1")[...] = ncnn.convert_pix(synthetic_frame(h, w, seed=i), h, w, "bgr24", fin, **depth).reshape(-1).view("u1")
    frames.append(buf)
outs = [ncnn.pix_empty(fout, 2 * h, 2 * w, ncnn.pinned_empty) for _ in range(3)]
inflight = []
t0 = None
for i in range(N + 10):
    if i == 10:
        while inflight:
            net.collect_u8(inflight.pop(0))
        t0 = time.perf_counter()
    if len(inflight) == 3:
        net.collect_u8(inflight.pop(0))
    inflight.append(net.submit_pix(frames[i % 4], h, w, fin, out=outs[i % 3], out_fmt=fout, tile_size=960, border=10,
                                   **chroma, **depth))
while inflight:
    net.collect_u8(inflight.pop(0))
dt = time.perf_counter() - t0
print(f"submit_pix {fin} -> {fout}{', 16-bit route' if depth else ''}, 1080p -> 2x, chroma {a.chroma_filter}{'/' + a.chroma_loc if chroma else ''}: "
      f"{N} frames in {dt:.3f} s = {N / dt:.1f} frames/s")
