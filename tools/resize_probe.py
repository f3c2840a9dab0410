"""The resampler measured on the MI355X -> profiles/resize/.

    python tools/resize_probe.py all [--out DIR]      every step below, each a process of its own under its own time limit,
                                                       chained: the first step that fails ends the run
    python tools/resize_probe.py case NAME [frames]   1080p frames through Net.submit_pix(out_size=...) with three in flight: the
                                                       run `rocprofv3 --kernel-trace --stats` profiles (a run of its own per case:
                                                       two cases can share a kernel instantiation)
    python tools/resize_probe.py route [frames]       tools/rawvideo_pix_bench.py's form, yuv420p both ways, `-s 2` without and
                                                       with --out-size 2560x1440, alternated three times, profiler off

Kernel times: microseconds per launch and effective TB/s over the compulsory bytes (the source read once + the result written
once).  Route: the resized route's best wall against the unresized route's best wall and the spread of the three unresized runs."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 1080, 1920
# name -> (net, bit depth, output size or None)
CASES = {
    "plain_u8": ("2x_Compact_Pretrain", 8, None), "plain_u16": ("2x_Compact_Pretrain", 16, None),
    "2160_to_1440_u8": ("2x_Compact_Pretrain", 8, (1440, 2560)), "2160_to_1440_u16": ("2x_Compact_Pretrain", 16, (1440, 2560)),
    "2160_to_1620_u8": ("2x_Compact_Pretrain", 8, (1620, 2880)), "2160_to_1620_u16": ("2x_Compact_Pretrain", 16, (1620, 2880)),
    "4320_to_2160_u8": ("4x_Compact_Pretrain", 8, (2160, 3840)), "4320_to_2160_u16": ("4x_Compact_Pretrain", 16, (2160, 3840)),
}


def run_case(name, frames):
    from upscale_video_amd import ncnn
    from upscale_video_amd.rawvideo import load_net
    from upscale_video_amd.synth import synthetic_frame
    stem, depth, size = CASES[name]
    net = load_net(stem, 0, os.path.join(ROOT, "models"))
    s = net.scale
    fmt = "yuv420p10le" if depth == 16 else "yuv420p"
    ins = []
    for i in range(4):
        buf = ncnn.pix_empty(fmt, H, W, ncnn.pinned_empty)
        buf[...] = ncnn.convert_pix(synthetic_frame(H, W, seed=i), H, W, "bgr24", fmt, bit_depth=depth)
        ins.append(buf)
    oh, ow = size or (H * s, W * s)
    outs = [ncnn.pix_empty(fmt, oh, ow, ncnn.pinned_empty) for _ in range(3)]
    kw = {"bit_depth": 16} if depth == 16 else {}
    if size:
        kw["out_size"] = size
    inflight, t0 = [], None
    for i in range(frames + 5):
        if i == 5:
            while inflight:
                net.collect_u8(inflight.pop(0))
            t0 = time.perf_counter()
        if len(inflight) == 3:
            net.collect_u8(inflight.pop(0))
        inflight.append(net.submit_pix(ins[i % 4], H, W, fmt, out=outs[i % 3], out_fmt=fmt, tile_size=960, border=10, **kw))
    while inflight:
        net.collect_u8(inflight.pop(0))
    dt = time.perf_counter() - t0
    print("%s: %s %d-bit, 1080p -> %dx -> %dx%d %s: %d frames in %.3f s = %.1f frames/s"
          % (name, stem, depth, s, ow, oh, fmt, frames, dt, frames / dt), flush=True)


def run_route(frames):
    from upscale_video_amd import ncnn
    from upscale_video_amd.synth import synthetic_frame
    src = "/dev/shm/uva_resize_in.yuv420p"
    packed = [ncnn.convert_pix(synthetic_frame(H, W, seed=i), H, W, "bgr24", "yuv420p").tobytes() for i in range(4)]
    with open(src, "wb") as o:
        for i in range(frames):
            o.write(packed[i % 4])
    base = [sys.executable, "-m", "upscale_video_amd.rawvideo", "-W", str(W), "-H", str(H), "-s", "2", "--in-pix-fmt", "yuv420p",
            "--out-pix-fmt", "yuv420p"]
    variants = {"unresized (3840x2160 out)": [], "--out-size 2560x1440": ["--out-size", "2560x1440"]}

    def wall(cmd, shell=False):
        t0 = time.perf_counter()
        # (no timeout here: with one, subprocess polls and the wall comes in steps of 50 ms)
        subprocess.run(cmd, shell=shell, check=True, stderr=subprocess.DEVNULL, stdout=subprocess.DEVNULL if not shell else None, cwd=ROOT)
        return time.perf_counter() - t0
    try:
        walls = {(v, how): [] for v in variants for how in ("file", "pipe")}
        start = {v: wall(base + extra + ["-i", src, "-o", "/dev/null", "--frames", "1"]) for v, extra in variants.items()}
        for rnd in range(3):
            for v, extra in variants.items():
                walls[(v, "file")].append(wall(base + extra + ["-i", src, "-o", "/dev/null"]))
                walls[(v, "pipe")].append(wall("cat %s | %s 2>/dev/null | cat > /dev/null" % (src, " ".join(base + extra)), shell=True))
        print("rawvideo -s 2, 1080p yuv420p -> yuv420p, %d frames from /dev/shm, three alternated rounds (walls in s; rate = (frames - 1) / "
              "(best wall - the 1-frame run's wall))" % frames)
        ok = True
        for how, label in (("file", "file -> /dev/null"), ("pipe", "pipe -> pipe     ")):
            best = {}
            for v in variants:
                ws = walls[(v, how)]
                best[v] = min(ws)
                print("%s  %-26s walls %s  best %.2f  start-up %.2f  = %.1f frames/s"
                      % (label, v, " ".join("%.2f" % x for x in ws), min(ws), start[v], (frames - 1) / (min(ws) - start[v])))
            plain = walls[("unresized (3840x2160 out)", how)]
            spread = (max(plain) - min(plain)) / min(plain)
            margin = min(spread, 0.037)          # the README's box-to-box +-3.7 % is the ceiling of the margin
            excess = best["--out-size 2560x1440"] / best["unresized (3840x2160 out)"] - 1.0
            verdict = "within" if excess <= margin else "OUTSIDE"
            ok = ok and excess <= margin
            print("%s  resized best wall %+.1f %% against the unresized best; spread of the three unresized runs %.1f %% (margin %.1f %%): %s"
                  % (label, 100 * excess, 100 * spread, 100 * margin, verdict))
        print("route held" if ok else "route NOT held")
        return 0
    finally:
        os.remove(src)


def kernel_rows(stats_dir):
    """(kernel name, calls, average ns) of the resampler and the output conversions from rocprofv3's kernel_stats.csv"""
    rows = []
    for path in glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r.get("Name", "")
            if "resize_kernel" in name or "from_bgr" in name:
                rows.append((name, int(r["Calls"]), float(r["AverageNs"]), float(r["MinNs"]), float(r["MaxNs"])))
    return rows


def run_all(out):
    os.makedirs(out, exist_ok=True)
    py = sys.executable
    me = os.path.abspath(__file__)

    def step(cmd, limit, log=None):
        print("+ " + " ".join(cmd), flush=True)
        r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if log:
            open(os.path.join(out, log), "w").write(r.stdout)
        if r.returncode != 0:
            print(r.stdout[-3000:])
            print("step failed with exit status %d: stopping here" % r.returncode)
            sys.exit(r.returncode)
        return r.stdout
    lines = ["resampler kernels, rocprofv3 --kernel-trace --stats, one run per case (40 frames of 1080p yuv420p / yuv420p10le through",
             "Net.submit_pix, 960/10 tiles, three frames in flight); us per launch, effective TB/s over source read once + result written once", ""]
    import tempfile
    for name, (stem, depth, size) in CASES.items():
        with tempfile.TemporaryDirectory(prefix="uva_resize_prof_") as tmp:
            txt = step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "p", "--", py, me, "case", name, "40"], 240)
            lines.append([ln for ln in txt.splitlines() if ln.startswith(name)][-1])
            s = 4 if stem.startswith("4x") else 2
            bps = depth // 8
            for kname, calls, avg, mn, mx in sorted(kernel_rows(tmp)):
                oh, ow = size or (H * s, W * s)
                if "resize_kernel" in kname:
                    nbytes = (H * s * W * s + oh * ow) * 3 * bps
                else:       # BGR in, 4:2:0 out at the output size
                    nbytes = oh * ow * 3 * bps + oh * ow * 3 // 2 * bps
                lines.append("    %-60s %4d launches  avg %8.1f us  (min %.1f, max %.1f)  %.2f TB/s over %.1f MB"
                             % (kname[:60], calls, avg / 1e3, mn / 1e3, mx / 1e3, nbytes / avg / 1e3, nbytes / 1e6))
    open(os.path.join(out, "kernel_stats.txt"), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    print(step([py, me, "route", "600"], 600, "rawvideo_bench.txt"), flush=True)
    print(step([py, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "200", "--warmup", "20"], 600, "bench.txt"), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["all", "case", "route"])
    ap.add_argument("args", nargs="*")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize"))
    a = ap.parse_args()
    if a.mode == "case":
        run_case(a.args[0], int(a.args[1]) if len(a.args) > 1 else 40)
    elif a.mode == "route":
        sys.exit(run_route(int(a.args[0]) if a.args else 600))
    else:
        run_all(a.out)
