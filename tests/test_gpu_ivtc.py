"""Inverse telecine on the MI355X (-m gpu).  Everything is integer arithmetic and every comparison is bit
for bit: ivtc_metrics_kernel against tests/ivtc_ref.py for every format and field order, the stateful handle against the
reference on 2:3 pulldown streams, and the command line file to file against runs on the frames the reference gives back."""
import ctypes
import functools
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ivtc_ref as ref                  # noqa: E402
import yadif_ref                        # noqa: E402

pytestmark = pytest.mark.gpu

FORMATS = list(ref.FORMATS)
ORDERS = ["tff", "bff"]


@functools.lru_cache(maxsize=None)
def sequence(fmt, n, h, w, dirty=False):
    return tuple(yadif_ref.sequence_frames(fmt, n, h, w, seed=h * 100 + w + 1, dirty=dirty))


def neighbours(fr, k):
    return (fr[k - 1] if k else None), fr[k], (fr[k + 1] if k + 1 < len(fr) else None)


# ---- the kernel against the reference ---------------------------------------------------------------------------------------
# 4 x 1: two rows of the metric, rows of 1 ... 6 bytes; 5 x 7, 9 x 6: short ragged rows; 16 x 48: whole slots only for byte luma;
# 37 x 53: odd, ragged, rows at every alignment
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("h,w", [(4, 1), (5, 7), (9, 6), (16, 48), (37, 53)])
def test_metrics_against_the_reference(uva, fmt, h, w):
    n = 3
    fr = sequence(fmt, n, h, w, True)
    for order in ORDERS:
        for k in range(n):                          # first frame (prev None), middle frame, last frame (next None)
            want = ref.metrics(*neighbours(fr, k), fmt, h, w, order)
            got = uva.ivtc_metrics(*neighbours(fr, k), fmt, h, w, order)
            print(fmt, h, w, order, k, got)
            assert got == want, (fmt, h, w, order, k)
    assert uva.ivtc_metrics(*neighbours(fr, 1), fmt, h, w, "tff", thresh=0) == ref.metrics(*neighbours(fr, 1), fmt, h, w, "tff", 0)
    assert uva.ivtc_metrics(*neighbours(fr, 1), fmt, h, w, "bff", thresh=40) == ref.metrics(*neighbours(fr, 1), fmt, h, w, "bff", 40)


# 70 x 300: rows of 300, 600 or 1800 bytes start at every alignment that the sample width allows and end in ragged slots;
# 130 x 1030: several runs of slots per row and many rows -- on a grid of 3 workgroups or of 1 every wave walks many
@pytest.mark.parametrize("fmt", ["yuv420p", "p010le", "bgr48le"])
@pytest.mark.parametrize("h,w,max_groups", [(70, 300, None), (130, 1030, None), (130, 1030, 3), (130, 1030, 1)])
def test_metrics_on_larger_frames(uva, fmt, h, w, max_groups):
    fr = sequence(fmt, 3, h, w)
    for order in ORDERS:
        want = ref.metrics(fr[0], fr[1], fr[2], fmt, h, w, order)
        assert uva.ivtc_metrics(fr[0], fr[1], fr[2], fmt, h, w, order, max_groups=max_groups) == want, (fmt, h, w, order, max_groups)


def saturated(fmt, h, w):
    nb = ref.frame_bytes(fmt, h, w)
    top = {8: 255, 10: 1023, 16: 65535}[ref.depth(fmt)] << (6 if fmt == "p010le" else 0)
    zero = np.zeros(nb, np.uint8)
    full = (np.full(nb, top, np.uint8) if ref.depth(fmt) == 8 else np.full(nb // 2, top, "<u2").view(np.uint8))
    comb = full.copy()
    for off, ph, pw, st in ref.memory_planes(fmt, h, w):
        ref.words(comb, fmt)[off:off + ph * pw * st].reshape(ph, pw * st)[0::2] = 0
    return zero, full, comb


@pytest.mark.parametrize("fmt", ["yuv420p", "p010le", "bgr48le"])
def test_saturated_frames_on_one_workgroup(uva, fmt):
    """all 0, all maximum, rows alternating 0 / maximum -- every sample combed by the full range, the maximum of N and M -- with
    all of it added up by one workgroup's lanes"""
    h, w = 130, 1030
    zero, full, comb = saturated(fmt, h, w)
    _, ph, pw, st = ref.memory_planes(fmt, h, w)[0]
    top = (1 << ref.depth(fmt)) - 1
    for trio in ((zero, zero, zero), (full, full, full), (comb, comb, comb), (zero, comb, full), (comb, full, comb)):
        for order in ORDERS:
            want = ref.metrics(*trio, fmt, h, w, order)
            assert uva.ivtc_metrics(*trio, fmt, h, w, order, thresh=0, max_groups=1) == ref.metrics(*trio, fmt, h, w, order, 0)
            assert uva.ivtc_metrics(*trio, fmt, h, w, order, max_groups=1) == want
    assert ref.metrics(comb, comb, comb, fmt, h, w)[:2] == ((ph - 2) * pw * st, (ph - 2) * pw * st * top)


def test_frames_in_hbm(uva):
    import torch
    fmt, h, w = "p010le", 70, 300
    fr = sequence(fmt, 3, h, w)
    d = [torch.from_numpy(f.copy()).cuda() for f in fr]
    torch.cuda.synchronize()
    got = uva.ivtc_metrics(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), fmt, h, w, "bff", device=True)
    assert got == ref.metrics(fr[0], fr[1], fr[2], fmt, h, w, "bff")
    got = uva.ivtc_metrics(None, d[1].data_ptr(), None, fmt, h, w, device=True)
    assert got == ref.metrics(None, fr[1], None, fmt, h, w)


def test_a_null_neighbour_is_the_frame_itself(uva):
    fmt, h, w = "nv12", 37, 53
    fr = sequence(fmt, 3, h, w)
    a = uva.ivtc_metrics(None, fr[0], None, fmt, h, w)
    assert a == uva.ivtc_metrics(fr[0], fr[0], fr[0], fmt, h, w) == ref.metrics(None, fr[0], None, fmt, h, w)
    assert a[0:2] == a[2:4] == a[4:6]


# ---- the stateful handle ------------------------------------------------------------------------------------------------------
H, W, N = 48, 64, 20


@functools.lru_cache(maxsize=None)
def telecined(fmt, phase, order, h=H, w=W, n=N):
    film = ref.film_frames(fmt, 24, h, w, seed=7)
    return tuple(ref.pulldown(film, fmt, h, w, n, phase, order)[0])


def run_handle(dt, frames):
    """-> (delivered frames, frames produced per call: pushes, then flush steps)"""
    out = np.empty(frames[0].size, np.uint8)
    got, counts = [], []
    for f in frames:
        counts.append(dt.push(f, out))
        if counts[-1]:
            got.append(out.copy())
    while True:
        counts.append(dt.flush(out))
        if not counts[-1]:
            return got, counts
        got.append(out.copy())


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, x) for g, x in zip(got, want))


@pytest.mark.parametrize("fmt", ["yuv420p", "p010le", "bgr24"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("phase", [0, 2, 4])
def test_handle_against_the_reference(uva, fmt, order, phase):
    video = telecined(fmt, phase, order)
    want, info = ref.detelecine(video, fmt, H, W, order)
    assert len(want) == 16
    with uva.Detelecine(fmt, H, W, order) as dt:
        out = np.empty(video[0].size, np.uint8)
        assert dt.flush(out) == 0                                    # nothing pushed: nothing to flush
        got, counts = run_handle(dt, video)
        assert set(counts) <= {0, 1} and counts[-1] == 0 and sum(counts) == 16
        assert same(got, want), (fmt, order, phase, info["match"])
        assert tuple(dt.stats().values()) == info["stats"]
        # a second stream after the flush equals a fresh handle's; the counters go on
        want2, info2 = ref.detelecine(video[3:15], fmt, H, W, order)
        again, _ = run_handle(dt, video[3:15])
        assert same(again, want2)
        assert tuple(dt.stats().values()) == tuple(a + b for a, b in zip(info["stats"], info2["stats"]))
        # reset in mid-stream forgets the frames pushed and the open cycle
        for f in video[:7]:
            dt.push(f, out)
        dt.reset()
        third, _ = run_handle(dt, video[3:15])
        assert same(third, want2)


def test_handle_keep_all(uva):
    fmt, order = "yuv420p", "tff"
    video = telecined(fmt, 2, order)
    want, info = ref.detelecine(video, fmt, H, W, order, keep_all=True)
    assert len(want) == N
    with uva.Detelecine(fmt, H, W, order, keep_all=True) as dt:
        got, counts = run_handle(dt, video)
        assert same(got, want) and sum(counts) == N
        assert tuple(dt.stats().values()) == info["stats"] and dt.stats()["dropped"] == 0


def test_handle_combed_policies(uva):
    """one truly interlaced frame spliced into the stream: no candidate matches, `keep` leaves the woven frame, `yadif` puts
    yadif's output A of the same three frames in its place"""
    fmt, order = "yuv420p", "tff"
    video = list(telecined(fmt, 0, order))
    k = 8
    video[k] = yadif_ref.sequence_frames(fmt, 2, H, W, seed=5)[1]
    want_a = yadif_ref.deinterlace(video[k - 1], video[k], video[k + 1], fmt, H, W, order)[0]
    outs = {}
    for policy in ("keep", "yadif"):
        want, info = ref.detelecine(video, fmt, H, W, order, combed=policy, keep_all=True)
        assert info["combed"][k]
        with uva.Detelecine(fmt, H, W, order, combed=policy, keep_all=True) as dt:
            got, _ = run_handle(dt, video)
            assert same(got, want) and dt.stats()["combed"] == sum(info["combed"])
        outs[policy] = got[k]
    assert np.array_equal(outs["yadif"], want_a) and not np.array_equal(outs["keep"], want_a)
    # with decimation too
    want, info = ref.detelecine(video, fmt, H, W, order)
    with uva.Detelecine(fmt, H, W, order) as dt:
        got, _ = run_handle(dt, video)
        assert same(got, want) and tuple(dt.stats().values()) == info["stats"]


def test_push_between_flush_steps_is_refused(uva):
    fmt = "yuv420p"
    video = telecined(fmt, 0, "tff")
    out = np.empty(video[0].size, np.uint8)
    with uva.Detelecine(fmt, H, W) as dt:
        for f in video[:3]:
            dt.push(f, out)
        assert dt.flush(out) == 1
        with pytest.raises(Exception, match="flush"):
            dt.push(video[3], out)
        while dt.flush(out):
            pass
        assert dt.push(video[3], out) == 0


# ---- the route ------------------------------------------------------------------------------------------------------------------
SIZE = ["-W", str(W), "-H", str(H)]
YUV = ["--in-pix-fmt", "yuv420p", "--out-pix-fmt", "yuv420p"]


@pytest.fixture(scope="module")
def films(tmp_path_factory):
    """the 20-frame pulldown stream as a file, and the reference's 16 frames next to it"""
    d = tmp_path_factory.mktemp("ivtc")
    video = telecined("yuv420p", 0, "tff")
    want, _ = ref.detelecine(video, "yuv420p", H, W)
    src, pre = d / "video.raw", d / "film.raw"
    src.write_bytes(b"".join(f.tobytes() for f in video))
    pre.write_bytes(b"".join(f.tobytes() for f in want))
    return d, str(src), str(pre)


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_cli_gives_the_bytes_of_a_run_on_the_film_frames(uva, films, capfd):
    from upscale_video_amd import rawvideo
    d, src, pre = films
    out_a, out_b = str(d / "a.raw"), str(d / "b.raw")
    assert rawvideo.main(["-i", pre, "-o", out_a, "-s", "2"] + SIZE + YUV) == 0
    capfd.readouterr()
    assert rawvideo.main(["-i", src, "-o", out_b, "-s", "2", "--detelecine"] + SIZE + YUV) == 0
    err = capfd.readouterr().err
    want = read(out_a)
    assert len(want) == 16 * uva.pix_frame_bytes("yuv420p", 2 * H, 2 * W) and read(out_b) == want
    assert "detelecine: 20 frames in, 16 out" in err and "4 dropped" in err
    # --frames counts input frames: 12 in, 10 out
    want12, _ = ref.detelecine(telecined("yuv420p", 0, "tff")[:12], "yuv420p", H, W)
    (d / "film12.raw").write_bytes(b"".join(f.tobytes() for f in want12))
    assert rawvideo.main(["-i", str(d / "film12.raw"), "-o", out_a, "-s", "2"] + SIZE + YUV) == 0
    assert rawvideo.main(["-i", src, "-o", out_b, "-s", "2", "--detelecine", "--frames", "12"] + SIZE + YUV) == 0
    assert len(read(out_a)) == 10 * uva.pix_frame_bytes("yuv420p", 2 * H, 2 * W) and read(out_b) == read(out_a)


def test_cli_copy_through_is_a_detelecine_only_run(uva, films):
    from upscale_video_amd import rawvideo
    d, src, pre = films
    out = str(d / "c.raw")
    assert rawvideo.main(["-i", src, "-o", out, "-s", "1", "--detelecine"] + SIZE + YUV) == 0
    assert read(out) == read(pre)


def test_cli_two_lanes_on_one_file_take_the_frames_round_robin(uva, films, capfd, monkeypatch):
    from upscale_video_amd import rawvideo
    d, src, pre = films
    monkeypatch.setenv("UVA_RAW_TMPFS_SEGMENTS", "1")        # (segments would be taken also where the output lies on tmpfs)
    out_a, out_b = str(d / "e.raw"), str(d / "f.raw")
    assert rawvideo.main(["-i", pre, "-o", out_a, "-s", "2"] + SIZE + YUV) == 0
    capfd.readouterr()
    assert rawvideo.main(["-i", src, "-o", out_b, "-s", "2", "-g", "0,0", "--detelecine"] + SIZE + YUV) == 0
    assert "round-robin" in capfd.readouterr().err
    assert read(out_b) == read(out_a)


def test_pipe_form(uva, films):
    from conftest import load_net
    from upscale_video_amd import rawvideo
    d, src, pre = films
    pix = rawvideo.PixFormats("yuv420p", "yuv420p")
    nets = [(load_net(uva, "2x"), 0)]
    want, got = io.BytesIO(), io.BytesIO()
    assert rawvideo.stream(io.BytesIO(read(pre)), want, H, W, nets, pix=pix) == 16
    spec = rawvideo.DetelecineSpec()
    assert rawvideo.stream(io.BytesIO(read(src)), got, H, W, nets, pix=pix, deint=spec) == 16
    assert got.getvalue() == want.getvalue()
    assert spec.totals["frames_in"] == 20 and spec.totals["dropped"] == 4


# ---- nothing stays behind -----------------------------------------------------------------------------------------------------
def _live():
    from upscale_video_amd import _lib
    c = (ctypes.c_longlong * 4)()
    _lib.load().uva_debug_live_resources(c)
    return list(c)


def _child():
    from upscale_video_amd import ncnn
    before = _live()
    video = telecined("yuv420p", 0, "tff")
    dt = ncnn.Detelecine("yuv420p", H, W)
    got, _ = run_handle(dt, video)
    during = _live()
    dt.close()
    after_close = _live()
    ncnn.destroy_gpu_instance()
    print(json.dumps(dict(before=before, during=during, after_close=after_close, after=_live(), frames=len(got))))


def test_a_fresh_process_leaves_no_resources(uva):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    res = json.loads(r.stdout.strip().split("\n")[-1])
    assert res["frames"] == 16
    assert res["before"] == [0, 0, 0, 0] and res["after"] == [0, 0, 0, 0] and res["after_close"] == [0, 0, 0, 0]
    # three source frames, a ring of ten, the sums; one stream
    assert res["during"] == [14, 0, 1, 0]


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    _child()
