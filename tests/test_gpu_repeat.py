"""Repeated frames on the MI355X (-m gpu): the frame-difference kernel against the numpy restatement
(tests/repeat_ref.py), all three numbers equal; sequences with repeats through submit / collect, every frame's bytes those the
same net gives, skipping off, for the frame the restatement says it repeats; the kept result overwritten while skipped frames
still download it; the kept frame living on the device; and the streamer end to end, byte for byte the run without the option."""
import io

import numpy as np
import pytest

import repeat_ref as ref
from conftest import load_net
from upscale_video_amd import rawvideo

pytestmark = pytest.mark.gpu

THRESHOLDS = (0, 1, 2, 255)
KERNEL_CASES = [("bgr24", 9, 17), ("bgr24", 48, 64), ("yuv420p", 34, 66), ("p010le", 48, 64), ("yuv422p10le", 10, 18), ("bgr48le", 7, 33),
                ("bgr24", 1080, 1920)]


def _random_frame(fmt, h, w, rng):
    """raw bytes of one frame with legal code values everywhere (10-bit formats: the bits the converter ignores are zero)"""
    n = ref.frame_bytes(fmt, h, w)
    if fmt in ref.EIGHT_BIT:
        return rng.integers(0, 256, n, dtype=np.uint8)
    words = rng.integers(0, 65536 if fmt == "bgr48le" else 1024, n // 2).astype("<u2")
    if fmt == "p010le":
        words = (words << 6).astype("<u2")
    return words.view(np.uint8).copy()


def _step(fmt):
    """one code value, in the units of the stored sample"""
    return 64 if fmt == "p010le" else 1


def _add_codes(frame, fmt, index, codes):
    """a copy of `frame` whose sample `index` is moved by `codes` code values (towards the middle of the range: no wrap)"""
    out = frame.copy()
    v = out if fmt in ref.EIGHT_BIT else out.view("<u2")
    top = 255 if fmt in ref.EIGHT_BIT else (65535 if fmt in ("bgr48le", "p010le") else 1023)
    d = codes * _step(fmt)
    v[index] = v[index] + d if int(v[index]) + d <= top else v[index] - d
    return out


def _check(uva, a, b, fmt, h, w, what):
    d = np.abs(ref.samples(a, fmt, h, w) - ref.samples(b, fmt, h, w))
    for t in THRESHOLDS:
        want = (int((d > t).sum()), int(d.max()), int(d.sum()))
        got = uva.frame_diff(a, b, fmt, h, w, threshold=t)
        assert got == want, (what, fmt, h, w, t, got, want)


@pytest.mark.parametrize("fmt,h,w", KERNEL_CASES)
def test_kernel_against_numpy(uva, fmt, h, w):
    import torch
    rng = np.random.default_rng(h * 131 + w)
    nbytes = ref.frame_bytes(fmt, h, w)
    bps = 1 if fmt in ref.EIGHT_BIT else 2
    nsamples = nbytes // bps
    a = _random_frame(fmt, h, w, rng)
    _check(uva, a, a.copy(), fmt, h, w, "equal frames")
    _check(uva, a, _add_codes(a, fmt, 0, 1), fmt, h, w, "first sample")
    _check(uva, a, _add_codes(a, fmt, nsamples - 1, 3), fmt, h, w, "last sample")
    # each of the 16 byte positions of a unit: the frame's last whole unit, and in the small frames one of its middle
    units = nbytes // 16
    for unit in sorted({units // 2 if nbytes < (1 << 20) else units - 1, max(units - 1, 0)}) if units else []:
        for pos in range(16):
            b = a.copy()
            b[unit * 16 + pos] ^= 0x41      # bit 6 and bit 0: a code bit in either byte of every 16-bit format, 65 or 1 codes in a byte
            _check(uva, a, b, fmt, h, w, "unit %d byte %d" % (unit, pos))
    if nbytes % 16:                          # the last partial unit: its first sample, and all of it
        first = units * 16 // bps
        _check(uva, a, _add_codes(a, fmt, first, 2), fmt, h, w, "partial unit, first sample")
        b = a.copy()
        for i in range(first, nsamples):
            b = _add_codes(b, fmt, i, 1 + i % 3)
        _check(uva, a, b, fmt, h, w, "partial unit, every sample")
    else:
        assert (fmt, h, w) != KERNEL_CASES[0]
    # random pairs: a near one (differences of 0 ... 3 codes, where the thresholds 0, 1, 2 part) and an unrelated one
    v = a if bps == 1 else a.view("<u2")
    top = 255 if bps == 1 else (65535 if fmt in ("bgr48le", "p010le") else 1023)
    delta = rng.integers(0, 4, nsamples) * _step(fmt)
    near = np.where(v.astype(np.int64) + delta <= top, v.astype(np.int64) + delta, v.astype(np.int64) - delta).astype(v.dtype).view(np.uint8)
    _check(uva, a, near, fmt, h, w, "near pair")
    far = _random_frame(fmt, h, w, rng)
    _check(uva, a, far, fmt, h, w, "random pair")
    if fmt == "p010le":                      # bits the converter ignores cannot break a repeat
        low = (a.view("<u2") | rng.integers(0, 64, nsamples).astype("<u2")).view(np.uint8)
        assert not np.array_equal(low, a)
        for t in THRESHOLDS:
            assert uva.frame_diff(a, low, fmt, h, w, threshold=t) == (0, 0, 0)
    if fmt == "yuv422p10le":
        high = (a.view("<u2") | (rng.integers(0, 64, nsamples) << 10).astype("<u2")).view(np.uint8)
        assert uva.frame_diff(a, high, fmt, h, w) == (0, 0, 0)
    # the device entry on the same frames
    da, dn, df = (torch.from_numpy(x.copy()).cuda() for x in (a, near, far))
    torch.cuda.synchronize()
    for t in THRESHOLDS:
        for dx, x in ((dn, near), (df, far), (da, a)):
            assert uva.frame_diff(da.data_ptr(), dx.data_ptr(), fmt, h, w, threshold=t, device=True) == uva.frame_diff(a, x, fmt, h, w, threshold=t)


# ---- sequences through submit / collect ---------------------------------------------------------------------------------

H, W = 40, 48


def _config(uva, name):
    """-> (net, input format, submit(frame, out), out buffer maker(alloc))"""
    if name == "2x bgr24":
        net = load_net(uva, "2x")
        return net, "bgr24", lambda f, out: net.submit_u8(f.reshape(H, W, 3), out=out), lambda alloc: uva.pix_empty("bgr24", 2 * H, 2 * W, alloc)
    if name == "2x yuv420p -> nv12":
        net = load_net(uva, "2x")
        return (net, "yuv420p", lambda f, out: net.submit_pix(f, H, W, "yuv420p", out=out, out_fmt="nv12"),
                lambda alloc: uva.pix_empty("nv12", 2 * H, 2 * W, alloc))
    if name == "4x p010le 16 bit":
        net = load_net(uva, "4x")
        return (net, "p010le", lambda f, out: net.submit_pix(f, H, W, "p010le", out=out, out_fmt="p010le", bit_depth=16),
                lambda alloc: uva.pix_empty("p010le", 4 * H, 4 * W, alloc))
    if name == "1x":
        net = load_net(uva, "1x")
        return net, "bgr24", lambda f, out: net.submit_u8(f.reshape(H, W, 3), out=out), lambda alloc: uva.pix_empty("bgr24", H, W, alloc)
    if name == "2x tiles 16/4":
        net = load_net(uva, "2x")
        return (net, "bgr24", lambda f, out: net.submit_u8(f.reshape(H, W, 3), out=out, tile_size=16, border=4),
                lambda alloc: uva.pix_empty("bgr24", 2 * H, 2 * W, alloc))
    assert name == "2x out_size"
    net = load_net(uva, "2x")
    return (net, "bgr24", lambda f, out: net.submit_pix(f, H, W, "bgr24", out=out, out_fmt="bgr24", out_size=(60, 100), resize_filter="bicubic"),
            lambda alloc: uva.pix_empty("bgr24", 60, 100, alloc))


def _run(net, frames, submit, mk_out, depth, alloc=None, pin_in=None):
    """the frames through submit / collect with `depth` of them in flight and a ring of result buffers, as rawvideo.Stage does;
    -> the bytes of every result"""
    ring = [mk_out(alloc) for _ in range(2 * depth + 2)]
    if pin_in is not None:                     # page-locked inputs as well: copied from directly, alive until collected
        held = []
        for f in frames:
            p = pin_in((f.size,))
            p[...] = f
            held.append(p)
        frames = held
    inflight, got = [], []
    for k, f in enumerate(frames):
        if len(inflight) == depth:
            got.append(net.collect_u8(inflight.pop(0)).tobytes())
        inflight.append(submit(f, ring[k % len(ring)]))
    while inflight:
        got.append(net.collect_u8(inflight.pop(0)).tobytes())
    return got


def _baseline(net, distinct, submit, mk_out):
    """skipping off: the bytes the net gives for every distinct frame"""
    net.set_skip_repeats(None)
    return _run(net, distinct, submit, mk_out, 1)


def _twelve(fmt, rng):
    """A A A B B' B'' C A A C C B, B' and B'' being B plus one and plus two codes in one sample -> (distinct frames, sequence of
    indices into them)"""
    a, b, c = (_random_frame(fmt, H, W, rng) for _ in range(3))
    at = 777
    distinct = [a, b, _add_codes(b, fmt, at, 1), _add_codes(b, fmt, at, 2), c]
    assert ref.frame_diff(distinct[1], distinct[3], fmt, H, W, 1) == (1, 2, 2)
    return distinct, [0, 0, 0, 1, 2, 3, 4, 0, 0, 4, 4, 1]


@pytest.mark.parametrize("name", ["2x bgr24", "2x yuv420p -> nv12", "4x p010le 16 bit", "1x", "2x tiles 16/4", "2x out_size"])
def test_sequences_with_repeats(uva, name):
    net, fmt, submit, mk_out = _config(uva, name)
    distinct, order = _twelve(fmt, np.random.default_rng(len(name)))
    frames = [distinct[i] for i in order]
    base = _baseline(net, distinct, submit, mk_out)
    assert len({base[0], base[1], base[4]}) == 3             # A, B and C have results of their own: a wrong one would show
    for t in (0, 1):
        kept = ref.kept_indices(frames, fmt, H, W, t)
        assert kept == ([0, 0, 0, 3, 4, 5, 6, 7, 7, 9, 9, 11] if t == 0 else [0, 0, 0, 3, 3, 5, 6, 7, 7, 9, 9, 11])
        want = [base[order[i]] for i in kept]
        for depth in (1, 3):
            for alloc, pin_in in ((None, None), (uva.pinned_empty, uva.pinned_empty)):
                net.set_skip_repeats(t)
                got = _run(net, frames, submit, mk_out, depth, alloc, pin_in)
                for k in range(len(frames)):
                    assert got[k] == want[k], (name, t, depth, alloc is not None, k)
                assert net.skip_stats() == (len(frames), ref.skipped(kept)), (name, t, depth)
    net.set_skip_repeats(None)
    assert _run(net, frames, submit, mk_out, 3) == [base[i] for i in order]
    assert net.skip_stats() == (0, 0)


def test_kept_result_overwritten_while_skipped_frames_download(uva):
    """three frames in flight: a frame that runs overwrites the kept result on the net's stream while the downloads of the frames
    that repeated the old one are still queued on the download stream"""
    net, fmt, submit, mk_out = _config(uva, "2x bgr24")
    rng = np.random.default_rng(40)
    distinct = [_random_frame(fmt, H, W, rng) for _ in range(4)]
    base = _baseline(net, distinct, submit, mk_out)
    order = [0]
    for _ in range(39):
        order.append(order[-1] if rng.random() < 0.6 else int((order[-1] + 1 + rng.integers(0, 3)) % 4))
    assert len(set(order)) == 4 and any(x == y for x, y in zip(order, order[1:]))
    for seq in (order, [0, 0, 1, 1, 0, 0]):
        frames = [distinct[i] for i in seq]
        kept = ref.kept_indices(frames, fmt, H, W, 0)
        for alloc in (None, uva.pinned_empty):
            net.set_skip_repeats(0)
            got = _run(net, frames, submit, mk_out, 3, alloc, alloc)
            assert got == [base[i] for i in seq]
            assert net.skip_stats() == (len(seq), ref.skipped(kept))
    assert ref.skipped(ref.kept_indices([distinct[i] for i in [0, 0, 1, 1, 0, 0]], fmt, H, W, 0)) == 3


def test_kept_frame_lives_on_the_device(uva):
    net, fmt, submit, mk_out = _config(uva, "2x yuv420p -> nv12")
    a = _random_frame(fmt, H, W, np.random.default_rng(4))
    want, = _baseline(net, [a], submit, mk_out)
    for alloc in (None, uva.pinned_empty):
        net.set_skip_repeats(0)
        out = mk_out(alloc)
        assert net.collect_u8(submit(a, out)).tobytes() == want
        out[...] = 0                                          # the caller reuses its ring: the kept frame's host bytes are gone
        assert net.collect_u8(submit(a, out)).tobytes() == want
        other = mk_out(alloc)
        other[...] = 7
        assert net.collect_u8(submit(a, other)).tobytes() == want
        assert net.skip_stats() == (3, 2)


def test_a_repeat_needs_equal_arguments(uva):
    net = load_net(uva, "2x")
    a = _random_frame("bgr24", H, W, np.random.default_rng(5))
    calls = [dict(out_fmt="bgr24", tile_size=0, border=0), dict(out_fmt="bgr24", tile_size=16, border=4), dict(out_fmt="nv12", tile_size=16, border=4),
             dict(out_fmt="nv12", tile_size=16, border=2), dict(out_fmt="nv12", tile_size=16, border=2, colour="bt709")]

    def go(kw):
        return net.collect_u8(net.submit_pix(a, H, W, "bgr24", **kw)).tobytes()
    base = [go(kw) for kw in calls]
    assert len(base[2]) != len(base[1])
    net.set_skip_repeats(0)
    for n, kw in enumerate(calls):
        assert go(kw) == base[n]
        assert net.skip_stats() == (2 * n + 1, n)             # other arguments: the frame runs
        assert go(kw) == base[n]
        assert net.skip_stats() == (2 * n + 2, n + 1)         # the same ones: it repeats
    # the synchronous calls take no part
    assert np.array_equal(net.process_u8(a.reshape(H, W, 3)), net.process_u8(a.reshape(H, W, 3)))
    assert net.skip_stats() == (2 * len(calls), len(calls))


def test_state_and_counters(uva):
    net, fmt, submit, mk_out = _config(uva, "2x bgr24")
    a = _random_frame(fmt, H, W, np.random.default_rng(6))
    # never set: twelve equal frames, none skipped
    got = _run(net, [a] * 12, submit, mk_out, 3)
    assert len(set(got)) == 1 and net.skip_stats() == (0, 0)
    net.set_skip_repeats(0)
    assert _run(net, [a] * 3, submit, mk_out, 1) == got[:3] and net.skip_stats() == (3, 2)
    net.reset_reference()                                      # the next frame runs whatever it holds
    assert _run(net, [a] * 2, submit, mk_out, 1) == got[:2] and net.skip_stats() == (5, 3)
    net.set_skip_repeats(0)                                    # setting it forgets the kept frame and zeroes the counters
    assert _run(net, [a] * 2, submit, mk_out, 1) == got[:2] and net.skip_stats() == (2, 1)
    net.set_skip_repeats(None)
    assert _run(net, [a] * 2, submit, mk_out, 1) == got[:2] and net.skip_stats() == (0, 0)
    # the drift x, x + 1, x + 2 at T = 1: the third frame runs (the comparison is with the kept frame)
    drift = [a, _add_codes(a, fmt, 5, 1), _add_codes(a, fmt, 5, 2)]
    base = _baseline(net, drift, submit, mk_out)
    net.set_skip_repeats(1)
    assert _run(net, drift, submit, mk_out, 3) == [base[0], base[0], base[2]] and net.skip_stats() == (3, 1)


@pytest.mark.parametrize("route", ["-s 2", "-m a -s 2", "yuv420p"])
def test_streamer_end_to_end(uva, route, tmp_path, capsys):
    fmt = "yuv420p" if route == "yuv420p" else "bgr24"
    distinct, order = _twelve(fmt, np.random.default_rng(70))
    frames = [distinct[i] for i in order]
    data = b"".join(f.tobytes() for f in frames)
    models = rawvideo.MODEL_FILES
    import os
    mp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "models")
    chain = ([(rawvideo.load_net(models[1], 0, mp), 0)] if route == "-m a -s 2" else []) + [(rawvideo.load_net(models[2], 0, mp), 32)]
    pix = rawvideo.PixFormats(fmt, fmt)

    def go():
        fout = io.BytesIO()
        assert rawvideo.stream(io.BytesIO(data), fout, H, W, chain, pix=pix) == len(frames)
        return fout.getvalue()
    want = go()
    assert len(want) == 12 * ref.frame_bytes(fmt, 2 * H, 2 * W)
    rawvideo.set_skip_repeats(chain, 0)
    assert go() == want
    k = ref.skipped(ref.kept_indices(frames, fmt, H, W, 0))
    assert k == 4
    if len(chain) == 2:         # the second stage finds the repeats itself, in the first stage's results
        mid = [chain[0][0].process_u8(f.reshape(H, W, 3)) for f in distinct]
        k += ref.skipped(ref.kept_indices([mid[i] for i in order], "bgr24", H, W, 0))
        assert k >= 8
    assert rawvideo.skip_summary(chain) == "skipped %d of %d" % (k, 12 * len(chain))
    if route != "-s 2":
        return
    # ... and the command line: the same bytes, the count in the closing line
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(data)
    argv = ["-i", str(src), "-o", str(dst), "-W", str(W), "-H", str(H), "-s", "2", "--tile", "32"]
    capsys.readouterr()
    assert rawvideo.main(argv + ["--skip-repeats"]) == 0
    assert "12 frames, skipped 4 of 12" in capsys.readouterr().err and dst.read_bytes() == want
    assert rawvideo.main(argv) == 0
    err = capsys.readouterr().err
    assert "12 frames" in err and "skipped" not in err and dst.read_bytes() == want
