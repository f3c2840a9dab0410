"""Repeated frames without a GPU: the numpy restatement (tests/repeat_ref.py) on hand-made cases, the
command line's refusals, uva_net_set_skip_repeats' range checks and counters, the exported symbols, and the compute entries
failing loudly when there is no device."""
import ctypes

import numpy as np
import pytest

import repeat_ref as ref
from conftest import load_net
from upscale_video_amd import rawvideo


def _bgr(h, w, v=0):
    return np.full((h, w, 3), v, np.uint8)


def test_restatement_counts_bytes():
    a = _bgr(2, 3, 10)
    b = a.copy()
    assert ref.frame_diff(a, b, "bgr24", 2, 3, 0) == (0, 0, 0)
    b[0, 0, 0] = 13                   # +3
    b[1, 2, 2] = 9                    # -1
    assert ref.frame_diff(a, b, "bgr24", 2, 3, 0) == (2, 3, 4)
    assert ref.frame_diff(a, b, "bgr24", 2, 3, 1) == (1, 3, 4)
    assert ref.frame_diff(a, b, "bgr24", 2, 3, 3) == (0, 3, 4)
    assert ref.frame_diff(b, a, "bgr24", 2, 3, 1) == (1, 3, 4)


def test_restatement_reads_the_code_the_converter_reads():
    h, w = 2, 2
    n = ref.frame_bytes("p010le", h, w) // 2
    assert n == 6 and ref.frame_bytes("yuv422p10le", h, w) == 16 and ref.frame_bytes("yuv420p", 3, 3) == 9 + 8
    a = (np.arange(n, dtype=np.uint16) * 37 + 5) << 6
    b = a | 0x3f                                     # the low six bits of p010le carry nothing
    assert ref.frame_diff(a, b, "p010le", h, w, 0) == (0, 0, 0)
    b = a.copy()
    b[3] += 2 << 6
    assert ref.frame_diff(a, b, "p010le", h, w, 0) == (1, 2, 2) and ref.frame_diff(a, b, "p010le", h, w, 2) == (0, 2, 2)
    a = np.arange(n, dtype=np.uint16) * 100
    b = a | 0xfc00                                   # the high six bits of yuv420p10le carry nothing
    assert ref.frame_diff(a, b, "yuv420p10le", h, w, 0) == (0, 0, 0)
    a = np.zeros(6, np.uint16)
    b = a.copy()
    b[5] = 65535                                    # bgr48le: whole words
    assert ref.frame_diff(a, b, "bgr48le", 1, 2, 255) == (1, 65535, 65535)


def test_kept_indices_compare_with_the_kept_frame_not_the_predecessor():
    x = _bgr(2, 2, 100)
    drift = [x, x + 1, x + 2]
    assert ref.kept_indices(drift, "bgr24", 2, 2, 1) == [0, 0, 2]
    assert ref.kept_indices(drift, "bgr24", 2, 2, 0) == [0, 1, 2]
    assert ref.kept_indices(drift, "bgr24", 2, 2, 2) == [0, 0, 0]
    a, b = _bgr(2, 2, 1), _bgr(2, 2, 9)
    seq = [a, a, a, b, b, a, a]
    idx = ref.kept_indices(seq, "bgr24", 2, 2, 0)
    assert idx == [0, 0, 0, 3, 3, 5, 5] and ref.skipped(idx) == 4
    assert ref.kept_indices([], "bgr24", 2, 2, 0) == []


def test_cli_refusals(capsys, tmp_path):
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(2 * 8 * 8 * 3))
    io_args = ["-i", str(src), "-o", str(tmp_path / "out.raw")]
    cases = ((["--skip-repeats", "65536"], "0 ... 65535"), (["--skip-repeats", "-1"], "0 ... 65535"),
             (["--skip-repeats", "-g", "0,0"], "nothing would ever repeat"),                       # pipes: dealt one by one
             (io_args + ["--skip-repeats", "1", "-g", "0,0", "--round-robin"], "nothing would ever repeat"))
    for argv, msg in cases:
        with pytest.raises(SystemExit):
            rawvideo.main(["-W", "8", "-H", "8"] + argv)
        err = capsys.readouterr().err
        assert msg in err, (argv, err)
    assert "one -g entry" in err.replace("\n", " ") and "segments" in err


def test_set_skip_repeats_range_and_counters(uva):
    """host only: no device is touched"""
    net = load_net(uva, "2x")
    assert net.skip_stats() == (0, 0)
    for t in (0, 1, 255, 65535, -1, None):
        net.set_skip_repeats(t)
        assert net.skip_stats() == (0, 0)
    from upscale_video_amd._lib import UvaError
    for t in (-2, 65536, 1 << 20):
        with pytest.raises(UvaError, match="65535"):
            net.set_skip_repeats(t)
    net.reset_reference()
    L = uva._lib.load()
    assert L.uva_net_set_skip_repeats(None, 0) != 0 and L.uva_net_reset_reference(None) != 0
    assert L.uva_net_skip_stats(None, None, None) != 0


def test_new_symbols_are_exported():
    from upscale_video_amd import _lib, build
    build.build_lib()
    names = ("uva_frame_diff", "uva_frame_diff_device", "uva_net_set_skip_repeats", "uva_net_reset_reference", "uva_net_skip_stats")
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert n in _lib.SYMBOLS and hasattr(L, n), n
    assert "uva_repeat.hip" in build.SOURCES
    # every unit that calls the kernel's launcher: the submit stages (through uva_net.h), the generic executor that shares
    # uva_net.h with them, and the stateless uva_frame_diff entries
    for user in ("uva_api.hip", "uva_generic_run.hip", "uva_frames.hip"):
        assert "uva_repeat.h" in build.SOURCES[user], user


def test_frame_diff_refuses_bad_arguments_and_fails_loudly_without_gpu(uva):
    from upscale_video_amd._lib import UvaError
    L = uva._lib.load()
    a = np.zeros(12, np.uint8)
    st = (ctypes.c_ulonglong * 3)()
    bad = ((None, a.ctypes.data, 0, 2, 2, 0, "null"), (a.ctypes.data, a.ctypes.data, 4, 2, 2, 0, "unknown pixel format"),
           (a.ctypes.data, a.ctypes.data, 99, 2, 2, 0, "unknown pixel format"), (a.ctypes.data, a.ctypes.data, 0, 0, 2, 0, "size"),
           (a.ctypes.data, a.ctypes.data, 0, 2, 2, -1, "threshold"), (a.ctypes.data, a.ctypes.data, 0, 2, 2, 65536, "threshold"))
    for fn in (L.uva_frame_diff, L.uva_frame_diff_device):
        for pa, pb, fmt, h, w, t, msg in bad:
            assert fn(0, pa, pb, fmt, h, w, t, st) != 0
            assert msg in L.uva_last_error().decode(), (fmt, h, w, t)
        assert fn(0, a.ctypes.data, a.ctypes.data, 0, 2, 2, 0, None) != 0
    with pytest.raises(ValueError):
        uva.frame_diff(a, a, "rgb24", 2, 2)
    with pytest.raises(ValueError):
        uva.frame_diff(a, a[:11], "bgr24", 2, 2)
    if uva.get_gpu_count() == 0:
        with pytest.raises(UvaError, match="no HIP device|no CPU path"):
            uva.frame_diff(a, a, "bgr24", 2, 2)
