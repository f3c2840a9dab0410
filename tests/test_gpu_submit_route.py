"""The pipelined host route's options together in one call (-m gpu).  Every option has a test of its own
next to its kernels (test_gpu_pixfmt, _bitdepth16, _resize, _repeat, _crop, _png16); here they meet: the 16-bit route, an input
window narrower than the frame (the column compaction), an output size and skip-repeats in the same submit, tiled 32 / 10 --
byte for byte against the composition of the separate calls (test_gpu_resize._composition) on the host-cropped frame."""
import numpy as np
import pytest

import cropdetect_ref as crop
from conftest import load_net
from test_gpu_crop import random_frame, submit_all
from test_gpu_resize import _composition

pytestmark = pytest.mark.gpu

SH, SW = 40, 56                     # the source frame
X, Y, H, W = 8, 4, 32, 40           # the window: narrower than the frame, so its columns are compacted on the GPU
SIZE, FILT = (2 * H - 10, 2 * W + 6), "bicubic"


@pytest.mark.parametrize("pinned", [False, True])
def test_16_bit_window_with_columns_sized_and_skip_repeats_in_one_call(uva, pinned):
    net = load_net(uva, "2x")
    in_fmt, out_fmt = "p010le", "yuv422p10le"
    kw = dict(in_fmt=in_fmt, out_fmt=out_fmt, bit_depth=16, tile_size=32, border=10, out_size=SIZE, resize_filter=FILT)
    rng = np.random.default_rng(31)
    distinct = [random_frame(uva, in_fmt, SH, SW, rng) for _ in range(3)]
    order = (0, 0, 1, 1, 1, 2, 0)                       # a stream that repeats frames: four run, three are skipped
    want = [_composition(uva, net, crop.window(f, in_fmt, SH, SW, X, Y, H, W), H, W, in_fmt, out_fmt, SIZE, 32, 10, 16, FILT).tobytes()
            for f in distinct]
    assert len(set(want)) == 3 and len(want[0]) == uva.pix_frame_bytes(out_fmt, *SIZE)
    ring = [uva.pinned_empty((uva.pix_frame_bytes(in_fmt, SH, SW),)) for _ in range(4)] if pinned else None
    net.set_input_window(SH, SW, X, Y)
    try:
        net.set_skip_repeats(0)
        # a small window first, so that the kept frame's buffers are live and too small when the real calls arrive: they move
        small = dict(kw, out_size=None)
        a, b = submit_all(net, [distinct[0]] * 2, 8, 8, small, ring)
        assert a == b and net.skip_stats() == (2, 1)
        got = submit_all(net, [distinct[i] for i in order], H, W, kw, ring)
        assert got == [want[i] for i in order]
        assert net.skip_stats() == (2 + 7, 1 + 3)
        # skipping off: the same bytes from seven runs
        net.set_skip_repeats(None)
        assert submit_all(net, [distinct[i] for i in order], H, W, kw, ring) == [want[i] for i in order]
    finally:
        net.set_skip_repeats(None)
        net.set_input_window()
