"""The PNG route at 16 bits on the MI355X (-m gpu): png_deflate_kernel16 against its host restatement,
byte for byte, and the net -> deflate -> download route (Net.submit_u16_png) against Net.process_u16, decoded by the independent
decoder of tests/png16_ref.py."""
import numpy as np
import pytest

from conftest import load_net
from png16_ref import decode16, frames, host_encode16
from upscale_video_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(frames()))
def test_kernel_equals_host_restatement(uva, name):
    img = frames()[name]
    h, w, _ = img.shape
    ws = uva.PngWorkspace(h, w, bit_depth=16)
    L = _lib.load()
    _lib.check(L.uva_png_deflate_u16(0, img.ctypes.data, h, w, w * 6, ws.buf.ctypes.data, ws.buf.nbytes))
    png = bytes(ws.file_bytes())
    ref, _ = host_encode16(img)
    assert png == ref
    np.testing.assert_array_equal(decode16(png), img)


def through_png(net, imgs, spaces, depth, **tiling):
    """the files of `imgs` with at most `depth` frames in flight, over the ring `spaces`"""
    tickets, got = [], []
    for i, im in enumerate(imgs):
        if len(tickets) == depth:
            got.append(bytes(net.collect_u8(tickets.pop(0)).file_bytes()))
        tickets.append(net.submit_u16_png(im, workspace=spaces[i % len(spaces)], **tiling))
    while tickets:
        got.append(bytes(net.collect_u8(tickets.pop(0)).file_bytes()))
    return got


@pytest.fixture(scope="module")
def net2x(uva):
    return load_net(uva, "2x")


@pytest.mark.parametrize("tiling", [dict(tile_size=0), dict(tile_size=64, border=10)], ids=["whole", "tiled"])
def test_2x_net_through_the_png_route_equals_process_u16(uva, net2x, tiling):
    rng = np.random.default_rng(21)
    imgs = [rng.integers(0, 65536, (96, 160, 3), dtype=np.uint16) for _ in range(5)]
    want = [net2x.process_u16(im, **tiling).copy() for im in imgs]
    spaces = [uva.PngWorkspace(192, 320, bit_depth=16) for _ in range(3)]
    for png, ref in zip(through_png(net2x, imgs, spaces, 3, **tiling), want):
        np.testing.assert_array_equal(decode16(png), ref)


def test_1x_net_whole_frame(uva):
    net = load_net(uva, "1x")
    img = np.random.default_rng(22).integers(0, 65536, (90, 161, 3), dtype=np.uint16)   # odd width: dense rows 966 bytes apart
    with pytest.raises(_lib.UvaError):
        net.submit_u16_png(img)                          # refused until asked for
    net.enable_u16_1x()
    with pytest.raises(_lib.UvaError, match="whole frames"):
        net.submit_u16_png(img, tile_size=64, border=10)
    want = net.process_u16(img).copy()
    png = bytes(net.collect_u8(net.submit_u16_png(img)).file_bytes())
    np.testing.assert_array_equal(decode16(png), want)


def alternate(uva, net, h, w, seed):
    """flat frames alternating with noise through `net`, one and three in flight: every file decodes to process_u16's frame;
    -> the file sizes of the last pass"""
    rng = np.random.default_rng(seed)
    imgs = [np.full((h, w, 3), 9000 * i + 4000, np.uint16) if i % 2 == 0 else rng.integers(0, 65536, (h, w, 3), dtype=np.uint16)
            for i in range(6)]
    want = [net.process_u16(im).copy() for im in imgs]
    s = net.scale
    spaces = [uva.PngWorkspace(h * s, w * s, bit_depth=16) for _ in range(3)]
    for depth in (1, 3):                                  # one at a time (the guess is always the previous frame), and pipelined
        got = through_png(net, imgs, spaces, depth, tile_size=0)
        for png, ref in zip(got, want):
            np.testing.assert_array_equal(decode16(png), ref)
        sizes = [len(g) for g in got]
        print("png16 alternate %dx net %dx%d depth %d: file sizes %s" % (s, w, h, depth, sizes))
    return sizes


def test_a_frame_that_compresses_worse_than_the_one_before_it(uva):
    """Flat frames (small files) alternate with noise (the largest): what a frame has beyond the guess that travelled with its
    download -- the previous frame's bytes + 1/16 + 64 KiB -- is fetched by collect_u8.
    Through the 1x net, 270 x 480: a flat frame's result is constant except in the band of about ten pixels along the edges that
    the ten convolutions' zero padding reaches, 11 % of this frame, so its file is near the 1-bit-per-byte floor and the noise
    files are more than 4x as large.  (Through the 2x net a flat frame's result is NOT flat at 16 bits: the four pixel-shuffle
    phases differ by a few hundred codes, every low-byte residual is one of two large values, and the file is half the raw size
    -- measured 0.28 to 0.52 of raw at 96 x 160 against 1.00 for noise; that net's case below only shows the path taken.)"""
    net = load_net(uva, "1x")
    net.enable_u16_1x()
    sizes = alternate(uva, net, 270, 480, 23)
    assert min(sizes[1::2]) > 4 * max(sizes[0::2])        # the test does alternate small and large


def test_worse_than_the_frame_before_through_the_2x_net(uva, net2x):
    """the same through the 2x net (see above for its sizes): the large files exceed the guess made from the small ones, so
    collect_u8 fetches the rest here too"""
    sizes = alternate(uva, net2x, 96, 160, 23)
    assert min(sizes[1::2]) > max(sizes[0::2]) * 17 // 16 + 65536


def test_8_and_16_bit_png_submits_interleaved_on_one_net(uva, net2x):
    from PIL import Image
    import io
    rng = np.random.default_rng(24)
    img8 = rng.integers(0, 256, (96, 160, 3), dtype=np.uint8)
    img16 = rng.integers(0, 65536, (96, 160, 3), dtype=np.uint16)
    want8, want16 = net2x.process_u8(img8).copy(), net2x.process_u16(img16).copy()
    ws8, ws16 = uva.PngWorkspace(192, 320), uva.PngWorkspace(192, 320, bit_depth=16)
    for _ in range(2):                                    # the second round starts from the first round's guesses
        t8 = net2x.submit_u8_png(img8, workspace=ws8)
        t16 = net2x.submit_u16_png(img16, workspace=ws16)
        png8 = bytes(net2x.collect_u8(t8).file_bytes())
        png16 = bytes(net2x.collect_u8(t16).file_bytes())
        with Image.open(io.BytesIO(png8)) as im:
            assert im.mode == "RGB"
            np.testing.assert_array_equal(np.asarray(im)[:, :, ::-1], want8)
        np.testing.assert_array_equal(decode16(png16), want16)
    with pytest.raises(ValueError):
        net2x.submit_u16_png(img16, workspace=ws8)        # a workspace of the other kind
