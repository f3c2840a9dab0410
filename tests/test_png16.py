"""The PNG route at 16 bits, CPU part: the 16-bit encoder's tables, block headers, checksum
combination and framing through the host restatement of png_deflate_kernel16 (uva_debug_png_deflate_host16) and an independent
decoder (tests/png16_ref.py: zlib + numpy); the 16-bit reader (uva_png_decode_bgr16) on files written here with zlib and struct;
the workspace rules; the size of the files against zlib's own; _imageio and the frame pool at bit_depth 16."""
import ctypes
import io
import os
import struct
import zlib

import numpy as np
import pytest

from png16_ref import chunks, decode16, filtered_rows, frames, host_encode16, idat_bytes, noisy16, smooth16, widened
from upscale_video_amd import _imageio, _lib


# ---- the host restatement, decoded independently ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(frames()))
def test_host_restatement_decodes_to_the_frame(name):
    img = frames()[name]
    png, _ = host_encode16(img)
    h, w, rows = filtered_rows(png)                      # chunk walk, CRCs, IHDR 16 / 2, zlib.decompress (Adler-32)
    assert (h, w) == img.shape[:2]
    assert (rows[:, 0] == 1).all()
    np.testing.assert_array_equal(decode16(png), img)
    from PIL import Image
    with Image.open(io.BytesIO(png)) as im:              # Pillow opens it; what it keeps of a 16-bit RGB file is the high bytes
        assert im.size == (w, h)
        np.testing.assert_array_equal(np.asarray(im.convert("RGB"))[:, :, ::-1], (img >> 8).astype(np.uint8))


# ---- the reader ----------------------------------------------------------------------------------------------------------
def paeth(a, b, c):
    p = a.astype(int) + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def write_png(pix, depth, ctype, filters=(0, 1, 2, 3, 4), idat_split=None):
    """pix: [h][w][channels] of u8 / u16 samples in file order; one filter type per line, cycling through `filters`"""
    h, w, ch = pix.shape
    raw = (pix.astype(">u2").view(np.uint8) if depth == 16 else pix.astype(np.uint8)).reshape(h, -1).astype(int)
    bpp = ch * depth // 8
    out = bytearray()
    prev = np.zeros(raw.shape[1], int)
    for y in range(h):
        cur = raw[y]
        left = np.concatenate([np.zeros(bpp, int), cur[:-bpp]]) if cur.size > bpp else np.zeros(cur.size, int)
        upleft = np.concatenate([np.zeros(bpp, int), prev[:-bpp]]) if cur.size > bpp else np.zeros(cur.size, int)
        ft = filters[y % len(filters)]
        pred = [np.zeros_like(cur), left, prev, (left + prev) // 2, paeth(left, prev, upleft)][ft]
        out.append(ft)
        out += ((cur - pred) % 256).astype(np.uint8).tobytes()
        prev = cur
    z = zlib.compress(bytes(out), 6)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    parts = [z] if not idat_split else [z[:idat_split], z[idat_split:]]
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0)) +
            b"".join(chunk(b"IDAT", p) for p in parts) + chunk(b"IEND", b""))


def read16(png, cap=None):
    L = _lib.load()
    h, w = ctypes.c_int(0), ctypes.c_int(0)
    rc = L.uva_png_decode_bgr16(png, len(png), None, 0, h, w)
    if rc:
        return rc, None
    out = np.zeros((h.value, w.value, 3), np.uint16)
    rc = L.uva_png_decode_bgr16(png, len(png), out.ctypes.data, out.nbytes if cap is None else cap, h, w)
    return rc, out


SHAPES = [(1, 1), (1, 7), (9, 1), (37, 53)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["rgb", "rgba", "grey"])
def test_reader_takes_every_filter_type_at_16_bits(shape, kind):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    ch, ctype = {"rgb": (3, 2), "rgba": (4, 6), "grey": (1, 0)}[kind]
    pix = rng.integers(0, 65536, shape + (ch,), dtype=np.uint16)
    want = np.repeat(pix, 3, 2) if ch == 1 else pix[:, :, 2::-1]
    for filters in ((0, 1, 2, 3, 4), (4, 3, 2, 1, 0), (3,), (4,)):
        rc, got = read16(write_png(pix, 16, ctype, filters, idat_split=5 if filters == (3,) else None))
        assert rc == 0, _lib.load().uva_last_error()
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name", sorted(frames()))
def test_reader_reads_back_what_the_host_restatement_wrote(name):
    rc, got = read16(host_encode16(frames()[name])[0])
    assert rc == 0, _lib.load().uva_last_error()
    np.testing.assert_array_equal(got, frames()[name])


@pytest.mark.parametrize("kind", ["rgb", "rgba", "grey", "grey_alpha"])
def test_reader_widens_8_bit_files_by_257(kind):
    rng = np.random.default_rng(8)
    ch, ctype = {"rgb": (3, 2), "rgba": (4, 6), "grey": (1, 0), "grey_alpha": (2, 4)}[kind]
    pix = rng.integers(0, 256, (23, 31, ch), dtype=np.uint8)
    png = write_png(pix, 8, ctype)
    want8 = np.repeat(pix[:, :, :1], 3, 2) if ch <= 2 else pix[:, :, 2::-1]
    rc, got = read16(png)
    assert rc == 0
    np.testing.assert_array_equal(got, want8.astype(np.uint16) * 257)
    # ... and is the 8-bit reader's frame, widened
    L = _lib.load()
    h, w = ctypes.c_int(0), ctypes.c_int(0)
    out8 = np.zeros((23, 31, 3), np.uint8)
    assert L.uva_png_decode_bgr(png, len(png), out8.ctypes.data, out8.size, h, w) == 0
    np.testing.assert_array_equal(got, out8.astype(np.uint16) * 257)


def test_the_8_bit_reader_still_declines_16_bit_files():
    L = _lib.load()
    png, _ = host_encode16(frames()["smooth"])
    h, w = ctypes.c_int(0), ctypes.c_int(0)
    assert L.uva_png_decode_bgr(png, len(png), None, 0, h, w) == 2


def test_reader_declines_what_it_does_not_take():
    pix = np.zeros((4, 4, 1), np.uint8)
    for depth, ctype in ((8, 3), (4, 0), (16, 3)):
        png = bytearray(write_png(pix, 8, 0))
        ihdr = bytearray(chunks(bytes(png))[0][1])
        ihdr[8], ihdr[9] = depth, ctype
        png[16:29] = ihdr
        png[29:33] = struct.pack(">I", zlib.crc32(b"IHDR" + bytes(ihdr)) & 0xFFFFFFFF)
        assert read16(bytes(png))[0] == 2


def rebuilt(png, edit):
    """the file with edit(kind, body) applied to every chunk and the chunk CRCs made right again"""
    out = bytearray(png[:8])
    for kind, body in chunks(png):
        body = edit(kind, bytearray(body))
        out += struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + bytes(body)) & 0xFFFFFFFF)
    return bytes(out)


def test_reader_refuses_damaged_files():
    L = _lib.load()
    png, _ = host_encode16(frames()["noisy"])
    assert read16(png)[0] == 0
    for cut in (0, 7, 20, 40, len(png) // 2, len(png) - 13, len(png) - 1):
        assert read16(png[:cut])[0] == 1                              # truncation
    bad = bytearray(png)
    bad[len(png) // 2] ^= 0x10
    assert read16(bytes(bad))[0] == 1                                 # a flipped bit: chunk CRC
    assert b"CRC" in L.uva_last_error()

    def wrong_adler(kind, body):
        if kind == b"IDAT":
            body[-1] ^= 1
        return body
    assert read16(rebuilt(png, wrong_adler))[0] == 1                  # a wrong Adler-32 behind a right chunk CRC
    assert b"Adler" in L.uva_last_error()

    def huge(kind, body):
        if kind == b"IHDR":
            body[0:8] = struct.pack(">II", 1 << 24, 1 << 24)
        return body
    h, w = ctypes.c_int(0), ctypes.c_int(0)
    lie = rebuilt(png, huge)
    assert L.uva_png_decode_bgr16(lie, len(lie), None, 0, h, w) == 1   # refused on the size query: nothing to allocate from
    assert b"larger than its data" in L.uva_last_error()
    buf = np.zeros(16, np.uint16)
    assert L.uva_png_decode_bgr16(lie, len(lie), buf.ctypes.data, 1 << 60, h, w) == 1
    # an output buffer that is too small is an error, not an overrun
    assert read16(png, cap=97 * 131 * 6 - 2)[0] == 1


# ---- workspace rules ------------------------------------------------------------------------------------------------------
def test_workspace_rules():
    L = _lib.load()
    assert L.uva_png_workspace_bytes16(10, 8192) == 0                 # one filtered row, 6w + 1 bytes, must fit a block
    assert L.uva_png_workspace_bytes16(10, 8191) > 0
    assert L.uva_png_workspace_bytes16(0, 10) == 0
    assert L.uva_png_workspace_bytes16(4320, 7680) > 0
    ln = ctypes.c_size_t(0)
    ws = np.zeros(L.uva_png_workspace_bytes16(8, 8), np.uint8)
    assert L.uva_png_assemble16(ws.ctypes.data, 8, 8, None, 0, ln) != 0     # never filled: refused, not framed
    assert b"kernel not run" in L.uva_last_error()


def test_a_workspace_is_framed_only_by_its_own_kind():
    L = _lib.load()
    ln = ctypes.c_size_t(0)
    out = np.zeros(1 << 20, np.uint8)
    img16 = frames()["smooth"]
    h, w, _ = img16.shape
    _, ws16 = host_encode16(img16)
    assert L.uva_png_assemble(ws16.ctypes.data, h, w, out.ctypes.data, out.size, ln) != 0
    assert b"16-bit encoder" in L.uva_last_error()
    img8 = (img16 >> 8).astype(np.uint8)
    n8 = L.uva_png_workspace_bytes(h, w)
    ws8 = np.zeros(max(n8, L.uva_png_workspace_bytes16(h, w)), np.uint8)
    assert L.uva_debug_png_deflate_host(img8.ctypes.data, h, w, w * 3, ws8.ctypes.data, n8) == 0
    assert L.uva_png_assemble16(ws8.ctypes.data, h, w, out.ctypes.data, out.size, ln) != 0
    assert b"8-bit encoder" in L.uva_last_error()
    assert L.uva_png_assemble(ws8.ctypes.data, h, w, out.ctypes.data, out.size, ln) == 0      # ... and still by its own


# ---- size --------------------------------------------------------------------------------------------------------------
def zlib_rle_bytes(rows):
    """what cv2.imwrite runs on the same filtered bytes: level 1, Z_RLE"""
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return len(c.compress(rows.tobytes()) + c.flush())


SIZE_FRAMES = {
    "smooth": lambda: smooth16(256, 256),
    "noisy": lambda: noisy16(256, 256, np.random.default_rng(3)),
    "widened": lambda: widened(256, 256),
}
# zlib's size x 1.05: the margin covers the per-block headers and sync flushes its single stream does not pay.  The widened
# frame misses that with any fixed table set -- its residuals take five values of nearly equal weight, zlib builds the code for
# exactly those, the encoder picks among fixed Laplacian shapes --: its bar is the measured ratio, 1.2188
# (profiles/png16/sizes.txt), + 0.02
SIZE_BARS = {"smooth": 1.05, "noisy": 1.05, "widened": 1.2388}


@pytest.mark.parametrize("name", sorted(SIZE_FRAMES))
def test_size_against_zlib_on_the_same_filtered_bytes(name):
    img = SIZE_FRAMES[name]()
    png, _ = host_encode16(img)
    _, _, rows = filtered_rows(png)
    ours, theirs = idat_bytes(png), zlib_rle_bytes(rows)
    print("png16 size %s: IDAT %d bytes, zlib level 1 Z_RLE %d bytes, ratio %.4f, of raw %.4f" % (name, ours, theirs, ours / theirs, ours / img.nbytes))
    assert ours <= theirs * SIZE_BARS[name], (name, ours / theirs)


def test_size_bars_that_follow_from_the_construction():
    flat = np.full((256, 256, 3), 32896, np.uint16)
    png, _ = host_encode16(flat)
    assert len(png) / flat.nbytes <= 0.14                             # >= 1 bit per byte, + the blocks' headers
    rnd = np.random.default_rng(4).integers(0, 65536, (256, 256, 3), dtype=np.uint16)
    png, _ = host_encode16(rnd)
    assert len(png) / rnd.nbytes <= 1.15                              # the flattest table costs <= 9 bits per byte


# ---- _imageio ---------------------------------------------------------------------------------------------------------------
def test_imageio_round_trip_at_16_bits(tmp_path):
    img = frames()["noisy"]
    path = str(tmp_path / "a.png")
    assert _imageio.imwrite(path, img)
    back = _imageio.imread(path, bit_depth=16)
    assert back.dtype == np.uint16
    np.testing.assert_array_equal(back, img)
    if _imageio._cv2 is None:                            # the host writer's file is the encoder's kind: Sub on every line
        np.testing.assert_array_equal(decode16(open(path, "rb").read()), img)
    # an 8-bit file read at 16 bits: widened; an unreadable one: None
    img8 = (img >> 8).astype(np.uint8)
    assert _imageio.imwrite(path, img8)
    np.testing.assert_array_equal(_imageio.imread(path, bit_depth=16), img8.astype(np.uint16) * 257)
    np.testing.assert_array_equal(_imageio.imread(path), img8)
    open(path, "wb").write(b"not a png")
    assert _imageio.imread(path, bit_depth=16) is None
    assert _imageio.imread(str(tmp_path / "missing.png"), bit_depth=16) is None


# ---- the frame pool -----------------------------------------------------------------------------------------------------
@pytest.fixture
def fake16(monkeypatch, tmp_path):
    from upscale_video_amd import upscale_processing as up
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(up, "PERSISTENT_WORKERS", True)
    monkeypatch.setattr(up, "NET_FACTORY", "png16_fake_net:make")
    yield up, str(tmp_path)
    up.shutdown_workers()


def test_frame_pool_takes_16_bit_tasks(fake16, monkeypatch):
    up, path = fake16
    rng = np.random.default_rng(1)
    f16 = {n: rng.integers(300, 60000, (6, 10, 3), dtype=np.uint16) for n in (1, 2, 3)}
    for n, img in f16.items():
        img[0, 0, 0] = n
        _imageio.imwrite("%d.extract.png" % n, img)
    monkeypatch.setattr(up, "BIT_DEPTH", 16)
    up.upscale_frames(1, 1, 3, "extract", 2, [0], 0, path, "x_fake", "input", "output")
    for n, img in f16.items():
        want = np.repeat(np.repeat(img, 2, 0), 2, 1) + 1
        assert not os.path.exists("%d.extract.png" % n)
        data = open("%d.png" % n, "rb").read()
        assert struct.unpack(">IIBB", chunks(data)[0][1][:10])[2:] == (16, 2)          # a 16-bit RGB file
        np.testing.assert_array_equal(_imageio.imread("%d.png" % n, bit_depth=16), want)
    seen = [line.split() for line in open(os.path.join(path, "dtypes.txt"))]
    assert sorted(int(s[0]) for s in seen) == [1, 2, 3] and all(s[1:] == ["uint16", "uint16"] for s in seen)
    # a task without the key -- BIT_DEPTH 8 puts none in -- on the same pool: 8 bits in, 8 bits out, as before
    monkeypatch.setattr(up, "BIT_DEPTH", 8)
    img8 = rng.integers(0, 200, (6, 10, 3), dtype=np.uint8)
    img8[0, 0, 0] = 9
    _imageio.imwrite("9.extract.png", img8)
    up.upscale_frames(1, 9, 9, "extract", 2, [0], 0, path, "x_fake", "input", "output")
    data = open("9.png", "rb").read()
    assert struct.unpack(">IIBB", chunks(data)[0][1][:10])[2:] == (8, 2)
    np.testing.assert_array_equal(_imageio.imread("9.png"), np.repeat(np.repeat(img8, 2, 0), 2, 1) + 1)
    seen = [line.split() for line in open(os.path.join(path, "dtypes.txt"))]
    assert seen[-1] == ["9", "uint8", "uint8"]


def test_what_the_16_bit_route_does_not_have_is_refused_with_a_reason(fake16, monkeypatch):
    up, path = fake16
    monkeypatch.setattr(up, "BIT_DEPTH", 16)
    with pytest.raises(ValueError, match="no 16-bit denoise"):
        up.process_denoise(3, "extract", 5)
    with pytest.raises(ValueError, match="-m r"):
        up.upscale_frames(1, 1, 3, "extract", 4, [0], 0, path, "x_Valar_v1", "input", "output")
    monkeypatch.setattr(up, "PERSISTENT_WORKERS", False)
    with pytest.raises(ValueError, match="PERSISTENT_WORKERS"):
        up.process_model(3, path, "x_fake", 1, "input", "output", "extract", "anime", [0], 0)
