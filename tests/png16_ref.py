"""Shared by tests/test_png16.py and tests/test_gpu_png16.py: the u16 fixtures, the host restatement of the 16-bit PNG encoder
driven through the C ABI, and a decoder of 16-bit RGB PNGs that uses nothing of the library -- zlib for the stream, numpy for the
Sub filter (the encoder writes no other)."""
import ctypes
import functools
import struct
import zlib

import numpy as np

from upscale_video_amd import _lib


def smooth16(h, w):
    """three slow waves: a sample moves by a few hundred codes per pixel at most, so high bytes change by 0 or +-1 and low
    bytes run through all values -- what a net's 16-bit result looks like away from edges"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([32768 + 20000 * np.sin(xx / 37.0 + yy / 53.0), 30000 + 25000 * np.cos(xx / 61.0 - yy / 29.0),
                     33000 + 30000 * np.sin(xx / 83.0 + 1.0) * np.cos(yy / 71.0)], -1).round().astype(np.uint16)


def noisy16(h, w, rng):
    return np.clip(smooth16(h, w).astype(np.int64) + rng.integers(-6, 7, (h, w, 3)), 0, 65535).astype(np.uint16)


def widened(h, w):
    """8-bit values widened x257: the high and the low byte of every sample are equal"""
    return (smooth16(h, w) >> 8).astype(np.uint16) * np.uint16(257)


@functools.lru_cache(maxsize=None)
def frames():
    rng = np.random.default_rng(16)
    r16 = lambda h, w: rng.integers(0, 65536, (h, w, 3), dtype=np.uint16)   # noqa: E731
    f = {
        "smooth": smooth16(97, 131),                     # odd width: the row stride, 786 bytes, is no multiple of 4
        "noisy": noisy16(97, 131, rng),
        "random": r16(64, 200),
        "flat": np.full((33, 17, 3), 32896, np.uint16),
        "1x1": np.array([[[1, 258, 65535]]], np.uint16),
        "one_row": r16(1, 500),
        "many_blocks": r16(40, 2500),                    # 3 rows per block, ragged last block
        "narrow_tall": r16(5200, 3),                     # thousands of short rows per block
        "one_wide_stage_bound": r16(7100, 1),            # 8 staged bytes per 7 filtered ones: the staging area bounds the block's rows
        "widest": r16(2, 8191),
        "widened": widened(97, 131),
        "low_bytes_zero": r16(50, 77) & np.uint16(0xff00),
        "high_bytes_zero": r16(50, 77) & np.uint16(0x00ff),
        "black_and_white": rng.integers(0, 2, (45, 64, 3)).astype(np.uint16) * np.uint16(65535),
    }
    for a in f.values():
        a.setflags(write=False)
    return f


def host_encode16(img):
    """-> (file bytes, workspace) from uva_debug_png_deflate_host16 + uva_png_assemble16"""
    L = _lib.load()
    img = np.ascontiguousarray(img, np.uint16)
    h, w, _ = img.shape
    n = L.uva_png_workspace_bytes16(h, w)
    assert n > 0
    ws = np.zeros(n, np.uint8)
    assert L.uva_debug_png_deflate_host16(img.ctypes.data, h, w, w * 6, ws.ctypes.data, n) == 0, L.uva_last_error()
    ln = ctypes.c_size_t(0)
    L.uva_png_assemble16(ws.ctypes.data, h, w, None, 0, ln)          # size query
    out = np.zeros(ln.value, np.uint8)
    assert L.uva_png_assemble16(ws.ctypes.data, h, w, out.ctypes.data, out.size, ln) == 0, L.uva_last_error()
    return out.tobytes(), ws


def chunks(png):
    """[(kind, body)] with every chunk CRC checked against zlib.crc32"""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(png):
        n, = struct.unpack(">I", png[pos:pos + 4])
        kind, body = png[pos + 4:pos + 8], png[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        out.append((kind, body))
        pos += 12 + n
    assert pos == len(png)
    return out


def filtered_rows(png):
    """-> (h, w, the decompressed scanlines [h][1 + 6w]) of a file the 16-bit encoder wrote"""
    ch = chunks(png)
    assert [k for k, _ in ch] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", ch[0][1])
    assert (depth, ctype, comp, filt, lace) == (16, 2, 0, 0, 0)
    raw = zlib.decompress(ch[1][1])                                  # (checks the combined Adler-32)
    assert len(raw) == h * (6 * w + 1)
    return h, w, np.frombuffer(raw, np.uint8).reshape(h, 6 * w + 1)


def decode16(png):
    """the u16 BGR frame of a file the 16-bit encoder wrote"""
    h, w, rows = filtered_rows(png)
    assert (rows[:, 0] == 1).all()                                   # every scanline: filter type Sub
    d = rows[:, 1:].reshape(h, w, 6)
    be = np.cumsum(d, axis=1, dtype=np.uint64).astype(np.uint8)      # Sub undone: running sums over pixels, mod 256
    rgb = np.ascontiguousarray(be).view(">u2").reshape(h, w, 3)
    return rgb[:, :, ::-1].astype(np.uint16)


def idat_bytes(png):
    return sum(len(b) for k, b in chunks(png) if k == b"IDAT")
