"""Drop-in for the slice of `from ncnn_vulkan import ncnn` that davlee1972/upscale_video uses,
backed by the MI355X HIP engine (libuva.so, include/uva.h).

The reference touches exactly these names (upscale/upscale_processing.py:65-73, :265-281,
:292, :437-453, :458; test_gpus.py:47-67):

    ncnn.Net(); net.opt.use_vulkan_compute; net.set_vulkan_device(i)
    net.load_param(path); net.load_model(path)
    ncnn.Mat.from_pixels(arr, ncnn.Mat.PixelType.PIXEL_BGR, w, h)
    mat.substract_mean_normalize(mean_vals, norm_vals)
    ex = net.create_extractor(); ex.input(name, mat); ret, mat_out = ex.extract(name)
    np.array(mat_out)
    ncnn.destroy_gpu_instance(); ncnn.get_gpu_count(); ncnn.get_default_gpu_index()
    ncnn.get_gpu_info(i).type() / .device_name()

Same names, argument meaning and error behaviour (load_*/extract return 0 on success).  Mat is a
host-side f32 planar container like ncnn::Mat; all network arithmetic runs in HIP kernels.  There
is no CPU path: without an MI355X every extract raises.
"""
import ctypes

import numpy as np

from . import _lib


def get_gpu_count():
    """test_gpus.py:47"""
    return _lib.load().uva_get_gpu_count()


def get_default_gpu_index():
    """test_gpus.py:53"""
    return _lib.load().uva_get_default_gpu_index()


class GpuInfo:
    def __init__(self, type_, name):
        self._type, self._name = type_, name

    def type(self):
        return self._type

    def device_name(self):
        return self._name


def get_gpu_info(i):
    """test_gpus.py:59-66"""
    t = ctypes.c_int()
    name = ctypes.create_string_buffer(256)
    _lib.check(_lib.load().uva_get_gpu_info(i, t, name, 256))
    return GpuInfo(t.value, name.value.decode())


def destroy_gpu_instance():
    """upscale_processing.py:292, :458"""
    _lib.load().uva_destroy_gpu_instance()


def pinned_empty(shape, dtype=np.uint8):
    """numpy array in page-locked host memory (include/uva.h uva_host_alloc): frames held in such
    arrays are copied to / from the GPU without a staging copy by Net.submit_u8 / process_u8."""
    L = _lib.load()
    dt = np.dtype(dtype)
    nbytes = int(np.prod(shape)) * dt.itemsize
    ptr = L.uva_host_alloc(max(1, nbytes))
    if not ptr:
        raise _lib.UvaError(L.uva_last_error().decode(errors="replace"))
    buf = (ctypes.c_ubyte * max(1, nbytes)).from_address(ptr)
    arr = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)
    import weakref
    weakref.finalize(buf, L.uva_host_free, ptr)     # freed when the last view of the buffer dies
    return arr


class PngWorkspace:
    """Page-locked memory the GPU's PNG encoder writes an h x w frame's deflate blocks into (include/uva.h
    uva_png_workspace_bytes); file_bytes() frames them as a PNG file on the host (zlib / PNG headers, Adler-32, chunk
    CRC: include/uva.h uva_png_assemble -- no GPU call, the GIL is released).  bit_depth=16: a workspace of the 16-bit encoder
    (uva_png_workspace_bytes16 / uva_png_assemble16: u16 frames, 16-bit RGB files) -- the two kinds differ
    in size and layout, and the library refuses to frame one kind's blocks as the other's."""

    def __init__(self, h, w, bit_depth=8):
        L = _lib.load()
        if bit_depth not in (8, 16):
            raise ValueError("bit_depth must be 8 or 16")
        if bit_depth == 16 and not hasattr(L, "uva_png_workspace_bytes16"):
            raise _lib.UvaError("this libuva build has no 16-bit PNG encoder: rebuild it")
        self._size = L.uva_png_workspace_bytes16 if bit_depth == 16 else L.uva_png_workspace_bytes
        self._assemble = L.uva_png_assemble16 if bit_depth == 16 else L.uva_png_assemble
        n = self._size(h, w)
        if n == 0:
            raise ValueError("the GPU PNG encoder does not take %dx%d frames at %d bits" % (w, h, bit_depth))
        self.h, self.w, self.bit_depth = h, w, bit_depth
        self.buf = pinned_empty((n,), np.uint8)
        self._out = None

    def file_bytes(self):
        """-> memoryview of the PNG file image (valid until the next file_bytes() of this workspace)."""
        L = _lib.load()
        n = ctypes.c_size_t(0)
        self._assemble(self.buf.ctypes.data, self.h, self.w, None, 0, ctypes.byref(n))      # size query (fails by design)
        if n.value == 0:
            raise _lib.UvaError(L.uva_last_error().decode(errors="replace"))
        if self._out is None or len(self._out) < n.value:
            self._out = bytearray(n.value + n.value // 8)          # the next frame of the stream is about the same size
        dst = (ctypes.c_ubyte * len(self._out)).from_buffer(self._out)
        _lib.check(self._assemble(self.buf.ctypes.data, self.h, self.w, dst, len(self._out), ctypes.byref(n)))
        del dst
        return memoryview(self._out)[:n.value]


def png_encode_u8(img_bgr, gpu=0, workspace=None):
    """cv2.imwrite's encoder for a frame in host memory, run on the GPU (include/uva.h uva_png_deflate_u8): -> bytes
    of the PNG file."""
    img = np.ascontiguousarray(img_bgr, dtype=np.uint8)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("frame must be u8 [h][w][3]")
    h, w, _ = img.shape
    ws = workspace or PngWorkspace(h, w)
    _lib.check(_lib.load().uva_png_deflate_u8(int(gpu), img.ctypes.data, h, w, w * 3, ws.buf.ctypes.data, ws.buf.nbytes))
    return bytes(ws.file_bytes())


def png_encode_u16(img_bgr, gpu=0, workspace=None):
    """png_encode_u8 for a u16 BGR frame (include/uva.h uva_png_deflate_u16): -> bytes of a 16-bit RGB PNG file that every
    reader decodes to exactly the frame."""
    img = np.ascontiguousarray(img_bgr, dtype=np.uint16)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("frame must be u16 [h][w][3]")
    h, w, _ = img.shape
    ws = workspace or PngWorkspace(h, w, bit_depth=16)
    if ws.bit_depth != 16 or (ws.h, ws.w) != (h, w):
        raise ValueError("workspace must be a PngWorkspace(%d, %d, bit_depth=16)" % (h, w))
    _lib.check(_lib.load().uva_png_deflate_u16(int(gpu), img.ctypes.data, h, w, w * 6, ws.buf.ctypes.data, ws.buf.nbytes))
    return bytes(ws.file_bytes())


# ---- raw-video pixel formats (include/uva.h UVA_PIX_*) -----------------------------------------
PIX_FORMATS = {"bgr24": 0, "yuv420p": 1, "nv12": 2, "p010le": 3}     # ffmpeg's -pix_fmt names (the first four)
# every format the calls take: + yuv420p10le (both routes), bgr48le (u16 BGR: the 16-bit route's own, bit_depth=16) and the
# 4:2:2 formats yuv422p / yuv422p10le (both routes).  Kept apart so that PIX_FORMATS still lists exactly
# the formats of the first pixel-format release
PIX_FORMATS_ALL = dict(PIX_FORMATS, yuv420p10le=5, bgr48le=6, yuv422p=7, yuv422p10le=8)      # (code 4 is not assigned)
PIX16_ONLY = ("bgr48le",)


def pix_depth(fmt):
    """bits per sample of a rawvideo pixel format's frames: 8, 10 or 16"""
    if fmt not in PIX_FORMATS_ALL:
        raise ValueError("unknown pixel format %r (%s)" % (fmt, ", ".join(PIX_FORMATS_ALL)))
    return 16 if fmt == "bgr48le" else 10 if fmt in ("p010le", "yuv420p10le", "yuv422p10le") else 8


COLORSPACES = {"bt601": 0, "bt709": 1}                              # ffmpeg's -colorspace names
COLOR_RANGES = {"tv": 0, "pc": 2}                                   # ffmpeg's -color_range names (limited, full)
# 4:2:0 chroma resampling: replicate = chroma repeated over its 2x2 block coming in and the 2x2 box
# going out (sections 7.3, 7.4); bilinear = interpolated for where the chroma samples sit (ffmpeg's chroma_sample_location
# names; H.264 / HEVC video is left, JPEG / MPEG-1 center, UHD BT.2020 material topleft).  A 4:2:2 format takes the horizontal
# half of either (section 7.7): left and topleft are the same there
CHROMA_FILTERS = {"replicate": 0, "bilinear": 4}
CHROMA_LOCS = {"left": 0, "center": 8, "topleft": 16}
# the resampler's filters (include/uva.h UVA_RESIZE_*)
RESIZE_FILTERS = {"lanczos": 0, "bicubic": 1, "bilinear": 2}


def pix_frame_bytes(fmt, h, w):
    """bytes of one dense h x w rawvideo frame of `fmt` (chroma planes ceil(w/2) x ceil(h/2), ceil(w/2) x h for the 4:2:2
    formats; include/uva.h uva_pix_frame_bytes)"""
    if fmt not in PIX_FORMATS_ALL:
        raise ValueError("unknown pixel format %r (%s)" % (fmt, ", ".join(PIX_FORMATS_ALL)))
    if h <= 0 or w <= 0:
        raise ValueError("frame size must be positive")
    c = 2 * ((w + 1) // 2) * ((h + 1) // 2)
    c422 = 2 * ((w + 1) // 2) * h
    return {"bgr24": 3 * w * h, "yuv420p": w * h + c, "nv12": w * h + c, "p010le": 2 * (w * h + c), "yuv420p10le": 2 * (w * h + c),
            "bgr48le": 6 * w * h, "yuv422p": w * h + c422, "yuv422p10le": 2 * (w * h + c422)}[fmt]


def colour_word(colour="bt601", color_range="tv", chroma_filter="replicate", chroma_loc="left"):
    """the C ABI's colour argument: UVA_CSP_* | UVA_RANGE_FULL | UVA_CHROMA_BILINEAR | UVA_CHROMA_CENTER / _TOPLEFT"""
    if colour not in COLORSPACES:
        raise ValueError("unknown colorspace %r (%s)" % (colour, ", ".join(COLORSPACES)))
    if color_range not in COLOR_RANGES:
        raise ValueError("unknown color range %r (%s)" % (color_range, ", ".join(COLOR_RANGES)))
    if chroma_filter not in CHROMA_FILTERS:
        raise ValueError("unknown chroma filter %r (%s)" % (chroma_filter, ", ".join(CHROMA_FILTERS)))
    if chroma_loc not in CHROMA_LOCS:
        raise ValueError("unknown chroma location %r (%s)" % (chroma_loc, ", ".join(CHROMA_LOCS)))
    if chroma_filter == "replicate" and chroma_loc != "left":
        raise ValueError("chroma_loc %r needs chroma_filter='bilinear': replicate knows no siting" % chroma_loc)
    return COLORSPACES[colour] | COLOR_RANGES[color_range] | CHROMA_FILTERS[chroma_filter] | CHROMA_LOCS[chroma_loc]


def pix_empty(fmt, h, w, alloc=None):
    """a buffer for one h x w frame of `fmt`: u8 [h][w][3] for bgr24, u16 [h][w][3] for bgr48le, a flat u8 array of
    pix_frame_bytes otherwise.  `alloc(shape)` -> u8 array (default np.empty; pinned_empty for page-locked memory)"""
    alloc = alloc or (lambda shape: np.empty(shape, np.uint8))
    if fmt == "bgr48le":
        return alloc((h, w, 6)).view(np.uint16)
    return alloc((h, w, 3)) if fmt == "bgr24" else alloc((pix_frame_bytes(fmt, h, w),))


def _pix_frame(buf, fmt, h, w, what):
    a = np.ascontiguousarray(buf)
    if a.nbytes != pix_frame_bytes(fmt, h, w):
        raise ValueError("%s holds %d bytes, a %dx%d %s frame has %d" % (what, a.nbytes, w, h, fmt, pix_frame_bytes(fmt, h, w)))
    return a


def _bit_depth(bit_depth, fmts):
    if bit_depth not in (8, 16):
        raise ValueError("bit_depth must be 8 or 16")
    for f in fmts:
        if f not in PIX_FORMATS_ALL:
            raise ValueError("unknown pixel format %r (%s)" % (f, ", ".join(PIX_FORMATS_ALL)))
        if bit_depth == 8 and f in PIX16_ONLY:
            raise ValueError("%s is a 16-bit format: it needs bit_depth=16" % f)


def convert_pix(buf, h, w, in_fmt, out_fmt, colour="bt601", color_range="tv", out=None, gpu=0, bit_depth=8,
                chroma_filter="replicate", chroma_loc="left"):
    """One dense h x w frame of in_fmt -> out_fmt on HIP device `gpu`, host to host, synchronous (include/uva.h
    uva_pix_convert; bit_depth=16: uva_pix_convert16, through u16 BGR).  Returns `out` (pix_empty's
    array for out_fmt; allocated when None).  chroma_filter="bilinear": the Y'CbCr conversions interpolate chroma sited at chroma_loc
    (DESIGN.md section 7.5)."""
    _bit_depth(bit_depth, (in_fmt, out_fmt))
    cw = colour_word(colour, color_range, chroma_filter, chroma_loc)
    src = _pix_frame(buf, in_fmt, h, w, "input")
    if out is None:
        out = pix_empty(out_fmt, h, w)
    if not out.flags.c_contiguous or out.nbytes != pix_frame_bytes(out_fmt, h, w):
        raise ValueError("out must be a C-contiguous buffer of %d bytes" % pix_frame_bytes(out_fmt, h, w))
    fn = _lib.load().uva_pix_convert16 if bit_depth == 16 else _lib.load().uva_pix_convert
    _lib.check(fn(int(gpu), src.ctypes.data, PIX_FORMATS_ALL[in_fmt], out.ctypes.data, PIX_FORMATS_ALL[out_fmt], h, w, cw))
    return out


def _resize_filter(name):
    if name not in RESIZE_FILTERS:
        raise ValueError("unknown resize filter %r (%s)" % (name, ", ".join(RESIZE_FILTERS)))
    return RESIZE_FILTERS[name]


def _resize_axis(n_in, n_out, what):
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError("resize: %s must be at least 1 (%d -> %d)" % (what, n_in, n_out))
    if n_out * 4 < n_in or n_out > n_in * 4:
        raise ValueError("resize: %s %d -> %d is outside the ratios [1/4, 4]" % (what, n_in, n_out))


def resize_taps(n_in, n_out, filter="lanczos"):
    """The tap table of one axis as the library builds it on the host (include/uva.h uva_resize_taps; no GPU needed):
    -> (first int32 [n_out], taps int16 [n_out][T]); output sample d is sum_k taps[d][k] * in[clamp(first[d] + k)] / 2^14."""
    f = _resize_filter(filter)
    _resize_axis(n_in, n_out, "axis")
    L = _lib.load()
    t = ctypes.c_int(0)
    L.uva_resize_taps(int(n_in), int(n_out), f, None, None, 0, ctypes.byref(t))          # size query (fails by design)
    if t.value <= 0:
        raise _lib.UvaError(L.uva_last_error().decode(errors="replace"))
    first = np.empty(int(n_out), np.int32)
    taps = np.empty((int(n_out), t.value), np.int16)
    _lib.check(L.uva_resize_taps(int(n_in), int(n_out), f, first.ctypes.data, taps.ctypes.data, taps.size, ctypes.byref(t)))
    return first, taps


def resize(img, size, filter="lanczos", gpu=0, out=None):
    """A BGR frame, u8 or u16 [h][w][3], resampled to size = (oh, ow) on HIP device `gpu` (include/uva.h uva_resize; DESIGN.md
    section 7.6): separable lanczos / bicubic / bilinear with an anti-aliasing support, per axis within the ratios [1/4, 4].
    `img` and `out` may be row-padded views (last two axes contiguous); what lies between the rows of `out` is left alone."""
    f = _resize_filter(filter)
    a = np.asarray(img)
    if a.dtype not in (np.uint8, np.uint16) or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("frame must be u8 or u16 [h][w][3]")
    if a.strides[2] != a.itemsize or a.strides[1] != 3 * a.itemsize or a.strides[0] < a.shape[1] * 3 * a.itemsize:
        a = np.ascontiguousarray(a)
    oh, ow = (int(v) for v in size)
    h, w, _ = a.shape
    _resize_axis(h, oh, "height")
    _resize_axis(w, ow, "width")
    if out is None:
        out = np.empty((oh, ow, 3), a.dtype)
    if (out.dtype != a.dtype or out.shape != (oh, ow, 3) or out.strides[2] != a.itemsize or out.strides[1] != 3 * a.itemsize
            or out.strides[0] < ow * 3 * a.itemsize):
        raise ValueError("out must be a %s [%d][%d][3] array with contiguous rows" % (a.dtype, oh, ow))
    _lib.check(_lib.load().uva_resize(int(gpu), a.ctypes.data, h, w, a.strides[0], out.ctypes.data, oh, ow, out.strides[0], f,
                                      8 * a.itemsize))
    return out


def frame_diff(a, b, fmt, h, w, threshold=0, gpu=0, device=False):
    """Two dense h x w frames of `fmt` compared sample by sample on HIP device `gpu` (include/uva.h uva_frame_diff; DESIGN.md
    section 7.8) -> (over, max_abs, sad): the samples with |a - b| > threshold, the largest |a - b| and the sum of |a - b|, in
    code values as the input conversion reads them (p010le: word >> 6; yuv420p10le / yuv422p10le: word & 1023).
    device=True: a and b are raw device pointers (ints) of frames in that GPU's HBM (uva_frame_diff_device)."""
    if fmt not in PIX_FORMATS_ALL:
        raise ValueError("unknown pixel format %r (%s)" % (fmt, ", ".join(PIX_FORMATS_ALL)))
    stats = (ctypes.c_ulonglong * 3)()
    L = _lib.load()
    if device:
        _lib.check(L.uva_frame_diff_device(int(gpu), ctypes.c_void_p(int(a)), ctypes.c_void_p(int(b)), PIX_FORMATS_ALL[fmt], int(h), int(w),
                                           int(threshold), stats))
    else:
        fa, fb = _pix_frame(a, fmt, h, w, "a"), _pix_frame(b, fmt, h, w, "b")
        _lib.check(L.uva_frame_diff(int(gpu), fa.ctypes.data, fb.ctypes.data, PIX_FORMATS_ALL[fmt], int(h), int(w), int(threshold), stats))
    return int(stats[0]), int(stats[1]), int(stats[2])


# ---- crop detection and cropped frames (include/uva.h uva_crop_*, uva_pix_window) ------------------
def _crop_lib(name):
    L = _lib.load()
    if not hasattr(L, name):
        raise _lib.UvaError("this libuva build has no %s: rebuild it" % name)
    return L


def crop_sums(frame, fmt, h, w, gpu=0, device=False, max_groups=None):
    """The exact sums of every row and every column of a dense h x w frame of `fmt` -- of its luma plane, or of all three
    components of a packed BGR frame -- on HIP device `gpu` (include/uva.h uva_crop_sums) -> (rows uint64 [h], cols uint64 [w]).
    device=True: `frame` is a raw device pointer (int) of a frame in that GPU's HBM (uva_crop_sums_device).  max_groups: the
    test hook uva_debug_crop_sums (a grid of at most that many workgroups)."""
    if fmt not in PIX_FORMATS_ALL:
        raise ValueError("unknown pixel format %r (%s)" % (fmt, ", ".join(PIX_FORMATS_ALL)))
    rows, cols = np.zeros(max(1, int(h)), np.uint64), np.zeros(max(1, int(w)), np.uint64)
    if device:
        L = _crop_lib("uva_crop_sums_device")
        _lib.check(L.uva_crop_sums_device(int(gpu), ctypes.c_void_p(int(frame)), PIX_FORMATS_ALL[fmt], int(h), int(w), rows.ctypes.data,
                                          cols.ctypes.data))
    else:
        L = _crop_lib("uva_crop_sums")
        f = _pix_frame(frame, fmt, h, w, "frame")
        if max_groups is None:
            _lib.check(L.uva_crop_sums(int(gpu), f.ctypes.data, PIX_FORMATS_ALL[fmt], int(h), int(w), rows.ctypes.data, cols.ctypes.data))
        else:
            _lib.check(L.uva_debug_crop_sums(int(gpu), f.ctypes.data, PIX_FORMATS_ALL[fmt], int(h), int(w), rows.ctypes.data,
                                             cols.ctypes.data, int(max_groups)))
    return rows[:h], cols[:w]


def crop_bounds(rows, cols, fmt, h, w, limit=24):
    """cropdetect's brightness test on a frame's line sums (include/uva.h uva_crop_bounds; no GPU needed) -> (first bright row,
    last bright row, first bright column, last bright column), -1 where there is none.  limit: 0 ... 255 on the 8-bit scale."""
    if fmt not in PIX_FORMATS_ALL:
        raise ValueError("unknown pixel format %r (%s)" % (fmt, ", ".join(PIX_FORMATS_ALL)))
    r, c = np.ascontiguousarray(rows, np.uint64), np.ascontiguousarray(cols, np.uint64)
    if r.shape != (int(h),) or c.shape != (int(w),):
        raise ValueError("rows / cols must hold h / w sums")
    b = (ctypes.c_int * 4)()
    _lib.check(_crop_lib("uva_crop_bounds").uva_crop_bounds(r.ctypes.data, c.ctypes.data, PIX_FORMATS_ALL[fmt], int(h), int(w), int(limit), b))
    return tuple(int(v) for v in b)


def crop_rect(state, round=16):
    """cropdetect's rectangle from a running state (x1, y1, x2, y2) (include/uva.h uva_crop_rect; no GPU needed) -> (W, H, X, Y)
    in ffmpeg's order, or None when the state holds no rectangle."""
    st = (ctypes.c_int * 4)(*(int(v) for v in state))
    rect = (ctypes.c_int * 4)()
    if _crop_lib("uva_crop_rect").uva_crop_rect(st, int(round), rect):
        return None
    return tuple(int(v) for v in rect)


def pix_window_check(fmt, src_h, src_w, x, y, h, w):
    """Raises UvaError with the reason if the window h x w at (x, y) of a src_h x src_w frame of `fmt` is one the library refuses
    (include/uva.h uva_pix_window_check; no GPU needed)."""
    if fmt not in PIX_FORMATS_ALL:
        raise ValueError("unknown pixel format %r (%s)" % (fmt, ", ".join(PIX_FORMATS_ALL)))
    _lib.check(_crop_lib("uva_pix_window_check").uva_pix_window_check(PIX_FORMATS_ALL[fmt], int(src_h), int(src_w), int(x), int(y), int(h), int(w)))


def pix_window(buf, fmt, src_h, src_w, x, y, h, w, out=None, gpu=0):
    """The dense h x w frame of `fmt` cut from the dense src_h x src_w frame `buf` at (x, y) on HIP device `gpu`, host to host
    (include/uva.h uva_pix_window).  Returns `out` (pix_empty's array; allocated when None)."""
    if fmt not in PIX_FORMATS_ALL:
        raise ValueError("unknown pixel format %r (%s)" % (fmt, ", ".join(PIX_FORMATS_ALL)))
    src = _pix_frame(buf, fmt, src_h, src_w, "input")
    if out is None:
        out = pix_empty(fmt, h, w)
    if not out.flags.c_contiguous or out.nbytes != pix_frame_bytes(fmt, h, w):
        raise ValueError("out must be a C-contiguous buffer of %d bytes" % pix_frame_bytes(fmt, h, w))
    _lib.check(_crop_lib("uva_pix_window").uva_pix_window(int(gpu), src.ctypes.data, PIX_FORMATS_ALL[fmt], int(src_h), int(src_w), int(x),
                                                          int(y), int(h), int(w), out.ctypes.data))
    return out


class CropDetector:
    """ffmpeg cropdetect's running state over the frames it is shown: update(frame) takes one dense
    h x w frame of `fmt` -- its line sums come from the GPU (crop_sums), the rest is host arithmetic -- and rect() is the
    rectangle (W, H, X, Y) after the frames so far, or None."""

    def __init__(self, h, w, fmt, limit=24, round=16, gpu=0):
        if fmt not in PIX_FORMATS_ALL:
            raise ValueError("unknown pixel format %r (%s)" % (fmt, ", ".join(PIX_FORMATS_ALL)))
        if not 0 <= int(limit) <= 255:
            raise ValueError("limit is 0 ... 255 on the 8-bit scale")
        self.h, self.w, self.fmt, self.limit, self.round, self.gpu = int(h), int(w), fmt, int(limit), int(round), int(gpu)
        self.state = (self.w - 1, self.h - 1, 0, 0)

    def update_sums(self, rows, cols):
        """the same from a frame's line sums (no GPU needed)"""
        r0, r1, c0, c1 = crop_bounds(rows, cols, self.fmt, self.h, self.w, self.limit)
        x1, y1, x2, y2 = self.state
        if r0 >= 0:
            y1, y2 = min(y1, r0), max(y2, r1)
        if c0 >= 0:
            x1, x2 = min(x1, c0), max(x2, c1)
        self.state = (x1, y1, x2, y2)
        return self.state

    def update(self, frame):
        return self.update_sums(*crop_sums(frame, self.fmt, self.h, self.w, gpu=self.gpu))

    def rect(self):
        return crop_rect(self.state, self.round)


# ---- deinterlacing (include/uva.h uva_deint_*) ---------------------------------------------------------
DEINT_MODES = {"frame": 0, "field": 1}               # UVA_DEINT_FIELD: outputs A and B, twice the frame rate
FIELD_ORDERS = {"tff": 0, "bff": 2}                  # UVA_DEINT_BFF


def deint_flags(mode="frame", field_order="tff"):
    """the C ABI's flags argument: UVA_DEINT_FIELD | UVA_DEINT_BFF"""
    if mode not in DEINT_MODES:
        raise ValueError("unknown deinterlace mode %r (%s)" % (mode, ", ".join(DEINT_MODES)))
    if field_order not in FIELD_ORDERS:
        raise ValueError("unknown field order %r (%s)" % (field_order, ", ".join(FIELD_ORDERS)))
    return DEINT_MODES[mode] | FIELD_ORDERS[field_order]


def deint_check(fmt, h, w, mode="frame", field_order="tff"):
    """Raises UvaError with the reason if the library refuses to deinterlace h x w frames of `fmt` (include/uva.h
    uva_deint_check; no GPU needed)."""
    if fmt not in PIX_FORMATS_ALL:
        raise ValueError("unknown pixel format %r (%s)" % (fmt, ", ".join(PIX_FORMATS_ALL)))
    _lib.check(_crop_lib("uva_deint_check").uva_deint_check(PIX_FORMATS_ALL[fmt], int(h), int(w), deint_flags(mode, field_order)))


def deint_frames(prev, cur, nxt, fmt, h, w, mode="frame", field_order="tff", gpu=0, device=False, host=False, max_groups=None,
                 out_a=None, out_b=None):
    """One dense h x w frame `cur` of `fmt` deinterlaced between `prev` and `nxt` (None: cur, the ends of a stream) by yadif's
    rule on HIP device `gpu` (include/uva.h uva_deint_frames) -> (A, B): A keeps cur's first field and
    interpolates the other rows, B (mode="field" only, else None) keeps the second.  Flat u8 arrays of the frame's bytes.
    device=True: the three frames and out_a / out_b (out_b: mode="field") are raw device pointers (ints) of frames in that
    GPU's HBM (uva_deint_frames_device); returns None.  host=True: the library's scalar restatement, no GPU
    (uva_debug_deint_host).  max_groups: the test hook uva_debug_deint_frames (a grid of at most that many workgroups)."""
    if fmt not in PIX_FORMATS_ALL:
        raise ValueError("unknown pixel format %r (%s)" % (fmt, ", ".join(PIX_FORMATS_ALL)))
    flags = deint_flags(mode, field_order)
    f, h, w = PIX_FORMATS_ALL[fmt], int(h), int(w)
    if device:
        ptr = lambda v: None if v is None else ctypes.c_void_p(int(v))          # noqa: E731
        _lib.check(_crop_lib("uva_deint_frames_device").uva_deint_frames_device(int(gpu), ptr(prev), ptr(cur), ptr(nxt), f, h, w, flags,
                                                                                ptr(out_a), ptr(out_b)))
        return None
    _lib.check(_crop_lib("uva_deint_check").uva_deint_check(f, h, w, flags))
    frames = [None if v is None else _pix_frame(v, fmt, h, w, what) for v, what in ((prev, "prev"), (cur, "cur"), (nxt, "next"))]
    p, c, n = (None if v is None else v.ctypes.data for v in frames)
    nb = pix_frame_bytes(fmt, h, w)
    a = np.empty(nb, np.uint8) if out_a is None else out_a
    b = (np.empty(nb, np.uint8) if out_b is None else out_b) if mode == "field" else None
    for o in (a, b):
        if o is not None and (not o.flags.c_contiguous or o.nbytes != nb):
            raise ValueError("an output must be a C-contiguous buffer of %d bytes" % nb)
    pb = None if b is None else b.ctypes.data
    if host:
        _lib.check(_crop_lib("uva_debug_deint_host").uva_debug_deint_host(p, c, n, f, h, w, flags, a.ctypes.data, pb))
    elif max_groups is None:
        _lib.check(_crop_lib("uva_deint_frames").uva_deint_frames(int(gpu), p, c, n, f, h, w, flags, a.ctypes.data, pb))
    else:
        _lib.check(_crop_lib("uva_debug_deint_frames").uva_debug_deint_frames(int(gpu), p, c, n, f, h, w, flags, a.ctypes.data, pb,
                                                                              int(max_groups)))
    return a, b


class Deinterlacer:
    """A stream of dense h x w frames of `fmt` deinterlaced on HIP device `gpu`, every frame uploaded once (include/uva.h
    uva_deint_create / uva_deint_push).  push(frame, outs) hands a frame in and writes the outputs of the
    frame BEFORE it -- which now has its successor -- into outs[0] (mode "field": outs[0] and outs[1]); it returns how many it
    wrote: 0 after the first push, then `per_frame` (1, or 2 for "field").  flush(outs) does the same for the last frame and
    leaves the object ready for another stream; reset() forgets the frames pushed so far."""

    def __init__(self, fmt, h, w, mode="frame", field_order="tff", gpu=0):
        if fmt not in PIX_FORMATS_ALL:
            raise ValueError("unknown pixel format %r (%s)" % (fmt, ", ".join(PIX_FORMATS_ALL)))
        self.fmt, self.h, self.w, self.mode, self.field_order, self.gpu = fmt, int(h), int(w), mode, field_order, int(gpu)
        self.flags = deint_flags(mode, field_order)
        self.per_frame = 2 if mode == "field" else 1
        self.nbytes = pix_frame_bytes(fmt, self.h, self.w)
        self._L = _crop_lib("uva_deint_create")
        self._h = ctypes.c_void_p()
        _lib.check(self._L.uva_deint_create(self.gpu, PIX_FORMATS_ALL[fmt], self.h, self.w, self.flags, ctypes.byref(self._h)))

    def _push(self, frame, outs):
        if self._h is None:
            raise ValueError("the deinterlacer is closed")
        if len(outs) < self.per_frame:
            raise ValueError("%d output buffers are needed" % self.per_frame)
        for o in outs[:self.per_frame]:
            if not o.flags.c_contiguous or o.nbytes != self.nbytes or not o.flags.writeable:
                raise ValueError("an output must be a writable C-contiguous buffer of %d bytes" % self.nbytes)
        n = ctypes.c_int(0)
        src = None if frame is None else _pix_frame(frame, self.fmt, self.h, self.w, "frame")
        _lib.check(self._L.uva_deint_push(self._h, None if src is None else src.ctypes.data, outs[0].ctypes.data,
                                          outs[1].ctypes.data if self.per_frame == 2 else None, ctypes.byref(n)))
        return n.value

    def push(self, frame, outs):
        if frame is None:
            raise ValueError("push() takes a frame; flush() ends the stream")
        return self._push(frame, outs)

    def flush(self, outs):
        return self._push(None, outs)

    def reset(self):
        if self._h is not None:
            _lib.check(self._L.uva_deint_reset(self._h))

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._L.uva_deint_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class Ticket:
    """One frame in flight on the pipelined host route; keeps its buffers alive."""

    def __init__(self, tid, img, out):
        self.id, self._img, self.out = tid, img, out


class Mat:
    """Host f32 planar [c][h][w] image, the subset of ncnn::Mat the reference uses."""

    class PixelType:
        PIXEL_RGB = 1
        PIXEL_BGR = 2

    def __init__(self, array):
        self._a = np.ascontiguousarray(array, dtype=np.float32)
        self.c, self.h, self.w = self._a.shape

    @staticmethod
    def from_pixels(array, pixel_type, w, h):
        """ncnn mat_pixel.cpp from_pixels: u8 HWC -> f32 planar, byte k of a pixel -> plane k
        (PIXEL_BGR keeps BGR order: no swap).  upscale_processing.py:265-270, :437-442"""
        if pixel_type not in (Mat.PixelType.PIXEL_BGR, Mat.PixelType.PIXEL_RGB):
            raise ValueError("unsupported pixel type")
        a = np.asarray(array)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[0] != h or a.shape[1] != w or a.shape[2] != 3:
            raise ValueError("from_pixels expects a u8 [h][w][3] array")
        return Mat(a.transpose(2, 0, 1).astype(np.float32))

    def substract_mean_normalize(self, mean_vals, norm_vals):
        """ncnn mat.cpp: per channel (x - mean) * norm in fp32.  upscale_processing.py:271-273"""
        for c in range(self.c):
            if mean_vals:
                self._a[c] -= np.float32(mean_vals[c])
            if norm_vals:
                self._a[c] *= np.float32(norm_vals[c])

    def __array__(self, dtype=None, copy=None):
        return self._a if dtype is None else self._a.astype(dtype)

    def numpy(self):
        return self._a


class _Option:
    def __init__(self):
        self.use_vulkan_compute = False  # accepted for source compatibility; HIP is always used


def _param_blob_names(path):
    """(input blob, output blob) of an ncnn text .param: the Input layer's top and the last layer's top (what the
    reference passes as model_input / model_output, upscale_processing.py:72-73, always "input" / "output" there)."""
    try:
        with open(path) as f:
            lines = [ln.split() for ln in f.read().splitlines()[2:] if len(ln.split()) >= 4]
    except OSError:
        return None
    first_in = next((p for p in lines if p[0] == "Input"), None)
    if first_in is None or not lines:
        return None
    last = lines[-1]
    nin, nout = int(last[2]), int(last[3])
    if nout < 1 or int(first_in[3]) < 1:
        return None
    return first_in[4 + int(first_in[2])], last[4 + nin + nout - 1]


class Extractor:
    def __init__(self, net):
        self._net = net
        self._in = None

    def input(self, name, mat):
        """ex.input(model_input, mat): the name must be the loaded graph's input blob (:278, :450)"""
        if name != self._net.blob_names[0]:
            return -1
        self._in = mat
        return 0

    def extract(self, name):
        """-> (ret, Mat).  upscale_processing.py:280, :452; the name must be the loaded graph's output blob"""
        if name != self._net.blob_names[1] or self._in is None:
            return -1, None
        out = self._net._extract(np.asarray(self._in))
        return 0, Mat(out)


class Net:
    """ncnn.Net stand-in bound to one HIP device (upscale_processing.py:65-71)."""

    def __init__(self):
        self._L = _lib.load()
        self._h = self._L.uva_net_create()
        self.opt = _Option()

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.uva_net_destroy(h)

    @property
    def device_index(self):
        """the HIP ordinal the net is bound to, as the library holds it (include/uva.h uva_net_device)"""
        return int(self._L.uva_net_device(self._h))

    def set_vulkan_device(self, device_index):
        _lib.check(self._L.uva_net_set_device(self._h, int(device_index)))

    blob_names = ("input", "output")     # of the loaded graph (load_param)

    def load_param(self, path):
        rc = self._L.uva_net_load_param(self._h, str(path).encode())
        if rc:
            self.last_error = self._L.uva_last_error().decode()
        else:
            self.blob_names = _param_blob_names(str(path)) or ("input", "output")
        return rc

    def load_model(self, path):
        rc = self._L.uva_net_load_model(self._h, str(path).encode())
        if rc:
            self.last_error = self._L.uva_last_error().decode()
        return rc

    def create_extractor(self):
        return Extractor(self)

    # --- facts -------------------------------------------------------------------------------
    @property
    def scale(self):
        return self._L.uva_net_scale(self._h)

    @property
    def num_features(self):
        return self._L.uva_net_num_features(self._h)

    @property
    def num_convs(self):
        return self._L.uva_net_num_convs(self._h)

    # --- compute -----------------------------------------------------------------------------
    def _extract(self, x_chw):
        x = np.ascontiguousarray(x_chw, dtype=np.float32)
        if x.ndim != 3 or x.shape[0] != 3:
            raise ValueError("input Mat must be [3][h][w]")
        s = self.scale
        if s <= 0:
            raise _lib.UvaError("net has no graph: load_param/load_model failed or were not called")
        _, h, w = x.shape
        out = np.empty((3, h * s, w * s), np.float32)
        _lib.check(self._L.uva_net_extract_f32(self._h, x.ctypes.data, h, w, out.ctypes.data))
        return out

    def process_u8(self, img_bgr, tile_size=0, border=0):
        """Fused device path for a whole frame: u8 HWC BGR -> u8 HWC BGR (include/uva.h
        uva_net_process_u8).  tile_size<=0: apply_model semantics; 960/10: upscale_image's."""
        img = np.ascontiguousarray(img_bgr, dtype=np.uint8)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("frame must be u8 [h][w][3]")
        s = self.scale
        if s <= 0:
            raise _lib.UvaError("net has no graph: load_param/load_model failed or were not called")
        h, w, _ = img.shape
        out = np.empty((h * s, w * s, 3), np.uint8)
        _lib.check(self._L.uva_net_process_u8(self._h, img.ctypes.data, h, w, w * 3, out.ctypes.data,
                                              w * s * 3, int(tile_size), int(border)))
        return out

    def process_u16(self, img_bgr, tile_size=0, border=0):
        """process_u8 on 16-bit samples (include/uva.h uva_net_process_u16): u16 HWC BGR (unorm16) ->
        u16 HWC BGR.  The 2x and 4x Compact nets, and the 1x net after enable_u16_1x() (whole frames only: tile_size 0;
        DESIGN.md section 7.9)."""
        img = np.ascontiguousarray(img_bgr, dtype=np.uint16)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("frame must be u16 [h][w][3]")
        s = self.scale
        if s <= 0:
            raise _lib.UvaError("net has no graph: load_param/load_model failed or were not called")
        h, w, _ = img.shape
        out = np.empty((h * s, w * s, 3), np.uint16)
        _lib.check(self._L.uva_net_process_u16(self._h, img.ctypes.data, h, w, w * 6, out.ctypes.data,
                                               w * s * 6, int(tile_size), int(border)))
        return out

    def enable_u16_1x(self, on=True):
        """Lets the 16-bit entries (process_u16, submit_pix with bit_depth=16) take this net if it is the 1x SubCompact net
        (include/uva.h uva_net_enable_u16_1x); off, the default, they refuse it.  Raises on any other
        net.  Needs no GPU."""
        _lib.check(self._L.uva_net_enable_u16_1x(self._h, 1 if on else 0))

    def submit_u8(self, img_bgr, out=None, tile_size=0, border=0):
        """Pipelined process_u8 (include/uva.h uva_net_submit_u8): returns a Ticket at once; up to 3
        frames may be in flight and their H2D copy, kernels and D2H copy overlap.  `out`: optional
        preallocated u8 [h*s][w*s][3] array (pinned_empty avoids the staging copy)."""
        img = np.ascontiguousarray(img_bgr, dtype=np.uint8)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("frame must be u8 [h][w][3]")
        s = self.scale
        if s <= 0:
            raise _lib.UvaError("net has no graph: load_param/load_model failed or were not called")
        h, w, _ = img.shape
        if out is None:
            out = np.empty((h * s, w * s, 3), np.uint8)
        if out.dtype != np.uint8 or out.shape != (h * s, w * s, 3) or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous u8 [h*s][w*s][3] array")
        t = self._L.uva_net_submit_u8(self._h, img.ctypes.data, h, w, w * 3, out.ctypes.data, w * s * 3,
                                      int(tile_size), int(border))
        if t < 0:
            raise _lib.UvaError(self._L.uva_last_error().decode(errors="replace"))
        return Ticket(t, img, out)

    def submit_pix(self, buf, h, w, in_fmt, out=None, out_fmt="bgr24", colour="bt601", color_range="tv", tile_size=0, border=0,
                   bit_depth=8, chroma_filter="replicate", chroma_loc="left", out_size=None, resize_filter="lanczos"):
        """submit_u8 with a rawvideo pixel format on either end (include/uva.h uva_net_submit_pix): `buf` holds one dense
        h x w frame of in_fmt, the result is one dense (h*s) x (w*s) frame of out_fmt; both conversions run on the GPU around
        the net.  `out`: optional preallocated result buffer of pix_frame_bytes(out_fmt, h*s, w*s) bytes (pix_empty; pinned
        memory avoids the staging copy).  Returns a Ticket that collect_u8 takes.  bit_depth=16: the 16-bit route
        (uva_net_submit_pix16): the frame reaches the net as u16 BGR and leaves it as u16 BGR, no 8-bit hop (the 2x and 4x
        Compact nets; the 1x net after enable_u16_1x(), at tile_size 0).
        chroma_filter="bilinear": both conversions interpolate chroma sited at chroma_loc.
        out_size=(oh, ow): the net's result is resampled to oh x ow with resize_filter between the net and the output
        conversion (uva_net_submit_pix_sized); the result is then one dense oh x ow frame of out_fmt."""
        _bit_depth(bit_depth, (in_fmt, out_fmt))
        cw = colour_word(colour, color_range, chroma_filter, chroma_loc)
        s = self.scale
        if s <= 0:
            raise _lib.UvaError("net has no graph: load_param/load_model failed or were not called")
        win = getattr(self, "_window", None)
        src = _pix_frame(buf, in_fmt, *(win[:2] if win else (h, w)), "input")     # (set_input_window: the source frame)
        rh, rw = h * s, w * s
        if out_size is not None:
            rf = _resize_filter(resize_filter)
            rh, rw = (int(v) for v in out_size)
            _resize_axis(h * s, rh, "height")
            _resize_axis(w * s, rw, "width")
        if out is None:
            out = pix_empty(out_fmt, rh, rw)
        if not out.flags.c_contiguous or out.nbytes != pix_frame_bytes(out_fmt, rh, rw):
            raise ValueError("out must be a C-contiguous buffer of %d bytes" % pix_frame_bytes(out_fmt, rh, rw))
        if out_size is not None:
            t = self._L.uva_net_submit_pix_sized(self._h, src.ctypes.data, PIX_FORMATS_ALL[in_fmt], h, w, out.ctypes.data,
                                                 PIX_FORMATS_ALL[out_fmt], cw, int(tile_size), int(border), rh, rw, rf, int(bit_depth))
            if t < 0:
                raise _lib.UvaError(self._L.uva_last_error().decode(errors="replace"))
            return Ticket(t, src, out)
        fn = self._L.uva_net_submit_pix16 if bit_depth == 16 else self._L.uva_net_submit_pix
        t = fn(self._h, src.ctypes.data, PIX_FORMATS_ALL[in_fmt], h, w, out.ctypes.data, PIX_FORMATS_ALL[out_fmt], cw, int(tile_size), int(border))
        if t < 0:
            raise _lib.UvaError(self._L.uva_last_error().decode(errors="replace"))
        return Ticket(t, src, out)

    def convert_pix_device(self, d_in, h, w, in_fmt, d_out, out_fmt, colour="bt601", color_range="tv", after=None,
                           chroma_filter="replicate", chroma_loc="left"):
        """A conversion of a frame in HBM queued IN FRONT of this net (include/uva.h uva_pix_convert_device), like
        denoise_u8_device: `after` (a net, or None) comes first, this net's next work waits for the frame."""
        _lib.check(self._L.uva_pix_convert_device(self.device_index, ctypes.c_void_p(d_in), PIX_FORMATS_ALL[in_fmt], ctypes.c_void_p(d_out),
                                                  PIX_FORMATS_ALL[out_fmt], h, w,
                                                  colour_word(colour, color_range, chroma_filter, chroma_loc),
                                                  after._h if after is not None else None, self._h))

    def resize_device(self, d_in, h, w, d_out, oh, ow, filter="lanczos", bit_depth=8, after=None, in_stride=None, out_stride=None):
        """The resampler on a BGR frame in HBM queued IN FRONT of this net (include/uva.h uva_resize_device), like
        convert_pix_device: `after` (a net, or None) comes first, this net's next work waits for the frame.  Raw device
        pointers (ints); strides in bytes (default: dense rows)."""
        bps = bit_depth // 8
        _lib.check(self._L.uva_resize_device(self.device_index, ctypes.c_void_p(d_in), h, w, in_stride or w * 3 * bps, ctypes.c_void_p(d_out),
                                             oh, ow, out_stride or ow * 3 * bps, _resize_filter(filter), int(bit_depth),
                                             after._h if after is not None else None, self._h))

    def set_input_window(self, src_h=0, src_w=0, x=0, y=0):
        """Cropped input frames (include/uva.h uva_net_set_input_window): while set, `buf` of every
        submit_pix call is a dense src_h x src_w frame of in_fmt and the call's h x w is the window at (x, y) of it -- only the
        window is uploaded, the result is that of a dense h x w frame.  All zeros (the default) switch it off.  Forgets the
        kept frame of set_skip_repeats and zeroes skip_stats().  Needs no GPU."""
        if not hasattr(self._L, "uva_net_set_input_window"):
            raise _lib.UvaError("this libuva build has no uva_net_set_input_window: rebuild it")
        _lib.check(self._L.uva_net_set_input_window(self._h, int(src_h), int(src_w), int(x), int(y)))
        self._window = (int(src_h), int(src_w), int(x), int(y)) if (src_h or src_w or x or y) else None

    def set_skip_repeats(self, threshold):
        """Repeated frames on the pipelined route (include/uva.h uva_net_set_skip_repeats): None or -1
        turns it off (the default), 0 ... 65535 is the largest difference in code values at which a frame submitted with
        submit_u8 / submit_pix still repeats the KEPT frame -- the last one the net ran on -- and gets that frame's result
        bytes instead of a run of its own.  Forgets the kept frame and zeroes skip_stats().  Needs no GPU."""
        _lib.check(self._L.uva_net_set_skip_repeats(self._h, -1 if threshold is None else int(threshold)))

    def reset_reference(self):
        """Forgets the kept frame: the next frame runs whatever it holds (a segment's start, a seek)."""
        _lib.check(self._L.uva_net_reset_reference(self._h))

    def skip_stats(self):
        """-> (submitted, skipped) since set_skip_repeats"""
        a, b = ctypes.c_longlong(), ctypes.c_longlong()
        _lib.check(self._L.uva_net_skip_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def collect_u8(self, ticket):
        """Waits for the frame of `ticket` and returns its u8 result array (submit_u8, submit_pix) or its PNG workspace
        (submit_u8_png)."""
        _lib.check(self._L.uva_net_collect_u8(self._h, ticket.id))
        return ticket.out

    def submit_u8_png(self, img_bgr, workspace=None, tile_size=0, border=0):
        """Pipelined like submit_u8, but the result frame stays on the GPU and is deflated there (include/uva.h
        uva_net_submit_u8_png): collect_u8(ticket) returns a PngWorkspace whose .file_bytes() is the PNG file
        cv2.imwrite would have been asked for (upscale_processing.py:288, :519).  `workspace`: a PngWorkspace of the
        result's size to reuse (they are page-locked; allocate a few and cycle them)."""
        img = np.ascontiguousarray(img_bgr, dtype=np.uint8)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("frame must be u8 [h][w][3]")
        s = self.scale
        if s <= 0:
            raise _lib.UvaError("net has no graph: load_param/load_model failed or were not called")
        h, w, _ = img.shape
        if workspace is None:
            workspace = PngWorkspace(h * s, w * s)
        if (workspace.h, workspace.w) != (h * s, w * s):
            raise ValueError("PNG workspace is for %dx%d frames, the result is %dx%d" % (workspace.w, workspace.h, w * s, h * s))
        if getattr(workspace, "bit_depth", 8) != 8:
            raise ValueError("submit_u8_png needs an 8-bit PNG workspace")
        t = self._L.uva_net_submit_u8_png(self._h, img.ctypes.data, h, w, w * 3, workspace.buf.ctypes.data, workspace.buf.nbytes,
                                          int(tile_size), int(border))
        if t < 0:
            raise _lib.UvaError(self._L.uva_last_error().decode(errors="replace"))
        return Ticket(t, img, workspace)

    def submit_u16_png(self, img_bgr, workspace=None, tile_size=0, border=0):
        """submit_u8_png on 16-bit samples (include/uva.h uva_net_submit_u16_png): a u16 BGR frame in, the
        u16 result deflated on the GPU as a 16-bit RGB PNG; collect_u8(ticket) returns the PngWorkspace (bit_depth=16).  The
        16-bit route's nets: 2x / 4x Compact, and the 1x net after enable_u16_1x() at tile_size 0."""
        img = np.ascontiguousarray(img_bgr, dtype=np.uint16)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("frame must be u16 [h][w][3]")
        s = self.scale
        if s <= 0:
            raise _lib.UvaError("net has no graph: load_param/load_model failed or were not called")
        h, w, _ = img.shape
        if workspace is None:
            workspace = PngWorkspace(h * s, w * s, bit_depth=16)
        if (workspace.h, workspace.w) != (h * s, w * s):
            raise ValueError("PNG workspace is for %dx%d frames, the result is %dx%d" % (workspace.w, workspace.h, w * s, h * s))
        if getattr(workspace, "bit_depth", 8) != 16:
            raise ValueError("submit_u16_png needs a PngWorkspace(..., bit_depth=16)")
        if not hasattr(self._L, "uva_net_submit_u16_png"):
            raise _lib.UvaError("this libuva build has no 16-bit PNG encoder: rebuild it")
        t = self._L.uva_net_submit_u16_png(self._h, img.ctypes.data, h, w, w * 6, workspace.buf.ctypes.data, workspace.buf.nbytes,
                                           int(tile_size), int(border))
        if t < 0:
            raise _lib.UvaError(self._L.uva_last_error().decode(errors="replace"))
        return Ticket(t, img, workspace)

    def process_u8_device(self, d_in, h, w, d_out, tile_size=0, border=0, in_stride=None, out_stride=None):
        """Asynchronous: raw device pointers (ints) of dense u8 HWC frames in this GPU's HBM."""
        s = self.scale
        _lib.check(self._L.uva_net_process_u8_device(
            self._h, ctypes.c_void_p(d_in), h, w, in_stride or w * 3, ctypes.c_void_p(d_out),
            out_stride or w * s * 3, int(tile_size), int(border)))

    def process_u8_device_batch(self, d_ins, h, w, d_outs, tile_size=0, border=0, in_stride=None, out_stride=None):
        """Asynchronous: several dense u8 HWC frames of ONE geometry in this GPU's HBM (lists of raw device pointers) in one
        call (include/uva.h uva_net_process_u8_device_batch).  The 1x net runs up to eight of them per kernel launch; the bytes
        are those of one process_u8_device call per frame."""
        n = len(d_ins)
        assert n == len(d_outs)
        s = self.scale
        ins = (ctypes.c_void_p * n)(*[int(p) for p in d_ins])
        outs = (ctypes.c_void_p * n)(*[int(p) for p in d_outs])
        _lib.check(self._L.uva_net_process_u8_device_batch(
            self._h, ins, outs, n, h, w, in_stride or w * 3, out_stride or w * s * 3, int(tile_size), int(border)))

    def denoise_u8_device(self, d_in, h, w, d_out, strength, after=None, in_stride=None, out_stride=None):
        """`-m n=K` on a frame in HBM, queued IN FRONT of this net (include/uva.h uva_denoise_u8_device): everything `after`
        (a net, or None) has been asked so far comes first, and whatever this net is asked from now on waits for the frame."""
        _lib.check(self._L.uva_denoise_u8_device(self.device_index, ctypes.c_void_p(d_in), h, w, in_stride or w * 3, ctypes.c_void_p(d_out),
                                                 out_stride or w * 3, float(strength), float(strength),
                                                 after._h if after is not None else None, self._h))

    def denoise_u16_device(self, d_in, h, w, d_out, strength, after=None, in_stride=None, out_stride=None):
        """`-m n=K` at 16 bits on a u16 BGR frame in HBM (include/uva.h uva_denoise_u16_device), queued
        like denoise_u8_device: `after` (a net, or None) comes first, this net's next work waits for the frame.  Strides in bytes."""
        if not hasattr(self._L, "uva_denoise_u16_device"):
            raise _lib.UvaError("this libuva build has no 16-bit denoise stage: rebuild it")
        _lib.check(self._L.uva_denoise_u16_device(self.device_index, ctypes.c_void_p(d_in), h, w, in_stride or w * 6, ctypes.c_void_p(d_out),
                                                  out_stride or w * 6, float(strength), float(strength),
                                                  after._h if after is not None else None, self._h))

    def wait_for(self, producer):
        """Device-side ordering: work queued on `producer` so far finishes before this net's next work."""
        _lib.check(self._L.uva_net_wait_for(self._h, producer._h))

    def synchronize(self):
        _lib.check(self._L.uva_net_synchronize(self._h))

    def set_profiling(self, on):
        _lib.check(self._L.uva_net_set_profiling(self._h, 1 if on else 0))

    def kernel_stats(self, kind):
        n, ms = ctypes.c_longlong(), ctypes.c_double()
        _lib.check(self._L.uva_net_kernel_stats(self._h, kind, n, ms))
        return n.value, ms.value

    def debug_generic_launches(self):
        """launches per kernel instantiation of the generic executor since this net was made (include/uva.h
        uva_net_debug_generic_launches lists the indices): a test's proof that the kernel it is about ran"""
        n = ctypes.c_int(0)
        _lib.check(self._L.uva_net_debug_generic_launches(self._h, None, 0, ctypes.byref(n)))
        counts = (ctypes.c_longlong * n.value)()
        _lib.check(self._L.uva_net_debug_generic_launches(self._h, counts, n.value, ctypes.byref(n)))
        return list(counts)

    def debug_read_activation(self, conv_idx, h, w):
        out = np.empty((self.num_features, h, w), np.float32)
        _lib.check(self._L.uva_net_debug_read_activation(self._h, conv_idx, out.ctypes.data, h, w))
        return out

    def debug_packed_weights(self, conv_idx):
        need = ctypes.c_size_t()
        _lib.check(self._L.uva_net_debug_packed_weights(self._h, conv_idx, None, 0, need))
        buf = np.empty(need.value, np.uint16)
        _lib.check(self._L.uva_net_debug_packed_weights(self._h, conv_idx, buf.ctypes.data, need.value, need))
        return buf


# ---- inverse telecine (include/uva.h uva_ivtc_*) -------------------------------------------------------
IVTC_COMBED = {"yadif": 0, "keep": 2}                # UVA_IVTC_KEEP_COMBED
IVTC_BFF, IVTC_KEEP_ALL = 1, 4                       # UVA_IVTC_BFF, UVA_IVTC_KEEP_ALL
IVTC_MATCHES = "cpn"
IVTC_STATS = ("frames_in", "frames_out", "match_c", "match_p", "match_n", "combed", "dropped")


def ivtc_flags(field_order="tff", combed="yadif", keep_all=False):
    """the C ABI's flags argument: UVA_IVTC_BFF | UVA_IVTC_KEEP_COMBED | UVA_IVTC_KEEP_ALL"""
    if field_order not in FIELD_ORDERS:
        raise ValueError("unknown field order %r (%s)" % (field_order, ", ".join(FIELD_ORDERS)))
    if combed not in IVTC_COMBED:
        raise ValueError("unknown policy for combed frames %r (%s)" % (combed, ", ".join(IVTC_COMBED)))
    return (IVTC_BFF if field_order == "bff" else 0) | IVTC_COMBED[combed] | (IVTC_KEEP_ALL if keep_all else 0)


def ivtc_check(fmt, h, w, field_order="tff", thresh=9, combed="yadif", combed_limit=1000, keep_all=False):
    """Raises UvaError with the reason if the library refuses to detelecine h x w frames of `fmt` (include/uva.h uva_ivtc_check;
    no GPU needed)."""
    if fmt not in PIX_FORMATS_ALL:
        raise ValueError("unknown pixel format %r (%s)" % (fmt, ", ".join(PIX_FORMATS_ALL)))
    _lib.check(_crop_lib("uva_ivtc_check").uva_ivtc_check(PIX_FORMATS_ALL[fmt], int(h), int(w), ivtc_flags(field_order, combed, keep_all),
                                                          int(thresh), int(combed_limit)))


def ivtc_metrics(prev, cur, nxt, fmt, h, w, field_order="tff", thresh=9, gpu=0, device=False, host=False, max_groups=None,
                 combed="yadif", combed_limit=1000):
    """The comb metric of the three frames that weave the first field of the dense h x w frame `cur` of `fmt` with the second field
    of cur, `prev` and `nxt` (None: cur), on HIP device `gpu` (include/uva.h uva_ivtc_metrics) ->
    (N_c, M_c, N_p, M_p, N_n, M_n), exact integers.  device=True: the frames are raw device pointers (ints) of frames in that
    GPU's HBM (uva_ivtc_metrics_device).  max_groups: the test hook uva_debug_ivtc_metrics.  host=True: the library's scalar
    restatement, no GPU (uva_debug_ivtc_host) -> (stats, woven [3][frame bytes] for c / p / n, chosen frame, match, combed)."""
    if fmt not in PIX_FORMATS_ALL:
        raise ValueError("unknown pixel format %r (%s)" % (fmt, ", ".join(PIX_FORMATS_ALL)))
    flags = ivtc_flags(field_order, combed)
    f, h, w, T = PIX_FORMATS_ALL[fmt], int(h), int(w), int(thresh)
    st = (ctypes.c_ulonglong * 6)()
    if device:
        ptr = lambda v: None if v is None else ctypes.c_void_p(int(v))          # noqa: E731
        _lib.check(_crop_lib("uva_ivtc_metrics_device").uva_ivtc_metrics_device(int(gpu), ptr(prev), ptr(cur), ptr(nxt), f, h, w, flags, T, st))
        return tuple(int(v) for v in st)
    _lib.check(_crop_lib("uva_ivtc_check").uva_ivtc_check(f, h, w, flags, T, int(combed_limit)))
    frames = [None if v is None else _pix_frame(v, fmt, h, w, what) for v, what in ((prev, "prev"), (cur, "cur"), (nxt, "next"))]
    p, c, n = (None if v is None else v.ctypes.data for v in frames)
    if host:
        nb = pix_frame_bytes(fmt, h, w)
        woven, chosen, dec = np.empty((3, nb), np.uint8), np.empty(nb, np.uint8), (ctypes.c_int * 2)()
        _lib.check(_crop_lib("uva_debug_ivtc_host").uva_debug_ivtc_host(p, c, n, f, h, w, flags, T, int(combed_limit), st, woven.ctypes.data,
                                                                        chosen.ctypes.data, dec))
        return tuple(int(v) for v in st), woven, chosen, int(dec[0]), bool(dec[1])
    if max_groups is None:
        _lib.check(_crop_lib("uva_ivtc_metrics").uva_ivtc_metrics(int(gpu), p, c, n, f, h, w, flags, T, st))
    else:
        _lib.check(_crop_lib("uva_debug_ivtc_metrics").uva_debug_ivtc_metrics(int(gpu), p, c, n, f, h, w, flags, T, st, int(max_groups)))
    return tuple(int(v) for v in st)


def ivtc_decimate(diffs, keep_all=False):
    """The numbers of the final frames that the decimator delivers, in order, for these diffs (the library's state machine driven
    as uva_ivtc_push drives it; uva_debug_ivtc_decimate, no GPU)."""
    n = len(diffs)
    d = (ctypes.c_ulonglong * max(1, n))(*[int(v) for v in diffs])
    out, k = (ctypes.c_longlong * max(1, n))(), ctypes.c_int(0)
    _lib.check(_crop_lib("uva_debug_ivtc_decimate").uva_debug_ivtc_decimate(d, n, IVTC_KEEP_ALL if keep_all else 0, out, ctypes.byref(k)))
    return [int(out[i]) for i in range(k.value)]


class Detelecine:
    """A stream of dense h x w frames of `fmt` detelecined on HIP device `gpu`, every frame uploaded once (include/uva.h
    uva_ivtc_create / uva_ivtc_push): field matching, yadif for frames that stay combed, and one frame of
    every five dropped.  push(frame, out) hands a frame in and returns 1 if it wrote a frame of the result into `out`, else 0;
    flush(out) is called until it returns 0 and leaves the object ready for another stream; reset() forgets the stream so far.
    Which call delivers which frame is not part of the contract, the sequence of delivered frames is.  stats(): a dict of
    IVTC_STATS since creation."""

    def __init__(self, fmt, h, w, field_order="tff", thresh=9, combed="yadif", combed_limit=1000, keep_all=False, gpu=0):
        if fmt not in PIX_FORMATS_ALL:
            raise ValueError("unknown pixel format %r (%s)" % (fmt, ", ".join(PIX_FORMATS_ALL)))
        self.fmt, self.h, self.w, self.gpu = fmt, int(h), int(w), int(gpu)
        self.flags = ivtc_flags(field_order, combed, keep_all)
        self.per_frame = 1
        self.nbytes = pix_frame_bytes(fmt, self.h, self.w)
        self._L = _crop_lib("uva_ivtc_create")
        self._h = ctypes.c_void_p()
        _lib.check(self._L.uva_ivtc_create(self.gpu, PIX_FORMATS_ALL[fmt], self.h, self.w, self.flags, int(thresh), int(combed_limit),
                                           ctypes.byref(self._h)))

    def _push(self, frame, out):
        if self._h is None:
            raise ValueError("the detelecine handle is closed")
        if not out.flags.c_contiguous or out.nbytes != self.nbytes or not out.flags.writeable:
            raise ValueError("the output must be a writable C-contiguous buffer of %d bytes" % self.nbytes)
        n = ctypes.c_int(0)
        src = None if frame is None else _pix_frame(frame, self.fmt, self.h, self.w, "frame")
        _lib.check(self._L.uva_ivtc_push(self._h, None if src is None else src.ctypes.data, out.ctypes.data, ctypes.byref(n)))
        return n.value

    def push(self, frame, out):
        if frame is None:
            raise ValueError("push() takes a frame; flush() ends the stream")
        return self._push(frame, out)

    def flush(self, out):
        return self._push(None, out)

    def reset(self):
        if self._h is not None:
            _lib.check(self._L.uva_ivtc_reset(self._h))

    def stats(self):
        if self._h is None:
            raise ValueError("the detelecine handle is closed")
        st = (ctypes.c_ulonglong * 7)()
        _lib.check(self._L.uva_ivtc_stats(self._h, st))
        return dict(zip(IVTC_STATS, (int(v) for v in st)))

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._L.uva_ivtc_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
