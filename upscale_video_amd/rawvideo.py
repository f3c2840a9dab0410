"""rawvideo.py -- stream raw video frames through the MI355X engine.

The reference moves every frame through PNG files on both sides of the net (ffmpeg writes
`%d.extract.png`, upscale/upscale_processing.py:203-255; workers imread / imwrite, :263,288,487,519;
ffmpeg re-reads `%d.png`, :604-640) and the PNG codecs, not the GPU, bound its file-to-file rate.
This module is the same per-frame arithmetic fed by a raw pipe instead, ffmpeg itself untouched:

    ffmpeg -i in.mkv -f rawvideo -pix_fmt bgr24 - \\
      | python -m upscale_video_amd.rawvideo -W 1920 -H 1080 -s 2 \\
      | ffmpeg -f rawvideo -pix_fmt bgr24 -s 3840x2160 -r 24 -i - out.mkv

or, with the colour conversion on the GPU and half the pipe bytes (--in-pix-fmt / --out-pix-fmt: bgr24, yuv420p, nv12,
p010le, yuv420p10le, and the 4:2:2 formats of capture and mezzanine material yuv422p, yuv422p10le; --colorspace bt601|bt709,
--color-range tv|pc, default bt601 / tv: DESIGN.md sections 7.3, 7.7):

    ffmpeg -i in.mkv -f rawvideo -pix_fmt yuv420p - \\
      | python -m upscale_video_amd.rawvideo -W 1920 -H 1080 -s 2 --in-pix-fmt yuv420p --out-pix-fmt p010le \\
      | ffmpeg -f rawvideo -pix_fmt p010le -s 3840x2160 -r 24 -i - -c:v libx265 out.mkv

--bit-depth 16 runs the 2x / 4x net on 16-bit samples so that 10-bit frames (p010le, yuv420p10le, yuv422p10le) keep their depth
(DESIGN.md section 7.4).  -m a goes with it: the 1x net then runs on 16-bit samples too and hands u16 BGR (bgr48le) frames to the
2x / 4x net, so the chain has no 8-bit hop either.  -m n=K goes with it as well: the film-grain denoise
then runs on 16-bit Lab planes (uva_denoise_u16: the 8-bit stage's non-local means with 16-bit samples, a sixteen times finer
weight table and 64-bit sums, K meaning what it means at 8 bits) and hands bgr48le on, instead of
sending 10-bit frames through 256 levels and an 8-bit Lab round trip; -m r runs at 8 bits only.  Either option wants
a format of more than 8 bits on at least one end (p010le, yuv420p10le, yuv422p10le, bgr48le); with 8-bit frames in and out it is
refused, as it always was.

--chroma-filter bilinear interpolates the 4:2:0 chroma on the way in and filters it on the way out for where its samples sit
 instead of repeating every chroma sample over its 2x2 block and averaging the block: the net then
sees no 2x2 colour steps to sharpen, and colour stays registered with luma.  --chroma-loc names the siting (ffmpeg's
chroma_sample_location): left (default) for video from H.264 / HEVC, center for JPEG / MPEG-1 material, topleft for UHD
BT.2020 material.  The default, replicate, keeps the earlier releases' bytes.  A 4:2:2 format (one chroma row per luma row)
takes the horizontal half of either mode: the pair instead of the 2x2 block, and left and topleft are the same there (DESIGN.md
section 7.7).

--out-size WxH (or --out-scale F, the total scale relative to the input frame, as Real-ESRGAN's --outscale) resamples the net's
2x / 4x result to the size asked for on the GPU, between the net and the output conversion (DESIGN.md section 7.6;
--resize-filter lanczos|bicubic|bilinear), so that no `-vf scale=` pass over 4K frames is left to the ffmpeg behind the pipe
and the pipe carries frames of the final size:

    ffmpeg -i in.mkv -f rawvideo -pix_fmt yuv420p - \\
      | python -m upscale_video_amd.rawvideo -W 1280 -H 720 -s 2 --out-size 2560x1440 --in-pix-fmt yuv420p --out-pix-fmt p010le \\
      | ffmpeg -f rawvideo -pix_fmt p010le -s 2560x1440 -r 24 -i - -c:v libx265 out.mkv

--crop W:H:X:Y (ffmpeg's order) cuts that window out of every input frame in front of the first stage: -W / -H
stay the size of the frames on the input, everything behind -- the nets, --out-size / --out-scale, --tile, the size of the frames
that leave -- works from the cropped size, and only the window's rows are uploaded.  --crop auto finds the window first, the way
the reference does (get_crop_detect, upscale/upscale_processing.py:137-181: ffmpeg's cropdetect at 100 places of the film, the most
frequent rectangle wins), with the per-frame pass on the GPU; it needs a regular file.  --cropdetect only analyses (pipes too) and
prints one `crop=W:H:X:Y` line for --crop or for ffmpeg's -vf.

--deinterlace frame|field takes interlaced frames (DVD, broadcast and tape material): every frame read goes
through yadif's spatio-temporal rule on the GPU in front of everything else, per component plane of the input format and exact
in integers, so no ffmpeg `yadif` process has to sit in front of the pipe and the nets never see a comb.  frame: one frame out per
frame in; field: one per field, so twice the frames leave at twice the rate (give the encoder behind the pipe `-r` accordingly).
--field-order tff|bff names the field that comes first in time (default tff).  --frames counts input frames.

--detelecine takes film carried as interlaced video by 2:3 pulldown (NTSC film and anime DVDs): in the
same place, every frame is matched with the field of itself, its predecessor or its successor that combs least, frames that
stay combed go through yadif's rule (--detelecine-combed keep: they stay), and of every five frames the one closest to its
predecessor, the repeat, is dropped: n frames in, n - n // 5 out, so tell the consumer 4/5 of the input's frame rate.  The nets
see four film frames where the input has five.  The rule is this project's own (tests/ivtc_ref.py): parity with ffmpeg's
fieldmatch / decimate filters is unpinned.  --detelecine-thresh T, --detelecine-combed-limit L, --detelecine-keep-all.

The first net of a lane takes the input format and its last net produces the output format (Net.submit_pix: the
conversions run on the net's stream around its kernels); nets in between pass u8 BGR (u16 BGR with --bit-depth 16).  A leading `-m n=K` stage converts
its frames with uva_pix_convert; `-s 1` without a net converts every frame once, or copies it when the formats are equal.

Frames go through Net.submit_u8 / collect_u8 (include/uva.h): page-locked rings on the host, H2D copy,
kernels and D2H copy of consecutive frames overlapped on three streams.  `-m a` runs the reference's
anime pass first (1x HurrDeblur, whole frame, re-quantised to u8 exactly like the PNG hop of
upscale_processing.py:909), then the 2x/4x net with the reference's 960-px tiles.

Flags follow upscale_video.py where they mean the same thing: -s/--scale 1|2|4, -m/--models a,n=K,r (in the reference's
order: denoise, anime pass, upscale; upscale/upscale_processing.py:880-920),
-g/--gpu a list of HIP ordinals, one worker per entry (duplicates allowed).  Pipes: one reader deals the frames
out round-robin, one writer puts the results out in frame order.  File to file: one contiguous segment of frames per
entry, each with its own reader, chain of nets and writer on its own file handles (stream_segments) -- no shared serial
copy, so the route scales with the GPUs.  Measured on the GPU box (profiles/r05_ab_results.txt blocks 8, 9): on a real file
system (the container's overlay) positional writes of several workers into ONE file scale -- 187 (one worker), 372 (two), 436
(four) frames/s at 1080p -> 4K = 0.93 of the /dev/null rate; on tmpfs (/dev/shm) one file takes ~200 frames/s = 5 GB/s whatever
writes into it and more writers make it worse -- its page allocation under the inode lock is the limit, and only `-o x,y,...`
(one file per worker: separate inodes, 457-477 frames/s) gets past it there.  Two things built to beat the inode lock and
measured no better, kept as options: MappedSegment (each worker copying through a shared mapping of its byte range,
UVA_RAW_MMAP=1: slower than write() on tmpfs, equal on overlay) and `--write-threads N` (a worker's frames cut into pieces
written with os.pwrite by a pool: +10 % for one worker on overlay, -40 % on tmpfs; default 1).
"""
import argparse
import ctypes
import mmap
import os
import sys
import threading
import queue

import numpy as np

from . import ncnn
from .upscale_processing import TILE_BORDER, TILE_SIZE

MODEL_FILES = {  # upscale/upscale_processing.py:880-916
    1: "1x_HurrDeblur_SubCompact_nf24-nc8_244k_net_g",
    2: "2x_Compact_Pretrain",
    4: "4x_Compact_Pretrain",
}
PIPE_DEPTH = 3   # include/uva.h: at most 3 frames in flight per net


class PixFormats:
    """the raw-video formats of a stream's two ends and the colour arithmetic between them (ncnn.PIX_FORMATS_ALL etc.)"""

    def __init__(self, in_fmt="bgr24", out_fmt="bgr24", colour="bt601", color_range="tv", bit_depth=8, chroma_filter="replicate",
                 chroma_loc="left", out_size=None, resize_filter="lanczos", crop=None):
        for f in (in_fmt, out_fmt):
            if f not in ncnn.PIX_FORMATS_ALL:
                raise ValueError("unknown pixel format %r (%s)" % (f, ", ".join(ncnn.PIX_FORMATS_ALL)))
        if bit_depth not in (8, 16):
            raise ValueError("bit depth must be 8 or 16")
        for f in (in_fmt, out_fmt):
            if bit_depth == 8 and f in ncnn.PIX16_ONLY:
                raise ValueError("%s is a 16-bit format: it needs --bit-depth 16" % f)
        ncnn.colour_word(colour, color_range, chroma_filter, chroma_loc)              # (checks the names)
        self.chroma_filter, self.chroma_loc = chroma_filter, chroma_loc
        self.in_fmt, self.out_fmt, self.colour, self.color_range = in_fmt, out_fmt, colour, color_range
        self.bit_depth = bit_depth     # 16: the net runs on u16 BGR, no 8-bit hop at either end
        if resize_filter not in ncnn.RESIZE_FILTERS:
            raise ValueError("unknown resize filter %r (%s)" % (resize_filter, ", ".join(ncnn.RESIZE_FILTERS)))
        if out_size is not None and (len(out_size) != 2 or min(out_size) < 1):
            raise ValueError("out_size must be (height, width), both at least 1")
        # (oh, ow): a lane's last stage resamples its result to this size; None: the nets' own size
        self.out_size = None if out_size is None else (int(out_size[0]), int(out_size[1]))
        self.resize_filter = resize_filter
        # (W, H, X, Y), ffmpeg's order: the window of every input frame that the first stage of a lane takes;
        # None: whole frames
        if crop is not None and (len(crop) != 4 or min(crop[:2]) < 1 or min(crop[2:]) < 0):
            raise ValueError("crop must be (W, H, X, Y), W and H at least 1, X and Y at least 0")
        self.crop = None if crop is None else tuple(int(v) for v in crop)

    def net_size(self, h, w):
        """the size of the frames the first stage works on, of h x w frames on the input"""
        return (self.crop[1], self.crop[0]) if self.crop is not None else (h, w)

    def window(self, h, w):
        """Net.set_input_window's arguments for h x w frames on the input, or None"""
        return (h, w, self.crop[2], self.crop[3]) if self.crop is not None else None

    def cut(self, frame, h, w, out=None, gpu=0):
        """the window of one h x w input frame, host to host (ncnn.pix_window): for first stages that are no net"""
        ch, cw = self.net_size(h, w)
        return ncnn.pix_window(frame, self.in_fmt, h, w, self.crop[2], self.crop[3], ch, cw, out=out, gpu=gpu)

    def depth_kw(self):
        """the keyword the 16-bit calls take (none at 8 bits: those calls are the first pixel-format release's)"""
        return {"bit_depth": 16} if self.bit_depth == 16 else {}

    def chroma_kw(self):
        """the keywords of the interpolating chroma modes (none for replicate: those calls are the earlier releases')"""
        if self.chroma_filter == "replicate":
            return {}
        return {"chroma_filter": self.chroma_filter, "chroma_loc": self.chroma_loc}

    def resize_kw(self):
        """the keywords of the resampler (none without an output size: those calls are the earlier releases')"""
        if self.out_size is None:
            return {}
        kw = {"out_size": self.out_size}
        if self.resize_filter != "lanczos":
            kw["resize_filter"] = self.resize_filter
        return kw

    def result_size(self, h, w):
        """the size of the frames that leave a lane whose nets produce h x w"""
        return self.out_size if self.out_size is not None else (h, w)

    def frame_bytes(self, h, w, out=False):
        return ncnn.pix_frame_bytes(self.out_fmt if out else self.in_fmt, h, w)


BGR = PixFormats()


def load_net(stem, gpu, model_path):
    net = ncnn.Net()
    net.opt.use_vulkan_compute = True
    net.set_vulkan_device(gpu)
    base = os.path.join(model_path, stem)
    if net.load_param(base + ".param") != 0 or net.load_model(base + ".bin") != 0:
        raise RuntimeError(getattr(net, "last_error", "cannot load " + base))
    return net


def _real_nets(lanes_spec):
    """the nets of a worker's chain, or of a list of chains (the denoise stage is no net)"""
    chains = lanes_spec if lanes_spec and isinstance(lanes_spec[0], list) else [lanes_spec]
    return [net for chain in chains for net, _ in chain if not isinstance(net, tuple)]


def set_skip_repeats(lanes_spec, threshold):
    """--skip-repeats on every net of every lane (Net.set_skip_repeats).  In the `-m a` chain the second
    stage finds the repeats itself: the first stage's outputs for them are equal bytes."""
    for net in _real_nets(lanes_spec):
        net.set_skip_repeats(threshold)


def skip_summary(lanes_spec):
    """'skipped k of n': the net runs --skip-repeats saved, of the frames submitted to the nets (every net of a chain counts)"""
    stats = [net.skip_stats() for net in _real_nets(lanes_spec)]
    return "skipped %d of %d" % (sum(k for _, k in stats), sum(n for n, _ in stats))


def read_exact(f, view):
    """Fill `view` from f; returns False on a clean EOF before the first byte, raises on a torn frame."""
    got = 0
    n = len(view)
    while got < n:
        k = f.readinto(view[got:])
        if not k:
            if got == 0:
                return False
            raise EOFError("input ended inside a frame (%d of %d bytes)" % (got, n))
        got += k
    return True


class Stage:
    """One net with its own ring of page-locked result buffers and up to PIPE_DEPTH frames in flight."""

    def __init__(self, net, h, w, tile_size, alloc, in_fmt="bgr24", out_fmt="bgr24", pix=BGR, resize=False, window=None):
        self.net, self.tile = net, tile_size
        # window (src_h, src_w, x, y): the frames submitted are src_h x src_w frames of which the net takes h x w at (x, y)
        # (Net.set_input_window: the window's rows are all that is uploaded); a lane's first stage with --crop
        self.window = window
        if window is not None:
            net.set_input_window(*window)
        elif getattr(net, "_window", None) is not None:
            net.set_input_window()             # (a net that an earlier, cropped stream used)
        self.h, self.w, self.in_fmt, self.out_fmt, self.pix = h, w, in_fmt, out_fmt, pix
        s = net.scale
        # resize: the lane's last stage, whose result is resampled to pix.out_size behind the net (Net.submit_pix(out_size=...))
        self.resize_kw = pix.resize_kw() if resize else {}
        oh, ow = pix.result_size(h * s, w * s) if resize else (h * s, w * s)
        # A result buffer stays in use while its frame is in flight here (<= depth frames) and then
        # while the consumer holds it -- the next stage reads it as pinned input until that stage's
        # collect (<= depth frames), or the writer thread (queue of 2 + 1 being written).  Frames stay
        # in order, so 2*depth + 2 buffers can never wrap onto a live one.
        self.outs = [ncnn.pix_empty(out_fmt, oh, ow, alloc) for _ in range(2 * PIPE_DEPTH + 2)]
        self.n = 0
        self.inflight = []

    def full(self):
        return len(self.inflight) >= PIPE_DEPTH

    def submit(self, frame):
        out = self.outs[self.n % len(self.outs)]
        self.n += 1
        border = TILE_BORDER if self.tile else 0
        if self.in_fmt == self.out_fmt == "bgr24" and self.pix.bit_depth == 8 and not self.resize_kw and self.window is None:
            self.inflight.append(self.net.submit_u8(frame, out=out, tile_size=self.tile, border=border))
        else:
            self.inflight.append(self.net.submit_pix(frame, self.h, self.w, self.in_fmt, out=out, out_fmt=self.out_fmt,
                                                     colour=self.pix.colour, color_range=self.pix.color_range,
                                                     tile_size=self.tile, border=border, **self.pix.depth_kw(),
                                                     **self.pix.chroma_kw(), **self.resize_kw))

    def collect(self):
        return self.net.collect_u8(self.inflight.pop(0))


class DenoiseStage:
    """`-m n=K` (apply_denoise, upscale/upscale_processing.py:350-354) as a stage of a lane: cv2.fastNlMeansDenoisingColored's
    arithmetic on the lane's GPU (include/uva.h uva_denoise_u8), host frame in, host frame out like the nets' stages -- the call
    takes about a millisecond per 1080p frame and releases the interpreter lock, the nets behind it keep their frames in flight.
    Frames of another format than bgr24 on either end are converted on the same GPU (include/uva.h uva_pix_convert).
    pix.bit_depth 16: the stage's native format is bgr48le and the call is uva_denoise_u16 -- in_fmt ->
    bgr48le with convert_pix(bit_depth=16), the 16-bit non-local means, bgr48le handed on mid-chain or converted to out_fmt."""

    class _Scale1:
        scale = 1

    def __init__(self, gpu, strength, h, w, alloc, in_fmt="bgr24", out_fmt="bgr24", pix=BGR, window=None):
        self.gpu, self.strength = gpu, float(strength)
        # window (src_h, src_w, x, y): the frames submitted are src_h x src_w frames, cut to h x w first (ncnn.pix_window)
        self.window = window
        self._cut = ncnn.pix_empty(in_fmt, h, w, alloc) if window is not None else None
        self.net = self._Scale1()
        self.in_fmt, self.out_fmt, self.pix = in_fmt, out_fmt, pix
        self.native = "bgr48le" if pix.bit_depth == 16 else "bgr24"
        self.outs = [ncnn.pix_empty(out_fmt, h, w, alloc) for _ in range(2 * PIPE_DEPTH + 2)]
        self._bgr_in = ncnn.pix_empty(self.native, h, w, alloc) if in_fmt != self.native else None      # (used and done with inside submit)
        self._bgr_out = ncnn.pix_empty(self.native, h, w, alloc) if out_fmt != self.native else None
        self.h, self.w = h, w
        self.n = 0
        self.inflight = []

    def full(self):
        return len(self.inflight) >= 1

    def denoise(self, frame, dst):
        """the stage's arithmetic on one native frame (bgr24, or bgr48le at 16 bits), host to host"""
        from . import _lib
        L = _lib.load()
        if self.native == "bgr48le" and not hasattr(L, "uva_denoise_u16"):
            raise _lib.UvaError("this libuva build has no 16-bit denoise stage: rebuild it")
        fn = L.uva_denoise_u16 if self.native == "bgr48le" else L.uva_denoise_u8
        _lib.check(fn(self.gpu, frame.ctypes.data, self.h, self.w, frame.strides[0], dst.ctypes.data, dst.strides[0],
                      self.strength, self.strength))

    def submit(self, frame):
        out = self.outs[self.n % len(self.outs)]
        self.n += 1
        h, w = self.h, self.w
        pix = self.pix
        if self.window is not None:
            frame = pix.cut(frame, self.window[0], self.window[1], out=self._cut, gpu=self.gpu)
        if self.in_fmt != self.native:
            frame = ncnn.convert_pix(frame, h, w, self.in_fmt, self.native, pix.colour, pix.color_range, out=self._bgr_in, gpu=self.gpu,
                                     **pix.depth_kw(), **pix.chroma_kw())
        elif self.native == "bgr48le":
            frame = np.asarray(frame).reshape(-1).view(np.uint16).reshape(h, w, 3)      # (the reader's flat bytes)
        dst = out if self.out_fmt == self.native else self._bgr_out
        self.denoise(frame, dst)
        if self.out_fmt != self.native:
            ncnn.convert_pix(dst, h, w, self.native, self.out_fmt, pix.colour, pix.color_range, out=out, gpu=self.gpu,
                             **pix.depth_kw(), **pix.chroma_kw())
        self.inflight.append(out)

    def collect(self):
        return self.inflight.pop(0)


class Lane:
    """The chain of nets of ONE -g entry (one or two Stages on one GPU).  Frames go in with submit() and come out,
    in the order they went in, with pop()."""

    def __init__(self, nets_tiles, h, w, alloc, pix=BGR, src=None):
        """h x w: the frames the first stage works on; src (h, w): the frames submitted when pix.crop cuts them to that"""
        self.stages = []
        last = len(nets_tiles) - 1
        for k, (net, tile) in enumerate(nets_tiles):
            # the first stage takes the stream's input format, the last one produces its output format, u8 BGR in between
            # (--bit-depth 16: u16 BGR, so that the hop between the nets of `-m a` keeps the depth)
            mid = "bgr48le" if pix.bit_depth == 16 else "bgr24"
            fmts = dict(in_fmt=pix.in_fmt if k == 0 else mid, out_fmt=pix.out_fmt if k == last else mid, pix=pix)
            if k == 0 and src is not None and pix.crop is not None:
                fmts["window"] = pix.window(*src)
            if isinstance(net, tuple):         # ("denoise", gpu, K): the `-m n=K` stage
                if k == last and pix.out_size is not None:
                    raise ValueError("--out-size / --out-scale: the resampler sits behind a net, and this lane ends in the denoise "
                                     "stage (-s 1 -m n=K): add -m a or -s 2|4, or resize the denoised frames in a second run")
                self.stages.append(DenoiseStage(net[1], net[2], h, w, alloc, **fmts))
                continue
            self.stages.append(Stage(net, h, w, tile, alloc, **fmts, **({"resize": True} if k == last and pix.out_size is not None else {})))
            h, w = h * net.scale, w * net.scale
        self.count = 0                         # frames inside

    def _shift(self):
        """Finished frames move on to the next stage wherever that stage has room and this one is full."""
        for k in range(len(self.stages) - 2, -1, -1):
            while self.stages[k].full() and not self.stages[k + 1].full():
                self.stages[k + 1].submit(self.stages[k].collect())

    def full(self):
        self._shift()
        return self.stages[0].full()

    def submit(self, frame):
        assert not self.full()
        self.stages[0].submit(frame)
        self.count += 1

    def pop(self):
        """The oldest frame's result (blocks until the GPU is done with it)."""
        assert self.count > 0, "pop() on an empty lane"

        def ensure(k):
            assert k >= 0, "no frame in flight in any stage"
            if self.stages[k].inflight:
                return
            ensure(k - 1)
            self.stages[k].submit(self.stages[k - 1].collect())
        last = len(self.stages) - 1
        ensure(last)
        self.count -= 1
        return self.stages[last].collect()


class DeintSpec:
    """--deinterlace: yadif in front of everything else (ncnn.Deinterlacer).  mode "frame": one frame out
    per frame in; "field": two, at twice the frame rate.  field_order "tff" / "bff"."""

    def __init__(self, mode="frame", field_order="tff"):
        ncnn.deint_flags(mode, field_order)              # (checks the names)
        self.mode, self.field_order = mode, field_order
        self.per_frame = 2 if mode == "field" else 1

    def open(self, fmt, h, w, gpu):
        return ncnn.Deinterlacer(fmt, h, w, self.mode, self.field_order, gpu=gpu)


class DetelecineSpec:
    """--detelecine: inverse telecine of 2:3 pulldown in front of everything else, where --deinterlace would sit
    (ncnn.Detelecine).  n input frames give n - n // 5 frames (keep_all: n).  The handles it opens add
    their counters to `totals` when they close."""
    per_frame = 1

    def __init__(self, field_order="tff", thresh=9, combed="yadif", combed_limit=1000, keep_all=False):
        ncnn.ivtc_flags(field_order, combed, keep_all)      # (checks the names)
        if not 0 <= int(thresh) <= 255:
            raise ValueError("the comb threshold T is 0 ... 255 on the 8-bit scale, not %d" % thresh)
        if not 0 <= int(combed_limit) <= 1000000:
            raise ValueError("the combed limit L is 0 ... 1000000 parts per million, not %d" % combed_limit)
        self.field_order, self.thresh, self.combed, self.combed_limit, self.keep_all = field_order, int(thresh), combed, int(combed_limit), bool(keep_all)
        self.totals = dict.fromkeys(ncnn.IVTC_STATS, 0)
        self._lock = threading.Lock()

    def out_frames(self, n):
        return n if self.keep_all else n - n // 5

    def open(self, fmt, h, w, gpu):
        spec = self

        class Handle(ncnn.Detelecine):
            def close(self):
                if getattr(self, "_h", None) is not None:
                    with spec._lock:
                        for k, v in self.stats().items():
                            spec.totals[k] += v
                super().close()
        return Handle(fmt, h, w, self.field_order, self.thresh, self.combed, self.combed_limit, self.keep_all, gpu=gpu)

    def summary(self):
        t = self.totals
        return ("detelecine: %d frames in, %d out; matches c/p/n %d/%d/%d, %d combed, %d dropped"
                % (t["frames_in"], t["frames_out"], t["match_c"], t["match_p"], t["match_n"], t["combed"], t["dropped"]))


def _lane_gpu(spec):
    """the HIP ordinal of a lane's first stage"""
    first = spec[0][0]
    return first[1] if isinstance(first, tuple) else first.device_index


def deinterlaced(fin, di, raw, outs_for, max_frames=None, lead=False, trail=False):
    """The reader with --deinterlace: frames are read from fin into `raw` and pushed through the Deinterlacer `di`; yields the
    number of deinterlaced frames (0, 1 or 2) that a push or the final flush wrote into the buffers outs_for() named.
    max_frames counts input frames.  lead: the first frame read is the frame BEFORE the stream's first -- context only, it is
    read on top of max_frames and its outputs are discarded (yielded as 0).  trail: when max_frames frames were read, one more
    is read as the last frame's successor instead of flushing, if the input has one."""
    view = memoryview(raw).cast("B")
    limit = None if max_frames is None else max_frames + (1 if lead else 0)
    n_read = n_done = 0                  # frames read; frames whose outputs have been produced

    def produced(k):
        nonlocal n_done
        if k:
            n_done += 1
            if lead and n_done == 1:
                return 0
        return k
    while limit is None or n_read < limit:
        if not read_exact(fin, view):
            break
        n_read += 1
        yield produced(di.push(raw, outs_for()))
    if trail and limit is not None and n_read == limit and read_exact(fin, view):
        yield produced(di.push(raw, outs_for()))
        di.reset()
    else:
        yield produced(di.flush(outs_for()))


def detelecined(fin, dt, raw, outs_for, max_frames=None, lead=False, trail=False):
    """The reader with --detelecine, beside deinterlaced(): frames are read from fin into `raw` and pushed through the Detelecine
    handle `dt`; yields 1 whenever a push or a flush step wrote a frame into the buffer outs_for()[0] named, else 0.  At the end
    of the input it flushes until the handle is empty.  max_frames counts input frames.  A stream is never cut (its cycles of
    five would have to align), so there are no context frames: lead / trail must be False."""
    if lead or trail:
        raise ValueError("--detelecine: a stream is not cut into segments")
    view = memoryview(raw).cast("B")
    n_read = 0
    while max_frames is None or n_read < max_frames:
        if not read_exact(fin, view):
            break
        n_read += 1
        yield dt.push(raw, outs_for()[0])
    while True:
        k = dt.flush(outs_for()[0])
        if not k:
            return
        yield k


def _front_reader(spec):
    """the generator that reads frames through what `spec` (DeintSpec / DetelecineSpec) opens"""
    return detelecined if isinstance(spec, DetelecineSpec) else deinterlaced


class DeintReader:
    """A byte stream of deinterlaced frames over the input `fin`, for the routes that read frames with read_exact and run no lane
    (copy_through): readinto() serves the outputs of deinterlaced() one after the other.  max_frames counts input frames."""

    def __init__(self, fin, deint, fmt, h, w, gpu=0, max_frames=None):
        self._di = deint.open(fmt, h, w, gpu)
        nb = ncnn.pix_frame_bytes(fmt, h, w)
        self._outs = [np.empty(nb, np.uint8) for _ in range(deint.per_frame)]
        self._gen = _front_reader(deint)(fin, self._di, np.empty(nb, np.uint8), lambda: self._outs, max_frames)
        self._ready, self._pos = [], 0       # frames produced and not served yet; bytes served of the first

    def readinto(self, view):
        while not self._ready:
            k = next(self._gen, None)
            if k is None:
                return 0
            self._ready = [memoryview(o) for o in self._outs[:k]]
        src = self._ready[0]
        n = min(len(view), len(src) - self._pos)
        view[:n] = src[self._pos:self._pos + n]
        self._pos += n
        if self._pos == len(src):
            self._ready.pop(0)
            self._pos = 0
        return n

    def close(self):
        self._di.close()


def _regular_fd(f):
    """the descriptor behind f if it is a regular file we may write to with os.pwrite, else None"""
    import stat
    try:
        fd = f.fileno()
        return fd if stat.S_ISREG(os.fstat(fd).st_mode) else None
    except (AttributeError, OSError, ValueError):
        return None


def stream(fin, fout, h, w, nets_tiles, alloc=None, max_frames=None, write_threads=1, pix=None, deint=None, deint_lead=False,
           deint_trail=False):
    """Reads h x w frames of pix.in_fmt (PixFormats; default u8 [h][w][3] bgr24 at both ends) from fin until EOF, pushes each through the nets in order, writes the
    results to fout.  nets_tiles: list of (Net, tile_size) -- one GPU worker -- or a list of such lists,
    one per `-g` entry (duplicates allowed, as in the reference's worker list, README.md:45-61): ONE reader
    deals the frames out round-robin (the partition of upscale_processing.py:565-598, frames being
    independent units), every entry keeps up to PIPE_DEPTH frames in flight per net, and ONE writer puts
    the results out in frame order.  write_threads > 1 and fout a regular file: every result frame is cut into that many pieces
    written with os.pwrite by a small pool (one thread copies ~5 GB/s into the page cache: a 4K frame every 5 ms, half of what
    one GPU delivers).  Results are frames of pix.out_fmt.  Returns the number of frames written.
    deint (DeintSpec): every frame read goes through a Deinterlacer on the first lane's GPU first, and what comes out -- 0, 1 or 2
    frames of the input's format and size -- is dealt to the lanes as frames read from fin are without it; at the end of the
    input the deinterlacer is flushed.  max_frames counts input frames.  deint_lead / deint_trail: fin starts one frame before
    the stream / holds the frame after max_frames, as context (stream_segments; deinterlaced()).  deint may also be a
    DetelecineSpec (--detelecine): the same place, a Detelecine handle, and at the end of the input it is flushed until empty
    (detelecined()); a push hands out at most one frame, so the ring is that of per_frame 1."""
    alloc = alloc or ncnn.pinned_empty
    pix = pix or BGR
    lanes_spec = nets_tiles if nets_tiles and isinstance(nets_tiles[0], list) else [nets_tiles]
    src_h, src_w = h, w                    # the frames on the input; with pix.crop the lanes work on a window of them
    h, w = pix.net_size(h, w)
    lanes = [Lane(spec, h, w, alloc, pix, src=(src_h, src_w)) for spec in lanes_spec]
    nl = len(lanes)
    # an input buffer is free again once its frame has left its lane's first stage: at most PIPE_DEPTH per lane are
    # there, plus the one being read into
    ins = [ncnn.pix_empty(pix.in_fmt, src_h, src_w, alloc) for _ in range(nl * PIPE_DEPTH + 2)]
    if deint is not None:
        # with the deinterlacer the ring holds ITS outputs: a push writes up to two frames (A and B) before either is handed to
        # a lane, so beside the PIPE_DEPTH per lane that are in first stages two are being written, plus one to spare as above;
        # the frame read from the input has a buffer of its own (the push has uploaded it when it returns)
        ins += [ncnn.pix_empty(pix.in_fmt, src_h, src_w, alloc) for _ in range(deint.per_frame - 1)]
        raw = ncnn.pix_empty(pix.in_fmt, src_h, src_w, alloc)

    # writer thread: the blocking write of frame i overlaps the read of frame i+k and the GPUs
    wq = queue.Queue(maxsize=2)
    werr = []

    fd = _regular_fd(fout) if write_threads > 1 else None
    pool = None
    if fd is not None:
        from concurrent.futures import ThreadPoolExecutor
        fout.flush()
        pos0 = fout.tell()
        pool = ThreadPoolExecutor(max_workers=write_threads)

    def pwrite_all(view, pos):
        while len(view):
            k = os.pwrite(fd, view, pos)
            view, pos = view[k:], pos + k

    sink = PipeSink(fout, ring=min(len(lane.stages[-1].outs) for lane in lanes))

    def writer():
        pos = pos0 if fd is not None else 0
        try:
            while True:
                item = wq.get()
                if item is None:
                    if fd is not None:
                        fout.seek(pos)
                    return
                if fd is None:
                    sink.write(item)
                    continue
                view = memoryview(item).cast("B")
                n = len(view)
                per = -(-n // write_threads)
                piece = -(-per // (1 << 20)) * (1 << 20)              # whole MiB per writer
                jobs = [pool.submit(pwrite_all, view[o:o + piece], pos + o) for o in range(0, n, piece)]
                for j in jobs:
                    j.result()
                pos += n
        except Exception as e:  # noqa: BLE001
            werr.append(e)
            while wq.get() is not None:
                pass

    wt = threading.Thread(target=writer, daemon=True)
    wt.start()
    written = 0

    def pop_next():
        """frame number `written` comes out of its lane and goes to the writer"""
        nonlocal written
        res = lanes[written % nl].pop()
        if werr:
            raise werr[0]
        wq.put(res)
        written += 1

    n_in = 0
    di = None
    try:
        if deint is not None:
            di = deint.open(pix.in_fmt, src_h, src_w, _lane_gpu(lanes_spec[0]))
            for k in _front_reader(deint)(fin, di, raw, lambda: [ins[(n_in + j) % len(ins)] for j in range(deint.per_frame)], max_frames,
                                          deint_lead, deint_trail):
                for _ in range(k):
                    lane = lanes[n_in % nl]
                    while lane.full():
                        pop_next()
                    lane.submit(ins[n_in % len(ins)])
                    n_in += 1
        while deint is None and (max_frames is None or n_in < max_frames):
            buf = ins[n_in % len(ins)]
            if not read_exact(fin, memoryview(buf).cast("B")):
                break
            lane = lanes[n_in % nl]
            while lane.full():                 # frames leave in global order: at most nl pops free a slot of this lane
                pop_next()
            lane.submit(buf)
            n_in += 1
        while written < n_in:
            pop_next()
    finally:
        wq.put(None)
        wt.join()
        if pool is not None:
            pool.shutdown()
        if di is not None:
            di.close()
    if werr:
        raise werr[0]
    fout.flush()
    sink.drain()
    return written


def filesystem_type(path):
    """fstype of the mount `path` lives on (/proc/self/mountinfo, longest mount point that is a prefix); None if unknown"""
    try:
        real = os.path.realpath(path)
        best, kind = "", None
        for line in open("/proc/self/mountinfo"):
            left, _, right = line.partition(" - ")
            mp = left.split()[4].replace("\\040", " ")
            if (real == mp or real.startswith(mp.rstrip("/") + "/")) and len(mp) >= len(best):
                best, kind = mp, right.split()[0]
        return kind
    except (OSError, IndexError):
        return None


class MappedSegment:
    """The writer's end of ONE worker's byte range of a shared output file: a shared mapping of just that range, filled frame by
    frame with plain memory copies (numpy releases the interpreter lock for them).  Why not write(): every buffered write() /
    pwrite() on a file holds its inode lock for the whole copy -- ext4, xfs and tmpfs alike -- so N writers into ONE file
    proceed one at a time however disjoint their offsets (measured: four workers SLOWER than one,
    profiles/r04_final_rawvideo_bench.txt); stores through a mapping fault their pages in independently.  The pages of a
    frame are asked for in one call (MADV_POPULATE_WRITE, Linux 5.14+) instead of 6 075 faults where the kernel knows it."""
    _POPULATE_WRITE = getattr(mmap, "MADV_POPULATE_WRITE", 23)

    def __init__(self, f, offset, nbytes):
        self._f = f
        gran = mmap.ALLOCATIONGRANULARITY
        base = offset - offset % gran
        self._pos = offset - base
        try:
            self._mm = mmap.mmap(f.fileno(), self._pos + nbytes, access=mmap.ACCESS_WRITE, offset=base)
        except Exception:
            f.close()                            # (the handle was handed over: nobody else closes it)
            raise
        self._arr = np.frombuffer(self._mm, np.uint8)
        self._populate = hasattr(self._mm, "madvise")

    def write(self, view):
        src = np.frombuffer(view, np.uint8)
        n, p = src.size, self._pos
        if p + n > self._arr.size:
            raise ValueError("write past the end of the segment")
        if self._populate:
            a = p - p % mmap.PAGESIZE
            try:
                self._mm.madvise(self._POPULATE_WRITE, a, p + n - a)
            except (OSError, ValueError):
                self._populate = False          # an older kernel: plain page faults do the same, one page at a time
        np.copyto(self._arr[p:p + n], src)
        self._pos = p + n
        return n

    def flush(self):
        pass                                    # (the page cache has the bytes; durability is the caller's fsync, as with write())

    def close(self):
        self._arr = None
        self._mm.close()
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def stream_segments(in_path, out_path, h, w, lanes_spec, scale_total, max_frames=None, alloc=None, opener=open, mapped=None,
                    write_threads=1, pix=None, deint=None):
    """The same frames -> the same bytes as stream(), for regular FILES, with NO shared serial copy: one contiguous segment of
    frames per `-g` entry (the reference's batches, upscale/upscale_processing.py:923-948, are such segments), and every entry
    runs its own stream() -- its own reader, its own pipelined chain of nets, its own writer thread -- on its own file handles.
      in_path   one file: cut into len(lanes_spec) segments, each read at its offset;  a list: one input file per entry
      out_path  one file: sized first, then every entry writes at the offset its results belong to, on its own handle (`write_threads`
                positional writers per entry); `mapped=True` / UVA_RAW_MMAP=1: through a shared mapping of its byte range instead
                (MappedSegment; space checked with statvfs, blocks reserved with posix_fallocate where that is cheap -- measured
                slower than write() on tmpfs and on overlayfs, kept as an option);  a list: one output file per entry
    One reader and one writer thread copy ~10 GB/s each, two or three GPUs' worth of 1080p -> 4K frames; N independent pairs
    scale with the entries.  A worker that fails takes the output with it: the file(s) this call created are removed (a
    full-size file of zeros and holes is worse than none).  pix: PixFormats of the two ends (default bgr24).  Returns the number
    of frames written.
    deint (DeintSpec): every segment deinterlaces its own frames (stream(deint=...)).  A segment of ONE input file that does not
    begin the file reads the frame before its first as context, its outputs discarded, and one that does not end the stream
    reads the frame after its last instead of flushing: the bytes are those of a single lane.  Output counts, offsets and the
    file's size are in output frames, twice the input frames for mode "field".  One input file per entry: every file is a
    stream of its own."""
    pix = pix or BGR
    per = deint.per_frame if deint is not None else 1          # output frames per input frame
    ivtc = isinstance(deint, DetelecineSpec)
    if ivtc and not isinstance(in_path, (list, tuple)):
        raise ValueError("--detelecine: one input file is one stream and is not cut into segments (its cycles of five would have to "
                         "align); give every -g entry an input file of its own, or deal the frames out round-robin")
    net_h, net_w = pix.net_size(h, w)      # (pix.crop: the lanes work on a window of the h x w frames in the file)
    fb_in, fb_out = pix.frame_bytes(h, w), pix.frame_bytes(*pix.result_size(net_h * scale_total, net_w * scale_total), out=True)
    nl = len(lanes_spec)
    ins = list(in_path) if isinstance(in_path, (list, tuple)) else None
    outs = list(out_path) if isinstance(out_path, (list, tuple)) else None
    if (ins is not None and len(ins) != nl) or (outs is not None and len(outs) != nl):
        raise ValueError("one input / output file per -g entry: %d entries" % nl)
    if mapped is None:
        mapped = os.environ.get("UVA_RAW_MMAP", "0") == "1"
    for i in (ins if ins is not None else [in_path]):
        for o in (outs if outs is not None else [out_path]):
            if os.path.exists(o) and os.path.samefile(i, o):
                raise ValueError("%s is input and output at once: the output is sized (truncated) before anything is read" % o)

    def frames_of(path):
        size = os.path.getsize(path)
        if size % fb_in:
            raise EOFError("%s ends inside a frame (%d bytes, frames of %d)" % (path, size, fb_in))
        return size // fb_in
    if ins is None:
        total = frames_of(in_path)
        if max_frames is not None:
            total = min(total, max_frames)
        bounds = [total * k // nl for k in range(nl + 1)]
        counts = [bounds[k + 1] - bounds[k] for k in range(nl)]
        in_first = bounds[:nl]
    else:
        counts, left = [], max_frames
        for path in ins:                         # --frames counts through the files in order
            c = frames_of(path) if left is None else min(frames_of(path), left)
            left = None if left is None else left - c
            counts.append(c)
        in_first = [0] * nl
        total = sum(counts)
    in_total = total                                            # input frames of the stream
    out_counts = [deint.out_frames(c) if ivtc else c * per for c in counts]     # (--detelecine: every file loses its own repeats)
    out_first = [0] * nl if outs is not None else [sum(out_counts[:k]) for k in range(nl)]
    total = sum(out_counts)                                     # (from here on: output frames)
    created = [o for o in (outs if outs is not None else [out_path]) if not os.path.exists(o)]
    if outs is None:
        with opener(out_path, "wb") as f:       # the output exists at its full size before anybody writes into it
            f.truncate(total * fb_out)
            if mapped and total:
                # stores into a hole of a full file system end in SIGBUS, not in ENOSPC: make sure of the space first
                st = os.statvfs(out_path)
                if st.f_bavail * st.f_frsize < total * fb_out:
                    f.truncate(0)
                    raise OSError(28, "%s: %d bytes of results do not fit the file system (%d free)"
                                  % (out_path, total * fb_out, st.f_bavail * st.f_frsize))
                if filesystem_type(out_path) not in ("tmpfs", "ramfs", None):
                    try:
                        os.posix_fallocate(f.fileno(), 0, total * fb_out)
                    except OSError:
                        pass                     # (a file system without fallocate: the check above stands)
    done, errs = [0] * nl, []

    def work(k):
        try:
            # a segment starts with no kept frame (--skip-repeats; each lane has nets of its own, so this is for clarity)
            for net in _real_nets(lanes_spec[k]):
                if hasattr(net, "reset_reference"):
                    net.reset_reference()
            if counts[k] == 0:
                if outs is not None:
                    opener(outs[k], "wb").close()
                return
            kw = {}
            lead = False
            if deint is not None:
                # context frames: the one before the segment's first and the one after its last, where the stream has them
                lead = ins is None and in_first[k] > 0
                kw = dict(deint=deint, deint_lead=lead, deint_trail=ins is None and in_first[k] + counts[k] < in_total)
            with opener(in_path if ins is None else ins[k], "rb") as fin:
                fin.seek((in_first[k] - (1 if lead else 0)) * fb_in)
                if outs is None and mapped:
                    with MappedSegment(opener(out_path, "r+b"), out_first[k] * fb_out, out_counts[k] * fb_out) as fout:
                        done[k] = stream(fin, fout, h, w, lanes_spec[k], alloc=alloc, max_frames=counts[k], pix=pix, **kw)
                else:
                    with opener(out_path if outs is None else outs[k], "r+b" if outs is None else "wb") as fout:
                        fout.seek(out_first[k] * fb_out)
                        done[k] = stream(fin, fout, h, w, lanes_spec[k], alloc=alloc, max_frames=counts[k], write_threads=write_threads,
                                         pix=pix, **kw)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    threads = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(nl)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errs:
        for o in created:
            try:
                os.remove(o)
            except OSError:
                pass
        raise errs[0]
    return sum(done)


def grow_pipe(f):
    """A frame is 6-100 MB and a pipe holds 64 KiB by default: ask for the largest buffer the system gives an
    unprivileged process (/proc/sys/fs/pipe-max-size, usually 1 MiB) -- 16 times fewer wake-ups per frame."""
    import fcntl
    import stat
    try:
        if not stat.S_ISFIFO(os.fstat(f.fileno()).st_mode):
            return
        want = int(open("/proc/sys/fs/pipe-max-size").read())
        fcntl.fcntl(f.fileno(), getattr(fcntl, "F_SETPIPE_SZ", 1031), want)
    except (OSError, ValueError, AttributeError):
        pass


class PipeSink:
    """The writer's end of a PIPE (stdout into ffmpeg): result frames go in with vmsplice(2) -- the pipe then refers to the pages
    of our page-locked result buffer and the only copy left is the reader's -- instead of write(2), which allocates a pipe page
    and copies into it for every 4 KiB (one thread manages ~6 GB/s of that: 250 4K frames a second, half of what one GPU
    delivers; profiles/r05_final_rawvideo_bench.txt).  No SPLICE_F_GIFT: the pages stay ours, so a buffer must not be rewritten
    while the pipe still refers to it -- vmsplice returns once the LAST piece of a frame is in the pipe, whose capacity is far
    below one frame, so when frame k + 1 has been handed over frame k has been read completely; the result rings hold eight
    buffers (Stage.outs; `ring`, when given, is checked to be at least PIPE_DEPTH + 4 before anything is spliced: the frames in
    flight, the writer's queue and the frame in the pipe).  Falls back to write() for good the first time the kernel refuses
    (memory it cannot take references on, a pipe that went away is an error as before)."""

    class _IoVec(ctypes.Structure):
        _fields_ = [("base", ctypes.c_void_p), ("len", ctypes.c_size_t)]

    def __init__(self, f, ring=None):
        import stat
        self._f = f
        self._ring = ring
        self._fd = None
        self._cap = None            # the pipe's capacity, asked for at the first frame (grow_pipe may come after the constructor)
        self.spliced = 0            # frames that went through vmsplice (tests, the bench's log line)
        try:
            fd = f.fileno()
            if stat.S_ISFIFO(os.fstat(fd).st_mode) and os.environ.get("UVA_RAW_VMSPLICE", "1") != "0":
                self._libc = ctypes.CDLL(None, use_errno=True)
                self._libc.vmsplice.restype = ctypes.c_ssize_t
                self._fd = fd
        except (AttributeError, OSError, ValueError):
            self._fd = None

    def write(self, arr):
        """arr: a C-contiguous numpy array (a result buffer of a Stage)"""
        if self._fd is not None and self._cap is None:
            import fcntl
            try:
                self._cap = fcntl.fcntl(self._fd, getattr(fcntl, "F_GETPIPE_SZ", 1032))
            except OSError:
                self._cap = 1 << 30
        if self._fd is None or arr.nbytes < self._cap:        # (frames smaller than the pipe: several could sit in it, still referred to)
            self._f.write(memoryview(arr).cast("B"))
            return
        assert self._ring is None or self._ring >= PIPE_DEPTH + 4, "a ring of %d result buffers is too short to splice from" % self._ring
        self._f.flush()             # (nothing of ours is buffered in front of the spliced bytes)
        addr, n, off = arr.ctypes.data, arr.nbytes, 0
        while off < n:
            iov = self._IoVec(addr + off, n - off)
            k = self._libc.vmsplice(self._fd, ctypes.byref(iov), 1, 0)
            if k < 0:
                err = ctypes.get_errno()
                if err == 4:        # EINTR
                    continue
                if off == 0 and err in (14, 22, 38):      # EFAULT / EINVAL / ENOSYS: this memory or this kernel cannot
                    self._fd = None
                    self._f.write(memoryview(arr).cast("B"))
                    return
                raise OSError(err, os.strerror(err))
            off += k
        self.spliced += 1

    def flush(self):
        self._f.flush()

    def drain(self, timeout=60.0):
        """After the LAST frame: wait until the reader has taken every spliced byte out of the pipe (FIONREAD = 0).  The pipe
        refers to our buffers' pages; the caller is about to free them (page-locked memory goes back to the driver's pool), and
        what the reader then found in the pipe's last megabyte would be whatever the pool did with those pages."""
        if self._fd is None or not self.spliced:
            return
        import array
        import fcntl
        import termios
        import time
        t0 = time.monotonic()
        n = array.array("i", [0])
        while time.monotonic() - t0 < timeout:
            try:
                fcntl.ioctl(self._fd, termios.FIONREAD, n, True)
            except OSError:
                return                      # (the reader went away: nothing to protect)
            if n[0] == 0:
                return
            time.sleep(0.001)


def copy_through(fin, fout, h, w, max_frames=None, pix=None, gpu=0, deint=None):
    """`-s 1` without `-m a`: the reference renames the frames, nothing is computed (:924-929).  Formats that differ at the two
    ends (pix): every frame is converted once on HIP device `gpu` (include/uva.h uva_pix_convert; with pix.bit_depth 16
    uva_pix_convert16, through u16 BGR).  With pix.out_size every frame is converted to BGR, resampled (include/uva.h uva_resize)
    and converted to the output format at the new size.  deint (DeintSpec): the frames are deinterlaced first, on the same
    device (DeintReader; max_frames counts input frames) -- with equal formats at both ends a deinterlace-only run; a
    DetelecineSpec likewise: a detelecine-only run."""
    pix = pix or BGR
    if deint is not None:
        reader = DeintReader(fin, deint, pix.in_fmt, h, w, gpu=gpu, max_frames=max_frames)
        try:
            return copy_through(reader, fout, h, w, None, pix=pix, gpu=gpu)
        finally:
            reader.close()
    src_h, src_w = h, w
    h, w = pix.net_size(h, w)              # (pix.crop: every frame is cut first, ncnn.pix_window)
    if pix.out_size is not None and pix.out_size != (h, w):
        return _copy_through_sized(fin, fout, src_h, src_w, max_frames, pix, gpu)
    buf = bytearray(pix.frame_bytes(src_h, src_w))
    cut = np.empty(pix.frame_bytes(h, w), np.uint8) if pix.crop is not None else None
    res = ncnn.pix_empty(pix.out_fmt, h, w) if pix.in_fmt != pix.out_fmt else None
    n = 0
    while max_frames is None or n < max_frames:
        if not read_exact(fin, memoryview(buf)):
            break
        frame = buf
        if cut is not None:
            frame = memoryview(pix.cut(np.frombuffer(buf, np.uint8), src_h, src_w, out=cut, gpu=gpu))
        if res is None:
            fout.write(frame)
        else:
            ncnn.convert_pix(np.frombuffer(frame, np.uint8), h, w, pix.in_fmt, pix.out_fmt, pix.colour, pix.color_range, out=res, gpu=gpu,
                             **pix.depth_kw(), **pix.chroma_kw())
            fout.write(memoryview(res).cast("B"))
        n += 1
    fout.flush()
    return n


def _copy_through_sized(fin, fout, h, w, max_frames, pix, gpu):
    """copy_through with a resampler: in_fmt -> BGR (u8, or u16 at 16 bits) -> pix.out_size -> out_fmt, synchronous calls"""
    oh, ow = pix.out_size
    native = "bgr48le" if pix.bit_depth == 16 else "bgr24"
    kw = dict(colour=pix.colour, color_range=pix.color_range, gpu=gpu, **pix.depth_kw(), **pix.chroma_kw())
    src_h, src_w = h, w
    h, w = pix.net_size(h, w)
    whole = ncnn.pix_empty(pix.in_fmt, src_h, src_w)
    buf = ncnn.pix_empty(pix.in_fmt, h, w) if pix.crop is not None else whole
    small = ncnn.pix_empty(native, h, w)
    big = ncnn.pix_empty(native, oh, ow)
    res = ncnn.pix_empty(pix.out_fmt, oh, ow)
    n = 0
    while max_frames is None or n < max_frames:
        if not read_exact(fin, memoryview(whole).cast("B")):
            break
        if pix.crop is not None:
            pix.cut(whole, src_h, src_w, out=buf, gpu=gpu)
        bgr = buf if pix.in_fmt == native else ncnn.convert_pix(buf, h, w, pix.in_fmt, native, out=small, **kw)
        ncnn.resize(bgr, (oh, ow), pix.resize_filter, gpu=gpu, out=big)
        done = big if pix.out_fmt == native else ncnn.convert_pix(big, oh, ow, native, pix.out_fmt, out=res, **kw)
        fout.write(memoryview(done).cast("B"))
        n += 1
    fout.flush()
    return n


def out_scale_size(h, w, f):
    """--out-scale F at an h x w input: per axis 2 floor(n F / 2 + 0.5), at least 2 (even sizes: 4:2:0 formats, encoders)"""
    import math
    return tuple(max(2, 2 * int(math.floor(n * f / 2 + 0.5))) for n in (h, w))


def parse_crop(text):
    """'W:H:X:Y' (ffmpeg's order; a leading 'crop=' is accepted, as --cropdetect and ffmpeg print it) -> (W, H, X, Y)"""
    import re
    m = re.fullmatch(r"(?:crop=)?(\d+):(\d+):(\d+):(\d+)", text.strip())
    if not m:
        raise ValueError("--crop takes W:H:X:Y (ffmpeg's order, e.g. 1920:800:0:140) or auto, not %r" % text)
    cw, ch, x, y = (int(g) for g in m.groups())
    if cw < 1 or ch < 1:
        raise ValueError("--crop: the window must be at least 1x1, not %dx%d" % (cw, ch))
    return cw, ch, x, y


def crop_sample_positions(n_frames):
    """Where --crop auto and --cropdetect look at a file of n_frames frames: the reference's recipe (get_crop_detect,
    upscale/upscale_processing.py:144-152: `-ss (i + 1) * int(duration / 120)` for i = 10 ... 109, two frames each) in frames
    instead of seconds -- min((i + 1) * (n_frames // 120), n_frames - 2), never below 0, duplicates dropped, in order."""
    step = n_frames // 120
    out = []
    for i in range(10, 110):
        p = max(0, min((i + 1) * step, n_frames - 2))
        if p not in out:
            out.append(p)
    return out if n_frames > 0 else []


class CropVotes:
    """One vote per frame shown: the rectangle after that frame.  The most frequent wins, ties go to the larger area, then to the
    rectangle seen first."""

    def __init__(self):
        self.count = {}         # (W, H, X, Y) -> votes, in order of first appearance

    def add(self, rect):
        if rect is not None:
            self.count[rect] = self.count.get(rect, 0) + 1

    def winner(self):
        best = None
        for rect, c in self.count.items():
            if best is None or (c, rect[0] * rect[1]) > (self.count[best], best[0] * best[1]):
                best = rect
        return best


def detect_crop_file(path, h, w, fmt, limit=24, round=16, gpu=0, max_frames=None, detector=None):
    """--crop auto / --cropdetect on a regular file of h x w frames of fmt: at every position of crop_sample_positions a fresh
    detector (ncnn.CropDetector: the line sums on the GPU) sees two consecutive frames and casts one vote per frame.  Returns
    (W, H, X, Y) or None."""
    detector = detector or ncnn.CropDetector
    fb = ncnn.pix_frame_bytes(fmt, h, w)
    size = os.path.getsize(path)
    if size % fb:
        raise EOFError("%s ends inside a frame (%d bytes, frames of %d)" % (path, size, fb))
    n = size // fb if max_frames is None else min(size // fb, max_frames)
    votes = CropVotes()
    buf = np.empty(fb, np.uint8)
    with open(path, "rb") as f:
        for p in crop_sample_positions(n):
            det = detector(h, w, fmt, limit=limit, round=round, gpu=gpu)
            f.seek(p * fb)
            for _ in range(min(2, n - p)):
                if not read_exact(f, memoryview(buf)):
                    break
                det.update(buf)
                votes.add(det.rect())
    return votes.winner()


def detect_crop_pipe(fin, h, w, fmt, limit=24, round=16, gpu=0, stride=240, max_frames=None, detector=None):
    """--cropdetect on a pipe: the whole input is read, and every `stride` frames a fresh detector sees a pair of frames, one vote
    per frame.  Returns (W, H, X, Y) or None."""
    detector = detector or ncnn.CropDetector
    if stride < 2:
        raise ValueError("--cropdetect-stride: at least 2 frames (a pair is looked at every so many)")
    buf = np.empty(ncnn.pix_frame_bytes(fmt, h, w), np.uint8)
    votes = CropVotes()
    det, n = None, 0
    while max_frames is None or n < max_frames:
        if not read_exact(fin, memoryview(buf)):
            break
        if n % stride == 0:
            det = detector(h, w, fmt, limit=limit, round=round, gpu=gpu)
        if n % stride < 2:
            det.update(buf)
            votes.add(det.rect())
        n += 1
    return votes.winner()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("-i", "--input", default="-", help="rawvideo file (--in-pix-fmt), '-' = stdin; a,b,...: one segment file per -g entry")
    ap.add_argument("-o", "--output", default="-", help="rawvideo file (--out-pix-fmt), '-' = stdout; x,y,...: one output file per -g entry "
                                                        "(a single input is cut into segments, segment k goes to the k-th file)")
    ap.add_argument("-W", "--width", type=int, required=True)
    ap.add_argument("-H", "--height", type=int, required=True)
    ap.add_argument("-s", "--scale", type=int, default=2, choices=[1, 2, 4])
    ap.add_argument("-m", "--models", default="", help="upscale_video.py -m: a = 1x HurrDeblur pass first, n=K = film-grain denoise "
                                                       "(K 1..30) before everything, on 16-bit samples with --bit-depth 16 (K means "
                                                       "the same at both depths), r = the x_Valar_v1 model (scale 4, needs its .bin, "
                                                       "8 bits only)")
    ap.add_argument("-g", "--gpu", default="0",
                    help="HIP ordinals, one worker per entry, e.g. 0,1,2,3 or 0,0,1 (upscale_video.py -g; default 0)")
    ap.add_argument("--tile", type=int, default=TILE_SIZE, help="reference tile size of the final pass (960); 0 = whole frame")
    ap.add_argument("--frames", type=int, default=None, help="stop after this many frames")
    ap.add_argument("--write-threads", type=int, default=1,
                    help="positional writers per worker for a regular output file (default 1: more gained 10 %% on a disk-backed file "
                         "system and lost 40 %% on tmpfs)")
    ap.add_argument("--round-robin", action="store_true",
                    help="file to file with several -g entries: deal the frames out one by one through ONE reader and ONE writer "
                         "(what pipes get) instead of one contiguous segment of frames, reader and writer per entry")
    ap.add_argument("--in-pix-fmt", default="bgr24", choices=list(ncnn.PIX_FORMATS_ALL),
                    help="ffmpeg -pix_fmt of the input frames (default bgr24; 4:2:0: yuv420p, nv12, p010le, yuv420p10le; 4:2:2: yuv422p, "
                         "yuv422p10le); converted to BGR on the GPU")
    ap.add_argument("--out-pix-fmt", default="bgr24", choices=list(ncnn.PIX_FORMATS_ALL),
                    help="ffmpeg -pix_fmt of the output frames (default bgr24; the same names); converted from the net's BGR on the GPU")
    ap.add_argument("--colorspace", default="bt601", choices=list(ncnn.COLORSPACES),
                    help="Y'CbCr matrix of the Y'CbCr formats' frames (default bt601: what ffmpeg applies to the reference's "
                         "untagged PNGs)")
    ap.add_argument("--color-range", default="tv", choices=list(ncnn.COLOR_RANGES), help="tv = limited (default), pc = full")
    ap.add_argument("--bit-depth", type=int, default=8, choices=[8, 16],
                    help="16: the 2x / 4x net runs on 16-bit samples, so 10-bit frames (p010le, yuv420p10le, yuv422p10le) keep their "
                         "depth (default 8); of the -m options it takes -m a, whose 1x net then runs on 16-bit samples as well, "
                         "and -m n=K, whose non-local means then runs on 16-bit Lab planes (both with a 10- or 16-bit pixel format "
                         "on at least one end); -m r runs at 8 bits only")
    ap.add_argument("--model-path", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "models"))
    ap.add_argument("--chroma-filter", default="replicate", choices=list(ncnn.CHROMA_FILTERS),
                    help="chroma resampling in the Y'CbCr conversions (4:2:2 formats: along the row alone; DESIGN.md section 7.7): "
                         "replicate (default: every chroma sample repeated over its "
                         "2x2 block coming in, the block's average going out; the earlier releases' bytes) or bilinear (interpolated "
                         "for where the chroma samples sit, so the net is not fed 2x2 colour steps and colour stays registered with "
                         "luma; DESIGN.md section 7.5)")
    ap.add_argument("--chroma-loc", default=None, choices=list(ncnn.CHROMA_LOCS),
                    help="with --chroma-filter bilinear: where the chroma samples sit (ffmpeg's chroma_sample_location).  left "
                         "(default): video from H.264 / HEVC; center: JPEG / MPEG-1; topleft: UHD BT.2020 material")
    ap.add_argument("--out-size", default=None, metavar="WxH",
                    help="resample the result to this size on the GPU, behind the net and in front of the output conversion "
                         "(e.g. -s 2 --out-size 2560x1440 at 720p input; each axis within [1/4, 4] of the net's result; DESIGN.md "
                         "section 7.6)")
    ap.add_argument("--out-scale", type=float, default=None, metavar="F",
                    help="the same, as the total scale relative to the INPUT frame (Real-ESRGAN's --outscale): per axis "
                         "2 floor(n F / 2 + 0.5), at least 2; not together with --out-size")
    ap.add_argument("--resize-filter", default="lanczos", choices=list(ncnn.RESIZE_FILTERS),
                    help="the resampler's filter (default lanczos: sinc(x) sinc(x/3); bicubic: Keys, a = -0.5; bilinear); widened when "
                         "an axis shrinks")
    ap.add_argument("--skip-repeats", type=int, nargs="?", const=0, default=None, metavar="T",
                    help="do not run a net on a frame that repeats the last frame the net ran on: its result is delivered again "
                         "(animation on twos and threes, screen captures, telecined film).  T (default 0: exact, the output is "
                         "byte for byte what it is without the option) is the largest difference in code values, 0 ... 65535, "
                         "at which a sample still counts as equal; DESIGN.md section 7.8")
    ap.add_argument("--crop", default=None, metavar="W:H:X:Y|auto",
                    help="cut this window (ffmpeg's order) out of every -W x -H input frame in front of the first stage; everything "
                         "behind works from the cropped size and only the window is uploaded.  auto: find it first as the "
                         "reference does (cropdetect's rule at 100 places of the file, the most frequent rectangle; regular files "
                         "only).  Y'CbCr formats: X and W even, 4:2:0 formats also Y and H; DESIGN.md section 7.12")
    ap.add_argument("--cropdetect", action="store_true",
                    help="analysis only: read the whole input (a pipe too), write no frames, print one crop=W:H:X:Y line for --crop "
                         "or for ffmpeg's -vf.  A file is sampled as --crop auto samples it, a pipe every --cropdetect-stride frames")
    ap.add_argument("--cropdetect-stride", type=int, default=240, metavar="N",
                    help="--cropdetect on a pipe: a pair of frames is looked at every N frames (default 240)")
    ap.add_argument("--crop-limit", type=int, default=24, metavar="L",
                    help="--crop auto / --cropdetect: a line is picture when its mean is above L on the 8-bit scale (0 ... 255; "
                         "cropdetect's default 24)")
    ap.add_argument("--crop-round", type=int, default=16, metavar="R",
                    help="--crop auto / --cropdetect: width and height are rounded down to a multiple of R (cropdetect's default 16)")
    ap.add_argument("--deinterlace", default=None, metavar="frame|field",
                    help="deinterlace the input on the GPU in front of everything else, by yadif's spatio-temporal rule per component "
                         "plane (DVD, broadcast and tape material; DESIGN.md section 7.13).  frame: one frame out per frame in; "
                         "field: one per field, twice the frames at twice the rate.  --frames counts input frames.  --crop auto "
                         "and --cropdetect keep sampling the source frames directly: bars are black in both fields")
    ap.add_argument("--field-order", default=None, metavar="tff|bff",
                    help="with --deinterlace or --detelecine: which rows come first in time, tff (default: the even rows, top field "
                         "first) or bff")
    ap.add_argument("--detelecine", action="store_true",
                    help="inverse telecine on the GPU in front of everything else: NTSC film and anime carried as interlaced video "
                         "by 2:3 pulldown get their film frames back by field matching, and one frame of every five, the repeat, "
                         "is dropped (DESIGN.md section 7.15; the rule is this project's own, parity with ffmpeg's fieldmatch / "
                         "decimate is unpinned).  n input frames give n - n // 5 frames: tell the consumer a frame rate of 4/5 of "
                         "the input's (24000/1001 for 30000/1001).  --frames counts input frames.  Not together with --deinterlace")
    ap.add_argument("--detelecine-thresh", type=int, default=None, metavar="T",
                    help="with --detelecine: a sample counts as combed when it differs from both vertical neighbours, in the same "
                         "direction, by more than T on the 8-bit scale (0 ... 255, default 9)")
    ap.add_argument("--detelecine-combed", default=None, metavar="yadif|keep",
                    help="with --detelecine: a frame that stays combed after matching is deinterlaced by yadif's rule (default) or "
                         "kept as matched")
    ap.add_argument("--detelecine-combed-limit", type=int, default=None, metavar="L",
                    help="with --detelecine: a matched frame is combed when more than L parts per million of its samples are "
                         "(0 ... 1000000, default 1000: a guess, no telecined real material was at hand to set it; an option, "
                         "not a tested bar)")
    ap.add_argument("--detelecine-keep-all", action="store_true",
                    help="with --detelecine: match fields but drop nothing (n frames out for n in, the repeats stay)")
    a = ap.parse_args(argv)
    if a.width <= 0 or a.height <= 0:
        ap.error("frame size must be positive")
    deint = None
    if a.field_order is not None and a.deinterlace is None and not a.detelecine:
        ap.error("--field-order needs --deinterlace frame|field or --detelecine")
    if a.detelecine and a.deinterlace is not None:
        ap.error("--detelecine and --deinterlace exclude each other: telecined film is matched, not interpolated (frames that stay "
                 "combed go through yadif anyway, --detelecine-combed)")
    if not a.detelecine:
        for opt, val in (("--detelecine-thresh", a.detelecine_thresh), ("--detelecine-combed", a.detelecine_combed),
                         ("--detelecine-combed-limit", a.detelecine_combed_limit), ("--detelecine-keep-all", a.detelecine_keep_all or None)):
            if val is not None:
                ap.error("%s needs --detelecine" % opt)
    else:
        if a.field_order is not None and a.field_order not in ncnn.FIELD_ORDERS:
            ap.error("--field-order takes tff or bff, not %r" % a.field_order)
        if a.detelecine_combed is not None and a.detelecine_combed not in ncnn.IVTC_COMBED:
            ap.error("--detelecine-combed takes yadif or keep, not %r" % a.detelecine_combed)
        if a.detelecine_thresh is not None and not 0 <= a.detelecine_thresh <= 255:
            ap.error("--detelecine-thresh is 0 ... 255 on the 8-bit scale, not %d" % a.detelecine_thresh)
        if a.detelecine_combed_limit is not None and not 0 <= a.detelecine_combed_limit <= 1000000:
            ap.error("--detelecine-combed-limit is 0 ... 1000000 parts per million, not %d" % a.detelecine_combed_limit)
        if a.height < 4:
            ap.error("--detelecine: frames of fewer than 4 rows (-H %d) have no two rows of either field in every plane" % a.height)
        deint = DetelecineSpec(a.field_order or "tff", 9 if a.detelecine_thresh is None else a.detelecine_thresh,
                               a.detelecine_combed or "yadif", 1000 if a.detelecine_combed_limit is None else a.detelecine_combed_limit,
                               a.detelecine_keep_all)
    if a.deinterlace is not None:
        if a.deinterlace not in ncnn.DEINT_MODES:
            ap.error("--deinterlace takes frame or field, not %r" % a.deinterlace)
        if a.field_order is not None and a.field_order not in ncnn.FIELD_ORDERS:
            ap.error("--field-order takes tff or bff, not %r" % a.field_order)
        if a.height < 4:
            ap.error("--deinterlace: frames of fewer than 4 rows (-H %d) have no two rows of either field in every plane" % a.height)
        deint = DeintSpec(a.deinterlace, a.field_order or "tff")
    if a.skip_repeats is not None and not 0 <= a.skip_repeats <= 65535:
        ap.error("--skip-repeats takes a threshold T of 0 ... 65535 code values, not %d" % a.skip_repeats)
    try:
        gpus = [int(tok) for tok in str(a.gpu).split(",") if tok != ""] or [0]
    except ValueError:
        ap.error("-g takes a comma-separated list of GPU ordinals")
    if not 0 <= a.crop_limit <= 255:
        ap.error("--crop-limit is 0 ... 255 on the 8-bit scale, not %d" % a.crop_limit)
    if a.cropdetect_stride < 2:
        ap.error("--cropdetect-stride: at least 2 frames")
    if a.in_pix_fmt in ncnn.PIX16_ONLY and a.bit_depth != 16:
        ap.error("%s is a 16-bit format: it needs --bit-depth 16" % a.in_pix_fmt)
    crop = None
    if a.cropdetect or (a.crop is not None and a.crop.strip() == "auto"):
        what = "--cropdetect" if a.cropdetect else "--crop auto"
        is_file = a.input != "-" and os.path.isfile(a.input)
        if not a.cropdetect and not is_file:
            ap.error("--crop auto looks at 100 places of the input and then reads it again, so it needs a regular file, not a pipe "
                     "(%s): run --cropdetect on the stream first and hand its crop=W:H:X:Y to --crop" % a.input)
        kw = dict(limit=a.crop_limit, round=a.crop_round, gpu=gpus[0], max_frames=a.frames)
        if is_file:
            crop = detect_crop_file(a.input, a.height, a.width, a.in_pix_fmt, **kw)
        else:
            fin = sys.stdin.buffer if a.input == "-" else open(a.input, "rb")
            grow_pipe(fin)
            try:
                crop = detect_crop_pipe(fin, a.height, a.width, a.in_pix_fmt, stride=a.cropdetect_stride, **kw)
            finally:
                if fin is not sys.stdin.buffer:
                    fin.close()
        if a.cropdetect:
            if crop is None:
                print("%s: no frame had a bright line, no rectangle" % what, file=sys.stderr)
            else:
                print("crop=%d:%d:%d:%d" % crop)
            ncnn.destroy_gpu_instance()
            return 0 if crop is not None else 1
        if crop is None:
            print("--crop auto: no frame had a bright line, no rectangle: the frames go uncropped", file=sys.stderr)
        else:
            print("--crop auto: crop=%d:%d:%d:%d" % crop, file=sys.stderr)
    elif a.crop is not None:
        try:
            crop = parse_crop(a.crop)
        except ValueError as e:
            ap.error(str(e))
    if crop is not None:
        from ._lib import UvaError
        try:
            ncnn.pix_window_check(a.in_pix_fmt, a.height, a.width, crop[2], crop[3], crop[1], crop[0])
        except UvaError as e:
            ap.error("--crop %d:%d:%d:%d of %dx%d %s frames: %s" % (crop + (a.width, a.height, a.in_pix_fmt, e)))
        if crop == (a.width, a.height, 0, 0):
            crop = None                         # the whole frame: today's calls
    # the size the lanes work on: everything below that used to take -W / -H takes this
    net_h, net_w = (crop[1], crop[0]) if crop is not None else (a.height, a.width)
    out_size = None
    if a.out_size is not None and a.out_scale is not None:
        ap.error("--out-size and --out-scale exclude each other")
    if a.out_size is not None:
        import re
        m = re.fullmatch(r"(\d+)[xX](\d+)", a.out_size.strip())
        if not m or int(m.group(1)) < 1 or int(m.group(2)) < 1:
            ap.error("--out-size takes WIDTHxHEIGHT, both at least 1 (e.g. 2560x1440), not %r" % a.out_size)
        out_size = (int(m.group(2)), int(m.group(1)))
    elif a.out_scale is not None:
        if not a.out_scale > 0 or a.out_scale != a.out_scale or a.out_scale == float("inf"):
            ap.error("--out-scale takes a positive number")
        out_size = out_scale_size(net_h, net_w, a.out_scale)
    if out_size is not None:
        flag = "--out-size" if a.out_size is not None else "--out-scale"
        for n_out, n_net, what in ((out_size[0], net_h * a.scale, "height"), (out_size[1], net_w * a.scale, "width")):
            if n_out * 4 < n_net or n_out > n_net * 4:
                ap.error("%s: %s %d is outside [1/4, 4] of the net's result (%d with -s %d)" % (flag, what, n_out, n_net, a.scale))
        if out_size == (net_h * a.scale, net_w * a.scale):
            out_size = None                     # the nets' own size: nothing to resample, today's calls
    for f in (a.in_pix_fmt, a.out_pix_fmt):
        if f in ncnn.PIX16_ONLY and a.bit_depth != 16:
            ap.error("%s is a 16-bit format: it needs --bit-depth 16" % f)
    if a.chroma_loc is not None and a.chroma_filter != "bilinear":
        ap.error("--chroma-loc needs --chroma-filter bilinear: replicate knows no siting")
    pix = PixFormats(a.in_pix_fmt, a.out_pix_fmt, a.colorspace, a.color_range, a.bit_depth, a.chroma_filter, a.chroma_loc or "left",
                     out_size, a.resize_filter, crop)
    # upscale_video.py -m: a (anime pass), n=K (film-grain denoise, K = 1..30, :782-789), r (the x_Valar_v1 model instead of
    # x_Compact_Pretrain, :913-916); the reference runs them in the order n, a, upscale (:880-920) whatever the order given
    models = [m for m in a.models.split(",") if m]
    denoise = None
    for m in models:
        if m.startswith("n="):
            try:
                denoise = int(m[2:])
            except ValueError:
                ap.error("-m n=K takes an integer K")
            if not 1 <= denoise <= 30:
                ap.error("-m n=K: K must be between 1 and 30")
        elif m not in ("a", "r"):
            ap.error("unknown model option %r (a, n=K, r)" % m)
    deep = ", ".join(f for f in ncnn.PIX_FORMATS_ALL if ncnn.pix_depth(f) > 8)
    shallow = all(ncnn.pix_depth(f) == 8 for f in (a.in_pix_fmt, a.out_pix_fmt))
    if a.bit_depth == 16 and models and shallow and any(m != "a" for m in models):
        # (8-bit frames in and out, the default bgr24 among them: refused as before the 16-bit denoise stage existed, in the words
        # tests/test_rawvideo_bitdepth16_chain.py and tests/test_pixfmt16.py pin)
        ap.error("--bit-depth 16 takes the 2x and 4x Compact nets only: -m n=K and -m r run at 8 bits (-m %s with 8-bit frames, %s "
                 "in and %s out; with a 10- or 16-bit format -- %s -- on at least one end -m n=K and -m a run on 16-bit samples, "
                 "-m r never)" % (a.models, a.in_pix_fmt, a.out_pix_fmt, deep))
    if a.bit_depth == 16 and "r" in models:
        ap.error("--bit-depth 16 takes the Compact nets, -m a and -m n=K: -m r has no 16-bit weights to run on and runs at 8 bits "
                 "(-m %s)" % a.models)
    if a.bit_depth == 16 and models and shallow:
        # (the plain pair, with the default bgr24 at both ends, is held to a refusal by a pinned test, tests/test_pixfmt16.py;
        # what the 16-bit chain is for -- frames of more than 8 bits -- names such a format on at least one end)
        ap.error("--bit-depth 16 -m %s is for frames of more than 8 bits: name a 10- or 16-bit format (%s) with --in-pix-fmt or "
                 "--out-pix-fmt, or run the chain at 8 bits (%s in, %s out)" % (a.models, deep, a.in_pix_fmt, a.out_pix_fmt))
    if out_size is not None and a.scale == 1 and denoise is not None and "a" not in models:
        ap.error("--out-size / --out-scale: the resampler sits behind a net, and -s 1 -m n=K ends in the denoise stage: add -m a or "
                 "-s 2|4")
    final_stem = MODEL_FILES[a.scale]
    if "r" in models:
        if a.scale != 4:
            ap.error("-m r: the reference has x_Valar_v1 at scale 4 only (models/4x_Valar_v1.param)")
        final_stem = "4x_Valar_v1"
        if not os.path.exists(os.path.join(a.model_path, final_stem + ".bin")):
            ap.error("-m r: %s.bin is not in %s (a missing blob upstream: supply it with --model-path)" % (final_stem, a.model_path))
    # upscale_video.py: `-m a` runs the 1x HurrDeblur pass (process_model, :888-909), `-s 2|4` the Compact net
    # (upscale_frames, :930-944), and `-s 1` performs NO network pass of its own: its frames are only renamed
    # (:924-929).  So `-s 1` alone copies frames through, `-s 1 -m a` is the HurrDeblur pass alone.
    nets = []                     # one chain of nets per -g entry
    for gpu in gpus:
        chain = []
        if denoise is not None:
            chain.append((("denoise", gpu, denoise), 0))
        if "a" in models:
            chain.append((load_net(MODEL_FILES[1], gpu, a.model_path), 0))          # apply_model: whole frame
            if a.bit_depth == 16:
                chain[-1][0].enable_u16_1x()
        if a.scale != 1:
            chain.append((load_net(final_stem, gpu, a.model_path), a.tile))
        if chain:
            nets.append(chain)
    # file -> file with several workers: one contiguous segment of frames per worker, each with its own reader and writer.
    # "a,b,..." is a LIST only where a list means something -- more than one -g entry -- and only if no file of exactly that
    # name exists (a path may contain a comma)
    def as_list(arg):
        if len(gpus) > 1 and "," in arg and not os.path.exists(arg):
            return arg.split(",")
        return [arg]
    ins, outs = as_list(a.input), as_list(a.output)
    if len(ins) > 1 or len(outs) > 1:
        if not nets:
            ap.error("-i / -o lists give every -g entry's NETWORK PASS a file of its own; `-s 1` without -m a / n=K only copies "
                     "frames through (upscale_processing.py:924-929): one input, one output")
        if (len(ins) > 1 and len(ins) != len(nets)) or (len(outs) > 1 and len(outs) != len(nets)) or "-" in ins + outs:
            ap.error("-i / -o lists: one regular file per -g entry (%d entries)" % len(nets))
    for i in ins:
        for o in outs:
            if i != "-" and o != "-" and os.path.exists(i) and os.path.exists(o) and os.path.samefile(i, o):
                ap.error("%s is input and output at once" % o)
    wthreads = max(1, a.write_threads)
    regular = all(os.path.isfile(f) for f in ins) and all(not os.path.exists(f) or os.path.isfile(f) for f in outs)
    # ONE output file on tmpfs: every write into it allocates its pages under the inode's lock, so several workers writing their
    # segments into it are SLOWER than one (246.7 -> 208.3 -> 162.4 frames/s at 1 / 4 / 8 workers, profiles/r05_final_rawvideo_bench.txt;
    # a disk-backed file system scales: 201 -> 431 -> 614).  There the workers feed ONE writer thread instead (the pipe route's
    # shape: one reader, frames dealt round-robin, results written in order) -- never slower than one worker.  `-o a,b,..` (a file
    # per worker) is the way past the lock and keeps its segments.
    one_file_on_tmpfs = (len(nets) > 1 and len(outs) == 1 and a.output != "-" and
                         filesystem_type(os.path.dirname(os.path.abspath(a.output)) or ".") in ("tmpfs", "ramfs") and
                         os.environ.get("UVA_RAW_TMPFS_SEGMENTS") != "1")
    segments = bool(nets) and (len(ins) > 1 or len(outs) > 1 or (len(nets) > 1 and not a.round_robin and not one_file_on_tmpfs and
                                                                  a.input != "-" and a.output != "-" and regular))
    if isinstance(deint, DetelecineSpec) and segments and len(ins) == 1:
        # one input file is one stream: its cycles of five would have to align with the segments' borders
        print("--detelecine: one input file is not cut into segments; the %d -g entries take its frames round-robin" % len(nets),
              file=sys.stderr)
        segments = False
    summary = lambda n: "%d frames" % n                                               # noqa: E731
    if a.skip_repeats is not None and nets:
        if len(nets) > 1 and not segments:
            ap.error("--skip-repeats with %d -g entries on a route that deals the frames out one by one (pipes, --round-robin, one "
                     "output file on tmpfs): consecutive frames land in different lanes and nothing would ever repeat.  Use one -g "
                     "entry, or file-to-file segments" % len(nets))
        set_skip_repeats(nets, a.skip_repeats)
        summary = lambda n: "%d frames, %s" % (n, skip_summary(nets))                 # noqa: E731
    if segments:
        if not regular:
            ap.error("-i / -o lists take regular files")
        scale_total = 1
        for net, _ in nets[0]:
            scale_total *= 1 if isinstance(net, tuple) else net.scale
        n = stream_segments(ins if len(ins) > 1 else ins[0], outs if len(outs) > 1 else outs[0], a.height, a.width, nets, scale_total,
                            max_frames=a.frames, write_threads=wthreads, pix=pix, **({"deint": deint} if deint is not None else {}))
        print(summary(n), file=sys.stderr)
        if isinstance(deint, DetelecineSpec):
            print(deint.summary(), file=sys.stderr)
        ncnn.destroy_gpu_instance()
        return 0
    fin = sys.stdin.buffer if a.input == "-" else open(a.input, "rb")
    created = a.output != "-" and not os.path.exists(a.output)
    fout = sys.stdout.buffer if a.output == "-" else open(a.output, "wb")
    for f in (fin, fout):
        grow_pipe(f)
    ok = False
    try:
        if nets:
            n = stream(fin, fout, a.height, a.width, nets, max_frames=a.frames, write_threads=wthreads, pix=pix,
                       **({"deint": deint} if deint is not None else {}))
        else:
            n = copy_through(fin, fout, a.height, a.width, a.frames, pix=pix, gpu=gpus[0], **({"deint": deint} if deint is not None else {}))
        ok = True
    finally:
        if fin is not sys.stdin.buffer:
            fin.close()
        if fout is not sys.stdout.buffer:
            fout.close()
            if not ok and created and os.path.isfile(a.output):
                os.remove(a.output)                # half a stream under the name of a whole one helps nobody
    print(summary(n), file=sys.stderr)
    if isinstance(deint, DetelecineSpec):
        print(deint.summary(), file=sys.stderr)
    ncnn.destroy_gpu_instance()
    return 0


if __name__ == "__main__":
    sys.exit(main())
