/*
 * uva.h -- C ABI of libuva.so, the MI355X (gfx950) per-frame super-resolution engine that
 * replaces the `ncnn_vulkan` surface used by davlee1972/upscale_video's worker functions.
 *
 * Every entry point cites the reference call site (file:line under /root/reference) whose
 * ncnn call it replaces.  Plain pointers and sizes only; no torch / numpy types.
 * All functions returning int return 0 on success and non-zero on error (ncnn's
 * convention for load_param/load_model/extract); uva_last_error() gives the message of the
 * last failure on the calling thread.
 *
 * Threading: a uva_net belongs to one thread at a time (the reference holds one
 * process-global net per pool worker, upscale/upscale_processing.py:22,57,65).  HIP is
 * initialised lazily inside the calling process, so the library is safe to load in a
 * multiprocessing "spawn" worker (:321, :565).
 *
 * There is NO CPU path: with no usable HIP device every compute entry point fails.
 */
#ifndef UVA_H
#define UVA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UVA_ABI_VERSION 15  /* 2: + uva_net_submit_u8 / uva_net_collect_u8 / uva_host_alloc / uva_host_free;
                               3: + uva_get_gpu_pci_bus_id, uva_debug_trunk2_schedule;
                               4: + uva_denoise_u8, uva_debug_denoise_stage; generic graphs (4x_Valar_v1) load;
                               5: + uva_debug_sub10_rows;
                               6: + uva_net_submit_u8_png, uva_png_workspace_bytes, uva_png_assemble, uva_png_deflate_u8,
                                  uva_debug_png_deflate_host;
                               7: + uva_png_decode_bgr, uva_debug_zlib_decompress;
                               8: + uva_net_debug_generic_plan;
                               9: + uva_debug_generic_segments (generic graphs: the fused residual-dense-block kernels);
                               10: + uva_debug_generic_segments_planes (a frame's reference tiles through those kernels in one launch);
                               11: + uva_debug_generic_batches;
                               12: + uva_debug_trunkw_schedule (trunkw_kernel: fused trunk pairs as Winograd F(2,3));
                               13: + uva_denoise_u8_device, uva_denoise_synchronize;
                               14: + uva_net_device, uva_debug_sub5_rows (sub5_kernel: the 1x net as two launches of five layers);
                               15: + uva_net_process_u8_device_batch (several frames of one geometry per call; the 1x net takes up to
                                   eight per launch), uva_debug_sub10_rows_batch;
                               15 + pixel formats: + uva_pix_frame_bytes, uva_net_submit_pix, uva_pix_convert, uva_pix_convert_device
                                   (additive: every entry point of 15 is unchanged)
                               15 + 16-bit route: + UVA_PIX_YUV420P10LE, UVA_PIX_BGR48LE, uva_net_process_u16_device,
                                   uva_net_process_u16, uva_net_submit_pix16, uva_pix_convert16 (additive as well)
                               15 + chroma siting: + UVA_CHROMA_BILINEAR, UVA_CHROMA_CENTER, UVA_CHROMA_TOPLEFT in the colour word of
                                   every pixel-format entry (additive: colour words 0-3 mean what they meant)
                               15 + resampler: + uva_resize_taps, uva_resize, uva_resize_device, uva_net_submit_pix_sized, UVA_RESIZE_*
                                   (additive: every earlier entry keeps its signature and its bytes)
                               15 + repeated frames: + uva_frame_diff, uva_frame_diff_device, uva_net_set_skip_repeats,
                                   uva_net_reset_reference, uva_net_skip_stats (additive: off unless asked for)
                               15 + 16 bits through the 1x net: + uva_net_enable_u16_1x, kind 3 of uva_net_kernel_stats (additive: off
                                   unless asked for)
                               15 + launch census: + uva_net_debug_generic_launches (additive: a host-side test hook)
                               15 + 16-bit PNGs: + uva_png_workspace_bytes16, uva_png_assemble16, uva_png_deflate_u16,
                                   uva_debug_png_deflate_host16, uva_png_decode_bgr16, uva_net_submit_u16_png (additive: every 8-bit PNG
                                   entry keeps its signature and its bytes)
                               15 + 16-bit denoise: + uva_denoise_u16, uva_denoise_u16_device, uva_debug_denoise16_stage (additive: the
                                   8-bit stage keeps its kernels and its bytes)
                               15 + deinterlacing: + uva_deint_check, uva_deint_frames, uva_deint_frames_device, uva_debug_deint_frames,
                                   uva_debug_deint_host, uva_deint_create, uva_deint_push, uva_deint_reset, uva_deint_destroy,
                                   UVA_DEINT_* (additive: nothing runs unless asked for)
                               15 + inverse telecine: + uva_ivtc_check, uva_ivtc_metrics, uva_ivtc_metrics_device, uva_debug_ivtc_metrics,
                                   uva_debug_ivtc_host, uva_debug_ivtc_decimate, uva_ivtc_create, uva_ivtc_push, uva_ivtc_reset,
                                   uva_ivtc_stats, uva_ivtc_destroy, UVA_IVTC_* (additive: nothing runs unless asked for)
                               15 + live resources: + uva_debug_live_resources (additive: a test hook) */

typedef struct uva_net uva_net;

/* ---- device enumeration ------------------------------------------------------------ */

/* ncnn.get_gpu_count()            test_gpus.py:47 */
int uva_get_gpu_count(void);
/* ncnn.get_default_gpu_index()    test_gpus.py:53 */
int uva_get_default_gpu_index(void);
/* ncnn.get_gpu_info(i).type() / .device_name()   test_gpus.py:59-66
 * *type: 0 discrete, 1 integrated, 2 virtual, 3 cpu (ncnn's enumeration). */
int uva_get_gpu_info(int index, int* type, char* name, size_t name_len);
/* PCI address "dddd:bb:dd.f" of HIP device `index` (ncnn's GpuInfo has no counterpart; the worker layer
 * uses it to find the GPU's NUMA node in sysfs and to place a worker's feeder threads and page-locked
 * buffers next to the GPU it was given by its position in the -g list, upscale/upscale_processing.py:59). */
int uva_get_gpu_pci_bus_id(int index, char* out, size_t out_len);
/* ncnn.destroy_gpu_instance()     upscale/upscale_processing.py:292, :458
 * Frees every cached device allocation of every live net (nets stay loadable). */
void uva_destroy_gpu_instance(void);
/* Test hook: the HIP resources the library holds at this moment -- counts[0] device buffers, [1] page-locked host buffers,
 * [2] streams, [3] events.  Memory from uva_host_alloc belongs to the caller and is not counted.  All four are zero before
 * the first call that uses a GPU, and again once every uva_deint, every uva_ivtc and every net is destroyed and uva_destroy_gpu_instance
 * has run. */
void uva_debug_live_resources(long long counts[4]);

/* ---- net life cycle ---------------------------------------------------------------- */

/* ncnn.Net()                      upscale/upscale_processing.py:65 */
uva_net* uva_net_create(void);
/* net.opt.use_vulkan_compute = True; net.set_vulkan_device(gpus[gpu])   :67-68
 * device = HIP ordinal.  A negative index is rejected (no CPU path). */
int uva_net_set_device(uva_net* net, int device);
/* The HIP ordinal the net is bound to: what set_vulkan_device was given, 0 (ncnn's default GPU index,
 * test_gpus.py:53) if it never was.  The shim asks the library instead of remembering (uva_denoise_u8_device takes
 * the ordinal and refuses a net that sits elsewhere). */
int uva_net_device(const uva_net* net);
/* net.load_param(path)            :70   parses the ncnn text graph.  The SRVGGNetCompact
 * pattern (conv3x3+PReLU stack, conv3x3, PixelShuffle r, Interp nearest r, BinaryOp add) takes
 * the fused kernels; any other graph made of Input / Split / Convolution 3x3 or 1x1 (+ fused
 * LeakyReLU) / Concat / BinaryOp add / Eltwise sum / Interp nearest / PReLU / PixelShuffle --
 * 4x_Valar_v1, `-m r`, :913-916 -- takes the generic executor (ABI 4); a layer type outside that
 * list is an error naming it. */
int uva_net_load_param(uva_net* net, const char* param_path);
/* net.load_model(path)            :71   reads the .bin stream; every byte must be
 * consumed.  Weights are repacked for the MFMA kernels and uploaded on first use. */
int uva_net_load_model(uva_net* net, const char* bin_path);
/* ncnn::Net::~Net */
void uva_net_destroy(uva_net* net);

/* graph facts after load_param */
int uva_net_scale(const uva_net* net);        /* 1, 2 or 4 */
int uva_net_num_features(const uva_net* net); /* 64 or 24 */
int uva_net_num_convs(const uva_net* net);    /* 18 or 10 */

/* ---- inference --------------------------------------------------------------------- */

/* ex = net.create_extractor(); ex.input("input", mat_in); ret, mat_out = ex.extract("output");
 * np.array(mat_out)               upscale/upscale_processing.py:278-281, :450-453
 * in_chw : host f32 planar [3][h][w] (what Mat.from_pixels + substract_mean_normalize made)
 * out_chw: host f32 planar [3][h*s][w*s] (what np.array(mat_out) returns) */
int uva_net_extract_f32(uva_net* net, const float* in_chw, int h, int w, float* out_chw);

/* Fused frame call: from_pixels(PIXEL_BGR) + substract_mean_normalize + extract +
 * transpose*255 + cv2 convertTo(CV_8U), all on the device, i.e. the arithmetic of
 *   apply_model   upscale/upscale_processing.py:263-288   (tile_size <= 0: whole frame)
 *   upscale_image + process_tile   :395-519               (tile_size = 960, border = 10)
 * in : u8 HWC BGR [h][w][3], rows in_stride bytes apart
 * out: u8 HWC BGR [h*s][w*s][3], rows out_stride bytes apart
 * Host pointers; H2D/D2H staged through pinned buffers on the net's stream. */
int uva_net_process_u8(uva_net* net, const uint8_t* in, int h, int w, size_t in_stride,
                       uint8_t* out, size_t out_stride, int tile_size, int border);

/* Pipelined form of uva_net_process_u8 for callers that stream frames (SURVEY.md 8d "host-to-host
 * with stream overlap"): submit returns at once with a ticket >= 0 (-1 on error); the frame's H2D
 * copy, kernels and D2H copy run on three streams, so consecutive frames overlap.  At most 3 frames
 * may be in flight; tickets are collected in any order.  `in` must stay valid until submit returns
 * when it is pageable (it is staged) and until collect returns when it is pinned (uva_host_alloc,
 * hipHostMalloc, hipHostRegister: copied from directly); `out` must stay valid until collect
 * returns, which is when it holds the result.  uva_net_process_u8 == submit + collect. */
long long uva_net_submit_u8(uva_net* net, const uint8_t* in, int h, int w, size_t in_stride,
                            uint8_t* out, size_t out_stride, int tile_size, int border);
int uva_net_collect_u8(uva_net* net, long long ticket);
/* Page-locked host memory for frames handed to the two calls above (no staging copy). */
void* uva_host_alloc(size_t bytes);
void uva_host_free(void* p);

/* ---- raw-video pixel formats (csrc/uva_pixfmt.hip; the arithmetic: DESIGN.md section 7.3) ------------------- */

/* ffmpeg's rawvideo layouts, dense planes without row padding, chroma cw = ceil(w/2) x ch = ceil(h/2):
 *   UVA_PIX_BGR24    u8 [h][w][3] (what every _u8 call above takes)                 3wh bytes
 *   UVA_PIX_YUV420P  Y u8 [h][w], then U [ch][cw], then V [ch][cw]                  wh + 2 cw ch
 *   UVA_PIX_NV12     Y u8 [h][w], then [ch][cw][2] interleaved U, V                 wh + 2 cw ch
 *   UVA_PIX_P010LE   nv12's layout in little-endian 16-bit words, value << 6        2 (wh + 2 cw ch)
 *   UVA_PIX_YUV420P10LE  yuv420p's layout in little-endian 16-bit words, the value in the low 10 bits   2 (wh + 2 cw ch)
 *   UVA_PIX_BGR48LE  u16 [h][w][3], unorm16 (what the _u16 calls take; the 16-bit entries only)  6wh
 *   UVA_PIX_YUV422P  Y u8 [h][w], then U [h][cw], then V [h][cw]: 4:2:2, one chroma row per luma row   wh + 2 cw h
 *   UVA_PIX_YUV422P10LE  yuv422p's layout in little-endian 16-bit words, the value in the low 10 bits   2 (wh + 2 cw h)
 * The two 4:2:2 formats resample chroma along the row alone: the pair's average / replication, or with
 * UVA_CHROMA_BILINEAR the horizontal half of the siting's filters (left and topleft then give the same bytes).
 * colour = UVA_CSP_BT601 or UVA_CSP_BT709, | UVA_RANGE_FULL for full ("pc") range instead of limited ("tv": Y 16-235,
 * C 16-240, x4 at 10 bits).  BGR -> Y'CbCr: fixed-point textbook formulas, chroma of a 2x2 block from the block's sums;
 * Y'CbCr -> BGR: chroma replicated over its 2x2 block.  The reference's frames are untagged rgb24 PNGs, which ffmpeg merges
 * as BT.601 limited range (upscale/upscale_processing.py:604-640): colour 0.
 * | UVA_CHROMA_BILINEAR: both directions interpolate chroma for where its samples sit instead --
 * Y'CbCr -> BGR bilinear, BGR -> Y'CbCr the matching [1 2 1] / [1 1] filters, taps beyond the plane's edge replicated.  The
 * siting is ffmpeg's chroma_sample_location: left (neither siting bit: H.264 / HEVC video), | UVA_CHROMA_CENTER (JPEG,
 * MPEG-1) or | UVA_CHROMA_TOPLEFT (UHD BT.2020 material).  A siting bit without UVA_CHROMA_BILINEAR, both siting bits, or any
 * other bit is refused by every entry that takes a colour word, with uva_last_error set. */
#define UVA_PIX_BGR24 0
#define UVA_PIX_YUV420P 1
#define UVA_PIX_NV12 2
#define UVA_PIX_P010LE 3
#define UVA_PIX_YUV420P10LE 5   /* (4 is not assigned) */
#define UVA_PIX_BGR48LE 6
#define UVA_PIX_YUV422P 7
#define UVA_PIX_YUV422P10LE 8
#define UVA_CSP_BT601 0
#define UVA_CSP_BT709 1
#define UVA_RANGE_FULL 2
#define UVA_CHROMA_BILINEAR 4
#define UVA_CHROMA_CENTER 8
#define UVA_CHROMA_TOPLEFT 16
/* Bytes of one dense h x w frame of `fmt`; 0 for an unknown format or a size <= 0. */
size_t uva_pix_frame_bytes(int fmt, int h, int w);
/* uva_net_submit_u8 with a pixel format on either end, collected by uva_net_collect_u8: `in` holds one dense frame of
 * in_fmt (h x w), `out` receives one dense frame of out_fmt (h*s x w*s).  The packed frame is copied to the device, converted
 * to u8 BGR in front of the net and the net's u8 result converted to out_fmt behind it, both on the net's stream; the packed
 * result is copied back.  Slots, streams, the 3 frames in flight and the pinned / pageable rules are uva_net_submit_u8's.
 * BGR24 on both ends gives uva_net_submit_u8's bytes. */
long long uva_net_submit_pix(uva_net* net, const void* in, int in_fmt, int h, int w, void* out, int out_fmt, int colour,
                             int tile_size, int border);
/* Host to host on HIP device `device`, synchronous: one dense h x w frame of in_fmt -> out_fmt (through u8 BGR when neither
 * is BGR24; a copy when both are equal).  For tests, a lane whose first stage is `-m n=K` (the denoise stage takes host BGR)
 * and `-s 1` without a net. */
int uva_pix_convert(int device, const void* in, int in_fmt, void* out, int out_fmt, int h, int w, int colour);
/* The same with d_in / d_out resident in `device`'s HBM, asynchronous on the conversion's own stream; `after` / `before`
 * (may be null) as in uva_denoise_u8_device.  The frame is done once uva_net_synchronize(before) or a later uva_pix_convert
 * on the same device (same stream) has returned. */
int uva_pix_convert_device(int device, const void* d_in, int in_fmt, void* d_out, int out_fmt, int h, int w, int colour,
                           uva_net* after, uva_net* before);
/* (uva_pix_convert and uva_net_submit_pix refuse UVA_PIX_BGR48LE: it is the 16-bit route's.) */

/* ---- the 16-bit route ---------------------------------------------------------------------
 * The 2x and 4x Compact nets on u16 BGR samples (unorm16, v / 65535): head operand fp16(v / 257) times 1/255, tail output
 * clamp(rint(y * 65535), 0, 65535).  Y'CbCr frames reach the net without an 8-bit hop (10 bits in, 10 bits out); bgr24
 * frames go in as v * 257 and come out as rint(v / 257).  Every 16-bit entry refuses the 1x net (unless uva_net_enable_u16_1x
 * is on, below), generic graphs (x_Valar_v1) and frames whose byte offsets pass 32 bits, with uva_last_error set. */
/* uva_net_process_u8_device's analogue: d_in u16 [h][w][3], d_out u16 [h*s][w*s][3], strides in bytes (even). */
int uva_net_process_u16_device(uva_net* net, const void* d_in, int h, int w, size_t in_stride, void* d_out, size_t out_stride,
                               int tile_size, int border);
/* Host to host, synchronous (tests, Python); strides and frame addresses even, as above. */
int uva_net_process_u16(uva_net* net, const uint16_t* in, int h, int w, size_t in_stride, uint16_t* out, size_t out_stride,
                        int tile_size, int border);
/* uva_net_submit_pix's arguments and rules (collected by uva_net_collect_u8), converting to and from u16 BGR instead of u8:
 * BGR48LE on both ends is uva_net_process_u16's frame. */
long long uva_net_submit_pix16(uva_net* net, const void* in, int in_fmt, int h, int w, void* out, int out_fmt, int colour,
                               int tile_size, int border);
/* 16 bits through the 1x net.
 * 1: uva_net_process_u16, uva_net_process_u16_device and uva_net_submit_pix16 (uva_net_submit_pix_sized with bits = 16) take this
 * net if it is the 1x SubCompact net (24 features, 10 convolutions, scale 1, not a generic graph); 0 (the default): they refuse it
 * as before.  Returns non-zero with uva_last_error set on any other net.  Loading another graph into the net switches it off.
 * The default is a refusal only because a pinned test holds the 16-bit entries to their earlier message on this net; nothing in
 * the arithmetic makes the route second-rate: same head operand, same tail rounding as the 2x / 4x nets, in one launch of
 * sub10_kernel16.
 * The route takes whole frames only, as apply_model runs this net.  Refused with uva_last_error set, never run at 8 bits instead:
 * tile_size > 0; frames whose row lists do not fit the fused kernel (beyond roughly 2160p); input and output frames that overlap
 * (the kernel reads the input again for the residual while it stores).  UVA_SUB10=0 and UVA_SUB5=1 select among the u8 kernels
 * and do not apply to this route. */
int uva_net_enable_u16_1x(uva_net* net, int on);
/* uva_pix_convert through u16 BGR (any two formats, UVA_PIX_BGR48LE included). */
int uva_pix_convert16(int device, const void* in, int in_fmt, void* out, int out_fmt, int h, int w, int colour);

/* ---- the resampler (csrc/uva_resize.hip; the arithmetic: DESIGN.md section 7.6) ------------------------------------
 * BGR frames (u8 [h][w][3] with bits = 8, u16 with bits = 16; channels independent, code values as they are) to any oh x ow with
 * 1/4 <= oh / h <= 4 and 1/4 <= ow / w <= 4, by a separable polyphase filter with integer taps (every row of a table sums to
 * 2^14; shrinking widens the filter).  Pixel centres: output sample d sits at (d + 0.5) n_in / n_out - 0.5; a tap beyond the
 * plane reads the nearest sample inside.  Sizes below 1, a ratio outside [1/4, 4], an unknown filter, bits other than 8 / 16 and
 * odd strides or addresses at 16 bits are refused with uva_last_error set. */
#define UVA_RESIZE_LANCZOS 0    /* sinc(x) sinc(x / 3), |x| < 3 */
#define UVA_RESIZE_BICUBIC 1    /* Keys, a = -0.5, |x| < 2 */
#define UVA_RESIZE_BILINEAR 2   /* triangle, |x| < 1 */
/* Host only, no device needed: the table of one axis as the kernel uses it.  *ntaps receives T = 2 ceil(a max(1, n_in / n_out))
 * (also when the call then fails for want of room: first needs n_out ints, taps n_out * T <= cap int16s); output sample d is
 * sum_k taps[d * T + k] * in[clamp(first[d] + k, 0, n_in - 1)] / 2^14. */
int uva_resize_taps(int n_in, int n_out, int filter, int32_t* first, int16_t* taps, size_t cap, int* ntaps);
/* Frames resident in `device`'s HBM, asynchronous on the conversions' stream (uva_pix_convert_device's); strides in bytes;
 * `after` / `before` (may be null) as in uva_pix_convert_device. */
int uva_resize_device(int device, const void* d_in, int h, int w, size_t in_stride, void* d_out, int oh, int ow, size_t out_stride,
                      int filter, int bits, uva_net* after, uva_net* before);
/* Host to host, synchronous (tests, Python, `-s 1` without a net).  Bytes between the rows of a padded `out` are left alone. */
int uva_resize(int device, const void* in, int h, int w, size_t in_stride, void* out, int oh, int ow, size_t out_stride, int filter,
               int bits);
/* uva_net_submit_pix (bits = 8) / uva_net_submit_pix16 (bits = 16) with the resampler between the net's tail and the output
 * conversion, on the net's stream: `out` receives one dense oh x ow frame of out_fmt; chroma is subsampled and sited at the
 * output size.  Collected by uva_net_collect_u8; slots, streams, the 3 frames in flight and the pinned / pageable rules are
 * uva_net_submit_u8's.  oh == h*s and ow == w*s: the resampler is skipped, the bytes are uva_net_submit_pix's. */
long long uva_net_submit_pix_sized(uva_net* net, const void* in, int in_fmt, int h, int w, void* out, int out_fmt, int colour,
                                   int tile_size, int border, int oh, int ow, int filter, int bits);

/* ---- repeated frames (csrc/uva_repeat.hip) ---------------------------------------------------
 * Two dense h x w frames of one pixel format compared sample by sample in code values, as the input conversion reads them: bytes
 * for the 8-bit formats, word >> 6 for p010le, word & 1023 for yuv420p10le / yuv422p10le (bits the converter ignores make no
 * difference), whole words for bgr48le.  stats[0] = over, the samples with |a - b| > threshold; stats[1] = max_abs, the largest
 * |a - b|; stats[2] = sad, the sum of |a - b|.  Integer sums: exact and the same on every call.  Null pointers, an unknown
 * format, a size below 1 and a threshold outside 0 ... 65535 are refused with uva_last_error set. */
/* Host to host on HIP device `device`, synchronous. */
int uva_frame_diff(int device, const void* a, const void* b, int fmt, int h, int w, int threshold, unsigned long long* stats);
/* The same with d_a / d_b resident in `device`'s HBM at 16-byte aligned addresses and complete (the call orders itself behind no
 * stream of the caller's); stats is host memory.  Synchronous as well. */
int uva_frame_diff_device(int device, const void* d_a, const void* d_b, int fmt, int h, int w, int threshold,
                          unsigned long long* stats);
/* Repeated frames on the pipelined route.  threshold -1: off, the default; 0 ... 65535: on -- every uva_net_submit_* entry except
 * uva_net_submit_u8_png then compares the frame it is given with the net's KEPT frame, the last frame the net actually ran on
 * (never merely the predecessor: with threshold 1 the frames x, x + 1, x + 2 run, skip, run).  A frame of which no sample differs
 * from the kept frame's by more than threshold, submitted with the same h, w, in_fmt, out_fmt, colour word, bit depth, tile_size,
 * border, output size and filter, is not computed: the kept frame's result bytes are downloaded into its `out` from a copy in
 * HBM (the kept frame's own `out` plays no part, callers reuse their rings).  It still takes a slot and a ticket and is collected
 * like any other.  Any other frame runs as always and becomes the kept frame.  With threshold 0 the stream of results is byte for
 * byte what it is with skipping off.  Cost when on: the host waits in submit for the comparison, and the net holds one input and
 * one result frame more in HBM.  The synchronous uva_net_process_* calls and the PNG entry ignore the setting.  Setting it (to
 * any value) forgets the kept frame and zeroes the counters; another value is refused.  Host only: works with no GPU present. */
int uva_net_set_skip_repeats(uva_net* net, int threshold);
/* Forgets the kept frame: the next frame runs whatever it holds (a segment's start, a seek). */
int uva_net_reset_reference(uva_net* net);
/* Frames that went through the comparison's route since uva_net_set_skip_repeats, and how many of them were skipped. */
int uva_net_skip_stats(uva_net* net, long long* submitted, long long* skipped);

/* ---- crop detection and cropped input frames (csrc/uva_crop.hip, csrc/uva_crop_host.cpp) ------
 * The reference looks for black bars first: get_crop_detect (upscale/upscale_processing.py:137-181) runs ffmpeg's cropdetect at
 * 100 places of the film and extract_frames (:227-230) applies the most frequent crop=W:H:X:Y.  These entries are that filter's
 * rule restated (its definition for this project: tests/cropdetect_ref.py; parity with ffmpeg itself is unpinned) and the means
 * to apply the result in front of a net.  Samples are code values as the input conversion reads them (bytes; word >> 6 for
 * p010le; word & 1023 for yuv420p10le / yuv422p10le; whole words for bgr48le), of depth 8, 10 or 16.  A LINE is a row or a column
 * of the luma plane, or of all three components of a packed BGR frame (n = w or h samples; 3w or 3h for bgr24 / bgr48le). */
/* The exact sums of every line of a dense h x w frame of fmt (upscale/upscale_processing.py:137-181: the detector's per-frame
 * pass), computed on HIP device `device`: rows[h], cols[w].  Host to host, synchronous.  Null pointers, an unknown format and a
 * size below 1 are refused with uva_last_error set. */
int uva_crop_sums(int device, const void* frame, int fmt, int h, int w, unsigned long long* rows, unsigned long long* cols);
/* The same (upscale/upscale_processing.py:137-181) with the frame resident in `device`'s HBM at a 16-byte aligned address and
 * complete; rows / cols are host memory.  Synchronous as well. */
int uva_crop_sums_device(int device, const void* d_frame, int fmt, int h, int w, unsigned long long* rows, unsigned long long* cols);
/* Test hook: uva_crop_sums (upscale/upscale_processing.py:137-181) on a grid of at most max_groups workgroups (0: the kernel's own
 * bound), so that a small frame exercises the kernel's grid-stride walk. */
int uva_debug_crop_sums(int device, const void* frame, int fmt, int h, int w, unsigned long long* rows, unsigned long long* cols,
                        int max_groups);
/* Host only, no GPU needed: cropdetect's brightness test (upscale/upscale_processing.py:137-181) on a frame's line sums.  A line
 * with sum S over n samples is bright iff floor(S / n) > limit << (depth - 8); limit is on the 8-bit scale, 0 ... 255 (ffmpeg's
 * default: 24), anything else is refused.  bounds = {first bright row, last bright row, first bright column, last bright
 * column}, -1 where there is none. */
int uva_crop_bounds(const unsigned long long* rows, const unsigned long long* cols, int fmt, int h, int w, int limit, int bounds[4]);
/* Host only: cropdetect's rectangle (upscale/upscale_processing.py:137-181, the crop=W:H:X:Y it prints) from a running state
 * {x1, y1, x2, y2} -- initially {w - 1, h - 1, 0, 0}; every frame lowers x1 / y1 to its first bright column / row and raises
 * x2 / y2 to its last -- and `round` (<= 1 means 16, an odd value is doubled): x = (x1 + 1) & ~1, cw = x2 - x + 1, k = cw % round,
 * cw -= k, x += (k / 2 + 1) & ~1, and the same for y and ch.  rect = {W, H, X, Y}, all even and inside the frame.  Returns
 * non-zero (uva_last_error set) when there is no rectangle: cw or ch not positive at some point. */
int uva_crop_rect(const int state[4], int round, int rect[4]);
/* Host only: is the window h x w at (x, y) of a src_h x src_w frame of fmt one that uva_pix_window and the submit entries take
 * (upscale/upscale_processing.py:227-230 applies any crop ffmpeg printed; here the formats' chroma grids decide)?  Refused,
 * never rounded: a window that leaves the frame, x or w odd for a Y'CbCr format, y or h odd for a 4:2:0 format.  bgr24 / bgr48le
 * take any window. */
int uva_pix_window_check(int fmt, int src_h, int src_w, int x, int y, int h, int w);
/* The crop itself (extract_frames' `-vf crop=...`, upscale/upscale_processing.py:227-230): out <- the dense h x w frame of fmt cut
 * from the dense src_h x src_w frame `in` at (x, y), every plane at its own resolution, on HIP device `device`.  Host to host,
 * synchronous.  For lanes whose first stage is no net (`-m n=K`, `-s 1` without a net). */
int uva_pix_window(int device, const void* in, int fmt, int src_h, int src_w, int x, int y, int h, int w, void* out);
/* The same (upscale/upscale_processing.py:227-230) between frames in `device`'s HBM, both complete; d_out at a 16-byte aligned
 * address.  Synchronous. */
int uva_pix_window_device(int device, const void* d_in, int fmt, int src_h, int src_w, int x, int y, int h, int w, void* d_out);
/* The crop in front of a net (upscale/upscale_processing.py:227-230: no net ever sees a black bar).  While a window is set, `in` of
 * every uva_net_submit_pix, uva_net_submit_pix16 and uva_net_submit_pix_sized call is a dense src_h x src_w frame of in_fmt and
 * the call's own h x w is the window at (x, y) of it: only the window's rows are uploaded -- one copy per plane, and for a window
 * narrower than the frame a small kernel on the upload stream that compacts the columns -- and everything behind the upload, `out`
 * included, is what it is for a dense h x w frame.  A window uva_pix_window_check refuses makes the submit call fail.  All zeros
 * switch it off (the default).  Setting it forgets the kept frame of uva_net_set_skip_repeats and zeroes its counters: the
 * comparison is between uploaded windows.  Host only: works with no GPU present. */
int uva_net_set_input_window(uva_net* net, int src_h, int src_w, int x, int y);

/* ---- deinterlacing (csrc/uva_deint.hip, csrc/uva_deint_host.cpp) ---------------------------------
 * DVD, broadcast and tape material is interlaced: the rows of a frame alternate between two instants, and every moving edge is a
 * comb that a net would sharpen.  These entries are yadif's spatio-temporal rule restated (its definition for this project:
 * tests/yadif_ref.py; parity with ffmpeg's yadif filter is unpinned) on frames of any UVA_PIX_* format, exact in integers, per
 * component plane: the interleaved chroma of nv12 / p010le is two planes, a packed BGR frame three; the chroma rows of a 4:2:0
 * frame alternate fields as luma rows do.  Samples are code values as the input conversion reads them (bytes; word >> 6 for
 * p010le; word & 1023 for yuv420p10le / yuv422p10le; whole words for bgr48le).
 * A frame `cur` between `prev` and `next` has two outputs.  A keeps the rows of cur's first field byte for byte (bits the
 * converter ignores too) and interpolates the others between prev and cur; B keeps the second field's rows and interpolates the
 * others between cur and next.  Interpolated samples are clean code values in the format's placement.  The first field is the
 * even rows (top field first) unless UVA_DEINT_BFF is set.  Without UVA_DEINT_FIELD only A exists (one frame out per frame in);
 * with it A and B (two out per frame in, twice the frame rate). */
#define UVA_DEINT_FIELD 1
#define UVA_DEINT_BFF 2
typedef struct uva_deint uva_deint;
/* Host only, no GPU needed: are h x w frames of fmt with these flags ones the entries below take?  Refused, never rounded, with
 * uva_last_error set: an unknown format, unknown flag bits, a size below 1 or above 2^28 pixels, h < 4 (a 4:2:0 chroma plane
 * then has fewer than two rows).  Any w >= 1 is taken. */
int uva_deint_check(int fmt, int h, int w, int flags);
/* One frame, stateless: out_a / out_b <- the outputs A / B of `cur` on HIP device `device`.  Host to host, synchronous.  prev /
 * next NULL mean cur (the first / last frame of a stream).  Either output may be NULL, not both; out_b without UVA_DEINT_FIELD is
 * refused.  Everything is refused before a GPU is looked for. */
int uva_deint_frames(int device, const void* prev, const void* cur, const void* next, int fmt, int h, int w, int flags, void* out_a,
                     void* out_b);
/* The same between frames in `device`'s HBM, all complete and at 16-byte aligned addresses.  Synchronous. */
int uva_deint_frames_device(int device, const void* d_prev, const void* d_cur, const void* d_next, int fmt, int h, int w, int flags,
                            void* d_out_a, void* d_out_b);
/* Test hook: uva_deint_frames on a grid of at most max_groups workgroups (0: the kernel's own bound), so that a small frame
 * exercises the kernel's grid-stride walk. */
int uva_debug_deint_frames(int device, const void* prev, const void* cur, const void* next, int fmt, int h, int w, int flags, void* out_a,
                           void* out_b, int max_groups);
/* Test hook, host only, no GPU needed: uva_deint_frames by the scalar restatement of the rule in csrc/uva_deint_host.cpp. */
int uva_debug_deint_host(const void* prev, const void* cur, const void* next, int fmt, int h, int w, int flags, void* out_a, void* out_b);
/* A stream, stateful, so that every frame is uploaded once: the handle keeps three frames in `device`'s HBM and a stream of its
 * own.  uva_deint_push uploads `frame` and produces the outputs of the frame pushed BEFORE it (which now has its next): *produced
 * is 0 after the first push, else 1 (A in out_a) or, with UVA_DEINT_FIELD, 2 (A in out_a, B in out_b); it returns when they are
 * in out_a / out_b.  frame NULL flushes: the last frame's outputs with next = cur (0 when nothing was pushed), after which the
 * handle is as after uva_deint_reset, ready for another stream.  out_a is needed always, out_b with UVA_DEINT_FIELD. */
int uva_deint_create(int device, int fmt, int h, int w, int flags, uva_deint** out);
int uva_deint_push(uva_deint* d, const void* frame, void* out_a, void* out_b, int* produced);
int uva_deint_reset(uva_deint* d);
void uva_deint_destroy(uva_deint* d);

/* ---- inverse telecine (csrc/uva_ivtc.hip, csrc/uva_ivtc_host.cpp) ---------------------------------
 * NTSC film and anime DVDs are 24000/1001 film carried as 30000/1001 interlaced video by 2:3 pulldown: of five frames two mix
 * the fields of two film frames and one repeats nothing new.  These entries give the film frames back: field matching, then
 * decimation (the rule's definition for this project: tests/ivtc_ref.py; parity with ffmpeg's fieldmatch / decimate filters is
 * unpinned).  Formats, planes, samples, the first field and NULL neighbours are those of the deinterlacing entries above.
 * For a frame `cur` between `prev` and `next` the candidates c / p / n weave cur's first field (even rows unless UVA_IVTC_BFF)
 * with the other rows of cur / prev / next, in every plane, byte for byte.  On plane 0 of a candidate (luma, or all of a packed
 * BGR frame), for rows 1 ... ph - 2, a sample b between its vertical neighbours a and c is combed when b - a and b - c have the
 * same sign, are non-zero and m = min(|b - a|, |b - c|) > T << (depth - 8); N counts them, M sums m.  stats is
 * (N_c, M_c, N_p, M_p, N_n, M_n), exact.  The match is the candidate of the smallest M (ties: c, p, n); it is combed when
 * N * 10^6 > L * (ph - 2) * (samples of a row), and then replaced by yadif's output A of the same three frames unless
 * UVA_IVTC_KEEP_COMBED.  The frames so made are grouped in fives from the start of the stream; of a full five the one with the
 * smallest sum of absolute differences to the frame before it (the first of a stream: 2^64 - 1) is dropped, ties the earliest,
 * unless UVA_IVTC_KEEP_ALL.  T is on the 8-bit scale, 0 ... 255 (9 is the route's default); L is parts per million, 0 ... 10^6
 * (1000 is the route's default, a guess: no telecined real material was at hand). */
#define UVA_IVTC_BFF 1
#define UVA_IVTC_KEEP_COMBED 2
#define UVA_IVTC_KEEP_ALL 4
typedef struct uva_ivtc uva_ivtc;
/* Host only, no GPU needed.  Refused, never rounded, with uva_last_error set: what uva_deint_check refuses, T or L out of range,
 * unknown flag bits.  Any w >= 1 is taken. */
int uva_ivtc_check(int fmt, int h, int w, int flags, int T, int L);
/* One frame, stateless: stats[6] <- the six sums on HIP device `device`.  Host frames, synchronous.  prev / next NULL mean cur.
 * Everything is refused before a GPU is looked for. */
int uva_ivtc_metrics(int device, const void* prev, const void* cur, const void* next, int fmt, int h, int w, int flags, int T,
                     unsigned long long* stats);
/* The same for frames in `device`'s HBM, complete and at 16-byte aligned addresses (stats is host memory).  Synchronous. */
int uva_ivtc_metrics_device(int device, const void* d_prev, const void* d_cur, const void* d_next, int fmt, int h, int w, int flags, int T,
                            unsigned long long* stats);
/* Test hook: uva_ivtc_metrics on a grid of at most max_groups workgroups (0: the kernel's own bound). */
int uva_debug_ivtc_metrics(int device, const void* prev, const void* cur, const void* next, int fmt, int h, int w, int flags, int T,
                           unsigned long long* stats, int max_groups);
/* Test hook, host only, no GPU needed: the scalar restatement in csrc/uva_ivtc_host.cpp.  stats[6] as above; woven (may be NULL)
 * <- the three candidates c, p, n, a frame each; chosen (may be NULL) <- the frame the rule makes of cur; decision (may be NULL)
 * <- {match 0 / 1 / 2, combed 0 / 1}. */
int uva_debug_ivtc_host(const void* prev, const void* cur, const void* next, int fmt, int h, int w, int flags, int T, int L,
                        unsigned long long* stats, void* woven, void* chosen, int* decision);
/* Test hook, host only: the decimator driven as uva_ivtc_push drives it over n frames with these diffs, then flushed:
 * delivered[*n_delivered] (room for n) <- the numbers of the frames that leave, in order.  flags: UVA_IVTC_KEEP_ALL counts. */
int uva_debug_ivtc_decimate(const unsigned long long* diffs, int n, int flags, long long* delivered, int* n_delivered);
/* A stream, stateful, so that every frame is uploaded once: the handle keeps three source frames, a ring of the frames it has
 * made, its sums and a stream of its own in `device`'s HBM.  uva_ivtc_push uploads `frame` and hands out at most one frame of the
 * result: *produced is 0 or 1, and with 1 the frame is in `out` when the call returns.  frame NULL is a flush step: call it until
 * it produces 0, after which the handle is as after uva_ivtc_reset, ready for another stream; a frame pushed in between is
 * refused.  Which call delivers which frame is the implementation's business (a five is decided when it is complete); the
 * sequence of delivered frames is the rule's: n frames in, n - n / 5 out. */
int uva_ivtc_create(int device, int fmt, int h, int w, int flags, int T, int L, uva_ivtc** out);
int uva_ivtc_push(uva_ivtc* d, const void* frame, void* out, int* produced);
int uva_ivtc_reset(uva_ivtc* d);
/* stats[7] <- since creation: frames in, frames out, matches c, p, n, frames found combed, frames dropped.  Host only. */
int uva_ivtc_stats(uva_ivtc* d, unsigned long long* stats);
void uva_ivtc_destroy(uva_ivtc* d);

/* ---- the imwrite side on the device (csrc/uva_png.hip.h) -------------------------------- */

/* cv2.imwrite(frame.png) of the result frame (upscale_processing.py:288, :519), with the deflate work done on the GPU:
 * like uva_net_submit_u8, but the result frame stays in HBM, a kernel behind the net compresses it (Sub filter, fixed
 * Huffman tables, one deflate block per group of rows) and the copy engine brings the compressed blocks into `png_ws`:
 * page-locked memory (uva_host_alloc) of uva_png_workspace_bytes(h*scale, w*scale) bytes that must stay untouched until
 * uva_net_collect_u8(ticket) has returned (collect completes the workspace: a frame that compressed worse than the
 * one before it has its last bytes fetched there).  uva_png_assemble() -- host only, any thread -- then turns the workspace into
 * the bytes of the PNG file: *len receives the size; out may be NULL to ask for it (the call then fails after setting
 * *len).  h, w there are the RESULT frame's.  Any PNG reader decodes the file to exactly the frame
 * uva_net_submit_u8 would have returned.  uva_png_workspace_bytes() returns 0 for frames the encoder does not take
 * (wider than 16 383 pixels). */
long long uva_net_submit_u8_png(uva_net* net, const uint8_t* in, int h, int w, size_t in_stride, void* png_ws,
                                size_t png_ws_bytes, int tile_size, int border);
size_t uva_png_workspace_bytes(int h, int w);
int uva_png_assemble(const void* png_ws, int h, int w, uint8_t* out, size_t cap, size_t* len);
/* The same encoder for a frame in host memory (synchronous: H2D copy, kernel, wait): imwrite for frames that did not
 * come out of a net of this library, e.g. the denoise pass (upscale_processing.py:336-338). */
int uva_png_deflate_u8(int gpu, const uint8_t* bgr, int h, int w, size_t stride, void* png_ws, size_t png_ws_bytes);
/* cv2.imread(path) (upscale_processing.py:263, :487) for a file image already in memory, host only, any thread: a
 * from-scratch inflate + PNG un-filter straight into cv2's u8 HWC BGR layout, 2-3x a zlib-based reader.  8-bit RGB,
 * RGBA (alpha dropped), grey (replicated), non-interlaced.  out == NULL: only *h, *w are set.  Returns 0, 1 for a
 * corrupt file (chunk CRC, Adler-32 and stream length are all checked; uva_last_error says what), 2 for a PNG of
 * another kind (16-bit, palette, interlaced): use a general reader for those. */
int uva_png_decode_bgr(const uint8_t* file, size_t len, uint8_t* out, size_t cap, int* h, int* w);
/* Test hook: the inflate alone on a zlib-wrapped stream that must expand to exactly out_len bytes. */
int uva_debug_zlib_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t out_len);
/* Test hook (host only): the kernel's arithmetic restated on the host, block for block and bit for bit, into an
 * ordinary buffer of uva_png_workspace_bytes(h, w) bytes. */
int uva_debug_png_deflate_host(const uint8_t* bgr, int h, int w, size_t stride, void* png_ws, size_t png_ws_bytes);

/* ---- the PNG route at 16 bits (csrc/uva_png.hip.h png_deflate_kernel16) -------------------
 * The reference extracts its frames as rgb24 PNGs (upscale/upscale_processing.py:223-232) and merges the result frames with
 * -pix_fmt p010le by default (upscale_video.py:28-30, upscale/upscale_processing.py:632-633): 10-bit video out of 256 levels.
 * With the frames extracted as rgb48be instead, these entries keep 16 bits from file to file: u16 HWC BGR frames (unorm16,
 * little-endian samples, addresses and strides even) and 16-bit RGB PNGs -- colour type 2, depth 16, Sub on every scanline
 * (bpp 6), one deflate block per group of rows with one of eight fixed literal codes. */
/* uva_png_workspace_bytes for the 16-bit encoder (cv2.imwrite of a CV_16U frame, :288, :519): the workspaces of the two
 * encoders differ in size and layout.  0 for frames it does not take (wider than 8 191 pixels). */
size_t uva_png_workspace_bytes16(int h, int w);
/* uva_png_assemble for a workspace the 16-bit encoder filled (cv2.imwrite's framing, :288, :519): IHDR with depth 16, the same
 * checksum combination.  A workspace remembers which encoder filled it: this call refuses an 8-bit one, uva_png_assemble a
 * 16-bit one, each with uva_last_error saying so -- never a file framed with the wrong depth. */
int uva_png_assemble16(const void* png_ws, int h, int w, uint8_t* out, size_t cap, size_t* len);
/* uva_png_deflate_u8 for a u16 BGR frame in host memory (cv2.imwrite(frame.png) of a CV_16U frame, :288, :519); stride in
 * bytes.  png_ws: page-locked, uva_png_workspace_bytes16(h, w) bytes. */
int uva_png_deflate_u16(int gpu, const uint16_t* bgr, int h, int w, size_t stride, void* png_ws, size_t png_ws_bytes);
/* Test hook (host only): png_deflate_kernel16's arithmetic restated on the host, block for block and bit for bit, into an
 * ordinary buffer of uva_png_workspace_bytes16(h, w) bytes (the kernel's reference; what cv2.imwrite's encoder is to the
 * reference, :288). */
int uva_debug_png_deflate_host16(const uint16_t* bgr, int h, int w, size_t stride, void* png_ws, size_t png_ws_bytes);
/* cv2.imread(path, cv2.IMREAD_UNCHANGED) of a 16-bit frame (the reference reads its frames at :263, :487) for a file image in
 * memory, host only, any thread: 16-bit RGB, RGBA (alpha dropped) or grey (replicated), all five filter types, into u16 HWC BGR;
 * cap counts BYTES (h*w*6 are needed).  An 8-bit file of a kind uva_png_decode_bgr takes comes back widened v * 257, the 16-bit
 * route's convention for 8-bit samples (above).  out == NULL: only *h, *w are set.  Returns 0, 1 for a corrupt file (chunk CRC,
 * Adler-32 and stream length are checked; a header that promises more pixels than its data can hold is refused before anything
 * is allocated, on the size query too), 2 for palette, interlaced and 1/2/4-bit files. */
int uva_png_decode_bgr16(const uint8_t* file, size_t len, uint16_t* out, size_t cap, int* h, int* w);
/* uva_net_submit_u8_png on 16-bit samples (the imread -> net -> imwrite hop of :263-288 and :487-519 without its 8-bit files):
 * `in` is a u16 BGR frame (in_stride in bytes), the u16 result stays in HBM, png_deflate_kernel16 follows the net on its stream
 * and the blocks reach `png_ws` (page-locked, uva_png_workspace_bytes16(h*scale, w*scale) bytes) as in the 8-bit call: the same
 * guess of the download's size, the rest fetched by uva_net_collect_u8(ticket); then uva_png_assemble16.  Tiling arguments as in
 * uva_net_submit_u8.  Nets: the 16-bit route's -- the 1x net only after uva_net_enable_u16_1x and with tile_size 0; refused
 * with uva_last_error set otherwise.  Takes no part in uva_net_set_skip_repeats, like the 8-bit PNG entry. */
long long uva_net_submit_u16_png(uva_net* net, const uint16_t* in, int h, int w, size_t in_stride, void* png_ws,
                                 size_t png_ws_bytes, int tile_size, int border);

/* Same, with in/out already resident in this device's HBM (dense rows: in_stride = 3*w,
 * out_stride = 3*w*s unless stated).  Asynchronous on the net's stream; follow with
 * uva_net_synchronize().  This is the call bench.py times. */
int uva_net_process_u8_device(uva_net* net, const void* d_in, int h, int w, size_t in_stride,
                              void* d_out, size_t out_stride, int tile_size, int border);

/* `count` frames of ONE geometry in one call, every d_in[i] / d_out[i] resident in this device's HBM: what a worker that
 * holds several decoded frames (the raw-video route, the frame pool, `-m a` in front of the 2x pass) hands over instead of
 * `count` calls of apply_model (upscale/upscale_processing.py:258-299) -- the reference has no such call, its unit is the frame.
 * The 1x HurrDeblur net runs up to eight of them per kernel launch (the launch's pipeline fill and the strips' warm-up rows
 * are then paid once per launch, not once per frame); every other net, and whatever does not fit, is processed frame by
 * frame.  The result bytes are exactly those of `count` uva_net_process_u8_device calls.  Asynchronous on the net's stream. */
int uva_net_process_u8_device_batch(uva_net* net, const void* const* d_in, void* const* d_out, int count, int h, int w,
                                    size_t in_stride, size_t out_stride, int tile_size, int border);

int uva_net_synchronize(uva_net* net);

/* Device-side ordering between two nets of one process (each net owns a stream): everything
 * `producer` has been asked to do so far completes before anything `net` is asked to do from now
 * on.  Used to chain the 1x HurrDeblur pass into the 2x pass without leaving the GPU (the reference
 * hops through an 8-bit PNG between them, upscale/upscale_processing.py:888-909; a u8 frame in HBM
 * carries exactly the same information). */
int uva_net_wait_for(uva_net* net, uva_net* producer);

/* ---- `-m n=K` film-grain denoise ------------------------------------------------------------ */

/* cv2.fastNlMeansDenoisingColored(cv2.UMat(img), None, K, K, 5, 9)   upscale/upscale_processing.py:350-354
 * (apply_denoise; K = 1..30 from `-m n=K`, :782-789): BGR -> 8-bit Lab (linear light), non-local means on L
 * with h_luma and on (a, b) with h_color (template 5, search 9), Lab -> BGR; on HIP device `device`.
 * in / out: host u8 HWC BGR [h][w][3].  OpenCV's integer weighting scheme and its 8-bit fixed-point Lab conversions
 * (RGB2Lab_b / Lab2RGBinteger: gamma tables, 2^12-scaled matrices, LabCbrtTab_b) are restated from the published 4.x
 * source (csrc/uva_denoise.hip.h; PARITY UNPINNED: no cv2 in this image to check a constant against). */
int uva_denoise_u8(int device, const uint8_t* in, int h, int w, size_t in_stride, uint8_t* out, size_t out_stride,
                   float h_luma, float h_color);
/* The same stage on a frame that is already in HBM (`-m n=K` in front of `-m a` and the 2x / 4x pass without leaving the
 * GPU: the reference's order, upscale/upscale_processing.py:880-886, 888-909, 913-920): d_in / d_out are device pointers, the
 * call returns once the work is queued on the stage's own stream.  `after` (may be null): everything that net has been
 * asked to do so far completes first; `before` (may be null): whatever that net is asked to do from now on waits for this
 * frame -- the two ends of uva_net_wait_for.  uva_denoise_synchronize waits for the stage's stream on `device`. */
int uva_denoise_u8_device(int device, const void* d_in, int h, int w, size_t in_stride, void* d_out, size_t out_stride,
                          float h_luma, float h_color, uva_net* after, uva_net* before);
int uva_denoise_synchronize(int device);
/* Test hook: one stage of the above on dense host arrays.  stage 0: BGR -> Lab [h][w][3]; 1: Lab -> BGR;
 * 2: non-local means on a 1-channel image; 3: on a 2-channel image (strength = h). */
int uva_debug_denoise_stage(int device, int stage, const uint8_t* in, int h, int w, float strength, uint8_t* out);

/* `-m n=K` at --bit-depth 16 (csrc/uva_denoise16.hip.h): the same stage on u16 samples, for frames of
 * more than 8 bits.  in / out: host u16 HWC BGR [h][w][3] (bgr48le), strides in BYTES.  BGR16 -> Lab16 (L * 65535 / 100,
 * (a + 128) * 257, (b + 128) * 257: the 8-bit planes' scales x 257; linear light, the CIE formulas in fixed point), non-local
 * means on L16 with h_luma and on (a16, b16) with h_color (template 5, search 9; squared differences `>> 8` per sample, a weight
 * table sixteen times finer than the 8-bit one holding the same function of the mean squared patch difference, so a strength
 * means what it means at 8 bits; 64-bit accumulators), Lab16 -> BGR16.  Strengths in (0, 64].  Integer arithmetic throughout,
 * bit-exact against its numpy definition (tests/nlm16_ref.py); BGR16 -> Lab16 -> BGR16 alone moves a sample by at most 12 codes
 * of 65535 (the 8-bit stage's Lab hop: up to 5 levels of 255 = 1285 codes). */
int uva_denoise_u16(int device, const uint16_t* in, int h, int w, size_t in_stride, uint16_t* out, size_t out_stride,
                    float h_luma, float h_color);
/* The same on a frame in HBM, asynchronous on the denoise stage's stream (the 8-bit stage's: uva_denoise_synchronize waits for
 * both); `after` / `before` as in uva_denoise_u8_device.  Pointers and strides 2-byte aligned. */
int uva_denoise_u16_device(int device, const void* d_in, int h, int w, size_t in_stride, void* d_out, size_t out_stride,
                           float h_luma, float h_color, uva_net* after, uva_net* before);
/* Test hook: uva_debug_denoise_stage's stages 0 - 3 on dense u16 arrays. */
int uva_debug_denoise16_stage(int device, int stage, const uint16_t* in, int h, int w, float strength, uint16_t* out);

/* ---- introspection used by the parity tests and bench.py ------------------------------ */

/* Activation after convolution #conv_idx (+PReLU) of the last extract/process call with
 * tile_size <= 0, converted to host f32 planar [cout][h][w].  conv_idx in [0, nconv-2]. */
int uva_net_debug_read_activation(uva_net* net, int conv_idx, float* out_chw, int h, int w);

/* Per-kernel-kind timing with HIP events recorded on the net's stream around each launch.
 * kind: 0 head conv, 1 trunk conv (the dominant kernel), 2 tail conv.  Generic graphs (4x_Valar_v1): 1 = rdb4_kernel
 * (a residual dense block's first four convolutions, all planes of the frame), 2 = the block's 192 -> 64 convolution; 0 unused.
 * kind 3: sub10_kernel16, the 1x net's launches on the 16-bit route (uva_net_enable_u16_1x); its u8 launches count under 1 as before.
 * enable != 0 starts (and resets) collection; stats are valid after uva_net_synchronize. */
int uva_net_set_profiling(uva_net* net, int enable);
int uva_net_kernel_stats(uva_net* net, int kind, long long* launches, double* total_ms);

#ifdef UVA_INSTRUMENT   /* instrumented builds only (python -m upscale_video_amd.build --instrument) */
/* Debug: replays one trunk-layer launch on the last call's workspace with in-kernel cycle stamps
 * of workgroup 0 / wave 0: out[8*i + {0,1,2,3,4}] = tile i {start, k-loop done, barrier passed,
 * epilogue done, epilogue staging written} in s_memtime ticks (out holds 8*max_tiles values).
 * *tiles = tiles that workgroup processed.  ablate: 0 real kernel, 1 memory traffic only (no MFMA /
 * LDS reads), 2 compute only (L2-resident input, stores to a sink), 3 the u8 tail kernel instead, 4 memory
 * traffic and LDS fragment reads without MFMAs; bits 8.. = hundreds of timed launches instead of 10 (sustained,
 * power-limited state); *kernel_ms = mean launch time. */
int uva_net_debug_trunk_stamps(uva_net* net, unsigned long long* out, int max_tiles, int* tiles, int ablate,
                               float* kernel_ms);
/* Debug (generic graphs, UVA_RDB_STAMPS=1 in the environment): s_memtime stamps of rdb4_kernel's workgroup 0 in its last
 * launch, out[(step * 4 + wave) * 4 + {0: step start, 1: first part done, 2: at the barrier, 3: barrier passed}]. */
int uva_net_debug_rdb_stamps(uva_net* net, unsigned long long* out, int max_steps);
#endif

/* Test hook (host only, no device needed): the fp16 MFMA A-operand image convolution #conv_idx is
 * repacked into, [k-step][m-frag][lane][8].  *needed receives the element count.  conv_idx -1: the
 * last convolution as tail_kernel reads it (64-feature nets). */
int uva_net_debug_packed_weights(uva_net* net, int conv_idx, uint16_t* out, size_t out_halfs, size_t* needed);

/* Test hook (host only): the step lists trunk2_kernel (two fused trunk layers per launch) would walk for an
 * h x w frame cut into reference tiles (tile_size, border; <= 0: one plane) on `grid` workgroups.  Every
 * workgroup has `*stride` 32-byte entries of 8 words (csrc/uva_kernels.hip.h Trunk2Step), nsteps[b] of them
 * real.  plane_hw receives h, w, activation pitch and array offset (pixels) of up to max_planes planes.
 * Returns non-zero if steps_words (capacity in 32-bit words) is too small; *needed_words says how many. */
int uva_debug_trunk2_schedule(int h, int w, int tile_size, int border, int grid, uint32_t* steps_words,
                              size_t capacity_words, size_t* needed_words, int* nsteps, int* stride,
                              long long* plane_info, int max_planes, int* nplanes, long long* guard_bytes);

/* Test hook (host only): the same for trunkw_kernel (csrc/uva_wino.hip.h: the fused pair as 1-D Winograd F(2,3)), whose
 * segments start without the two input rows shared with the step above: entry layout in that file (TrunkwArgs). */
int uva_debug_trunkw_schedule(int h, int w, int tile_size, int border, int grid, uint32_t* steps_words,
                              size_t capacity_words, size_t* needed_words, int* nsteps, int* stride,
                              long long* plane_info, int max_planes, int* nplanes, long long* guard_bytes);

/* Test hook (host only, after load_param of a generic graph such as 4x_Valar_v1): what the executor planned --
 * info[0] dense chains sharing one array, [1] Concat layers, [2] of them free (every input already in place), [3] copying
 * their first input only, [4] 3x3 convolutions that take the LDS-tiled kernel, [5] channels of the widest shared array, [6] residual dense blocks
 * whose first four convolutions run as one launch (rdb4_kernel).  info: at least 8 ints. */
int uva_net_debug_generic_plan(const uva_net* net, int* info);

/* Test hook (host only): how often the generic executor has launched each of its kernel instantiations on this net since
 * uva_net_create -- counted on the host next to the launch, nothing on the GPU.  *n = the number of counters (also with
 * counts == NULL); capacity < *n is an error.  Index: 11-14 g_conv3_lds<1..4> (3x3, weights through LDS), 15 / 23
 * g_conv3_lds<4 / 2, 3, true, 8> (16-row tiles), 16-19 g_conv3_lds<1..4, 1> (1x1), 21 / 22 g_conv3_lds<2 / 4, 3, true> (weights in
 * registers); g_conv3_sw: 24 <6,1,false,2,0>, 25 <6,1,false,2,2>, 26 <2,2,false,1,0>, 27 <2,2,true,0,0>, 29 <6,1,false,0,0>,
 * 30 <2,2,false,0,0>, 31 <2,2,true,0,0,true> (the 2x Interp folded in); 28 rdb4_kernel; g_conv3_sk: 32 <2,0>, 33 <2,2>, 34 <0,0>;
 * 40 g_conv<1>, 41 g_conv<3>, g_conv3_sww: 42 no sum, 43 one sum, 44 two sums; 45 g_axpby, 46 g_axpby_strided, 47 g_concat_part,
 * 48 g_interp_nearest, 49 g_prelu, 50 g_pixelshuffle, 51 g_input_f32, 52 g_input_u8, 53 g_output_f32, 54 g_output_u8. */
int uva_net_debug_generic_launches(const uva_net* net, long long* counts, int capacity, int* n);

/* Test hook (host only): the work lists of the generic executor's persistent kernels for an h x w plane on `grid`
 * workgroups -- kind 0: rdb4_kernel (a residual dense block's first four convolutions, models/4x_Valar_v1.param:6-19),
 * kind 1 / 2: g_conv3_sw with 32 / 64-column strips (the 192 -> 64 and 64 -> 64 convolutions).  Every segment is 8 words
 * {c0, y_begin, y_end, own0, own1, plane, 0, 0}: the kernel computes columns c0.. of rows [y_begin, y_end) and writes
 * columns [own0, own1) of them; seg_begin (grid + 1 ints): workgroup g owns segments seg_begin[g] .. seg_begin[g+1]. */
int uva_debug_generic_segments(int kind, int h, int w, int grid, int32_t* segs_words, size_t capacity_words, size_t* needed_words,
                               int* seg_begin);
/* The same for a BATCH of planes sharing one launch (the reference tiles of a frame, upscale_processing.py:499-516):
 * dims = {h0, w0, h1, w1, ...}, nplanes <= 16; word 5 of a segment is the index of its plane. */
int uva_debug_generic_segments_planes(int kind, const int* dims, int nplanes, int grid, int32_t* segs_words, size_t capacity_words,
                                      size_t* needed_words, int* seg_begin);

/* Test hook (host only): how the generic executor groups the planes (reference tiles) of an h x w frame into the batches
 * that go through the graph together.  Four words per plane {h, w, batch, class}; planes of a batch have one class, at
 * most 16 members and -- unless a single plane exceeds it -- at most batch_pixels input pixels (<= 0: the default). */
int uva_debug_generic_batches(int h, int w, int tile_size, int border, long long batch_pixels, int32_t* words, size_t capacity_words,
                              size_t* needed_words);

/* Test hook (host only): the row lists sub10_kernel (the whole 24-feature 1x net, one launch) walks for an h x w
 * frame on `grid` workgroups.  Every workgroup has `*stride` 16-byte entries of 4 words {y, x0, emit, 0}
 * (csrc/uva_sub10.h Sub10Args), nrows[b] of them real: the kernel computes columns x0 .. x0+79 of row y and
 * writes columns x0+10 .. x0+69 of it when emit is set. */
int uva_debug_sub10_rows(int h, int w, int grid, uint32_t* rows_words, size_t capacity_words, size_t* needed_words,
                         int* nrows, int* stride);
/* ... for `frames` (1..8) frames of that geometry in one launch: the sequence runs over (frame, strip, row); the frame of an
 * entry is emit >> 8 (emit & 1 as above), the fourth word the distance to the nearest row of the segment that is written out. */
int uva_debug_sub10_rows_batch(int h, int w, int frames, int grid, uint32_t* rows_words, size_t capacity_words, size_t* needed_words,
                               int* nrows, int* stride);
/* The same for sub5_kernel (UVA_SUB5=1: that net as two launches of five layers, two pipelines -- a PAIR of 54-column strips --
 * per workgroup; csrc/uva_sub5.hip.h).  Entries {row y, column of computed column 0 of the pair's first strip, 1 = written
 * out, 0}; both launches walk the same lists. */
int uva_debug_sub5_rows(int h, int w, int grid, uint32_t* rows_words, size_t capacity_words, size_t* needed_words,
                        int* nrows, int* stride);

const char* uva_last_error(void);
int uva_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* UVA_H */
