/*
 * ffl.h -- C ABI of libffl_hip.so: the MI355X (gfx950) implementation of Funscript-Flow's
 * per-frame-pair motion path.  Plain pointers and sizes only; every entry point returns an int
 * status (FFL_OK == 0) unless stated otherwise and records a message readable through
 * ffl_last_error().  There is NO CPU fallback: without a usable HIP device ffl_create() fails.
 *
 * What each entry point replaces in the reference (FF = FunscriptFlow.pyw):
 *
 *   ffl_device_count        availability probe get_available_backends()            FF:32-63
 *   ffl_create/ffl_destroy  (no counterpart: the reference's pair kernel is stateless; the context
 *                           owns the device buffers the CUDA variant allocates per call, FF:984-987)
 *   ffl_upload_frame        the p0/p1 ndarrays handed to precompute_flow_info       FF:843, 1188-1191
 *                           (cuda_GpuMat.upload in the CUDA variant, FF:986-987); also does the
 *                           cv2.cvtColor(..., COLOR_RGB2GRAY) of FF:1082 when given 3 channels
 *   ffl_upload_frames_raw   the decoded frame's way to that operand: cv2.cvtColor(BGR2RGB) FF:182,
 *                           cv2.resize(frame, (256, 256)) FF:185-186 (non-VR) or cv2.resize(f, (512, 512))
 *                           + crop f[256:, :256] FF:1076-1079 (VR), cv2.cvtColor(RGB2GRAY) FF:1079/1082
 *   ffl_upload_frames_yuv   the same operand from a decoder's native 4:2:0 output (I420 / NV12): the decoder's own
 *                           YUV->BGR conversion before FF:182, then as ffl_upload_frames_raw
 *   ffl_upload_frames_yuv16 the same from 9- to 16-bit 4:2:0 (yuv420p10le, P010 / P016): each sample reduced to 8 bits at
 *                           its load (appendix Y, rule Y5); ffl_upload_frames_device16 for such frames in device memory
 *   ffl_flow_pairs          cv2.calcOpticalFlowFarneback(p0,p1,None,0.5,3,15,3,5,1.2,0)  FF:878-879
 *                           + max_divergence(flow)  FF:884 -> FF:748-758
 *                           + cv2.cartToPolar / np.mean                             FF:889-890
 *                           for a whole batch of pairs (Pool.starmap, FF:1190-1191)
 *   ffl_pass1_result        the dict built at FF:898-907 (pos_center, val_pos, mean_mag, cut)
 *   ffl_radial              radial_motion_weighted(flow, center, is_cut, pov_mode)  FF:761-785
 *                           for a batch (ProcessPoolExecutor.submit loop, FF:1232-1236)
 *   ffl_radial_window       the centre window of FF:1203-1214, the cut test of FF:898-907 and radial_motion_weighted
 *                           FF:761-785 for a batch, behind the batches on the caller's stream: FF:1203-1236 without the host
 *   ffl_radial_axes, ffl_radial_window_axes  replace nothing: the reference reduces a field to its radial part alone.  They
 *                           are ffl_radial / ffl_radial_window with the rotation about the centre and the weighted shift
 *                           next to it, for multi-axis scripts
 *   ffl_cell_stats          center_of_mass_variance(flow, num_cells)                FF:721-746
 *                           for a batch, with its intermediate grid of regional mean flow, mean magnitude and variance
 *                           
 *   ffl_radial_window_axes_centres  ffl_radial_window_axes with the centre list of FF:1203-1214 read from device memory:
 *                           the variance centres of ffl_cell_stats, or any other estimator's
 *   ffl_consistency_weights replaces nothing (the reference's detect_cut is dead and nothing in it weights pixels): the
 *                           forward-backward check of a pair's two fields as a weight map for ffl_pass1_weighted and
 *                           ffl_radial_window_axes_weighted
 *   ffl_residual_weights    replaces nothing either: the photometric residual of a pair under its forward field (frame 1
 *                           sampled where the flow lands, against frame 0 and its local gradient) as such a weight map; needs
 *                           no backward field
 *   ffl_texture_weights     replaces nothing either: the local structure tensor of one frame (Noble's cornerness over a
 *                           window) as such a weight map or as the gate of the two above -- low on flat regions and on pure
 *                           stripes, where dense flow is unconstrained and both checks above approve of it; needs no flow
 *                           at all
 *   ffl_track_advance       replaces nothing: the reference finds a centre afresh for every pair (FF:748-758, or FF:721-746)
 *                           and has no way to say "the subject is here, follow it".  It advects caller-chosen points through
 *                           the fields of consecutive pairs; its records are centres for ffl_radial_window_axes_centres
 *                           
 *   ffl_roi_weights         replaces nothing either: an elliptical weight map about such a centre, which confines pass 1 and
 *                           pass 2 to the tracked region -- which pixels are the subject, not which are reliable (appendix E)
 *   ffl_radial_window_axes_weighted_centres  ffl_radial_window_axes_weighted about the centres of
 *                           ffl_radial_window_axes_centres: the two flags of the window form set together
 *   ffl_track_template, ffl_track_match  replace nothing: integrating a flow drifts, and these pull a tracked centre back
 *                           onto a template of the gray frame captured about it -- an integer SSD / zero-mean SSD search
 *                           within +-s pixels, verdicts FLAT / POOR / AMBIGUOUS, the centre overwritten in place so that
 *                           every call that reads centres from device memory reads corrected ones (DESIGN.md section 24,
 *                           appendix N)
 *   ffl_track_redetect      replaces nothing either: ffl_track_match looks only +-s <= 16 pixels about the centre, and a
 *                           track further from its subject than that stays lost.  This searches the WHOLE frame (or a wide
 *                           reach about the centre) for the template, only where a trigger word in device memory -- the
 *                           status of a match record -- says the local search failed, and writes the centre back on the
 *                           device.  Whole pixels, no scale or rotation, no template update (DESIGN.md section 25,
 *                           appendix L)
 *   ffl_motion_fit, ffl_motion_subtract  replace nothing: the reference cancels global motion only by the quadrant weights
 *                           of radial_motion_weighted ("Cancel out global motion by balancing the averages", FF:779-783), which
 *                           cancel a pan only about the image centre.  These fit a per-pair camera model (translation, rigid,
 *                           similarity or affine) to a field robustly and subtract it, ahead of pass 1 and pass 2 (DESIGN.md
 *                           section 19, appendix C)
 *   ffl_download_flow       the "flow" entry of that dict (tests / callers that want the array)
 *   ffl_upload_frames_device  ffl_upload_frames_raw / _yuv / ffl_upload_frames for frames already in device memory (a GPU
 *                           decoder's surfaces, torch tensors); ffl_export_flows: ffl_download_flow into device memory
 *   ffl_remap_create, ffl_upload_frames_remap, ffl_upload_frames_device_remap  replace nothing: the reference's VR mode is a
 *                           resize of the whole side-by-side frame and a crop, FF:1076-1079, which leaves the operand
 *                           equirectangular.  These form it through a per-pixel source map instead -- a pinhole view of one
 *                           eye, an undistortion; ffl_remap_check, ffl_remap_bytes and
 *                           ffl_remap_destroy belong to them
 *   ffl_import_flows        ffl_upload_flow for n fields already in device memory (float32, float16 or bfloat16, any
 *                           strides): the reductions of FF:884-894 on a flow the caller computed
 *   ffl_submit_pair         precompute_wrapper((p0, p1), params)                    FF:1019-1021
 *   ffl_flow_pairs_farneback  cv2.calcOpticalFlowFarneback(p0, p1, None, pyr_scale, levels, winsize, iterations, poly_n,
 *                           poly_sigma, 0) with the caller's values + the same reductions
 *   ffl_flow_pairs_farneback_ex  the same call with flags = OPTFLOW_FARNEBACK_GAUSSIAN and / or OPTFLOW_USE_INITIAL_FLOW
 *                           (flow = the pair's flow slot) as its mode
 *   ffl_flow_pairs_dis      cv2.DISOpticalFlow_create(cv2.DISOPTICAL_FLOW_PRESET_FAST).calc(p0, p1, None)
 *                           + max_divergence + cartToPolar of the "DNN" backend     FF:948-980
 *                           (rules restated in DESIGN.md appendix D; parity with cv2 itself is unpinned)
 *
 * Threading: a context is bound to one device and is internally stream-ordered.  Every entry point locks the
 * context, so calls may come from several host threads (an uploader, a submitter and a result collector working
 * on distinct slots).  The per-batch calls do not hold the context lock while they wait for the device or
 * copy frames into staging (ffl_pass1_result(s), ffl_download_flow, ffl_radial, ffl_upload_flow, ffl_sync,
 * ffl_host_free, ffl_upload_frames(_raw) all release it for that time, and wait on events only -- never on a stream
 * another thread may be capturing a graph on); uploads are serialised among themselves, pass-2 calls among themselves
 * (ffl_radial, ffl_radial_window, ffl_export_flows, ffl_import_flows and ffl_upload_flow share one stream; the three
 * device-memory calls among them only queue work and never wait for it).
 * ffl_flow_pairs waits under the lock only when a lane already has 16 batches queued or evicts a captured graph; the
 * test / measurement hooks (ffl_debug_pair, ffl_download_frame, ffl_profile_read) wait under it.
 * ffl_last_error() returns the message of the context's most recent failing call by any thread.
 * Options: ffl_set_option() changes the process-wide DEFAULTS; a context copies them when it is created and is from then
 * on changed only through ffl_ctx_set_option(), so two contexts of one process (one per GPU) share no knob.
 * Sizes: 16x16 <= width x height, 20 * width * height < 2^32 (32-bit plane offsets in the kernels).
 */
#ifndef FFL_H
#define FFL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFL_OK 0
#define FFL_ERR_INVALID 1   /* bad argument (slot out of range, size mismatch, NULL, ...) */
#define FFL_ERR_HIP 2       /* a HIP runtime call failed; see ffl_last_error */
#define FFL_ERR_NO_DEVICE 3 /* no usable gfx950 device */
#define FFL_ERR_STATE 4     /* slot not ready (e.g. result requested before ffl_flow_pairs) */

#define FFL_MAX_BATCH 256   /* pairs per ffl_flow_pairs / ffl_radial call */

typedef struct ffl_ctx ffl_ctx;

/* Number of HIP devices visible to this process (0 when none / no runtime). */
int ffl_device_count(void);

/* Create a context for frames of exactly width x height on `device`.
 *   n_frame_slots  gray frames resident on the device (>= 2)
 *   n_flow_slots   finished flow fields kept resident for pass 2 (a streaming two-pass schedule with two batches
 *                  in flight and the +-6 smoothing window of FF:1203-1214 needs >= 2 * max_batch + 13)
 *   max_batch      pairs processed per ffl_flow_pairs call (1..FFL_MAX_BATCH) */
int ffl_create(int device, int width, int height, int n_frame_slots, int n_flow_slots, int max_batch,
               ffl_ctx **out);
void ffl_destroy(ffl_ctx *ctx);

/* Last error text for ctx (or for the calling thread's failed ffl_create when ctx == NULL). Never NULL.  The text is a
 * per-thread copy taken under the context lock: valid until the calling thread's next ffl_last_error(). */
const char *ffl_last_error(const ffl_ctx *ctx);

/* Sizing a context before creating it (no counterpart in the reference, whose `precomputed` list simply grows in host
 * memory, FF:1191): free / total device memory of `device`, and the device + page-locked host bytes ffl_create would
 * allocate for these arguments under the current "lanes" option.  backend.precompute_all uses them to pick a batch size
 * that fits, or to refuse a chunk that cannot stay resident with a message instead of a failed hipMalloc. */
int ffl_device_mem_info(int device, size_t *free_bytes, size_t *total_bytes);
int ffl_estimate_bytes(int width, int height, int n_frame_slots, int n_flow_slots, int max_batch, size_t *device_bytes,
                       size_t *pinned_bytes);

/* Copy one frame into frame slot `fslot`.  `channels` is 1 (gray uint8, what the reference feeds
 * Farneback, FF:1082) or 3 (BGR uint8 as cv2.VideoCapture.read returns, FF:178; converted on the
 * device with OpenCV's 8-bit fixed-point luma).  `stride_bytes` is the row pitch of `data`.
 * The pixels are copied into pinned staging before the call returns (the caller may reuse its
 * array); the H2D transfer itself runs on a side stream and overlaps compute already queued. */
int ffl_upload_frame(ffl_ctx *ctx, int fslot, const uint8_t *data, int width, int height, int channels,
                     ptrdiff_t stride_bytes);

/* The same for n frames going to the consecutive slots first_slot .. first_slot+n-1, with one H2D transfer
 * (and one gray-conversion launch) for the whole run: the batched small-image path. */
int ffl_upload_frames(ffl_ctx *ctx, int first_slot, int n, const uint8_t *const *frames, int width, int height,
                      int channels, ptrdiff_t stride_bytes);

/* Input front-end: n decoded 3-channel uint8 frames of src_width x src_height (row pitch
 * stride_bytes; BGR as cv2.VideoCapture.read returns them, or RGB when rgb_order != 0) go to the frame
 * slots first_slot .. first_slot+n-1 as
 *     gray( resize(frame, (resize_width, resize_height)) [crop_y : crop_y+height, crop_x : crop_x+width] )
 * with width x height the context's frame size, cv2.resize's 8-bit INTER_LINEAR rule (11-bit weights; an
 * exact 2x2 down-scale takes INTER_AREA's 2x2 mean; equal sizes skip the resize) and cv2's 8-bit luma
 * (15-bit weights).  The reference's two uses: non-VR (256, 256, 0, 0) on a 256x256 context (FF:185-186,
 * FF:1082); VR (512, 512, 0, 256) on a 256x256 context (FF:1076-1079).  Only the source pixels the crop
 * window samples are read on the device.  Pixels are copied to pinned staging before the call returns. */
int ffl_upload_frames_raw(ffl_ctx *ctx, int first_slot, int n, const uint8_t *const *frames, int src_width,
                          int src_height, ptrdiff_t stride_bytes, int rgb_order, int resize_width, int resize_height,
                          int crop_x, int crop_y);

/* Stream metadata of the frames of one call (rules Y6 and Y7): what cv2.VideoCapture.read applies
 * to every frame before the reference sees a pixel (FF:178) and a decoder's raw planes do not carry.
 *   Y6  `rotate` in {0, 90, 180, 270} is the clockwise rotation that makes the stored src_width x src_height frame S
 *       upright, `mirror` in {0, 1} a left-right flip applied after it: U = np.rot90(S, -rotate / 90), then U[:, ::-1].
 *       Every rule of the call then applies to U: resize size, crop, resize mode, clamps and scales are in upright
 *       terms (U is src_height x src_width for 90 / 270); src_width, src_height, strides, pitches, planes and the
 *       transfer window stay in stored terms.  A pure index permutation: the operand is, bit for bit, that of the
 *       upright frame.  4:2:0 chroma stays sample (x >> 1, y >> 1) of the stored planes.
 *   Y7  `full_range` in {0, 1}, 4:2:0 sources only: 1 converts full-range ("JPEG", yuvj420p) samples with no offset and
 *       no 255/219 gain, B = sat8((yh + 1858077 u) >> 20), G = sat8((yh - 748826 v - 360853 u) >> 20), R = sat8((yh +
 *       1470104 v) >> 20) with yh = (Y << 20) + (1 << 19), u = U - 128, v = V - 128; 0 is appendix Y as it stands.  The
 *       library's own rule: swscale's table conversion is not reproducible and cv2 has no full-range 4:2:0 code.
 * Every front-end entry point has a sibling named with a _src suffix that takes its arguments plus this struct.  NULL or
 * all zeros is the call without the suffix, bit for bit, with the same messages.  Refused before any device work with
 * FFL_ERR_INVALID (the message names the rule): a rotate other than the four values, mirror or full_range outside 0 / 1,
 * full_range on a source that is not 4:2:0, and every refusal of the plain call, those about resize and crop in upright
 * terms.  A BGR frame out of cv2.VideoCapture.read is upright already: rotating it again is wrong. */
typedef struct ffl_source_info {
    int rotate;
    int mirror;
    int full_range;
} ffl_source_info;

/* ffl_upload_frames_raw for a stored frame with stream metadata (rule Y6 of ffl_source_info, FF:178): the operand of the
 * upright frame.  The whole stored frame travels, as without metadata; full_range is refused (BGR carries no range). */
int ffl_upload_frames_raw_src(ffl_ctx *ctx, int first_slot, int n, const uint8_t *const *frames, int src_width,
                              int src_height, ptrdiff_t stride_bytes, int rgb_order, int resize_width, int resize_height,
                              int crop_x, int crop_y, const ffl_source_info *src);

/* 4:2:0 layouts of ffl_upload_frames_yuv: cv2's single-array (H*3/2, W) uint8 frames.  I420: the Y plane, then U as
 * (H/2) x (W/2) contiguous bytes, then V (PyAV's yuv420p, `ffmpeg -pix_fmt yuv420p`).  NV12: the Y plane, then H/2 rows of
 * interleaved U,V (`ffmpeg -pix_fmt nv12`, hardware decoder surfaces). */
#define FFL_YUV_I420 0
#define FFL_YUV_NV12 1

/* The YUV input front-end: n decoded 4:2:0 frames of src_width x src_height (both even; `layout` FFL_YUV_I420 with
 * stride_bytes == src_width, or FFL_YUV_NV12 with stride_bytes >= src_width) go to the frame slots
 * first_slot .. first_slot+n-1 as
 *     gray( resize( cvtColor(frame, COLOR_YUV2BGR_I420 | COLOR_YUV2BGR_NV12), (resize_width, resize_height) )
 *           [crop_y : crop_y+height, crop_x : crop_x+width] )
 * -- the decoder's conversion of the reference's cv2.VideoCapture.read (FF:178), then FF:185-186 / FF:1076-1079 and
 * FF:1079/1082 exactly as ffl_upload_frames_raw computes them.  The conversion is BT.601 limited range in OpenCV's
 * 20-bit fixed point with nearest chroma; cv2.VideoCapture's own swscale conversion interpolates
 * chroma, so these operands are not those of the BGR path for the same video.  Only the source rectangle the crop
 * window reads (ffl_frontend_yuv_window) is transferred: out of ffl_host_alloc memory one 2-D copy per plane straight
 * from the buffer (leave it alone until the transfer is over, as for ffl_upload_frames), from anywhere else through a
 * staging copy made before the call returns.  Refused (FFL_ERR_INVALID, the message names the rule): odd sizes, an
 * unknown layout, I420 with stride != width, NV12 with stride < width, a crop that does not fit, NULL frames, a bad
 * slot range. */
int ffl_upload_frames_yuv(ffl_ctx *ctx, int first_slot, int n, const uint8_t *const *frames, int src_width,
                          int src_height, ptrdiff_t stride_bytes, int layout, int resize_width, int resize_height,
                          int crop_x, int crop_y);

/* The source rectangle ffl_upload_frames_yuv transfers for these arguments (out_w x out_h = the context's frame size):
 * win = {x, y, width, height} in source pixels, all even, a superset of every pixel the kernel reads (first and last
 * output row / column mapped back, widened by one pixel per side, rounded out to even, clamped to the frame); *bytes =
 * the bytes one frame transfers (width * height * 3 / 2).  Either output may be NULL.  No device needed.  The same
 * refusals as ffl_upload_frames_yuv (message through ffl_last_error(NULL)). */
int ffl_frontend_yuv_window(int src_w, int src_h, int layout, ptrdiff_t stride_bytes, int resize_w, int resize_h,
                            int crop_x, int crop_y, int out_w, int out_h, int win[4], size_t *bytes);

/* ffl_upload_frames_yuv and ffl_frontend_yuv_window for stored frames with stream metadata (rules Y6 and Y7 of
 * ffl_source_info: display rotation, mirroring and colour range, which cv2.VideoCapture.read applies at FF:178).  The
 * window is still a rectangle of the STORED frame: the upright span of the plain call mapped through Y6, then rounded out
 * on the stored axes (16 samples in x, 2 in y, all even, clamped); only it is transferred, under the same zero-copy rule. */
int ffl_upload_frames_yuv_src(ffl_ctx *ctx, int first_slot, int n, const uint8_t *const *frames, int src_width,
                              int src_height, ptrdiff_t stride_bytes, int layout, int resize_width, int resize_height,
                              int crop_x, int crop_y, const ffl_source_info *src);
int ffl_frontend_yuv_window_src(int src_w, int src_h, int layout, ptrdiff_t stride_bytes, int resize_w, int resize_h,
                                int crop_x, int crop_y, int out_w, int out_h, int win[4], size_t *bytes,
                                const ffl_source_info *src);

/* High-bit-depth 4:2:0 (rule Y5): the same single-array layouts with uint16 little-endian samples,
 * shape (H*3/2, W) counted in samples -- `ffmpeg -pix_fmt yuv420p10le|yuv420p12le` (FFL_YUV_I420, the significant bits
 * low: msb_aligned 0) and P010 / P012 / P016 decoder surfaces (FFL_YUV_NV12, the significant bits high: msb_aligned 1).
 * `depth` = 9..16 significant bits.  Every sample is reduced to 8 bits at its load, round half up with saturation,
 *     s  = msb_aligned ? raw >> (16 - depth) : raw;      v8 = min(255, (s + (1 << (depth - 9))) >> (depth - 8))
 * (defined for every 16-bit pattern: the bits below a high-aligned sample are ignored, a low-aligned sample >= 2^depth
 * gives 255) and then converted exactly as ffl_upload_frames_yuv converts its bytes.  This is the library's own rule:
 * swscale dithers such a reduction and cv2 has none.
 * The contract of ffl_upload_frames_yuv otherwise, with the window (ffl_frontend_yuv16_window) travelling at 2 bytes per
 * sample; stride_bytes is in BYTES.  Refused (FFL_ERR_INVALID, the message names the rule): depth outside 9..16, an odd
 * stride_bytes, a frame pointer that is not 2-byte aligned, I420 with stride_bytes != 2 * width, NV12 with stride_bytes <
 * 2 * width, and every refusal of ffl_upload_frames_yuv. */
int ffl_upload_frames_yuv16(ffl_ctx *ctx, int first_slot, int n, const uint16_t *const *frames, int src_width,
                            int src_height, ptrdiff_t stride_bytes, int layout, int depth, int msb_aligned,
                            int resize_width, int resize_height, int crop_x, int crop_y);

/* ffl_frontend_yuv_window for 16-bit frames: the same rectangle (in samples; columns rounded out to multiples of 16
 * samples) for the same geometry, *bytes = width * height * 3.  The refusals of ffl_upload_frames_yuv16. */
int ffl_frontend_yuv16_window(int src_w, int src_h, int layout, ptrdiff_t stride_bytes, int depth, int resize_w,
                              int resize_h, int crop_x, int crop_y, int out_w, int out_h, int win[4], size_t *bytes);

/* The two 16-bit calls with stream metadata (rules Y6 and Y7 of ffl_source_info, FF:178): as ffl_upload_frames_yuv_src and
 * ffl_frontend_yuv_window_src; rule Y5 reduces each sample first, unchanged, and Y7 then applies to the 8-bit values. */
int ffl_upload_frames_yuv16_src(ffl_ctx *ctx, int first_slot, int n, const uint16_t *const *frames, int src_width,
                                int src_height, ptrdiff_t stride_bytes, int layout, int depth, int msb_aligned,
                                int resize_width, int resize_height, int crop_x, int crop_y, const ffl_source_info *src);
int ffl_frontend_yuv16_window_src(int src_w, int src_h, int layout, ptrdiff_t stride_bytes, int depth, int resize_w,
                                  int resize_h, int crop_x, int crop_y, int out_w, int out_h, int win[4], size_t *bytes,
                                  const ffl_source_info *src);

/* ---- device-memory I/O ------------------------------------------------------------------------
 * Frames that already live in device memory (a GPU decoder's surfaces, torch tensors) go to frame slots without a round
 * trip through the host, and flow fields go from flow slots into caller device memory.  Same operands, same fields.
 *
 * A frame is described by its planes.  Byte offset of channel c of pixel (x, y) in plane 0:
 *     y * pitch[0] + x * pixel_stride + c * channel_stride
 * packed HWC BGR: pixel_stride 3, channel_stride 1 (BGRA: 4, 1 -- channel 3 is never read); planar CHW: pixel_stride 1,
 * channel_stride = the distance of the planes.  4:2:0 (pixel_stride and channel_stride unused): plane 0 = Y (pitch[0]),
 * I420: plane 1 = U, plane 2 = V (each (h/2) x (w/2) with its own pitch); NV12: plane 1 = the interleaved UV rows
 * (pitch[1]); plane 2 unused. */
typedef struct ffl_dev_frame {
    const void *plane[3];
    ptrdiff_t pitch[3];
    ptrdiff_t pixel_stride;
    ptrdiff_t channel_stride;
} ffl_dev_frame;
#define FFL_DEV_GRAY 0 /* 1 channel; the context's size, copied as it is (no resize, no crop) */
#define FFL_DEV_BGR 1  /* 3 channels, B first (cv2's order) */
#define FFL_DEV_RGB 2  /* 3 channels, R first */
#define FFL_DEV_I420 3
#define FFL_DEV_NV12 4
#define FFL_FLOW_NHWC 0 /* (n, H, W, 2): cv2's layout, u and v interleaved */
#define FFL_FLOW_NCHW 1 /* (n, 2, H, W): the u plane, then the v plane */

/* The geometry rules of ffl_upload_frames_device for one frame (out_w x out_h = the context's frame size).  Pure host
 * check: no device or context needed.  FFL_ERR_INVALID with the rule in ffl_last_error(NULL): an unknown format; a size
 * outside 1..32768; negative strides, or a pitch / pixel stride / channel stride too small for the extent (packed: pixel
 * stride >= 3 * channel stride >= 3 and pitch >= (w - 1) * pixel stride + 2 * channel stride + 1; planar: channel stride
 * >= pitch * h and pitch >= (w - 1) * pixel stride + 1; 4:2:0: pitch[0] >= w, I420 chroma pitches >= w / 2, NV12
 * pitch[1] >= w); odd 4:2:0 sizes; gray with a resize, a crop or a size other than the context's; a crop window that does
 * not fit the resized frame; a NULL plane the format needs. */
int ffl_dev_frame_check(int format, int src_w, int src_h, const ffl_dev_frame *f, int resize_w, int resize_h, int crop_x,
                        int crop_y, int out_w, int out_h);

/* n device-resident frames (format FFL_DEV_*, each src_w x src_h) -> frame slots first_slot .. first_slot+n-1, as
 *   gray( resize(frame, (resize_w, resize_h)) [crop_y : crop_y+height, crop_x : crop_x+width] )
 * with exactly the bytes of the host paths for the same pixels: ffl_upload_frames_raw's rules for BGR / RGB,
 * ffl_upload_frames_yuv's (appendix Y) for I420 / NV12, ffl_upload_frames' copy for gray.  Every frame is checked
 * (ffl_dev_frame_check) and every plane it reads must be device memory of the context's device, all of it inside one
 * allocation (hipPointerGetAttributes, hipMemGetAddressRange); page-locked host memory -- ffl_host_alloc's included -- is
 * refused: it belongs to the host upload calls.  Refusals happen before any device work.
 * Stream contract (`stream` is a hipStream_t as an integer; 0 = the null stream):
 *   - a stream that is capturing a graph is refused with FFL_ERR_STATE; that check is the first HIP call made on it;
 *   - the frames are read after the work queued on `stream` before the call (an event recorded on `stream`, waited for by
 *     the library's upload stream), by ONE k_frontend_dev launch for all n frames;
 *   - `stream` is made to wait (hipStreamWaitEvent) for that launch: work queued on it afterwards -- overwriting the
 *     sources, or the caching allocator reusing them -- runs after the frames have been read;
 *   - frame slots are published and their previous readers waited for as ffl_upload_frames_raw does it;
 *   - the host never waits for the device, except where the slot-reuse rules of the host uploads make it wait too.
 * Nothing of this call is ever captured into the library's graphs. */
int ffl_upload_frames_device(ffl_ctx *ctx, int first_slot, int n, const ffl_dev_frame *frames, int format, int src_w,
                             int src_h, int resize_w, int resize_h, int crop_x, int crop_y, uint64_t stream);

/* The device-memory calls for 16-bit 4:2:0 frames (rule Y5, see ffl_upload_frames_yuv16): format FFL_DEV_I420 or
 * FFL_DEV_NV12 only, the planes of ffl_dev_frame holding uint16 samples -- pitches in bytes, even and >= 2 * the samples of
 * a row (Y: w, I420 chroma: w / 2, NV12 UV: w), every plane 2-byte aligned.  Otherwise the rules, the memory checks (extents
 * in bytes), the stream contract and the single k_frontend_dev launch of ffl_dev_frame_check / ffl_upload_frames_device;
 * the operands are those of ffl_upload_frames_yuv16 for the same samples. */
int ffl_dev_frame_check16(int format, int depth, int src_w, int src_h, const ffl_dev_frame *f, int resize_w, int resize_h,
                          int crop_x, int crop_y, int out_w, int out_h);
int ffl_upload_frames_device16(ffl_ctx *ctx, int first_slot, int n, const ffl_dev_frame *frames, int format, int depth,
                               int msb_aligned, int src_w, int src_h, int resize_w, int resize_h, int crop_x, int crop_y,
                               uint64_t stream);

/* The four device-memory calls for stored frames with stream metadata (rules Y6 and Y7 of ffl_source_info: the display
 * rotation, mirroring and colour range cv2.VideoCapture.read applies at FF:178; a GPU decoder's surfaces carry neither).
 * src_w, src_h, the pitches, the extents and the one-allocation-per-plane check stay on the stored frame; resize and crop
 * are in upright terms, and an oriented gray frame's UPRIGHT size must be the context's.  Stream contract, slot publishing
 * and the single k_frontend_dev launch are those of the plain calls. */
int ffl_dev_frame_check_src(int format, int src_w, int src_h, const ffl_dev_frame *f, int resize_w, int resize_h, int crop_x,
                            int crop_y, int out_w, int out_h, const ffl_source_info *src);
int ffl_dev_frame_check16_src(int format, int depth, int src_w, int src_h, const ffl_dev_frame *f, int resize_w, int resize_h,
                              int crop_x, int crop_y, int out_w, int out_h, const ffl_source_info *src);
int ffl_upload_frames_device_src(ffl_ctx *ctx, int first_slot, int n, const ffl_dev_frame *frames, int format, int src_w,
                                 int src_h, int resize_w, int resize_h, int crop_x, int crop_y, uint64_t stream,
                                 const ffl_source_info *src);
int ffl_upload_frames_device16_src(ffl_ctx *ctx, int first_slot, int n, const ffl_dev_frame *frames, int format, int depth,
                                   int msb_aligned, int src_w, int src_h, int resize_w, int resize_h, int crop_x, int crop_y,
                                   uint64_t stream, const ffl_source_info *src);

/* ---- Map-driven reprojection -------------------------------------------------------
 * Every path above has one geometry: resize, an axis-aligned crop, luma.  The reference's VR mode is that too -- the whole
 * side-by-side equirectangular frame resized to 512 x 512 and a quadrant kept (FF:1076-1079) -- and everything behind the
 * operand assumes a rectilinear image, which a quadrant of an equirect or fisheye frame is not.  A per-output-pixel source
 * map, built once per stream on the host (frontend.view_map: a pinhole view of one eye; as well lens undistortion, a
 * rotation by any angle, an ROI zoom), is applied by a gather kernel where the operand is formed.  Nothing in the reference
 * does this: the rules are the library's own, in the fixed-point form of cv2.remap (5 fractional bits); parity with cv2 is
 * unpinned.
 *
 * A map serves a context of ow x oh with supersampling S in {1, 2, 4}: an (S*oh, S*ow, 2) array of int32 (qx, qy), upright
 * source coordinates in 1/32 px of an upright src_w x src_h source.
 *   R1  validity: qx == FFL_REMAP_NO_SOURCE marks a sample with no source (its qy is ignored).  Every other entry must
 *       satisfy 0 <= qx <= 32 * (src_w - 1) and 0 <= qy <= 32 * (src_h - 1).  Creation refuses a map with any other entry
 *       and names the first offender; it also refuses a map with no valid entry.  The kernel never range-checks.
 *   R2  taps: x0 = qx >> 5, fx = qx & 31, x1 = min(x0 + 1, src_w - 1); the same in y.
 *   R3  sample, per channel: r = (s00 (32-fx)(32-fy) + s01 fx (32-fy) + s10 (32-fx) fy + s11 fx fy + 512) >> 10.  The
 *       channels of a tap are those the resize paths fetch: BGR and RGB as stored; 4:2:0 converted per tap by appendix Y (by
 *       Y7 under full_range), after Y5's reduction of 16-bit samples; gray has one channel.  Rule Y6 (rotation, mirror)
 *       applies at the fetch: the map is in upright terms.
 *   R4  a sample with no source is 0 in every channel.
 *   R5  pixel: the channel value is (sum of the pixel's S*S samples + S*S/2) >> (2 log2 S); luma is then the 15-bit
 *       expression of every other path; a gray source stores the channel as it is.
 *   R6  window: the bounding box of all taps of valid entries (upright), mapped through Y6 and rounded out as the 4:2:0
 *       window is everywhere (columns to 16, rows to 2, clamped to the stored frame), is the only part of a host 4:2:0
 *       frame that is transferred, under the zero-copy and staging rule of ffl_upload_frames_yuv.  Host BGR / RGB frames
 *       travel whole.
 * An S = 1 map of integer coordinates gives the identity-mode operand of the resize paths, an S = 2 map of the integer
 * samples (2x + i, 2y + j) their 2x2-mean operand, bit for bit. */
enum { FFL_MAX_REMAPS = 8,                          /* maps alive per context */
       FFL_REMAP_NO_SOURCE = -2147483647 - 1 };     /* INT32_MIN: rule R1 */

/* Rules R1 and R6 for a map, and the rules of ffl_source_info.  Pure host function: no device or context needed; messages
 * through ffl_last_error(NULL).  src_w x src_h is the STORED size (src NULL: upright already).  win_upright = {x, y, w, h}
 * is the bounding box of the taps in the upright frame, win_stored the rectangle of the stored frame R6 names, *valid the
 * number of valid entries; any output may be NULL.  FFL_ERR_INVALID: a NULL map, supersample outside {1, 2, 4}, sizes
 * outside 1..32768, an entry outside R1 (named by its index), a map with no valid entry. */
int ffl_remap_check(const int32_t *map, int out_w, int out_h, int supersample, int src_w, int src_h /*stored*/,
                    const ffl_source_info *src, int win_upright[4], int win_stored[4], size_t *valid);

/* Device bytes one map adds to a context (8 * S * S * out_w * out_h); ffl_estimate_bytes does not count them. */
int ffl_remap_bytes(int out_w, int out_h, int supersample, size_t *bytes);

/* A map for this context (out size = the context's) over an upright src_w x src_h source: checked on the host (R1), copied
 * to the device; *id names it once it is resident, and the caller's array is no longer needed.  At most FFL_MAX_REMAPS are
 * alive per context: one more is refused.  ffl_remap_destroy frees one; it may follow an upload call that used the map at
 * once, for it waits for the last launch that reads the map.  ffl_destroy frees what is left. */
int ffl_remap_create(ffl_ctx *ctx, const int32_t *map, int supersample, int src_w, int src_h /*upright*/, int *id);
int ffl_remap_destroy(ffl_ctx *ctx, int id);

/* n host frames -> frame slots first_slot .. first_slot+n-1 through the map remap_id (rules R2 to R6; k_frontend_remap).
 * format: FFL_DEV_BGR or FFL_DEV_RGB ((h, w, 3) uint8 rows stride_bytes apart, depth 8) or FFL_DEV_I420 / FFL_DEV_NV12 (the
 * single-array layouts of ffl_upload_frames_yuv; depth 8, or 9..16 for uint16 samples with msb_aligned as
 * ffl_upload_frames_yuv16 takes them).  src_w x src_h is the STORED size; its upright size under `src` must be the map's.
 * Slot publishing, staging and direct transfer, locks and refusals are those of ffl_upload_frames_raw_src and
 * ffl_upload_frames_yuv_src / _yuv16_src.  Refused before any device work too: an unknown or destroyed id, an upright
 * source size other than the map's, FFL_DEV_GRAY (a host gray frame has no map path). */
int ffl_upload_frames_remap(ffl_ctx *ctx, int first_slot, int n, const uint8_t *const *frames, int format, int src_w,
                            int src_h /*stored*/, ptrdiff_t stride_bytes, int depth, int msb_aligned, int remap_id,
                            const ffl_source_info *src);

/* The same for n device-resident frames of any FFL_DEV_* format (a gray frame of any size is gathered like a channel), in
 * ONE k_frontend_remap_dev launch: the plane rules, memory checks and stream contract of ffl_upload_frames_device_src /
 * _device16_src (a capturing stream is refused with FFL_ERR_STATE) and the map refusals of ffl_upload_frames_remap. */
int ffl_upload_frames_device_remap(ffl_ctx *ctx, int first_slot, int n, const ffl_dev_frame *frames, int format, int depth,
                                   int msb_aligned, int src_w, int src_h, int remap_id, uint64_t stream,
                                   const ffl_source_info *src);

/* The finished flow fields of flow_slots[0..n) -> dst + i * item_stride_bytes, as (H, W, 2) float32 (FFL_FLOW_NHWC) or as
 * (2, H, W) float32 (FFL_FLOW_NCHW); each item is contiguous, items may be anywhere apart (|stride| >= 8 * W * H bytes).
 * dst must be 4-byte aligned device memory of the context's device with the whole extent in one allocation; the stride a
 * multiple of 4 (16-byte aligned items take the 16-byte path).  Refused: a slot out of range (FFL_ERR_INVALID) or holding
 * no flow (FFL_ERR_STATE), an unknown layout, a capturing `stream` (FFL_ERR_STATE, the first HIP call made on it).
 * Stream contract: the library's stream waits for the batches that produced the slots and for the work queued on
 * `stream` before the call (dst may still be being read), writes dst (k_export_flows), and `stream` is made to wait for
 * that.  The export counts as a use of the slots: a later batch that recycles one of them waits for it on the device.
 * The host never waits. */
int ffl_export_flows(ffl_ctx *ctx, int n, const int *flow_slots, float *dst, int layout, ptrdiff_t item_stride_bytes,
                     uint64_t stream);

/* n flow fields in device memory, as the caller's flow estimator left them: item i, pixel (x, y), component c (0 = u,
 * 1 = v) is at  base + i*item_stride + y*row_pitch + x*pixel_stride + c*channel_stride  (bytes).  This covers (n, H, W, 2)
 * (cv2's layout), (n, 2, H, W), sliced views with a padded row pitch and channels-last views. */
typedef struct ffl_dev_flow {
    const void *base;
    ptrdiff_t item_stride, row_pitch, pixel_stride, channel_stride;
} ffl_dev_flow;
#define FFL_F32 0
#define FFL_F16 1  /* IEEE half */
#define FFL_BF16 2

/* The geometry rules of ffl_import_flows for n width x height fields.  Pure host check: no device or context needed.
 * FFL_ERR_INVALID with the rule in ffl_last_error(NULL): an unknown dtype; n < 1; a size outside 2..32768; a NULL base;
 * negative strides or strides beyond 2^40; misaligned: a base or stride that is not a multiple of the element size;
 * overlap: pixel stride < element size, row pitch < (width - 1) * pixel stride + element size (transposed views are
 * refused), or a channel stride that makes u and v overlap -- it must be interleaved (element size <= channel stride <=
 * pixel stride - element size), planar (>= the extent of one component plane) or row-planar (the v row after the u row,
 * inside the row pitch).  Items may be any non-negative distance apart. */
int ffl_dev_flow_check(int dtype, int n, int width, int height, const ffl_dev_flow *f);

/* n caller fields (dtype FFL_F32 / FFL_F16 / FFL_BF16, the context's size) -> flow slots flow_slots[0..n), as float32, and
 * their pass-1 records: ffl_upload_flow for every field at once, without the host.  Each record is bit-identical to
 * ffl_upload_flow's for the float32 widening of the field (the widening is exact); results, radial, export and download
 * then work on the slots as on any other.  pov_mode as in ffl_flow_pairs.  Refused before any device work, each with its
 * rule in ffl_last_error: n outside 1..max_batch; a slot out of range or repeated; any rule of ffl_dev_flow_check; memory
 * that is not device memory of the context's device, or an extent outside one allocation (page-locked host memory,
 * ffl_host_alloc's included, belongs to ffl_upload_flow); a capturing `stream` (FFL_ERR_STATE).
 * Stream contract (`stream` is a hipStream_t as an integer; 0 = the null stream):
 *   - a stream that is capturing a graph is refused with FFL_ERR_STATE; that check is the first HIP call made on it;
 *   - the fields are read after the work queued on `stream` before the call and after the slots' last users (a batch, a
 *     pass 2 or an export that still reads them), by ONE k_import_pass1 launch for all n fields;
 *   - the slots are published as ffl_upload_flow publishes its slot;
 *   - `stream` is made to wait for the launch: the caller may overwrite or free the sources straight after the call;
 *   - the host never waits for the device, except where settling the library's event ring makes every call wait.
 * Nothing of this call is ever captured into the library's graphs. */
int ffl_import_flows(ffl_ctx *ctx, int n, const int *flow_slots, const ffl_dev_flow *f, int dtype, int pov_mode,
                     uint64_t stream);

/* Page-locked host memory owned by the context (freed by ffl_host_free or ffl_destroy).  A decoder that writes its
 * frames into such a buffer saves the library's staging copy: ffl_upload_frame(s) of tightly packed frames that lie
 * back to back inside ONE ffl_host_alloc buffer start the H2D transfer straight out of it.  The caller must then
 * leave those bytes alone until the transfer is over -- after ffl_sync(), or once a result of a batch that uses
 * the frames has been read (ffl_pass1_result).  Frames anywhere else keep the copy-before-return contract.
 * (No counterpart in the reference, whose CUDA variant uploads out of pageable ndarrays, FF:986-987.) */
int ffl_host_alloc(ffl_ctx *ctx, size_t bytes, void **out);
int ffl_host_free(ffl_ctx *ctx, void *ptr);

/* Queue Farneback flow + pass-1 reductions for n pairs: pair i = (frame fslot0[i], frame fslot1[i])
 * -> flow slot flow_slots[i].  Frames shared between pairs of the batch are expanded once.
 * pov_mode != 0 skips the divergence argmax (FF:880-882).  Asynchronous. */
int ffl_flow_pairs(ffl_ctx *ctx, int n, const int *fslot0, const int *fslot1, const int *flow_slots, int pov_mode);

/* Wait for the batch that produced `flow_slot` and return its pass-1 record (FF:898-907):
 * (x, y) = pos_center, div_val = val_pos, mean_mag, cut = mean_mag > cut_threshold.
 * Non-finite fields follow np.argmax(np.abs(div)) (FF:756): (x, y) is the FIRST pixel in row-major order whose divergence
 * is NaN, whatever the NaN's payload or origin (an input NaN, inf - inf formed on the device); without a NaN it is the first
 * maximum of |div|, +inf included.  div_val is then NaN / +-inf.  A field with a NaN has mean_mag = NaN and cut = 0 (NaN >
 * threshold is false); ffl_radial of it is NaN, or 0.0 when called with is_cut. */
int ffl_pass1_result(ffl_ctx *ctx, int flow_slot, float cut_threshold, int32_t *x, int32_t *y, float *div_val,
                     float *mean_mag, int *cut);

/* The same for n slots with one call (arrays of n elements; any output array may be NULL). */
int ffl_pass1_results(ffl_ctx *ctx, int n, const int *flow_slots, float cut_threshold, int32_t *x, int32_t *y,
                      float *div_val, float *mean_mag, int *cut);

/* radial_motion_weighted for n resident flow fields (FF:761-785); out[i] is float64.
 * is_cut[i] != 0 yields 0.0 without touching the device.  Synchronous. */
int ffl_radial(ffl_ctx *ctx, int n, const int *flow_slots, const double *cx, const double *cy, const int *is_cut,
               int pov_mode, double *out);

/* One record of ffl_radial_window: what FF:1203-1236 yields for one pair.  48 bytes, 8-byte aligned. */
typedef struct ffl_pass2_record {
    double dot;                 /* radial_motion_weighted, FF:761-785; +0.0 when cut */
    double cx, cy;              /* the window mean of pos_center, FF:1203-1214 */
    float mean_mag, div_val;    /* as ffl_pass1_results */
    int32_t x, y;               /* pos_center */
    int32_t cut, pad;           /* mean_mag > cut_threshold; pad = 0 */
} ffl_pass2_record;

#define FFL_MAX_RADIUS 32   /* widest centre window of ffl_radial_window: 2 * 32 + 1 pairs */

/* The centre window, the cut test and pass 2 on the device, behind the batches, without the host: ffl_pass1_results, the
 * +-radius mean of FF:1203-1214 and ffl_radial in one call that only queues work.  seq_slots[0..n_seq) are the flow slots
 * of consecutive pairs in time order; items first .. first+n-1 of them are computed into out_dev[0..n).
 *   window   of item j: seq indices max(0, j - radius) .. min(n_seq - 1, j + radius).  It clips at the ends of seq, so a
 *            chunk edge is expressed by where seq starts and ends.  cx, cy = (double)(exact integer sum of pos_center) /
 *            (double)count: one IEEE division, np.mean's value.
 *   cut      mean_mag = (float)(mag_sum / (width * height)) and cut = mean_mag > cut_threshold, the expressions of
 *            ffl_pass1_results; a record with a NaN follows the rule above: cut = 0 and dot NaN.
 *   dot      the bits ffl_radial returns for the same slot, centre and pov_mode (the same kernel body and reduction
 *            order); a cut item gets +0.0 and none of its flow is read.
 * Refused before any device work, each with its rule in ffl_last_error: n outside 1..FFL_MAX_BATCH; n_seq outside
 * 1..FFL_MAX_BATCH + 2 * FFL_MAX_RADIUS; first < 0 or first + n > n_seq; radius outside 0..FFL_MAX_RADIUS; a slot out of
 * range or repeated; a seq slot that holds no result, or a computed slot that holds no flow (FFL_ERR_STATE); out_dev that is
 * not 8-byte aligned device memory of the context's device, or whose n records do not lie inside one allocation
 * (page-locked host memory, ffl_host_alloc's included, belongs to ffl_radial); a capturing `stream` (FFL_ERR_STATE).
 * Stream contract (`stream` is a hipStream_t as an integer; 0 = the null stream):
 *   - a stream that is capturing a graph is refused with FFL_ERR_STATE; that check is the first HIP call made on it;
 *   - the library's stream waits for the batch, import or upload that produced every seq slot and for the work queued on
 *     `stream` before the call (out_dev may still be being read), then writes out_dev with three launches (k_window_plan,
 *     k_strip_sums<RadialSums<..>>, k_radial_final), and `stream` is made to wait for that;
 *   - the call counts as a use of every seq slot, the neighbours whose records alone are read included: a later batch that
 *     recycles one of them waits for it on the device;
 *   - the host never waits for the device, except where settling the library's event ring makes every call wait.
 * Nothing of this call is ever captured into the library's graphs. */
int ffl_radial_window(ffl_ctx *ctx, int n_seq, const int *seq_slots, int first, int n, int radius, float cut_threshold,
                      int pov_mode, ffl_pass2_record *out_dev, uint64_t stream);

/* ---- The four motion components about the centre ----
 * Per pixel (x, y) of a field with flow (u, v), centre (cx, cy), dx = x - cx, dy = y - cy and the quadrant weights wx, wy
 * of radial_motion_weighted (both 1 in pov_mode), all in float64 without contraction:
 *   FFL_AXIS_RADIAL      ((u dx + v dy) wx) wy   ffl_radial's term: the bits of ffl_radial / ffl_radial_window
 *   FFL_AXIS_TANGENTIAL  ((v dx - u dy) wx) wy   > 0: clockwise on screen (x to the right, y down)
 *   FFL_AXIS_SHIFT_X     (u wx) wy
 *   FFL_AXIS_SHIFT_Y     (v wx) wy
 * each summed over the image in ffl_radial's order and divided once by (double)width * (double)height.  The weights are
 * the radial term's own and are not normalised by their sum, as the reference does not normalise its dot.  A cut item is
 * +0.0 in all four and none of its flow is read; a non-finite field gives each component the IEEE result of its own terms. */
#define FFL_AXIS_RADIAL 0
#define FFL_AXIS_TANGENTIAL 1
#define FFL_AXIS_SHIFT_X 2
#define FFL_AXIS_SHIFT_Y 3
#define FFL_N_AXES 4

/* One record of ffl_radial_window_axes.  80 bytes, 8-byte aligned. */
typedef struct ffl_axes_record {
    ffl_pass2_record base;      /* byte for byte what ffl_radial_window writes; base.dot = component FFL_AXIS_RADIAL */
    double tangential, shift_x, shift_y;   /* components 1..3, the bits of ffl_radial_axes at (base.cx, base.cy) */
    double reserved;            /* +0.0 */
} ffl_axes_record;

/* ffl_radial with four components per item: out[i * FFL_N_AXES + component], float64.  ffl_radial's contract otherwise:
 * the same arguments, refusals and locks, is_cut[i] != 0 yields four 0.0 without touching the device, synchronous, timed
 * under FFL_K_RADIAL.  The first four-component call of a context allocates what ffl_axes_extra_bytes reports. */
int ffl_radial_axes(ffl_ctx *ctx, int n, const int *flow_slots, const double *cx, const double *cy, const int *is_cut,
                    int pov_mode, double *out);

/* ffl_radial_window with ffl_axes_record records: the same windows, cut test, refusals (out_dev must hold n records of 80
 * bytes inside one allocation), stream contract and use of every seq slot; never captured, no host wait.  Its three
 * launches are k_window_plan and the four-component k_strip_sums<RadialSums<..>> and k_radial_final. */
int ffl_radial_window_axes(ffl_ctx *ctx, int n_seq, const int *seq_slots, int first, int n, int radius, float cut_threshold,
                           int pov_mode, ffl_axes_record *out_dev, uint64_t stream);

/* Device memory the four-component calls add to a context of this size, allocated by the first such call and freed by
 * ffl_destroy: FFL_N_AXES partial sums per workgroup of the radial grid for FFL_MAX_BATCH items (ffl_estimate_bytes does
 * not count it; 20 KiB of page-locked records come with it).  Needs no device. */
int ffl_axes_extra_bytes(int width, int height, size_t *bytes);

/* ---- Per-pixel weight maps for pass 1 and the four-component pass 2 ----
 * A map is height x width uint8 in device memory, the context's size; the pixels of a row are contiguous.  Item i of a
 * call uses the map at  base + i*item_stride + y*row_pitch + x  (bytes); item_stride == 0: one map for all items (a static
 * mask).  The flow itself is never touched.  The rules:
 *   W1  the weight of a pixel is wt = (double)W[y][x], an integer 0..255.  W == 0 excludes the pixel by a select, never by
 *       a multiplication: a NaN or inf in an excluded pixel's flow reaches no sum, key or record.  SW = sum of wt, exact.
 *   W2  the divergence at a pixel is the unweighted one, from the same neighbours whatever their weights; only the pixel's
 *       candidacy for the argmax needs W > 0.  Among candidates: the first NaN of |div| in row-major order, else the first
 *       maximum (ffl_pass1_result's rule).
 *   W3  mean_mag = (float)(sum of (double)mag * wt / SW), added in pass 1's order; cut = mean_mag > cut_threshold.
 *   W4  each of the four components is (sum of term * wt) / SW: term is exactly the unweighted ((...) wx) wy, multiplied
 *       once more by wt, added in ffl_radial's order and divided once by (double)SW.
 *   W5  an empty map (SW == 0): the pass-1 record is x = width / 2, y = height / 2, div_val = +0.0, mean_mag = +0.0, cut = 0;
 *       all four components are +0.0.  No division by zero is executed.
 *   W6  a cut item gets +0.0 in all four components; neither its flow nor its map is read.
 * An all-ones map gives the bits of the unweighted calls, in either pov_mode. */
typedef struct ffl_dev_weights {
    const void *base;
    ptrdiff_t item_stride, row_pitch;   /* bytes */
} ffl_dev_weights;

/* The geometry rules of a weight descriptor for n maps of width x height.  Pure host check: no device or context needed.
 * FFL_ERR_INVALID with the rule in ffl_last_error(NULL): a NULL descriptor or base; n < 1; a size outside 2..32768;
 * negative strides or strides beyond 2^40; overlap: row_pitch < width, or 0 < item_stride < (height - 1) * row_pitch +
 * width.  The maps span (n - 1) * item_stride + (height - 1) * row_pitch + width bytes from base. */
int ffl_dev_weights_check(int n, int width, int height, const ffl_dev_weights *w);

/* Recompute the pass-1 records of flow slots flow_slots[0..n) under the maps (rules W2, W3, W5); the flow is only read.  The
 * records replace the slots' records until a later writer of the slot (a batch, ffl_upload_flow, ffl_import_flows) puts
 * an ordinary record back; ffl_pass1_results and the window calls read whichever record the slot holds.  Refusals, stream
 * contract and publishing are ffl_import_flows': n outside 1..max_batch; a slot out of range or repeated; a slot that
 * holds no flow (FFL_ERR_STATE); any rule of ffl_dev_weights_check; maps that are not device memory of the context's
 * device or do not lie inside one allocation (page-locked host memory is refused); a capturing `stream` (FFL_ERR_STATE).
 * Queued on the library's stream behind the work queued on `stream` and the slots' last users -- one k_pass1_weighted
 * launch for all n items plus its final kernel -- and `stream` waits for it; never captured; the host does not wait.  The
 * first weighted call of a context allocates what ffl_weights_extra_bytes reports. */
int ffl_pass1_weighted(ffl_ctx *ctx, int n, const int *flow_slots, const ffl_dev_weights *w, int pov_mode, uint64_t stream);

/* ffl_radial_window_axes under rule W4: `w` describes the maps of the n computed items (item i of the call, seq index
 * first + i); neighbours contribute their records only.  Windows, the centre mean and the cut test are
 * ffl_radial_window's, from whatever records the seq slots hold -- normally those of ffl_pass1_weighted; unweighted ones
 * are allowed.  The same refusals and stream contract, plus the map rules of ffl_pass1_weighted; out_dev is checked
 * before the maps.  Its three launches are k_window_plan and the weighted k_strip_sums<RadialSums<..>> and k_radial_final. */
int ffl_radial_window_axes_weighted(ffl_ctx *ctx, int n_seq, const int *seq_slots, int first, int n, int radius,
                                    float cut_threshold, int pov_mode, const ffl_dev_weights *w, ffl_axes_record *out_dev,
                                    uint64_t stream);

/* Device memory the weighted calls add to a context of this size, allocated by the first such call and freed by
 * ffl_destroy: FFL_N_AXES + 1 partial sums per workgroup of the radial grid for FFL_MAX_BATCH items, which pass 1's one
 * extra partial per workgroup shares (ffl_estimate_bytes does not count it).  Needs no device. */
int ffl_weights_extra_bytes(int width, int height, size_t *bytes);

/* ---- Forward-backward consistency weight maps ----
 * A confidence map of the flow itself, made on the device in the form rules W1 to W6 consume: follow the forward flow F
 * (pair f0 -> f1, components u, v) from a pixel, read the backward flow B (pair f1 -> f0) there, and see whether the two
 * cancel.  Both fields are resident flow slots of the context's size w x h.  All arithmetic is float32, one rounding per
 * written operation, no contraction.  For pixel (x, y):
 *   K1  landing: px = (float)x + u, py = (float)y + v; inside = px >= 0 && px <= (float)(w-1) && py >= 0 && py <= (float)(h-1)
 *       (a NaN or inf fails the test).  Not inside: W = 0, and nothing of B is read for that pixel.
 *   K2  sample: x0 = (int)floorf(px), x1 = min(x0 + 1, w - 1), ax = px - floorf(px), the same in y.  Per component of B with
 *       corners b00 = B[y0][x0], b01 = B[y0][x1], b10 = B[y1][x0], b11 = B[y1][x1]:  t = b00 + ax*(b01 - b00),
 *       s = b10 + ax*(b11 - b10), bc = t + ay*(s - t); this yields bu, bv.
 *   K3  ex = u + bu, ey = v + bv, e2 = ex*ex + ey*ey;  thr = alpha*((u*u + v*v) + (bu*bu + bv*bv)) + beta.
 *   K4  soft = 1: q = 1 - e2 / thr; q = q > 0 ? q : 0 (a select: a NaN gives 0); W = (int)(q*255 + 0.5f).
 *   K5  soft = 0: W = e2 < thr ? 255 : 0.  No division is executed.
 *   K6  with a gate map S (a weight descriptor, the rules of any map): W = min(W, S).
 * Accepted: 0 <= alpha <= 1, 0 < beta <= 1e6, both finite, soft in {0, 1}; the defaults are 0.01, 0.5, 1.  Non-finite
 * fields follow the IEEE result of these expressions; a NaN anywhere in a pixel's chain gives 0. */
typedef struct ffl_consistency_params {
    float alpha, beta;
    int soft;
} ffl_consistency_params;
int ffl_consistency_default_params(ffl_consistency_params *out);
/* Pure host check: no device or context needed.  FFL_ERR_INVALID with the rule in ffl_last_error(NULL). */
int ffl_consistency_params_check(const ffl_consistency_params *p);

/* The maps of n pairs of fields: item i is made from the forward field in flow slot fwd_slots[i] and the backward field in
 * bwd_slots[i].  `out` describes the n maps the call WRITES (the descriptor type is reused: base is written through, byte
 * (x, y) of item i at base + i*item_stride + y*row_pitch + x; bytes between rows and items are left alone); `gate` (NULL: none)
 * the maps S of rule K6, item_stride 0 for one static gate; p NULL: the defaults.  Refused before any device work, each with
 * its rule in the message: n outside 1..max_batch; a NULL list; a slot out of range, or repeated among the 2n; a slot that
 * holds no flow (FFL_ERR_STATE); any rule of ffl_consistency_params_check; any rule of ffl_dev_weights_check for out and for
 * gate; out with item_stride == 0 when n > 1; out or gate that is not device memory of the context's device inside one
 * allocation; out overlapping gate; a capturing `stream` (FFL_ERR_STATE).
 * ffl_pass1_weighted's protocol: ONE k_consistency launch, queued on the library's stream behind the work queued on
 * `stream` and the last users of all 2n slots; `stream` then waits for it, so the maps may be read, and the gate
 * overwritten, on `stream` straight after the call; it counts as a use of all 2n slots; never captured; the host does not
 * wait.  Flows and pass-1 records are only read.  No scratch memory: there is no *_extra_bytes call. */
int ffl_consistency_weights(ffl_ctx *ctx, int n, const int *fwd_slots, const int *bwd_slots, const ffl_consistency_params *p,
                            const ffl_dev_weights *gate, const ffl_dev_weights *out, uint64_t stream);

/* ---- Photometric-residual weight maps ----
 * A second confidence map in the form rules W1 to W6 consume, which needs no backward field: follow the forward flow F (pair
 * f0 -> f1, components u, v) from a pixel of frame 0, sample frame 1 there bilinearly, and see how well the grey values agree,
 * measured against the local gradient of frame 0.  I0 and I1 are the uint8 gray operands in frame slots f0 and f1, F a
 * resident flow slot, all of the context's size w x h.  All arithmetic is float32 unless stated otherwise, one rounding per
 * written operation, no contraction; integer steps are exact.  For pixel (x, y):
 *   P1  landing: px = (float)x + u, py = (float)y + v; inside = px >= 0 && px <= (float)(w-1) && py >= 0 && py <= (float)(h-1)
 *       (a NaN or inf fails the test).  Not inside: W = 0, and nothing of I1 is read for that pixel.
 *   P2  sample: x0 = (int)floorf(px), x1 = min(x0 + 1, w - 1), ax = px - floorf(px), the same in y.  The corners
 *       i00 = I1[y0][x0], i01 = I1[y0][x1], i10 = I1[y1][x0], i11 = I1[y1][x1] are converted to float exactly;
 *       t = i00 + ax*(i01 - i00), s = i10 + ax*(i11 - i10), ic = t + ay*(s - t).
 *   P3  a = fabsf(ic - (float)I0[y][x]);  gx = I0[y][min(x+1,w-1)] - I0[y][max(x-1,0)] and
 *       gy = I0[min(y+1,h-1)][x] - I0[max(y-1,0)][x], both as integers;  g = fabsf((float)gx) + fabsf((float)gy);
 *       thr = alpha*g + beta.
 *   P4  soft = 1: q = 1 - a / thr; q = q > 0 ? q : 0 (a select: a NaN gives 0); W = (int)(q*255 + 0.5f).
 *   P5  soft = 0: W = a < thr ? 255 : 0.  No division is executed.
 *   P6  with a gate map S (a weight descriptor, the rules of any map): W = min(W, S).
 * Accepted: 0 <= alpha <= 16, 0 < beta <= 255, both finite, soft in {0, 1}; the defaults are 0.5, 4, 1.  The defaults are
 * the project's own choice and are NOT tuned on footage.  Non-finite fields follow the IEEE result of these expressions. */
typedef struct ffl_residual_params {
    float alpha, beta;
    int soft;
} ffl_residual_params;
int ffl_residual_default_params(ffl_residual_params *out);
/* Pure host check: no device or context needed.  FFL_ERR_INVALID with the rule in ffl_last_error(NULL). */
int ffl_residual_params_check(const ffl_residual_params *p);

/* The maps of n pairs: item i is made from the frames in frame slots fslot0[i] and fslot1[i] and the forward field in flow slot
 * flow_slots[i].  `out`, `gate` and p are ffl_consistency_weights' (gate: the maps S of rule P6).  Refused before any device
 * work, each with its rule in the message: n outside 1..max_batch; a NULL list; a flow slot out of range or repeated, or one
 * that holds no flow (FFL_ERR_STATE); a frame slot out of range, or one that was never uploaded (FFL_ERR_STATE) -- frame slots
 * MAY repeat between items (frame j+1 of pair j is frame j of pair j+1); any rule of ffl_residual_params_check; any rule of
 * ffl_dev_weights_check for out and for gate; out with item_stride == 0 when n > 1; out or gate that is not device memory of
 * the context's device inside one allocation; out overlapping gate; a capturing `stream` (FFL_ERR_STATE).
 * ffl_consistency_weights' protocol: ONE k_residual launch, queued on the library's stream behind the work queued on `stream`,
 * the uploads that filled the frame slots and the last users of the n flow slots; `stream` then waits for it, so the maps may
 * be read, and the gate overwritten, on `stream` straight after the call; never captured; the host does not wait.  It counts
 * as a use of the n flow slots AND of the frame slots it reads: a later upload into one of those frame slots is ordered behind
 * it, as behind a flow call.  Frames, flows and pass-1 records are only read.  No scratch memory: there is no *_extra_bytes
 * call. */
int ffl_residual_weights(ffl_ctx *ctx, int n, const int *fslot0, const int *fslot1, const int *flow_slots,
                         const ffl_residual_params *p, const ffl_dev_weights *gate, const ffl_dev_weights *out, uint64_t stream);

/* ---- Texture (structure-tensor) weight maps ----
 * A third confidence map in the form rules W1 to W6 consume, which needs no flow at all: the local structure tensor of one
 * frame.  A flat region matches itself at any displacement and an edge or stripe pattern pins one flow component only (the
 * aperture problem); the consistency and the residual check approve of both, this map does not.  I is the uint8 gray operand
 * in one frame slot, of the context's size w x h.  All integer steps are exact; the float64 steps round once per written
 * operation, left to right, no contraction.  For pixel (x, y):
 *   T1  gradients, rule P3's clamped central differences, as integers:
 *       gx = I[y][min(x+1,w-1)] - I[y][max(x-1,0)],  gy = I[min(y+1,h-1)][x] - I[max(y-1,0)][x].
 *   T2  window sums Sxx = sum gx*gx, Sxy = sum gx*gy, Syy = sum gy*gy over the (2r+1)^2 offsets (i, j), |i|, |j| <= r, the
 *       gradient taken AT the clamped position (min(max(x+i,0),w-1), min(max(y+j,0),h-1)); N = (2r+1)^2 always.  The sums fit
 *       int32 (r = 8: at most 289 * 65025 = 18 792 225) and, being integers, have no order.
 *   T3  tr = Sxx + Syy (int32); det = Sxx*Syy - Sxy*Sxy in 64-BIT integers (>= 0 by Cauchy-Schwarz, at most 3.6e14 < 2^53,
 *       hence exact as a double).  tr == 0: c = 0 and no division is executed; otherwise c = (double)det / (double)tr, one IEEE
 *       division.  This is Noble's measure l1*l2 / (l1 + l2) of the tensor's eigenvalues: between lmin/2 and lmin, 0 for a
 *       flat patch and for a pure stripe pattern, no square root.
 *   T4  soft = 1: tn = (double)tau * (double)N; q = c / tn; q = q < 1.0 ? q : 1.0; W = (int)(q*255.0 + 0.5).
 *   T5  soft = 0: W = tr != 0 && (double)det >= tn * (double)tr ? 255 : 0.  No division is executed.
 *   T6  with a gate map S (a weight descriptor, the rules of any map): W = min(W, S).
 * Accepted: radius 1..8, 0 < tau <= 65025 and finite, soft in {0, 1}; the defaults are 7, 16, 1: the 15 x 15 window the
 * default Farneback call averages over at level 0, and about fifteen times the c / N that sensor noise of sigma 1 produces
 * (about 1.1).  The defaults are the project's own choice and are NOT tuned on footage. */
typedef struct ffl_texture_params {
    int radius;
    float tau;
    int soft;
} ffl_texture_params;
int ffl_texture_default_params(ffl_texture_params *out);
/* Pure host check: no device or context needed.  FFL_ERR_INVALID with the rule in ffl_last_error(NULL). */
int ffl_texture_params_check(const ffl_texture_params *p);

/* The maps of n frames: item i is the map of the frame in frame slot fslots[i] -- for a pair that is its frame 0, on whose
 * pixels the flow is defined.  No flow slot is involved.  `out`, `gate` and p are ffl_residual_weights' (gate: the maps S of
 * rule T6).  Refused before any device work, each with its rule in the message: n outside 1..max_batch; a NULL list; a frame
 * slot out of range, or one that was never uploaded (FFL_ERR_STATE) -- frame slots MAY repeat between items; any rule of
 * ffl_texture_params_check; any rule of ffl_dev_weights_check for out and for gate; out with item_stride == 0 when n > 1; out or
 * gate that is not device memory of the context's device inside one allocation; a capturing `stream` (FFL_ERR_STATE); out
 * overlapping gate -- with ONE exception: gate may be EXACTLY out (the same base, item stride and row pitch).  The call then
 * min-combines the texture into maps that are already there, in place: every byte is read and written by the lane that owns
 * the pixel.  ffl_residual_weights' protocol: ONE k_texture launch, queued on the library's stream behind the work queued on
 * `stream` and the uploads that filled the frame slots; `stream` then waits for it, so the maps may be read, and the gate
 * overwritten, on `stream` straight after the call; never captured; the host does not wait.  It counts as a reader of the frame
 * slots: a later upload into one of them is ordered behind it, as behind a flow call.  Frames are only read.  No scratch
 * memory: there is no *_extra_bytes call. */
int ffl_texture_weights(ffl_ctx *ctx, int n, const int *fslots, const ffl_texture_params *p, const ffl_dev_weights *gate,
                        const ffl_dev_weights *out, uint64_t stream);

/* ---- Per-cell flow statistics and the variance centre ----
 * center_of_mass_variance(flow, num_cells) of FF:721-746 and the grid it is formed from, on resident flow fields.  With
 * G = cells, gh = height / G and gw = width / G (integer divisions), cell (i, j) is rows i*gh .. (i+1)*gh-1 and columns
 * j*gw .. (j+1)*gw-1, the reference's slicing at FF:728-735; pixels at x >= G*gw or y >= G*gh belong to no cell and are
 * never read.  The rules:
 *   G1  1 <= G <= FFL_MAX_CELLS and G <= min(width, height).
 *   G2  per pixel m = sqrtf(u*u + v*v) in float32; K = m of the cell's top-left pixel; d = (double)m - (double)K; the cell
 *       sums S_u, S_v, S_d and S_dd = sum of d*d are float64.
 *   G3  a column of a cell is summed top to bottom; the columns of a cell inside one absolute 256-column block (x / 256)
 *       left to right into a block partial; a cell's block partials in ascending block order.  Every sum starts at +0.0.
 *   G4  with n = (double)(gh*gw): mean_u = S_u / n, mean_v = S_v / n, mean_mag = K + S_d / n, var_mag = (S_dd - S_d*S_d / n)
 *       / n, a result < 0 replaced by +0.0 (a NaN stays a NaN); a constant cell has var_mag = +0.0 exactly.
 *   G5  per cell row i, over j in order: t_i = sum var, x_i = sum (double)j*var; then over i in order T = sum t_i, X = sum
 *       x_i, Y = sum (double)i*t_i.  T == 0: cx = width / 2, cy = height / 2 (integer divisions), empty = 1 (FF:741-742);
 *       else cx = X*gw / T + gw / 2.0, cy = Y*gh / T + gh / 2.0, left to right (FF:744-745), empty = 0.  A NaN T gives NaN
 *       centres.
 *   G6  the window of ffl_radial_window_axes_centres over caller centres c[0..n_seq): acc = c[j]; for i = 1..radius: c[j-i] is
 *       added if j-i >= 0, then c[j+i] if j+i < n_seq; the centre is acc / (double)count, x and y separately -- np.mean(
 *       center_list, axis=0) of FF:1205-1213 in the order numpy adds the rows. */
#define FFL_MAX_CELLS 64
typedef struct ffl_cell_record {   /* 32 bytes; rule G4 */
    double mean_u, mean_v, mean_mag, var_mag;
} ffl_cell_record;
typedef struct ffl_grid_centre {   /* 32 bytes; rule G5.  total_var = T */
    double cx, cy, total_var;
    int32_t cells, empty;
} ffl_grid_centre;

/* Rule G1 for a width x height frame, and the cell size (either pointer may be NULL).  Pure host check: no device or
 * context needed.  FFL_ERR_INVALID with the rule in ffl_last_error(NULL). */
int ffl_cell_grid_check(int width, int height, int cells, int *cell_w, int *cell_h);

/* The cells x cells grid of flow slots flow_slots[0..n) (FF:728-737) and / or its centre of mass (FF:739-746).  cells_dev:
 * n * cells * cells records, item-major then row-major, or NULL; centres_dev: n records, or NULL; not both NULL.  The flow
 * is only read and no pass-1 record is touched.  Refused before any device work, each with its rule in the message: n
 * outside 1..max_batch; a slot out of range or repeated; a slot that holds no flow (FFL_ERR_STATE); cells outside rule G1;
 * both outputs NULL; an output that is not 8-byte aligned device memory of the context's device inside one allocation
 * (page-locked host memory is refused); a capturing `stream` (FFL_ERR_STATE).  Queued on the library's stream behind the
 * work queued on `stream` and the slots' last writers -- k_cell_stats for all n items, then k_grid_centre -- and `stream`
 * waits for it; it counts as a use of the slots; never captured; the host does not wait.  The first call of a context
 * allocates what ffl_cells_extra_bytes reports. */
int ffl_cell_stats(ffl_ctx *ctx, int n, const int *flow_slots, int cells, ffl_cell_record *cells_dev,
                   ffl_grid_centre *centres_dev, uint64_t stream);

/* ffl_radial_window_axes about caller centres (FF:1203-1214 with another centre estimator): entry k of centres_dev, two
 * doubles (cx, cy) at centres_dev + k * centre_stride_bytes, is the centre of seq item k, for all n_seq of them; the
 * window mean is rule G6.  A stride of 32 reads ffl_grid_centre records as ffl_cell_stats left them, a stride of 16 a plain
 * (n_seq, 2) float64 array.  mean_mag, cut, x, y and div_val of the records still come from the slots' pass-1 records;
 * the four components, the cut rule and the stream contract are ffl_radial_window_axes'.  Further refusals: a NULL or
 * misaligned centres_dev; a stride below 16 or no multiple of 8; centres that are not device memory of the context's
 * device inside one allocation over (n_seq - 1) * stride + 16 bytes (page-locked host memory is refused); out_dev is
 * checked before the centres.  Its three launches are k_window_plan over the centres and the four-component
 * k_strip_sums<RadialSums<..>> and k_radial_final. */
int ffl_radial_window_axes_centres(ffl_ctx *ctx, int n_seq, const int *seq_slots, int first, int n, int radius,
                                   float cut_threshold, int pov_mode, const void *centres_dev, ptrdiff_t centre_stride_bytes,
                                   ffl_axes_record *out_dev, uint64_t stream);

/* Device memory ffl_cell_stats adds to a context, allocated by its first call and freed by ffl_destroy: the two row sums
 * of rule G5 for FFL_MAX_CELLS rows of FFL_MAX_BATCH items (256 KiB whatever the size and the grid; the cell sums
 * themselves stay in LDS; ffl_estimate_bytes does not count it).  Needs no device. */
int ffl_cells_extra_bytes(int width, int height, int cells, size_t *bytes);

/* ---- Region tracking through the flow and ROI maps (appendices Q and E) ----
 * The argmax of pass 1 and the variance centre are found afresh for every pair and have no memory.  ffl_track_advance is the
 * estimator with one: it advects caller-chosen points through the flow fields of n consecutive pairs, in time order, and its
 * records are rule G6's centres.  The rules are the project's own (the reference has no such function).  For a context of
 * w x h; all arithmetic is float64, one rounding per written operation, left to right, no contraction; u, v widen exactly.
 *   Q1  sanitise: on load, each of x, home_x becomes c >= 0 ? (c <= w-1 ? c : w-1) : 0, and y, home_y likewise with h-1.
 *       Both steps are selects, so a NaN becomes 0: any bit pattern in caller memory gives an in-range anchor, and the kernel
 *       reads nothing outside a field whatever the state holds.
 *   Q2  window: ix = (int)floor(x + 0.5), iy alike.  Members are the pixels of columns max(ix-r, 0) .. min(ix+r, w-1) and
 *       rows max(iy-r, 0) .. min(iy+r, h-1): clipped, not clamped -- a pixel outside the image is no member.
 *   Q3  member weight: wt = 1.0 without a map, (double)W[y][x] with one (rule W1).  A member is dropped by a select when
 *       W == 0 or !(fabsf(u) <= FLT_MAX && fabsf(v) <= FLT_MAX) (rule C3's test): nothing of it reaches a sum.
 *   Q4  sums, each starting at +0.0.  Per window column, rows top to bottom: cS += wt; cU += wt*(double)u; cV += wt*(double)v.
 *       The column sums are then added left to right into S, U, V.  count is the number of kept members.
 *   Q5  cut: mean_mag is ffl_pass1_results' expression on the record the slot holds when the call runs;
 *       cut = mean_mag > cut_threshold.  A NaN is no cut, and a threshold of +inf never cuts.
 *   Q6  step.  Cut: du = dv = +0.0, sw = +0.0, count = 0, status gets CUT, and none of the item's flow or map is read.
 *       Otherwise, if S == 0: du = dv = +0.0, status gets LOST, lost_run += 1, and no division is executed.  Otherwise
 *       du = U / S, dv = V / S, lost_run = 0.  (lost_run and steps wrap as two's complement.)
 *   Q7  record (i, t) holds the sanitised position BEFORE the step -- the track's place in frame 0 of pair i, on whose pixels
 *       the field is defined, hence the centre for that pair's radial terms -- and du, dv, sw = S, count and status.
 *   Q8  move.  Cut with on_cut == FFL_TRACK_HOME: the position becomes (home_x, home_y).  Otherwise x' = x + du, y' = y + dv,
 *       each passed through Q1's select; a select whose result does not equal its operand sets CLAMPED in this item's status.
 *       In every case steps += 1.
 *   Q9  chaining and independence: one call of n items is, bit for bit, any split into consecutive calls that hand the state
 *       on; track t's records do not depend on n_tracks or on the other tracks.
 * Accepted: radius 1..FFL_MAX_TRACK_RADIUS, on_cut FFL_TRACK_HOLD or FFL_TRACK_HOME, a cut_threshold that is not NaN.  The
 * defaults are 12, HOLD and 7.0f (the reference's cut threshold, FF:876); the radius is the project's own choice and is NOT
 * tuned on footage.  Integrating a flow drifts: ffl_track_template and ffl_track_match below (appendix N) pull a track back
 * onto the appearance it started from, in place; choosing the start point, and re-capturing a template after a scene cut,
 * stay the caller's, which is why the state lives in caller memory. */
enum { FFL_MAX_TRACKS = 8, FFL_MAX_TRACK_RADIUS = 32 };
enum { FFL_TRACK_HOLD = 0, FFL_TRACK_HOME = 1 };                                            /* on_cut */
enum { FFL_TRACK_OK = 0, FFL_TRACK_CUT = 1, FFL_TRACK_LOST = 2, FFL_TRACK_CLAMPED = 4 };    /* status bits */
typedef struct ffl_track_params {
    int radius, on_cut;
    float cut_threshold;
} ffl_track_params;
typedef struct ffl_track_state {    /* 48 bytes; one per track, in device memory, read and written by every call */
    double x, y, home_x, home_y;
    int64_t steps;
    int32_t lost_run, pad;
} ffl_track_state;
typedef struct ffl_track_record {   /* 48 bytes; rule Q7.  Its head (x, y) is a centre of rule G6 / E1 */
    double x, y, du, dv, sw;
    int32_t count, status;
} ffl_track_record;
int ffl_track_default_params(ffl_track_params *out);
/* Pure host check: no device or context needed.  FFL_ERR_INVALID with the rule in ffl_last_error(NULL). */
int ffl_track_params_check(const ffl_track_params *p);

/* n_tracks points through the fields in flow slots seq_slots[0..n), in that order.  p NULL: the defaults.  weights: the maps
 * of the n items (rule Q3), or NULL.  state_dev: n_tracks states.  out_dev: n * n_tracks records, record (i, t) at index
 * i * n_tracks + t, so that a stride of 48 * n_tracks bytes reads one track.  Refused before any device work, each with its
 * rule in the message: n outside 1..max_batch or n_tracks outside 1..FFL_MAX_TRACKS; a NULL list; a slot out of range or
 * repeated; a slot that holds no flow (FFL_ERR_STATE); any rule of ffl_track_params_check; any rule of ffl_dev_weights_check
 * for the maps; state_dev or out_dev that is NULL, not 8-byte aligned or, like the maps, not device memory of the context's
 * device inside one allocation (page-locked host memory is refused); state_dev overlapping out_dev; a capturing `stream`
 * (FFL_ERR_STATE).  ffl_cell_stats' protocol: ONE k_track launch of n_tracks workgroups, queued on the library's stream
 * behind the work queued on `stream` and the slots' last writers; `stream` then waits for it; it counts as a use of the
 * slots; never captured; the host does not wait.  No scratch memory: there is no *_extra_bytes call. */
int ffl_track_advance(ffl_ctx *ctx, int n, const int *seq_slots, int n_tracks, const ffl_track_params *p,
                      const ffl_dev_weights *weights, ffl_track_state *state_dev, ffl_track_record *out_dev, uint64_t stream);

/* An elliptical weight map per item about a centre read from device memory, in the form rules W1 to W6 consume: it says
 * which pixels are the SUBJECT, where the maps of sections 16, 18, 21 and 22 say which are reliable.  Float64, one rounding
 * per written operation, no contraction.  For item i and pixel (x, y):
 *   E1  the centre (cx, cy) is two doubles at centres_dev + i * centre_stride_bytes; the stride is a multiple of 8 and at
 *       least 16: 48 * n_tracks reads one track's ffl_track_records, 32 ffl_grid_centre, 16 a plain (n, 2) array.
 *   E2  dx = ((double)x - cx) / (double)ax, dy = ((double)y - cy) / (double)ay, e = dx*dx + dy*dy.
 *   E3  soft = 1: q = 1.0 - e; q = q > 0.0 ? q : 0.0; W = (int)(q*255.0 + 0.5).  The second step is a select, so a NaN centre
 *       gives an all-zero map.
 *   E4  soft = 0: W = e <= 1.0 ? 255 : 0.
 *   E5  with a gate map S: W = min(W, S).
 * Accepted: 0.5 <= ax, ay <= 32768 and finite, soft in {0, 1}; the defaults are 48, 48, 1, the project's own choice and NOT
 * tuned on footage. */
typedef struct ffl_roi_params {
    float ax, ay;
    int soft;
} ffl_roi_params;
int ffl_roi_default_params(ffl_roi_params *out);
/* Pure host check: no device or context needed.  FFL_ERR_INVALID with the rule in ffl_last_error(NULL). */
int ffl_roi_params_check(const ffl_roi_params *p);

/* The maps of n items.  `out`, `gate` and the in-place exception (gate EXACTLY out) are ffl_texture_weights'; bytes between
 * rows and between items are left alone.  Refused before any device work, each with its rule in the message: n outside
 * 1..max_batch; any rule of ffl_roi_params_check; any rule of ffl_dev_weights_check for out and for gate; out with
 * item_stride == 0 when n > 1; out overlapping gate unless gate is exactly out; a NULL or misaligned centres_dev; a stride
 * below 16 or no multiple of 8; centres overlapping out; out, gate or the centres, over (n - 1) * stride + 16 bytes, that
 * are not device memory of the context's device inside one allocation; a capturing `stream` (FFL_ERR_STATE).
 * ffl_texture_weights' protocol without frame slots: ONE k_roi_weights launch, queued on the library's stream behind the
 * work queued on `stream`; `stream` then waits for it; never captured; the host does not wait.  It names no slot. */
int ffl_roi_weights(ffl_ctx *ctx, int n, const void *centres_dev, ptrdiff_t centre_stride_bytes, const ffl_roi_params *p,
                    const ffl_dev_weights *gate, const ffl_dev_weights *out, uint64_t stream);

/* The fifth window form: rule W4's terms about rule G6's centres -- ffl_radial_window_axes_weighted with the centres of
 * ffl_radial_window_axes_centres.  out_dev is checked first, then the maps, then the centres.  Its launches are
 * k_window_plan over the centres and the weighted four-component pair; no new kernel body.  An all-ones map gives the bits
 * of ffl_radial_window_axes_centres. */
int ffl_radial_window_axes_weighted_centres(ffl_ctx *ctx, int n_seq, const int *seq_slots, int first, int n, int radius,
                                            float cut_threshold, int pov_mode, const ffl_dev_weights *w,
                                            const void *centres_dev, ptrdiff_t centre_stride_bytes, ffl_axes_record *out_dev,
                                            uint64_t stream);

/* ---- Template-matching drift correction for tracked regions ----
 * ffl_track_advance integrates the flow, and a sub-pixel bias of the flow accumulates.  ffl_track_match searches the gray
 * frame in a frame slot for a template captured about the track (ffl_track_template) and overwrites the centre in place, so
 * that everything that reads centres from device memory (ffl_roi_weights, the *_centres window forms, the next
 * ffl_track_advance) reads corrected ones.  The rules are the project's own (the reference has no such function) and are
 * integer-exact: costs are integers, so there is no order of summation.  For a context of w x h: I is the uint8 gray operand
 * in a frame slot; Tm is track t's template, (2p+1)^2 uint8, row-major and tight, at templates_dev + t * (2p+1)^2;
 * N = (2p+1)^2.
 *   N1  anchor: the centre of (item i, track t) is two doubles at centres_dev + i * centre_stride_bytes + t * 48.  It passes
 *       through rule Q1's selects (any bit pattern is safe), and (ix, iy) is rule Q2's rounding, floor(c + 0.5).
 *   N2  samples: for candidate (dx, dy), |dx|, |dy| <= s, and template pixel (i, j) in 0..2p:
 *       d = I[clamp(iy+dy+j-p, 0, h-1)][clamp(ix+dx+i-p, 0, w-1)] - Tm[j][i], an integer.  Coordinates are clamped, never
 *       clipped; nothing outside the frame is read.
 *   N3  cost: S1 = sum d, S2 = sum d^2 in int32 (at p = 16 at most 277695 and 70812225).  FFL_MATCH_SSD: cost = N * S2.
 *       FFL_MATCH_ZSSD: cost = N * S2 - S1^2, which is >= 0 and invariant to a brightness offset.  Both in int64.
 *   N4  best: the lexicographic minimum of (cost, dx^2 + dy^2, dy, dx): on exact ties the smallest move wins, and an
 *       all-equal surface gives (0, 0).
 *   N5  runner-up: second = the minimum cost over candidates with max(|dx - bdx|, |dy - bdy|) > 1; if there are none (s = 1
 *       with the best at the centre) second = -1 and N6's ambiguity test is skipped.
 *   N6  verdict, float64, one rounding per written operation, left to right:
 *       FLAT       if (double)(N * sum Tm^2 - (sum Tm)^2) < min_var * (double)N * (double)N   (the sums in int64);
 *       POOR       if (double)cost > max_mse * (double)N * (double)N;
 *       AMBIGUOUS  if second >= 0 && (double)cost > ratio * (double)second.
 *       A match is accepted iff status == 0.  The cost surface is always evaluated: records are complete whatever the verdict.
 *   N7  record (i, t), at index i * n_tracks + t: x, y = ((double)(ix + bdx), (double)(iy + bdy)) through Q1's selects when
 *       accepted, else the sanitised centre unchanged; dx, dy the best offset, also when rejected; cost, second; status;
 *       pad = 0.  Its head is again a centre of rule G6 / E1.
 *   N8  write-back: with write_back = 1 an accepted match also stores x, y into the two doubles the centre was read from.  A
 *       rejected one stores nothing, not even the sanitised value.
 *   N9  independence: record (i, t) depends on item i's frame, track t's template and that one centre only.
 *   N10 capture: Tm[j][i] = I[clamp(iy+j-p, 0, h-1)][clamp(ix+i-p, 0, w-1)] about the anchor of rule N1.
 * Accepted: p 1..FFL_MAX_MATCH_P, s 1..FFL_MAX_MATCH_S, mode FFL_MATCH_SSD or FFL_MATCH_ZSSD, 0 <= min_var, 0 <= max_mse <=
 * 65025, 0 < ratio <= 1, all finite.  The defaults are 8, 8, ZSSD, 25, 400 and 0.8: the project's own choice, NOT tuned on
 * footage.  After a scene cut the template is stale: matches then read POOR and the track falls back to pure advection;
 * re-capture (ffl_track_template) is the caller's. */
enum { FFL_MAX_MATCH_P = 16, FFL_MAX_MATCH_S = 16 };
enum { FFL_MATCH_SSD = 0, FFL_MATCH_ZSSD = 1 };                                   /* mode */
enum { FFL_MATCH_FLAT = 1, FFL_MATCH_POOR = 2, FFL_MATCH_AMBIGUOUS = 4 };         /* status bits; 0: accepted */
typedef struct ffl_match_params {
    int p, s, mode, reserved;   /* reserved: not read */
    double min_var, max_mse, ratio;
} ffl_match_params;
typedef struct ffl_match_record {   /* 48 bytes; rule N7.  Its head (x, y) is a centre of rule G6 / E1 */
    double x, y;
    int32_t dx, dy;
    int64_t cost, second;
    int32_t status, pad;
} ffl_match_record;
int ffl_match_default_params(ffl_match_params *out);
/* Pure host check: no device or context needed.  FFL_ERR_INVALID with the rule in ffl_last_error(NULL). */
int ffl_match_params_check(const ffl_match_params *p);

/* n_tracks templates of (2p+1)^2 bytes out of frame slot fslot (rule N10): track t's centre is the two doubles at
 * centres_dev + t * 48, so an ffl_track_state array, or one item's ffl_track_records, is a valid argument.  Refused before
 * any device work, each with its rule in the message: n_tracks outside 1..FFL_MAX_TRACKS; a frame slot out of range, or never
 * uploaded (FFL_ERR_STATE); p outside 1..FFL_MAX_MATCH_P; a NULL pointer; a centres_dev that is not 8-byte aligned; the
 * centres (48 * (n_tracks - 1) + 16 bytes) or the templates (n_tracks * (2p+1)^2 bytes) that are not device memory of the
 * context's device inside one allocation, or that overlap; a capturing `stream` (FFL_ERR_STATE).  ffl_texture_weights'
 * protocol: ONE k_track_template launch, queued on the library's stream behind the work queued on `stream` and the upload that
 * filled the frame slot; `stream` then waits for it; it counts as a reader of the frame slot; never captured; the host does
 * not wait.  No scratch memory. */
int ffl_track_template(ffl_ctx *ctx, int fslot, int n_tracks, const void *centres_dev, int p, void *templates_dev,
                       uint64_t stream);

/* Item i searches frame slot fslots[i] (slots may repeat) for each of the n_tracks templates about its centre (rules N1 to
 * N9); p NULL: the defaults.  With n = 1, centres_dev = a state array, centre_stride_bytes = 48 * n_tracks and write_back = 1
 * the call corrects a track state in place; with centres_dev = a batch's track records (the same stride) it corrects the
 * centres that ffl_roi_weights and the window calls read afterwards.  Refused before any device work, each with its rule in
 * the message: n outside 1..max_batch or n_tracks outside 1..FFL_MAX_TRACKS; a NULL list; a frame slot out of range, or never
 * uploaded (FFL_ERR_STATE); any rule of ffl_match_params_check; a write_back that is not 0 or 1; a NULL pointer; centres_dev
 * or out_dev that is not 8-byte aligned; a stride that is no multiple of 8 or below 48 * (n_tracks - 1) + 16; any overlap
 * among the templates, the centres ((n - 1) * stride + 48 * (n_tracks - 1) + 16 bytes) and out_dev (n * n_tracks records);
 * any of the three that is not device memory of the context's device inside one allocation; a capturing `stream`
 * (FFL_ERR_STATE).  ffl_texture_weights' protocol: ONE k_track_match launch of (n_tracks, n) workgroups, queued on the
 * library's stream behind the work queued on `stream` and the uploads that filled the frame slots; `stream` then waits for
 * it; it counts as a reader of the frame slots; never captured; the host does not wait.  No scratch memory. */
int ffl_track_match(ffl_ctx *ctx, int n, const int *fslots, int n_tracks, const ffl_match_params *p, const void *templates_dev,
                    void *centres_dev, ptrdiff_t centre_stride_bytes, int write_back, ffl_match_record *out_dev,
                    uint64_t stream);

/* ---- Whole-frame template re-detection for tracked regions ----
 * ffl_track_match searches +-s <= 16 pixels about the advected centre.  Once the subject is further away than that (an
 * occlusion, a fast move the flow under-reads, a few POOR batches of pure advection) every local search reads POOR and the
 * track is gone.  ffl_track_redetect searches a whole frame, or a wide reach about the centre, for a track's template, decides
 * on the device and writes the centre back there; a trigger word per search, in device memory, says whether it runs at all,
 * so that the call can be queued behind every ffl_track_match without the host ever reading a status.  The rules are the
 * project's own and integer-exact; they reuse N1 to N3 and N6's thresholds.  I, Tm and N = (2p+1)^2 are appendix N's.
 *   L1  anchor and trigger: the centre of (item i, track t) is N1's: two doubles at centres_dev + i * centre_stride_bytes +
 *       t * 48, through Q1's selects and Q2's rounding to (ix, iy).  With a non-NULL trigger_dev the int32 word at trigger_dev
 *       + i * trigger_stride_bytes + t * 48 is read, and the search runs iff (word & trigger_mask) != 0; with NULL it always
 *       runs.  The `status` field of an ffl_match_record array (byte 40 of a 48-byte record) is the intended trigger.  A search
 *       that does not run writes the record of L7 with status FFL_REDETECT_SKIPPED, reads no frame byte and stores no centre.
 *   L2  candidates: all integer (cx, cy) with 0 <= cx < w, 0 <= cy < h and, when reach > 0, |cx - ix| <= reach and
 *       |cy - iy| <= reach.  reach = 0: the whole frame.  The set is never empty: the anchor lies in the frame.
 *   L3  samples and cost: N2 about the candidate, d = I[clamp(cy+j-p, 0, h-1)][clamp(cx+i-p, 0, w-1)] - Tm[j][i] (the frame
 *       edge-padded by p; clamped, never clipped); the cost is N3's: S1, S2 in int32, SSD N * S2 or ZSSD N * S2 - S1^2 in int64.
 *   L4  best: the lexicographic minimum of (cost, cy, cx): on exact ties the first candidate in row-major order wins.
 *   L5  runner-up: second = the minimum cost over candidates with max(|cx - bx|, |cy - by|) > exclude; -1 if there are none.
 *   L6  verdict, float64, one rounding per written operation, left to right: FLAT and POOR exactly N6's; AMBIGUOUS if
 *       second >= 0 && (double)cost >= ratio * (double)second.  The >= is deliberate and differs from N6: two exact copies of
 *       the template (cost 0 against second 0) must not be accepted silently by a global search.  Accepted iff status == 0.
 *   L7  record (i, t), an ffl_match_record at index i * n_tracks + t: x, y = ((double)bx, (double)by) through Q1's selects
 *       when accepted, else the sanitised centre; dx = bx - ix, dy = by - iy, also when rejected; cost, second, status;
 *       pad = 0.  Skipped (L1): x, y the sanitised centre, dx = dy = 0, cost = second = -1, status 8.
 *   L8  write-back: as N8.  With write_back = 1 an accepted search stores x, y into the two doubles it read; anything else
 *       stores nothing.
 *   L9  independence: record (i, t) depends on item i's frame, track t's template, that one centre and that one trigger
 *       word only.
 * Accepted: p 1..FFL_MAX_MATCH_P, mode FFL_MATCH_SSD or FFL_MATCH_ZSSD, exclude 1..FFL_MAX_REDETECT_EXCLUDE, reach 0 or
 * 1..32768, N6's ranges for min_var, max_mse and ratio.  The defaults are the match defaults (8, ZSSD, 25, 400, 0.8) with
 * exclude = p = 8, reach 0 and trigger_mask = FFL_MATCH_POOR: the project's own choice, NOT tuned on footage.
 * What this is NOT: whole pixels only; no scale or rotation; no template update.  After a scene cut the template is stale
 * and a global search reads POOR as well: re-capture (ffl_track_template) stays the caller's. */
enum { FFL_MAX_REDETECT_EXCLUDE = 32, FFL_REDETECT_SKIPPED = 8 };
typedef struct ffl_redetect_params {
    int p, mode, exclude, reach, trigger_mask, reserved;   /* reserved: not read */
    double min_var, max_mse, ratio;
} ffl_redetect_params;
int ffl_redetect_default_params(ffl_redetect_params *out);
/* Pure host check: no device or context needed.  FFL_ERR_INVALID with the rule in ffl_last_error(NULL). */
int ffl_redetect_params_check(const ffl_redetect_params *p);
/* The device memory a context of this size gains with its first ffl_track_redetect: one 64-bit word per 64 x 16 candidate
 * tile of the frame plus 20, for max_batch items x FFL_MAX_TRACKS tracks.  Needs no device.  ffl_estimate_bytes does not
 * count it. */
int ffl_redetect_extra_bytes(int width, int height, int max_batch, size_t *bytes);

/* Item i searches frame slot fslots[i] for each of the n_tracks templates (rules L1 to L9); p NULL: the defaults.
 * trigger_dev NULL: every search runs (trigger_stride_bytes is then not read).  Refused before any device work, each with its
 * rule in the message: everything ffl_track_match refuses; any rule of ffl_redetect_params_check; a trigger_dev that is not
 * 4-byte aligned; a trigger stride that is no multiple of 4 or below 48 * (n_tracks - 1) + 4; trigger words ((n - 1) * stride
 * + 48 * (n_tracks - 1) + 4 bytes) that are not device memory of the context's device inside one allocation, or that overlap
 * the centres, the templates or out_dev.  ffl_track_match's protocol: four launches (k_redetect_sweep over the candidate
 * tiles, k_redetect_pick, k_redetect_sweep over the tiles about the best with its neighbourhood masked, k_redetect_final),
 * queued on the library's stream behind the work queued on `stream` and the uploads that filled the frame slots; `stream`
 * then waits for them; the call counts as a reader of the frame slots; never captured; the host does not wait.  Scratch:
 * ffl_redetect_extra_bytes, allocated by the first call and freed by ffl_destroy. */
int ffl_track_redetect(ffl_ctx *ctx, int n, const int *fslots, int n_tracks, const ffl_redetect_params *p,
                       const void *templates_dev, void *centres_dev, ptrdiff_t centre_stride_bytes, const void *trigger_dev,
                       ptrdiff_t trigger_stride_bytes, int write_back, ffl_match_record *out_dev, uint64_t stream);

/* ---- Global-motion fit and compensation ----
 * A per-pair parametric camera model, fitted robustly to a resident flow field and subtracted from it, so that what pass 1
 * and pass 2 reduce is the subject's motion without the camera's.  The rules are the project's own (the reference has no
 * such function).  All arithmetic is float64, one rounding per written operation, left to right, no contraction; u, v are
 * widened exactly.
 *   C1  xc = (double)x - (width - 1) / 2.0, yc = (double)y - (height - 1) / 2.0 (both exact).
 *   C2  a model is six doubles; its flow at a pixel is mu = (a0 + a1*xc) + a2*yc, mv = (b0 + b1*xc) + b2*yc.
 *       TRANSLATION: a0, b0, the rest 0.  RIGID: a0, b0, r with a2 = -r, b1 = r, a1 = b2 = 0.  SIMILARITY: a0, b0, s, r with
 *       a1 = b2 = s, a2 = -r, b1 = r.  AFFINE: all six.
 *   C3  wt = (double)W[y][x] under a map (rule W1), else 1.  A pixel is excluded by a select, never a multiplication, when
 *       W == 0 or !(fabsf(u) <= FLT_MAX && fabsf(v) <= FLT_MAX): nothing of it reaches a sum.  With a prior model p:
 *       ru = u - mu_p, rv = v - mv_p, r2 = ru*ru + rv*rv, t2 = (double)tau * (double)tau, rho = t2 / (t2 + r2),
 *       omega = wt * rho (the Cauchy weight; one division).  Without a prior omega = wt.
 *   C4  the twelve sums, in this order: S = sum omega, Sx = sum omega*xc, Sy = sum omega*yc, Sxx = sum (omega*xc)*xc,
 *       Sxy = sum (omega*xc)*yc, Syy = sum (omega*yc)*yc, Su = sum omega*u, Sux = sum (omega*u)*xc, Suy = sum (omega*u)*yc,
 *       Sv, Svx, Svy alike.  Only the order of addition is the kernel's own (ffl_radial's); every sum starts at +0.0; no
 *       float atomics: the same bits from run to run.
 *   C5  the weighted least-squares normal equations of the sub-model over the twelve sums, solved by an LDL^T elimination
 *       without pivoting whose operation order DESIGN.md appendix C writes out line for line (ffl_motion_solve).
 *   C6  S == 0: all six +0.0, status EMPTY, no division executed.  A pivot that is not > 1e-12 * its diagonal entry before
 *       elimination (a NaN included): the TRANSLATION solution, status DEGENERATE.  Otherwise OK.
 *   C7  pass 1 uses the caller's prior or none, pass k + 1 the model of pass k: `iterations` passes are, bit for bit,
 *       `iterations` chained calls of one pass each.
 *   C8  u' = (float)((double)u - mu), v' alike: one rounding to float32; non-finite samples follow IEEE; a model of all
 *       zeros gives u' = u bit for bit.
 *   C9  SIMILARITY and AFFINE contain a zoom term (s; a1 and b2), and a zoom about the centre IS the radial signal pass 2
 *       measures: compensating with them removes part of what the scripts are made from.  The defaults -- TRANSLATION, 3
 *       iterations, tau = 1.0 px -- are the project's own choice and are not tuned on footage. */
enum { FFL_MOTION_TRANSLATION = 0, FFL_MOTION_RIGID = 1, FFL_MOTION_SIMILARITY = 2, FFL_MOTION_AFFINE = 3 };
enum { FFL_MOTION_OK = 0, FFL_MOTION_EMPTY = 1, FFL_MOTION_DEGENERATE = 2 };
enum { FFL_MOTION_N_SUMS = 12 };
typedef struct ffl_motion_params {   /* model FFL_MOTION_*; iterations 1..8; 0 < tau <= 1e6, finite */
    int model, iterations;
    float tau;
} ffl_motion_params;
typedef struct ffl_motion_record {   /* 64 bytes */
    double a0, a1, a2, b0, b1, b2;   /* rule C2 */
    double sw;                       /* S of the last pass */
    int32_t model, status;           /* FFL_MOTION_* */
} ffl_motion_record;

/* The defaults of rule C9. */
int ffl_motion_default_params(ffl_motion_params *out);
/* Pure host check: no device or context needed.  FFL_ERR_INVALID with the rule in ffl_last_error(NULL). */
int ffl_motion_params_check(const ffl_motion_params *p);

/* Rules C5 and C6 on twelve sums in rule C4's order: a pure host function, no device or context needed.  It compiles the
 * same source as the device's k_motion_solve, so out is, bit for bit, the record ffl_motion_fit writes for these sums.
 * FFL_ERR_INVALID for a NULL pointer or an unknown model. */
int ffl_motion_solve(const double *sums, int model, ffl_motion_record *out);

/* Device memory the fit adds to a context of this size, allocated by the first ffl_motion_fit and freed by ffl_destroy:
 * FFL_MOTION_N_SUMS float64 partial sums per workgroup of the radial grid for FFL_MAX_BATCH items (ffl_estimate_bytes does
 * not count it).  Needs no device. */
int ffl_motion_extra_bytes(int width, int height, size_t *bytes);

/* Fit the model of p (NULL: the defaults) to each of flow slots flow_slots[0..n) by p->iterations passes of rules C3 to C7.
 * weights: the maps of the n items (rule W1's descriptor), or NULL.  prior_dev: NULL, or the prior of item i as six doubles
 * (a0, a1, a2, b0, b1, b2) at prior_dev + i * prior_stride_bytes -- a stride of 64 reads ffl_motion_record's as this call
 * left them, a stride of 48 a plain (n, 6) float64 array of any estimator's.  models_dev: n records, written.  sums_dev:
 * NULL, or n * FFL_MOTION_N_SUMS doubles, the last pass's sums.  The flow and the pass-1 records are only read.
 * Refused before any device work, each with its rule in the message: n outside 1..max_batch; a NULL list; a slot out of
 * range or repeated; a slot that holds no flow (FFL_ERR_STATE); any rule of ffl_motion_params_check; any rule of
 * ffl_dev_weights_check; models_dev NULL; models_dev, sums_dev or prior_dev that is not 8-byte aligned device memory of the
 * context's device inside one allocation (page-locked host memory is refused); a prior stride below 48 or no multiple of 8;
 * models_dev overlapping prior_dev when iterations > 1; a capturing `stream` (FFL_ERR_STATE).
 * ffl_pass1_weighted's protocol: per pass one k_strip_sums<MotionSums<..>> launch for all n items plus k_motion_solve, queued
 * on the library's stream behind the work queued on `stream` and the slots' last users; `stream` then waits for it, so the records
 * may be read on `stream` straight after the call; it counts as a use of the slots; never captured; the host does not wait.
 * The first call of a context allocates what ffl_motion_extra_bytes reports. */
int ffl_motion_fit(ffl_ctx *ctx, int n, const int *flow_slots, const ffl_motion_params *p, const ffl_dev_weights *weights,
                   const void *prior_dev, ptrdiff_t prior_stride_bytes, ffl_motion_record *models_dev, double *sums_dev,
                   uint64_t stream);

/* Rule C8: flow slot dst_slots[i] = the field of src_slots[i] minus the model of item i, six doubles at models_dev + i *
 * model_stride_bytes (64: ffl_motion_fit's records; 48: a plain (n, 6) float64 array), then the pass-1 reductions of the dst
 * slots by the k_pass1 / k_pass1_final pair: each dst record is bit-identical to ffl_upload_flow's for the same float32 field
 * and replaces the slot's record, as ffl_pass1_weighted's does.  dst_slots[i] == src_slots[i] is allowed (in place: every
 * pixel is read and written by one lane); otherwise the dst slots are distinct among themselves and none is another item's
 * src.  Refused before any device work: n outside 1..max_batch; a NULL list; a src or dst slot out of range; a repeated src or
 * dst slot, or a dst slot that is another item's src; a src slot that holds no flow (FFL_ERR_STATE); models_dev that is NULL or
 * not 8-byte aligned device memory of the context's device inside one allocation; a stride below 48 or no multiple of 8; a
 * capturing `stream` (FFL_ERR_STATE).  ffl_pass1_weighted's protocol: k_motion_subtract, k_pass1 and k_pass1_final queued on
 * the library's stream behind `stream`'s work and the last users of all the slots; `stream` waits for it; it counts as a write
 * of the dst slots and a use of the src slots; never captured; the host does not wait. */
int ffl_motion_subtract(ffl_ctx *ctx, int n, const int *src_slots, const int *dst_slots, const void *models_dev,
                        ptrdiff_t model_stride_bytes, int pov_mode, uint64_t stream);

/* Copy a finished flow field to host memory as (height, width, 2) float32, cv2 layout. */
int ffl_download_flow(ffl_ctx *ctx, int flow_slot, float *dst);

/* Place a caller-provided (height, width, 2) float32 flow field into `flow_slot` and run the pass-1
 * reductions on it (lets the post path be checked against reference golden vectors). */
int ffl_upload_flow(ffl_ctx *ctx, int flow_slot, const float *src, int pov_mode);

/* One-pair convenience: upload prev/next into frame slots 2*slot, 2*slot+1 and queue the pair into
 * flow slot `slot` (mirrors precompute_wrapper, FF:1019-1021). */
int ffl_submit_pair(ffl_ctx *ctx, int slot, const uint8_t *prev, const uint8_t *next, int width, int height,
                    int channels, ptrdiff_t stride_bytes, int pov_mode);

/* Block until everything queued on the context has finished. */
int ffl_sync(ffl_ctx *ctx);

/* ---- DIS optical flow (the reference's "DNN" backend, FF:948-980; DESIGN.md "DIS path") ------------------------- */

/* Parameters of the DIS path.  Everything that changes results is here (never in ffl_set_option). */
typedef struct ffl_dis_params {
    int finest_scale, patch_size, patch_stride, grad_descent_iters, var_refine_iters;
    float vr_alpha, vr_gamma, vr_delta;
    int use_mean_norm, use_spatial_prop, stripes; /* stripes: 0 = one patch row per stripe */
} ffl_dis_params;

/* PRESET_FAST: finest 2, patch 8, stride 4, 16 descent iterations, 5 refinement iterations, alpha 20, gamma 10,
 * delta 5, mean normalisation and spatial propagation on, stripes 0. */
int ffl_dis_default_params(ffl_dis_params *out);

/* Scales of a width x height frame under p.  FFL_ERR_INVALID (with a message) when the size or the parameters are not
 * supported: only patch_size 8; coarsest = min((int)(log2(max(W,H) / 32) + 0.5), (int)log2(min(W,H) / 8)) must be
 * >= finest_scale, W and H divisible by 2^coarsest (every INTER_AREA reduction an exact integer factor), and every
 * scale a whole number of patch strides.  256x256 and 512x512 are supported; 640x360 and 1920x1080 are not. */
int ffl_dis_geometry(int width, int height, const ffl_dis_params *p, int *coarsest, int *finest);

/* Queue DIS flow + the same pass-1 reductions as ffl_flow_pairs for n pairs (same slot tables, events and result
 * calls; p == NULL: PRESET_FAST).  Asynchronous.  Batches are launched eagerly (never from a captured graph). */
int ffl_flow_pairs_dis(ffl_ctx *ctx, int n, const int *fslot0, const int *fslot1, const int *flow_slots, int pov_mode,
                       const ffl_dis_params *p);

/* Test hook: run ONE DIS pair (frame slots f0, f1) and copy one intermediate of scale `scale` to `out`:
 * stage 0 patch flows after pass 1, 1 after pass 2 (hs x ws x 2 floats), 2 the densified field, 3 the field after
 * variational refinement (lh x lw x 2), 4 the two level images I0, I1 (2 x lh x lw).  The final flow goes to flow
 * slot 0.  Synchronous. */
int ffl_debug_dis_pair(ffl_ctx *ctx, int f0, int f1, const ffl_dis_params *p, int scale, int stage, float *out);

/* ---- Farneback with caller-chosen parameters -------------------------------------- */

/* The six numeric parameters of cv2.calcOpticalFlowFarneback (and its flags).  Accepted: 0 < pyr_scale < 1,
 * 0 <= levels <= 12, winsize odd 3..63, 1 <= iterations <= 10, poly_n 5 or 7, 0 < poly_sigma <= 3, flags == 0
 * (cv2's two flags are not fields of the parameters: they are the `mode` of ffl_flow_pairs_farneback_ex, and refused
 * here).  Float fields are computed with as the double of their shortest decimal form (1.2f as 1.2). */
typedef struct ffl_farneback_params {
    float pyr_scale;
    int levels;
    int winsize;
    int iterations;
    int poly_n;
    float poly_sigma;
    int flags;
} ffl_farneback_params;

/* The reference's call: (0.5, 3, 15, 3, 5, 1.2, 0). */
int ffl_farneback_default_params(ffl_farneback_params *out);

/* Scales of a width x height frame under p after A.1's min_size = 32 rule (levels used + 1), and the per-pair working set
 * of the general kernels in bytes (two frames' expansions of every level + M + two level flows).  FFL_ERR_INVALID with a
 * message (ffl_last_error(NULL)) for parameters outside the rules above, or a level Gaussian wider than 191 taps. */
int ffl_farneback_geometry(int width, int height, const ffl_farneback_params *p, int *n_scales, size_t *work_bytes_per_pair);

/* Device bytes ffl_flow_pairs_farneback(p) may allocate on top of ffl_estimate_bytes for a context of this size and
 * max_batch under the current "lanes" option: 0 when every lane's buffers hold the working set, else the general-path
 * work areas (one per lane, allocated on first use, freed by ffl_destroy). */
int ffl_farneback_extra_bytes(int width, int height, int max_batch, const ffl_farneback_params *p, size_t *bytes);

/* ffl_flow_pairs with caller-chosen parameters (p == NULL: the defaults): same slots, events, lanes and pass-1 records.
 * p equal to the defaults calls ffl_flow_pairs (the tuned kernels and their graphs) unless the context option
 * "fb_general" is 1; any other p runs the general kernels, launched eagerly (never captured).  Parameters are refused
 * before any device work.  Asynchronous. */
int ffl_flow_pairs_farneback(ffl_ctx *ctx, int n, const int *fslot0, const int *fslot1, const int *flow_slots, int pov_mode,
                             const ffl_farneback_params *p);

/* cv2's two flags that change what is computed, as the mode of a call. */
#define FFL_FB_USE_INITIAL_FLOW 4u     /* cv2.OPTFLOW_USE_INITIAL_FLOW */
#define FFL_FB_GAUSSIAN_WINDOW  256u   /* cv2.OPTFLOW_FARNEBACK_GAUSSIAN */

/* ffl_flow_pairs_farneback under a mode.  mode == 0 is ffl_flow_pairs_farneback(p) itself (the defaults reach the tuned
 * path, the same bits).  Any other mode runs the general kernels, at the default numbers too; a bit other than the two
 * above is refused by name (FFL_ERR_INVALID).  p obeys the rules above unchanged: p->flags must be 0, winsize odd.
 *   FFL_FB_GAUSSIAN_WINDOW   the winsize x winsize window is the separable float Gaussian of sigma = 0.3 * (winsize / 2)
 *                            in place of the box.
 *   FFL_FB_USE_INITIAL_FLOW  flow_slots[b] is in/out as cv2's `flow` argument: it must already hold a flow (an earlier
 *                            batch's, ffl_upload_flow's or ffl_import_flows'; FFL_ERR_STATE before any device work when
 *                            it holds none), is read as the pair's starting field (reduced by INTER_AREA to the
 *                            coarsest level and scaled) behind its last writer, then overwritten with the result; its
 *                            pass-1 record is replaced by this batch's.
 * A mode adds no memory: ffl_farneback_geometry and ffl_farneback_extra_bytes hold for every mode.  Asynchronous. */
int ffl_flow_pairs_farneback_ex(ffl_ctx *ctx, int n, const int *fslot0, const int *fslot1, const int *flow_slots,
                                int pov_mode, const ffl_farneback_params *p, unsigned mode);

/* ---- parity-test hooks (used by tests/ only) ------------------------------------------------ */

/* Number of pyramid scales minus one for this context's size (3 for every BASELINE config). */
int ffl_num_levels(const ffl_ctx *ctx);
/* Level-k geometry: out_wh[0]=width, out_wh[1]=height. */
int ffl_level_size(const ffl_ctx *ctx, int level, int *out_wh);

/* Copy the resident gray frame of `fslot` to host memory (height * width bytes). */
int ffl_download_frame(ffl_ctx *ctx, int fslot, uint8_t *dst);

/* Run ONE pair (frame slots f0, f1) and capture the level-`level` intermediates as they stand
 * before blur iteration `iter` (0: right after the initial UpdateMatrices; 3: end of level).
 * Any of the output pointers may be NULL.  Planar layouts: R*, M = 5 planes of lh*lw floats;
 * I* = lh*lw; flow = lh*lw*2 interleaved.  The final full-resolution flow goes to flow slot 0. */
int ffl_debug_pair(ffl_ctx *ctx, int f0, int f1, int level, int iter, float *I0, float *I1, float *R0, float *R1,
                   float *M, float *flow);

/* The launch plan of k_blur_solve for a level of tiles_x x tiles_y tiles (64 x 16 pixels) and n_pairs pairs on a device
 * with `slots` resident workgroups, under the given values of the options "blur_rows", "blur_min_wgs", "blur_taper",
 * "blur_taper_pairs" and "tile_order" (below).  Needs no device: the host runs the kernel's own mapping.
 * segments: 3 rows of (first workgroup, first pair, pairs, tiles per strip, strips per tile column), *n_segments of them
 * used; *grid: workgroups of the launch; blocks (may be NULL; max_blocks >= *grid rows of 4 ints): workgroup ->
 * (pair, tile column, first tile row, tiles), pair -1 for a padding workgroup. */
int ffl_debug_blur_plan(int tiles_x, int tiles_y, int n_pairs, int slots, int blur_rows, int blur_min_wgs, int blur_taper,
                        int blur_taper_pairs, int tile_order, int *segments, int *n_segments, int *grid, int *blocks,
                        int max_blocks);

/* ---- measurement hooks (bench.py) -------------------------------------------------------------- */

/* Tuning knobs (results never depend on them).  ffl_set_option sets the process-wide default that contexts created
 * AFTERWARDS start from; ffl_ctx_set_option changes one live context (every knob but "lanes", which sizes the context's
 * buffers: FFL_ERR_STATE) and makes that context -- and no other -- re-capture its graphs; ffl_ctx_get_option reads a
 * context's value (ctx == NULL: the process-wide default).
 *   "blur_tile_h" = 16       rows of the 64-wide k_blur_solve LDS tile.  Fixed since the box-sum order
 *                            is anchored to blocks of 16 rows / columns (other values are refused); the
 *                            8 / 16 / 32 sweep of BASELINE configs[2] is recorded in profiles/README.md
 *   "blur_rows"   = 0..64    tiles a k_blur_solve workgroup walks down (0 = automatic, the default)
 *   "blur_min_wgs" = N >= 1  automatic strip length: a column of tiles is cut into the fewest equal strips that still
 *                            give the launch N workgroups (default 3500)
 *   "fuse_first"  = N >= 0   a level's flow init + first UpdateMatrices run inside its first k_blur_solve launch
 *                            when the level has at least N 64x16 tiles over the batch (default 10000; 0 = never,
 *                            1 = always)
 *   "lanes"       = 1..4     compute lanes (co-scheduled batches, each on its own stream and work
 *                            buffers) of contexts created afterwards; default 2
 *   "run_ahead"   = 0,       schedule of the frame-only kernels.  Fixed: they run serially on the lane's stream,
 *   "merge_expand" = 1       pyramid + PolyExp of all levels in three merged launches per batch (other values
 *                            are refused)
 *   "copy_threads" = 1..16   host threads that share a staging copy of 1 MiB or more (the caller + helpers owned by
 *                            the context); default 4.  One thread moves ~22 GB/s, a 1080p BGR stream at 5 k pairs/s
 *                            needs 31
 *   "graph"       = 0|1      1 (default): a batch's launches are captured once per (lane, batch shape, option set)
 *                            into a hipGraph and replayed; 0: launched one by one (timing events and the debug
 *                            capture always launch one by one)
 *   "pyr_coarse"  = 0|1      1 (default): the x1/4 and x1/8 pyramid levels of frames whose sides are multiples of 8
 *                            come from one LDS-staged pass (k_pyr_coarse); 0: horizontal + vertical kernel pairs
 *   "fuse_l0_blur" = 0|1     1 (default): PolyExp forms level 0's image (the 3-tap blur of the
 *                            gray frame) in its own tile loader and the level-0 image plane is neither written nor
 *                            read; 0: the pyramid launch writes it (the debug capture always does)
 *   "tile_order"  = 0|1      k_blur_solve / k_update_matrices workgroup order: 0 pair-major (default), 1 tile-major
 *                            (every tile for all pairs of the batch back to back; less fabric traffic, not faster)
 *   "blur_taper"  = 0|1      1: the pairs a k_blur_solve launch deals last walk shorter strips (half, then a quarter of
 *                            the bulk's), about half a round of the device's workgroup slots in all, so that the launch
 *                            drains faster; levels whose strips are 1 or 2 tiles, batches of fewer than 4 pairs and levels on which one pair
 *                            alone exceeds half a round are left alone.  Default 1 (+1.3 to
 *                            +3.3 % per step at the four bench shapes, profiles/blur_taper.md); 0: one uniform grid
 *   "blur_taper_pairs" = 0..256  P > 0: P pairs in each of the two taper segments, whatever "blur_taper" says (tests
 *                            and sweeps); default 0
 *   "fb_general"  = 0|1      1: ffl_flow_pairs_farneback runs the default parameters through the general kernels as well
 *                            (test and measurement hook; the results are the same bits) */
int ffl_set_option(const char *name, int value);
int ffl_ctx_set_option(ffl_ctx *ctx, const char *name, int value);
int ffl_ctx_get_option(ffl_ctx *ctx, const char *name, int *value);

/* hipGraph bookkeeping of a context: batch shapes captured, batches replayed from a graph, captures that FAILED.  A
 * failed capture is never silent: the batch is launched kernel by kernel (results unaffected), the context stops
 * capturing until one of its options changes, one line goes to stderr, and the failure is counted here -- bench.py
 * reports the three numbers (`config.graphs`) and the GPU tests assert capture_failures == 0. */
int ffl_graph_stats(ffl_ctx *ctx, int *captured, int *replayed, int *capture_failures);

/* HIP-event timing of kernel classes: every launch of a class whose bit (1u << FFL_K_*) is set in
 * class_mask is bracketed by events on the stream it is launched on.  0 switches timing off. */
int ffl_profile_enable(ffl_ctx *ctx, unsigned class_mask);
#define FFL_PROFILE_ALL 0xFFu
#define FFL_K_GRAY 0
#define FFL_K_PYRAMID 1
#define FFL_K_POLYEXP 2
#define FFL_K_FRONTEND 3 /* k_frontend of ffl_upload_frames_raw and ffl_upload_frames_yuv / _yuv16, k_frontend_dev of
                            ffl_upload_frames_device / _device16 (the x2 flow upsample, once class 3, runs inside k_update_matrices) */
#define FFL_K_UPDATE_MATRICES 4
#define FFL_K_BLUR_SOLVE 5
#define FFL_K_PASS1 6
#define FFL_K_RADIAL 7   /* ffl_radial's pair of launches; ffl_radial_window's three launches belong to no class */
#define FFL_K_COUNT 8
/* Read and reset the accumulated (launch count, total milliseconds) of one kernel class.
 * Synchronises the context. */
int ffl_profile_read(ffl_ctx *ctx, int kernel_class, int *launches, double *total_ms);
const char *ffl_kernel_name(int kernel_class);

#ifdef __cplusplus
}
#endif
#endif /* FFL_H */
