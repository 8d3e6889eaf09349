/*
 * rva.h -- C ABI of librva.so: the MI355X-native detect/track hot path.
 *
 * Boundary: everything the reference's Detector / Tracker plugin API computes between "a decoded
 * frame is available" and "tracks are visible to the host" (SURVEY.md section 8).  The reference is
 * pure Python and has no FFI of its own; each entry point below names the reference function(s)
 * it replaces (paths relative to /root/reference/src/realtime_analytics/).  Plain pointers and
 * sizes only: no torch / Python types cross this boundary.
 *
 * Conventions
 *   - `stream` is a hipStream_t passed as void*; NULL = the default stream.  All device work is
 *     enqueued on it and nothing synchronises unless the function says so ("host-synchronous").
 *   - "device" pointers are HIP device addresses (e.g. torch.Tensor.data_ptr()).
 *   - Return value: RVA_OK or an error code; rva_last_error(ctx) gives the text.
 *   - No function allocates device memory once rva_reserve()/…_create() have sized the context, so a
 *     caller may capture a whole tick into a hipGraph.
 *   - There is NO CPU fallback: if no HIP device is usable, rva_create() fails.
 */
#ifndef RVA_H
#define RVA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RVA_ABI_VERSION 1

enum rva_status {
    RVA_OK = 0,
    RVA_ERR_ARG = 1,         /* bad argument / unsupported shape */
    RVA_ERR_HIP = 2,         /* a HIP runtime call failed */
    RVA_ERR_CAPACITY = 3,    /* a capacity given at create/reserve time was exceeded */
    RVA_ERR_UNAVAILABLE = 4  /* optional component (rocDecode) not present on this machine */
};

enum rva_dtype { RVA_F16 = 0, RVA_F32 = 1, RVA_F64 = 2 /* only where an entry point says so */ };

typedef struct rva_ctx rva_ctx;
typedef struct rva_tracker rva_tracker;
typedef void *rva_stream_t;

int rva_abi_version(void);
int rva_create(int device, rva_ctx **out);
void rva_destroy(rva_ctx *ctx);
const char *rva_last_error(const rva_ctx *ctx);

/* Pre-size every scratch buffer for `batch` images x `anchors` head rows (host-synchronous; call
 * before graph capture).  Optional: buffers otherwise grow on first use. */
int rva_reserve(rva_ctx *ctx, int batch, int anchors);

/* ----------------------------------------------------------------------------------------------
 * Letterbox geometry -- detector.py:209-230 and the `meta` dict of :259-263.
 * -------------------------------------------------------------------------------------------- */
typedef struct rva_letterbox {
    int32_t src_w, src_h;   /* meta["orig_shape"] = (src_h, src_w) */
    int32_t dst_w, dst_h;   /* detector input size (input_hw) */
    int32_t new_w, new_h;   /* int(w*scale), int(h*scale) */
    int32_t pad_left, pad_top; /* meta["pad"] */
    double scale;           /* meta["scale"] (Python float) */
} rva_letterbox;

int rva_letterbox_meta(int src_w, int src_h, int dst_w, int dst_h, rva_letterbox *out);

/* ----------------------------------------------------------------------------------------------
 * K1 pre-process -- replaces _TensorRTBaseDetector._preprocess (detector.py:198-264) for a whole
 * tick of frames in ONE launch: [colour convert] -> cv2.resize(INTER_LINEAR) letterbox -> pad 114
 * -> BGR2RGB -> astype(dtype) * (1/255) -> CHW, written straight into the batch tensor
 * out[n, 3, dst_h, dst_w] (device).  n <= RVA_MAX_BATCH per call.
 *
 * nv12: y_ptrs[i] / uv_ptrs[i] are device pointers of pitch-linear NV12 surfaces (what a hardware
 *       decoder hands over instead of video_stream.py:173's BGR ndarray); BT.601 limited range,
 *       nearest chroma, converted at full resolution before the resize, as FFmpeg+OpenCV would.
 * bgr:  frames[i] is a device copy of the uint8 [src_h, src_w, 3] BGR frame of FramePacket.frame.
 * meta_out (host, may be NULL) receives the geometry shared by all n frames.
 * -------------------------------------------------------------------------------------------- */
#define RVA_MAX_BATCH 64

int rva_preprocess_nv12_batch(rva_ctx *ctx, const void *const *y_ptrs, const void *const *uv_ptrs,
                              const int32_t *pitches, int n, int src_w, int src_h, void *out,
                              int out_dtype, int dst_w, int dst_h, rva_letterbox *meta_out,
                              rva_stream_t stream);

/* Steady-state form of rva_preprocess_nv12_batch: writes only the CONTENT region of out[n, 3, dst_h, dst_w] -- the
 * letterbox border is a constant (114/255, detector.py:233-241) and the caller guarantees it is already there (an
 * earlier rva_preprocess_nv12_batch into the same tensor with the same geometry put it there).  Same values as the full
 * call; 1080p -> 640: 2,764,800 instead of 3,840,000 bytes of traffic per frame.  Geometries without an integer
 * source/content ratio fall back to writing the whole tensor. */
int rva_preprocess_nv12_content_batch(rva_ctx *ctx, const void *const *y_ptrs, const void *const *uv_ptrs,
                                      const int32_t *pitches, int n, int src_w, int src_h, void *out,
                                      int out_dtype, int dst_w, int dst_h, rva_letterbox *meta_out,
                                      rva_stream_t stream);

int rva_preprocess_bgr_batch(rva_ctx *ctx, const void *const *frames, const int32_t *row_bytes, int n,
                             int src_w, int src_h, void *out, int out_dtype, int dst_w, int dst_h,
                             rva_letterbox *meta_out, rva_stream_t stream);

/* Measurement aid (bench.py roofline leg): the NEXT integer-ratio K1 launch of this context is issued with
 * hipExtLaunchKernelGGL so that the two HIP events (hipEvent_t handles created with timing enabled) are written by
 * the kernel's own dispatch -- they bracket exactly that kernel.  One-shot; pass NULL, NULL to cancel. */
int rva_profile_next_preprocess(rva_ctx *ctx, void *start_event, void *stop_event);

/* Clip-frame pre-process -- replaces the per-frame body of CNNLSTMDetector._preprocess_sequence
 * (temporal_detector.py:340-359): stretch-resize to (dst_w, dst_h), BGR2RGB, /255.0, (x-mean)/std
 * (ImageNet constants), CHW; out[n, 3, dst_h, dst_w] in out_dtype (float32 math, cast last). */
int rva_preprocess_clip_nv12_batch(rva_ctx *ctx, const void *const *y_ptrs, const void *const *uv_ptrs,
                                   const int32_t *pitches, int n, int src_w, int src_h, void *out,
                                   int out_dtype, int dst_w, int dst_h, rva_stream_t stream);

int rva_preprocess_clip_bgr_batch(rva_ctx *ctx, const void *const *frames, const int32_t *row_bytes,
                                  int n, int src_w, int src_h, void *out, int out_dtype, int dst_w,
                                  int dst_h, rva_stream_t stream);

/* Frame pre-process of the remaining classification / temporal heads: stretch-resize to
 * (dst_w, dst_h) with cv2.resize defaults, BGR2RGB, image.astype(float32) / 255.0, (image - mean) / std, CHW.
 *   norm RVA_NORM_IMAGENET_F32: float32 ImageNet constants -- CNNLSTMDetector (temporal_detector.py:350-354) and the
 *        ResNet classifiers' _preprocess (detector.py:980-1001);
 *   norm RVA_NORM_VIDEO_F32:    float32 mean 0.45 / std 0.225 on every channel -- CNN3DDetector (:570-573);
 *   norm RVA_NORM_IMAGENET_F64: ImageNet constants held in float64 arrays, so the float32 image is promoted and the
 *        subtraction / division run in float64 -- ConvGRUDetector (:741-743).  The reference then hands over float64
 *        (out_dtype RVA_F64) or casts float64 -> float16 in one rounding (RVA_F16); RVA_F32 is that value rounded once.
 *   layout RVA_LAYOUT_NCHW: out[n][3][H][W] (frames stacked on axis 0: CNN-LSTM / ConvGRU clips [T,C,H,W], ResNet);
 *   layout RVA_LAYOUT_CNHW: out[3][n][H][W] (3D-CNN clips [C,T,H,W], temporal_detector.py:583-590).
 * RVA_F64 is accepted with RVA_NORM_IMAGENET_F64 only.  rva_preprocess_clip_* = (IMAGENET_F32, NCHW). */
enum rva_frame_norm { RVA_NORM_IMAGENET_F32 = 0, RVA_NORM_VIDEO_F32 = 1, RVA_NORM_IMAGENET_F64 = 2 };
enum rva_frame_layout { RVA_LAYOUT_NCHW = 0, RVA_LAYOUT_CNHW = 1 };
int rva_preprocess_frames_nv12_batch(rva_ctx *ctx, const void *const *y_ptrs, const void *const *uv_ptrs,
                                     const int32_t *pitches, int n, int src_w, int src_h, void *out,
                                     int out_dtype, int dst_w, int dst_h, int norm, int layout,
                                     rva_stream_t stream);
int rva_preprocess_frames_bgr_batch(rva_ctx *ctx, const void *const *frames, const int32_t *row_bytes,
                                    int n, int src_w, int src_h, void *out, int out_dtype, int dst_w,
                                    int dst_h, int norm, int layout, rva_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * K2+K3 post-process -- replaces _TensorRTBaseDetector._postprocess with _xywh2xyxy, _scale_boxes,
 * _nms and module _iou (detector.py:266-375, 469-481) for a batch of head tensors.
 *
 * raw: device, [batch, d1, d2] contiguous, float16 or float32 (float16 is widened exactly).  Each
 *      image is oriented like detector.py:282-283: d1 < d2 means [channels, anchors], otherwise
 *      [anchors, channels].  channels < 5 -> every count is 0 (detector.py:285-287).
 * metas: host array of `batch` geometries (or 1 entry broadcast when n_metas == 1).
 * classes: host array (config.classes) or NULL.
 * Outputs (device), per image b in NMS order (descending score; ties: ascending anchor):
 *   out_boxes[b][i][4] xyxy frame pixels, out_scores[b][i], out_cls[b][i],
 *   out_anchor[b][i]  anchor row of the detection, out_cand[b][i] its index among the thresholded
 *   candidates (the value the reference's `keep` list holds), out_counts[b], out_ncand[b].
 *   Arrays are [batch, max_det]; out_anchor/out_cand/out_ncand may be NULL.
 * The reference has no detection cap: pass max_det = anchors for exact behaviour; if an image keeps
 * more than max_det boxes the extra ones are dropped and bit 0 of rva_post_status() is set.
 * -------------------------------------------------------------------------------------------- */
int rva_postprocess_batch(rva_ctx *ctx, const void *raw, int raw_dtype, int batch, int d1, int d2,
                          double conf_thr, double iou_thr, const int32_t *classes, int n_classes,
                          const rva_letterbox *metas, int n_metas, int max_det, float *out_boxes,
                          float *out_scores, int32_t *out_cls, int32_t *out_anchor, int32_t *out_cand,
                          int32_t *out_counts, int32_t *out_ncand, rva_stream_t stream);

/* Host-synchronous: bit 0 = max_det overflow, bit 1 = candidate capacity overflow since the last call. */
/* The same post-process with the boxes taken from an fp32 side tensor (split mode of the fp16 plan, RVA_PLAN_BOX_F32): raw is
 * [batch, channels, anchors] only (channels >= 5, channels < anchors; float16 or float32), boxes is device float
 * [batch, 4, anchors] = cx, cy, w, h in input pixels.  Rows 0-3 of raw are never read; scores, the class-shift quirk, thresholds,
 * class filter, letterbox undo, division and clipping are the code of rva_postprocess_batch, as are K3 and all outputs.  K2 reads
 * channels x anchors x 2 B + 4 x anchors x 4 B per image (84 x 8400: +9.5 % over the fp16 head alone). */
int rva_postprocess_boxes_batch(rva_ctx *ctx, const void *raw, int raw_dtype, const float *boxes, int batch, int channels,
                                int anchors, double conf_thr, double iou_thr, const int32_t *classes, int n_classes,
                                const rva_letterbox *metas, int n_metas, int max_det, float *out_boxes, float *out_scores,
                                int32_t *out_cls, int32_t *out_anchor, int32_t *out_cand, int32_t *out_counts,
                                int32_t *out_ncand, rva_stream_t stream);

int rva_post_status(rva_ctx *ctx, rva_stream_t stream, int *flags);

/* Host-synchronous diagnostic: the number of images since the last call whose NMS scanned the kept list through the centre-bin
 * filter (K3: proper boxes -- x1 <= x2, y1 <= y2 for every candidate of the image -- and 0.15 <= iou_thr <= 0.999; other images
 * take the unfiltered scan, same result).  Nothing in the reference corresponds to it; the tests use it to know which path ran. */
int rva_post_filter_stats(rva_ctx *ctx, rva_stream_t stream, int *binned_images);

/* ----------------------------------------------------------------------------------------------
 * K4 tracker -- replaces IouTracker (tracker.py:45-147) for all streams of this process.
 *
 * One table per stream lives in HBM (structure-of-arrays, `capacity` rows, insertion order ==
 * the reference's dict order).  An update tick processes any subset of streams concurrently (one
 * wavefront per stream; the per-detection greedy loop of tracker.py:55-92 stays sequential inside
 * it), then rva_tracker_assign_ids() hands out the reference's GLOBAL ids (tracker.py:47) in the
 * canonical order "stream-minor within the tick".
 * Memory: 64 B per table row (n_streams x capacity rows) + eight pinned, device-mapped snapshot slots of the same size + the
 * float64 IoU matrix of the busy-scene form, n_streams x min(capacity, 512) x (capacity + 512) doubles capped at 512 MiB
 * (201 MB at 32 streams x capacity 1024); if that matrix cannot be allocated the tracker runs the in-loop form (same results).
 * -------------------------------------------------------------------------------------------- */
int rva_tracker_create(rva_ctx *ctx, int n_streams, int capacity, int max_age, double max_iou_distance,
                       int min_hits, rva_tracker **out);
void rva_tracker_destroy(rva_tracker *trk);

/* Detections straight from rva_postprocess_batch (device, float32, [batch, max_det] layout).
 * slot_of_stream: host int32[n_streams]; entry s = batch row holding stream s's detections this
 * tick, or -1 if stream s has no frame this tick (its table is untouched), or -2 for a skipped
 * frame (update(name, []) of pipeline.py:215: ages every track), or -3 when ANOTHER update launch of
 * the same tick owns stream s (a tick with several detectors / frame geometries issues one launch per
 * group; -3 leaves the stream's table and its new-track count alone).
 * filter_thr: filter_detections' threshold (pipeline.py:182), applied on the widened score. */
int rva_tracker_update_f32(rva_tracker *trk, const int32_t *slot_of_stream, const float *boxes,
                           const float *scores, const int32_t *cls, const int32_t *counts, int max_det,
                           double filter_thr, rva_stream_t stream);

/* The same update with the pre-detector gates of StreamWorker._process_packet decided ON THE DEVICE, so a gated
 * tick needs no host round trip (the detector has then run on every delivered frame; a gated-out frame becomes a
 * skipped frame here):
 *   motion gate (pipeline.py:156-163, utils/frame_filter.py:26-40): motion_row[s] (host int32[n_streams]) = row of
 *     the device array motion_counts (written by rva_motion_*_batch earlier on this stream) holding stream s's
 *     changed-pixel count, or -1 when the stream has no motion gate; a count of -1 (first frame) always passes, else
 *     the frame is processed iff count >= the stream's motion_min_count (rva_tracker_set_gates);
 *   adaptive-fps gate (pipeline.py:107-116, 165-170) and _adjust_adaptive_state (:242-262): frame index, idle
 *     frames and process_every live in HBM per stream and are advanced by this kernel with len(filtered) and
 *     len(tracks) of the update.
 * Streams whose slot is -2 are skipped by the caller's decision; their gate state advances like any other frame. */
int rva_tracker_update_gated_f32(rva_tracker *trk, const int32_t *slot_of_stream, const float *boxes,
                                 const float *scores, const int32_t *cls, const int32_t *counts, int max_det,
                                 double filter_thr, const int32_t *motion_counts, const int32_t *motion_row,
                                 rva_stream_t stream);

/* Gate parameters per stream (host int32[n_streams] each; host-synchronous): adaptive_enabled = StreamConfig.adaptive_fps,
 * max_process_every = max(1, int(round(target_fps / max(min_target_fps, 1)))), idle_tolerance =
 * max(int(idle_frame_tolerance), 1) (pipeline.py:107-116); motion_min_count = smallest changed-pixel count c with
 * float(c) / float(w * h) >= motion_threshold (0 when the stream has no motion gate).  reset_state != 0 also rewinds
 * every stream's frame index / idle counter / process_every to their initial values. */
int rva_tracker_set_gates(rva_tracker *trk, const int32_t *adaptive_enabled, const int32_t *max_process_every,
                          const int32_t *idle_tolerance, const int32_t *motion_min_count, int reset_state);

/* Detections supplied by the host API (IouTracker.update(stream_name, detections)): device arrays
 * double boxes[total][4], double conf[total], int64 cls[total]; stream s owns rows
 * [offsets[s], offsets[s+1]) when active[s] == 1 (host arrays, n_streams(+1) entries); active[s] == 0: no
 * update for the stream this tick; active[s] == 2: another update launch of this tick owns it (left alone). */
int rva_tracker_update_f64(rva_tracker *trk, const int32_t *active, const int32_t *offsets,
                           const double *boxes, const double *conf, const int64_t *cls,
                           rva_stream_t stream);

/* Per-stream multiplier applied (in float64) to the widened box of every detection fed through
 * rva_tracker_update_f32: _rescale_detections of pipeline.py:224-240 (1 / max(downsample_ratio, 1e-6); 1.0 = off).
 * Host-synchronous; scales: host double[n_streams]. */
int rva_tracker_set_box_scale(rva_tracker *trk, const double *scales);

/* Device address of int32 new_counts[n_streams] written by the last update (for the multi-GPU
 * all-gather of SURVEY.md 8e). */
int32_t *rva_tracker_new_counts(rva_tracker *trk);

/* Give final ids to the tracks created by the last update.  counts_all: device int32[n_global] =
 * new-track counts of ALL streams of the job in canonical order (NULL: this process owns every
 * stream; uses its own new_counts).  global_index: host int32[n_streams] position of each local
 * stream in that order (NULL: identity).  Advances the id counter by sum(counts_all). */
int rva_tracker_assign_ids(rva_tracker *trk, const int32_t *counts_all, int n_global,
                           const int32_t *global_index, rva_stream_t stream);

/* Host-synchronous read-back of one stream's table in insertion order (Track fields of
 * tracker.py:18-27).  Returns the row count in *n (rows beyond `cap` are not copied).
 * last_det[i] = index (within the stream's detection list of the latest update) of the last
 * detection that created/overwrote row i, or -1: lets the host carry the optional temporal
 * fields of tracker.py:58-67,88-90 without shipping strings to the device.  May be NULL. */
int rva_tracker_read(rva_tracker *trk, int stream_id, int cap, int64_t *ids, int32_t *cls, int32_t *age,
                     int32_t *hits, double *conf, double *boxes, int32_t *last_det, int32_t *n,
                     rva_stream_t stream);

/* Host-synchronous read-back of every stream at once: arrays are [n_streams, capacity(,4)],
 * counts[n_streams]; any pointer may be NULL.  Only rows [0, counts[s]) of stream s are written (one device
 * kernel gathers the live rows into a pinned slot); the rest of the caller's arrays is left untouched. */
int rva_tracker_read_all(rva_tracker *trk, int64_t *ids, int32_t *cls, int32_t *age, int32_t *hits,
                         double *conf, double *boxes, int32_t *last_det, int32_t *counts,
                         rva_stream_t stream);

#define RVA_SNAPSHOT_SLOTS 8   /* ticks whose tables may be on their way to the host at once */
/* Pipelined read-back: snapshot_async enqueues device-to-host copies of every table into pinned
 * staging slot 0 .. RVA_SNAPSHOT_SLOTS - 1 on `stream` (no host wait); snapshot_fetch (wait != 0) waits for that slot's
 * copies only and hands the arrays out ([n_streams, capacity(,4)] like read_all).  Lets tick k+1 be
 * enqueued before tick k's tracks are consumed.  When snapshot_async is captured into a hipGraph no
 * event is recorded: synchronise on the graph launch yourself and call snapshot_fetch with wait = 0. */
int rva_tracker_snapshot_async(rva_tracker *trk, int slot, rva_stream_t stream);
int rva_tracker_snapshot_fetch(rva_tracker *trk, int slot, int wait, int64_t *ids, int32_t *cls, int32_t *age,
                               int32_t *hits, double *conf, double *boxes, int32_t *last_det,
                               int32_t *counts);

/* What rides along in a snapshot slot besides the tables (no wait: call after snapshot_fetch / the graph launch has
 * completed): emitted[s] = len(filtered) of the stream's last update (pipeline.py:187), processed[s] = 1 processed /
 * 0 skipped frame / -1 no frame, *flags = tracker flags (bit 0: a table overflowed `capacity`, detections dropped)
 * | post-process flags << 8 (bit 8: more survivors than max_det, bit 9: more thresholded anchors than the sort holds).
 * The reference is unbounded in all three places, so a caller must treat a non-zero value as an error. */
int rva_tracker_snapshot_status(rva_tracker *trk, int slot, int32_t *emitted, int32_t *processed, int32_t *flags);

/* Host-synchronous: next id the counter will hand out; flags bit 0 = a table overflowed `capacity`. */
int rva_tracker_state(rva_tracker *trk, int64_t *next_id, int *flags, rva_stream_t stream);
int rva_tracker_set_next_id(rva_tracker *trk, int64_t next_id, rva_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * Fused detector primitives (NHWC float16) -- the arithmetic ONNX Runtime performs inside
 * `session.run` (detector.py:608) for a YOLOv8 graph, one pass per layer instead of MIOpen's
 * conv + bias + SiLU + concat chains.  Activations are [batch*H*W, channels] with a row stride
 * (ld, in elements) so layers read / write channel slices of shared concat buffers.
 *
 * rva_conv2d_nhwc_f16: out = [SiLU](conv(in, weights) + bias) [+ residual]; ksize 1 or 3 (pad ksize/2),
 *   stride 1 or 2, Cin % 8 == 0, Cout % 8 == 0.  weights: float16 [rva_conv_cout_pad(Cout)][ksize*ksize][CinPad]
 *   with CinPad = Cin rounded up to 32 (padding rows / channels zero), bias: float32 [rva_conv_cout_pad(Cout)].
 *   MFMA implicit GEMM, fp32 accumulate.
 * rva_stem_conv_f16: first layer, 3x3 stride 2 on the PLANAR tensor K1 writes ([batch,3,H,W]);
 *   weights float16 [64][32]: row = output channel (zero beyond Cout); column order with j = c*3 + ky:
 *   k = 2*j + kx for kx in {0,1}, k = 18 + j for kx = 2, zero for k >= 27; bias float32 [64]; Cout <= 64; NHWC out.
 * rva_maxpool5_nhwc_f16 / rva_upsample2x_nhwc_f16: SPPF pooling, FPN nearest upsample, on channel slices.
 * rva_yolo_head_f16: DFL expectation + dist2bbox + sigmoid of one pyramid level into
 *   out[batch, 4+nc, anchors_total] at anchor_offset -- the `[B,84,8400]` tensor rva_postprocess_batch reads.
 *   nc, ldb, ldc % 8 == 0; batch, h, w > 0; 0 <= anchor_offset and anchor_offset + h*w <= anchors_total, else RVA_ERR_ARG
 *   before any launch.  Logits must be finite (the running maximum of the DFL softmax starts at -1e30, not -inf).
 * -------------------------------------------------------------------------------------------- */
int rva_conv_cout_pad(int Cout);
/* number of explicit kernel variants rva_conv2d_nhwc_f16_v accepts (1..N); the plan's autotuner iterates over them */
int rva_conv_num_variants(void);
/* printable name of a variant number ("auto" for 0, e.g. "big<256,128>" for 21): what tools/show_tuning.py prints and the
 * tables under profiles/ record.  NULL for a number no kernel is assigned to. */
const char *rva_conv_variant_name(int variant);
int rva_conv2d_nhwc_f16(rva_ctx *ctx, const void *in, int ldi, const void *weights, const float *bias,
                        void *out, int ldo, const void *residual, int ldr, int batch, int H, int W, int Cin,
                        int Cout, int ksize, int stride, int act, rva_stream_t stream);
/* Same with an explicit kernel variant, so that a plan can time the applicable variants per layer once and keep the
 * fastest (0 = heuristic; 1..rva_conv_num_variants() = one kernel family and tile each, one row each of the table
 * kConvVariants in csrc/rva_conv.hip: register-staged gather / resident-chunk / row-reuse kernels, and the LDS-DMA
 * large-tile kernels -- row reuse for 3x3 stride 1, gather with 64- or 32-channel K-steps for 1x1 and strided 3x3).
 * RVA_ERR_ARG if a variant does not apply to the shape. */
int rva_conv2d_nhwc_f16_v(rva_ctx *ctx, const void *in, int ldi, const void *weights, const float *bias,
                          void *out, int ldo, const void *residual, int ldr, int batch, int H, int W, int Cin,
                          int Cout, int ksize, int stride, int act, int variant, rva_stream_t stream);
/* Same restricted to the output rows [y0, y1) of every image (y1 < 0 = up to the last row): only those rows are computed and
 * written, bit-identical to the whole launch; input rows are read wherever the window's receptive field lies and zero padding
 * is decided in the whole image.  The LDS-DMA gather variants (33..42, 64, 65, 74..79; variant 0 where it picks one: 1x1 and
 * 3x3 stride 2 with Cin % 64 == 0) and the patch variants (43..51, 61..63, 66) take a window; RVA_ERR_ARG for any other
 * variant unless the window is the whole image. */
int rva_conv2d_nhwc_f16_rows(rva_ctx *ctx, const void *in, int ldi, const void *weights, const float *bias,
                             void *out, int ldo, const void *residual, int ldr, int batch, int H, int W, int Cin,
                             int Cout, int ksize, int stride, int act, int variant, int y0, int y1, rva_stream_t stream);
/* Rows of a convolution's output that depend on the input rows [lo, hi) of an image H_in rows high (host only; k = 1 or 3,
 * pad k / 2, stride 1 or 2): the half-open window [*out_lo, *out_hi), clamped to the output.  Every output row outside it sees
 * only input rows outside [lo, hi) and zero padding.  RVA_ERR_ARG for a window outside [0, H_in] or lo >= hi. */
int rva_conv_rows_through(int k, int stride, int H_in, int lo, int hi, int32_t *out_lo, int32_t *out_hi);
/* 1x1 convolution whose input is torch.cat([nearest-2x-upsample(low), skip], channel) -- the FPN pattern -- without
 * materialising either the upsampled tensor or the concatenation: low is [batch, H/2, W/2, c_low], skip is
 * [batch, H, W, c_skip] (row strides ld_low / ld_skip), weights [rva_conv_cout_pad(Cout)][1][c_low + c_skip].
 * c_low % 64 == c_skip % 64 == 0, H and W even.  variant: 0 or one of the LDS-DMA gather variants 33..39. */
int rva_conv1x1_upcat_f16(rva_ctx *ctx, const void *low, int ld_low, int c_low, const void *skip, int ld_skip,
                          int c_skip, const void *weights, const float *bias, void *out, int ldo, int batch,
                          int H, int W, int Cout, int act, int variant, rva_stream_t stream);
/* Last 1x1 convolution of a detect-head branch fused with the head decode: mode 1 = box branch (Cout = 64 DFL logits ->
 * expectation + dist2bbox, rows 0..3 of out), mode 2 = class branch (Cout = nc logits -> sigmoid, rows 4..4+nc), written
 * straight into out[batch, 4+nc, anchors_total] at anchor_offset -- the logits never reach HBM.  Same arithmetic and
 * rounding points as rva_conv2d_nhwc_f16 followed by rva_yolo_head_f16 (bit-identical).  Cin % 64 == 0; variant 0 or 33..39. */
int rva_conv1x1_head_f16(rva_ctx *ctx, const void *in, int ldi, const void *weights, const float *bias, int batch,
                         int H, int W, int Cin, int Cout, int mode, void *out, int nc, int anchors_total,
                         int anchor_offset, float stride_px, int variant, rva_stream_t stream);
/* The box branch (mode 1, Cout = 64) of rva_conv1x1_head_f16 with the fp32 side tensor: out is written exactly as
 * rva_conv1x1_head_f16 writes it (rows 0-3 bit-identical), and boxes32[batch, 4, anchors_total] (device float, anchor axis
 * contiguous, same anchor_offset) receives the fp32 values that were rounded into those rows: (half)boxes32 == rows 0-3 bit for
 * bit.  Nothing outside [anchor_offset, anchor_offset + H*W) is written in either tensor. */
int rva_conv1x1_head_box32_f16(rva_ctx *ctx, const void *in, int ldi, const void *weights, const float *bias, int batch,
                               int H, int W, int Cin, void *out, float *boxes32, int nc, int anchors_total, int anchor_offset,
                               float stride_px, int variant, rva_stream_t stream);
int rva_stem_conv_f16(rva_ctx *ctx, const void *in_planar, const void *weights, const float *bias,
                      void *out, int ldo, int batch, int H, int W, int Cout, rva_stream_t stream);

/* rva_c2f_pair32_f16: one C2f bottleneck with 32 channels and a shortcut -- y = x + SiLU(conv3x3(SiLU(conv3x3(x)))) -- in one launch;
 * replaces two session-internal Conv nodes + Add of the reference's ONNX graph (`session.run`, detector.py:597-609) and two
 * rva_conv2d_nhwc_f16 launches of this library, bit-identical to them (same operations, same order); the 32-channel intermediate
 * stays in LDS.  in / out: NHWC fp16 slices with row strides ldi / ldo (halfs, multiples of 8), 32 channels each, not overlapping;
 * w1, w2: [64][9][32] fp16 as rva_conv2d_nhwc_f16 takes them (rows >= 32 unused), b1, b2: [64] fp32. */
int rva_c2f_pair32_f16(rva_ctx *ctx, const void *in, int ldi, const void *w1, const float *b1, const void *w2, const float *b2, void *out,
                       int ldo, int batch, int H, int W, rva_stream_t stream);

/* rva_stem2_f16: the stem and the first downsampling convolution of YOLOv8s (3 -> 32 -> 64 channels, both 3x3 stride 2
 * pad 1 with bias + SiLU; ultralytics model.0 and model.1, reference call site detector.py:597-609 via the exported graph)
 * in ONE launch: the half-resolution 32-channel tensor stays in LDS.  in_planar, w1 ([64][32] fp16, column order of
 * rva_stem_conv_f16) and b1 ([64] fp32) as for rva_stem_conv_f16 with Cout = 32; w2 / b2 in the layout of
 * rva_conv2d_nhwc_f16 for Cin = 32, Cout = 64 ([64][9][32] fp16, [64] fp32); out: NHWC fp16 [batch, Ho, Wo, 64] with row
 * stride ldo (>= 64, multiple of 8), Ho = ((H-1)/2)/2 + 1.  W % 8 == 0.  Results equal stem -> conv up to fp32 summation
 * order inside the stem's 27-tap dot product. */
int rva_stem2_f16(rva_ctx *ctx, const void *in_planar, const void *w1, const float *b1, const void *w2, const float *b2,
                  void *out, int ldo, int batch, int H, int W, rva_stream_t stream);
/* Same for the rows [y0, y1) of the quarter-resolution output only (y1 < 0 = up to the last row), bit-identical to them */
int rva_stem2_f16_rows(rva_ctx *ctx, const void *in_planar, const void *w1, const float *b1, const void *w2, const float *b2,
                       void *out, int ldo, int batch, int H, int W, int y0, int y1, rva_stream_t stream);

/* SPPF's three chained 5x5/1 max pools in one launch: out1 = pool5(in), out2 = pool5(out1) = pool9(in),
 * out3 = pool5(out2) = pool13(in) (stride 1, -inf padding), all three with row stride ldo.  H*W*64 bytes must fit LDS
 * (H*W <= 2400); larger maps use rva_maxpool5_nhwc_f16 three times. */
int rva_sppf_pool3_nhwc_f16(rva_ctx *ctx, const void *in, int ldi, void *out1, void *out2, void *out3, int ldo,
                            int batch, int H, int W, int C, rva_stream_t stream);
int rva_maxpool5_nhwc_f16(rva_ctx *ctx, const void *in, int ldi, void *out, int ldo, int batch, int H,
                          int W, int C, rva_stream_t stream);
int rva_upsample2x_nhwc_f16(rva_ctx *ctx, const void *in, int ldi, void *out, int ldo, int batch, int H,
                            int W, int C, rva_stream_t stream);
int rva_yolo_head_f16(rva_ctx *ctx, const void *box_logits, int ldb, const void *cls_logits, int ldc,
                      void *out, int batch, int h, int w, int nc, int anchors_total, int anchor_offset,
                      float stride, rva_stream_t stream);
/* The three pyramid levels (strides 8 / 16 / 32) in one launch; arrays of 3, anchor offsets follow from h*w. */
int rva_yolo_head3_f16(rva_ctx *ctx, const void *const *box_logits, const int32_t *ldb, const void *const *cls_logits,
                       const int32_t *ldc, void *out, int batch, const int32_t *h, const int32_t *w, int nc,
                       int anchors_total, const float *strides, rva_stream_t stream);
/* rva_yolo_head_f16 / rva_yolo_head3_f16 with the fp32 side tensor boxes32[batch, 4, anchors_total] of the box rows (same contract
 * as rva_conv1x1_head_box32_f16: out bit-identical to the plain call, (half)boxes32 == rows 0-3, nothing outside the levels'
 * anchor ranges written). */
int rva_yolo_head_box32_f16(rva_ctx *ctx, const void *box_logits, int ldb, const void *cls_logits, int ldc, void *out,
                            float *boxes32, int batch, int h, int w, int nc, int anchors_total, int anchor_offset, float stride,
                            rva_stream_t stream);
int rva_yolo_head3_box32_f16(rva_ctx *ctx, const void *const *box_logits, const int32_t *ldb, const void *const *cls_logits,
                             const int32_t *ldc, void *out, float *boxes32, int batch, const int32_t *h, const int32_t *w, int nc,
                             int anchors_total, const float *strides, rva_stream_t stream);
/* Any class count (a detector trained on its own class list: one, three, twenty classes): the three head launches above for
 * 1 <= nc <= 1024 (K2's class-filter limit).  out stays exactly [batch, 4+nc, anchors_total] -- a 5-row head is read as plain
 * scores by rva_postprocess_batch, a wider one as objectness times classes, so the tensor is never widened -- and the kernels
 * are the ones of the entries above: they still load the class logits eight at a time and store only the class rows < nc, so
 * for nc % 8 == 0 the result is bit-identical to those entries.  boxes32 may be NULL (no side tensor) or is written as by the
 * _box32 forms.
 *   rva_yolo_head_nc_f16 / rva_yolo_head3_nc_f16: ldb, ldc % 8 == 0 and ldc >= roundup(nc, 8): a class row holds the nc logits
 *     and pad columns up to the next multiple of 8 at least.  The pad columns may hold anything, NaN included: nothing of them
 *     reaches out.
 *   rva_conv1x1_head_nc_f16: mode 1 (Cout = 64; boxes32 optional) and mode 2 (Cout = roundup(nc, 8), weights and bias of the
 *     output channels >= nc are the caller's padding, zero in the plan; boxes32 must be NULL), Cin % 64 == 0, and the level
 *     must lie inside the anchor range.
 * Anything else returns RVA_ERR_ARG before any launch: nothing is written. */
int rva_yolo_head_nc_f16(rva_ctx *ctx, const void *box_logits, int ldb, const void *cls_logits, int ldc, void *out,
                         float *boxes32, int batch, int h, int w, int nc, int anchors_total, int anchor_offset, float stride,
                         rva_stream_t stream);
int rva_yolo_head3_nc_f16(rva_ctx *ctx, const void *const *box_logits, const int32_t *ldb, const void *const *cls_logits,
                          const int32_t *ldc, void *out, float *boxes32, int batch, const int32_t *h, const int32_t *w, int nc,
                          int anchors_total, const float *strides, rva_stream_t stream);
int rva_conv1x1_head_nc_f16(rva_ctx *ctx, const void *in, int ldi, const void *weights, const float *bias, int batch,
                            int H, int W, int Cin, int Cout, int mode, void *out, float *boxes32, int nc, int anchors_total,
                            int anchor_offset, float stride_px, int variant, rva_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * fp32 detector primitives (NHWC float32) -- the reference's default precision (`half: false`: an fp32
 * ONNX Runtime graph, detector.py:248-251, 597-609), everything fp32 in and out.
 *
 * rva_conv2d_nhwc_f32_v: out = [SiLU](conv(in, weights) + bias) [+ residual]; ksize 1 or 3 (pad ksize/2), stride 1 or 2,
 *   Cin % 16 == 0, row strides ldi (multiple of 4) / ldo / ldr in floats; in and weights 16-byte aligned.  weights: float32
 *   [Cout][ksize*ksize][Cin] (no padding), bias float32 [Cout] or NULL.  Implicit GEMM on the exact fp32-input MFMA; the
 *   k*k*Cin sum of an output element runs in ONE fixed order for every variant and every batch size (no split-K), so results
 *   are bit-identical across variants 1..rva_conv_f32_num_variants() and 0 (= heuristic).  Only channels [0, Cin) of the
 *   input slice are read and only channels [0, Cout) of the output slice are written.
 * rva_stem_conv_f32: 3x3 stride 2 pad 1 + SiLU on the PLANAR fp32 [batch,3,H,W] tensor K1 writes for half=0; weights = the
 *   checkpoint's float32 [Cout][3][3][3], Cout % 4 == 0; NHWC out with row stride ldo.
 * rva_maxpool5_nhwc_f32 / rva_upsample2x_nhwc_f32: SPPF pooling (5x5, stride 1, -inf padding), FPN nearest 2x upsample, on
 *   channel slices (C, ldi, ldo multiples of 4).
 * rva_yolo_head_f32: one pyramid level, the module's formula in fp32: DFL softmax (max-subtracted) -> expectation ->
 *   xywh = ((x1y1 + x2y2) / 2, x2y2 - x1y1) * stride, sigmoid scores, into out[batch, 4+nc, anchors_total] at anchor_offset.
 * -------------------------------------------------------------------------------------------- */
int rva_conv_f32_num_variants(void);
int rva_conv2d_nhwc_f32_v(rva_ctx *ctx, const void *in, int ldi, const void *weights, const float *bias,
                          void *out, int ldo, const void *residual, int ldr, int batch, int H, int W, int Cin,
                          int Cout, int ksize, int stride, int act, int variant, rva_stream_t stream);
int rva_stem_conv_f32(rva_ctx *ctx, const void *in_planar, const void *weights, const float *bias,
                      void *out, int ldo, int batch, int H, int W, int Cout, rva_stream_t stream);
int rva_maxpool5_nhwc_f32(rva_ctx *ctx, const void *in, int ldi, void *out, int ldo, int batch, int H,
                          int W, int C, rva_stream_t stream);
int rva_upsample2x_nhwc_f32(rva_ctx *ctx, const void *in, int ldi, void *out, int ldo, int batch, int H,
                            int W, int C, rva_stream_t stream);
int rva_yolo_head_f32(rva_ctx *ctx, const void *box_logits, int ldb, const void *cls_logits, int ldc,
                      void *out, int batch, int h, int w, int nc, int anchors_total, int anchor_offset,
                      float stride, rva_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * The fused YOLOv8 detector as ONE object (round 4) -- replaces `self.session.run` of the reference's ONNX Runtime
 * backend (/root/reference/src/realtime_analytics/detector.py:597-609; the network it runs is the exported ultralytics graph,
 * detector.py:575-586) for `half: true` (fp16 operands, fp32 accumulation) or, with RVA_PLAN_F32 in desc.flags, for
 * `half: false` in the reference's own fp32 precision.
 *
 * rva_yolov8_plan_create: `convs` = the network's n_convs convolutions with BatchNorm folded, in MODULE ORDER, each in the
 *   checkpoint's own layout (fp32 host arrays, weight [cout][cin][k][k], bias [cout] or NULL).  Module order: b0, b1, C2f(b2), b3,
 *   C2f(b4), b5, C2f(b6), b7, C2f(b8), SPPF(b9) = cv1 cv2, C2f(h12), C2f(h15), h16, C2f(h18), h19, C2f(h21), detect.box[0..2][0..2],
 *   detect.cls[0..2][0..2]; C2f(x) = cv1, cv2, then cv1 cv2 of every bottleneck (ultralytics model.0 .. model.22).  The call
 *   checks every shape against the descriptor (RVA_ERR_ARG names the first convolution that does not fit), packs the weights
 *   for the kernels above, allocates all activation buffers in HBM and lays down the static list of launches.
 * rva_yolov8_plan_run: input = fp16 planar [batch,3,height,width] (what rva_preprocess_* writes), output = fp16
 *   [batch, 4+nc, anchors] (fp32 input and output for an RVA_PLAN_F32 plan; what rva_postprocess_batch reads; anchors = H/8*W/8 + H/16*W/16 + H/32*W/32); every launch of the
 *   forward pass goes to `stream`, no host synchronisation, no allocation: capturable.  _run_lanes additionally forks the
 *   stride-8 / stride-16 detect branches onto two side streams (events inside the plan) and joins them at the end: +6 % for one
 *   pass at a time; with several passes in flight use _run.  _run_range(first, last) replays steps [first, last)
 *   (`quiet_step`: where the pass enters its 20x20 layers).
 * Kernel selection: every convolution step ("tunable") carries a kernel variant of rva_conv2d_nhwc_f16_v (0 = heuristic).
 *   A tuner times rva_yolov8_plan_launch_tunable(index, variant) on the plan's own buffers (RVA_ERR_ARG = variant does not
 *   apply to that layer) and fixes its choice with _set_variant; _tunable_desc gives "Cin->Cout kKsS HxW" (the key of a
 *   persisted selection).  Results do not depend on the variant beyond fp32 summation order.
 * RVA_PLAN_F32: the same graph, plan object and entry points with fp32 activation buffers and the fp32 primitives above (one
 *   stem launch, one convolution launch per Conv-BN-SiLU, three pool launches for SPPF, upsample launches into the concat
 *   buffers, one head launch per level on the level's detect lane); the tunable steps carry rva_conv2d_nhwc_f32_v variants, and
 *   the output does not depend on them at all (bit-identical).  RVA_PLAN_NO_STEM2 / NO_CIN_PAD / NO_PAIR32 have no effect on it.
 * RVA_PLAN_BOX_F32 (fp16 plans only, opt-in): the fp16 head's box rows carry the fp16 ulp (0.25 px between 256 and 512, 0.5 px
 *   above) although DFL + dist2bbox are computed in fp32.  With the flag the head kernels store those fp32 values as well:
 *   `output` of every run entry point is then ONE buffer of rva_yolov8_plan_output_layout's total_bytes -- the fp16 head
 *   [batch, 4+nc, anchors], written in full and bit-identical to the plan without the flag, followed at boxes_offset (a
 *   multiple of 256) by float boxes32[batch, 4, anchors] = cx, cy, w, h in input pixels, with (half)boxes32 == rows 0-3.  Feed
 *   both to rva_postprocess_boxes_batch.  Same launches, same kernel selection, still no allocation and no synchronisation.
 *   Without the flag boxes_offset is -1 and total_bytes is the size of the head tensor.
 * Static rows (fp16 plans): rva_yolov8_plan_set_static_rows(plan, top, bottom) is the caller's promise that the rows outside
 *   [top, bottom) of every image of `input` hold the same bytes on every later run until the next call (a letterbox border).
 *   Every step then carries the window of its output rows that depend on [top, bottom) (rva_conv_rows_through chained through
 *   the graph, _step_rows reads it); the other rows come out the same on every run.  The call, like create and _set_variant,
 *   leaves the plan unprimed: the next complete run (_run / _run_lanes, not under stream capture) launches every step over all
 *   rows and primes it, and from then on the steps whose kernel takes a row window (rva_conv2d_nhwc_f16_rows,
 *   rva_stem2_f16_rows) launch their window only.  Steps of other kernels keep running all rows.  _run_range never primes and
 *   launches windows only on a primed plan; a run under stream capture launches by the flag as it stands and leaves it alone.
 *   (0, height) switches windowing off (the default).  RVA_ERR_ARG for a window outside [0, height] or top >= bottom.  fp32
 *   plans accept the call and stay un-windowed.  RVA_PLAN_NO_STATIC_ROWS=1 in the environment makes the call a no-op (A/B).
 *   _tunable_desc carries a window that is not the whole image (" r[y0,y1)"): such layers are tuned, and persisted, apart.
 * Capacity (_run_n / _run_lanes_n / _run_range_n): desc.batch is the plan's capacity B, and a call runs the n leading images,
 *   1 <= n <= B (RVA_ERR_ARG otherwise, before anything is launched): input = [n,3,height,width]; images [0, n) of `output` are
 *   written, which keeps the layout [B, 4+nc, anchors] -- with RVA_PLAN_BOX_F32 boxes32 stays at the boxes_offset that
 *   _output_layout reports for B.  Image b lies where it lies in a full run, and nothing of the images >= n is written, in
 *   `output` or in any activation buffer.  Every step launches the kernel a full run launches -- variant 0 chooses from B, not from
 *   n -- so images [0, n) are bit-identical to the same images of a full run on the same plan, fp16 and fp32, whatever the images
 *   >= n hold.  _run / _run_lanes / _run_range are the _n forms with n = B.  (One plan of the largest batch serves every
 *   smaller one: no second set of buffers, weights or kernel selections, and a stream's result does not depend on how many
 *   other streams delivered a frame.)
 *   Static rows with a capacity: "primed" is a count P of leading images whose buffers hold a whole run's rows for the current
 *   windows and variants (_primed_images reads it).  Create, _set_static_rows and _set_variant set P = 0.  A complete run
 *   (_run_n / _run_lanes_n) outside stream capture launches row windows if n <= P; otherwise it launches all rows of all n
 *   images and sets P = n.  _run_range_n never changes P and launches windows only if n <= P; a run under stream capture
 *   launches by P as it stands and leaves it alone.  The promise of _set_static_rows covers every image the caller passes.
 *   Precondition (fp16 plans): a convolution whose Cin is not a multiple of 32 runs with Cin rounded up and zero weights for
 *   the extra channels, so it reads up to 31 channels past its slice: the next slice of the row, the next pixel or, behind the
 *   last pixel of image n - 1, stale bytes of image n.  Those bytes are multiplied by zero and must be FINITE.  Create
 *   zero-fills every buffer and every kernel writes finite values for finite inputs and weights, so the precondition holds as
 *   long as no run was fed non-finite input or weights; after such a run the images it covered must be run again with finite
 *   input (all rows: _set_static_rows first) before a smaller n is trusted.
 * Class count: desc.nc is any 1 <= nc <= 1024 (1024: K2's class-filter limit), in fp16 and fp32 plans.  `convs` are the
 *   module's own: the class branch with its real widths (interior max(c3, min(nc, 100)), last convolution Cout = nc).  Inside
 *   the plan every channel count of that branch the kernels need aligned is rounded up -- to 8 (fp16), to 16 where an fp32
 *   convolution reads it as Cin, the class logits to roundup(nc, 8) columns -- and weights and biases are zero-extended at
 *   upload: a pad channel is SiLU(0) = 0 and meets zero weights, so the result equals, bit for bit, a plan of the padded module.
 *   Output, _info (out_rows = 4 + nc) and _output_layout keep the real nc: the head tensor is exactly [batch, 4+nc, anchors].
 *   Where the branch widths allow the fused decode (box and padded class width multiples of 64: every scale for nc <= 64) the
 *   launch structure is the one of nc = 80; otherwise the plan ends in one rva_yolo_head3_nc_f16 launch.
 * -------------------------------------------------------------------------------------------- */
#define RVA_PLAN_NO_STEM2 1   /* rva_yolov8_desc.flags: stem and first downsampling convolution as two launches (A/B switch) */
#define RVA_PLAN_NO_CIN_PAD 2 /* ... convolutions with Cin % 32 != 0 keep their Cin (default: declared rounded up to 32, zero weights) */
#define RVA_PLAN_NO_PAIR32 4  /* ... the 32-channel C2f bottlenecks (YOLOv8s at 160 x 160) as two convolution launches instead of rva_c2f_pair32_f16 */
#define RVA_PLAN_F32 8        /* ... fp32 plan: fp32 input, buffers, weights and output (every convolution's Cin % 16 == 0) */
#define RVA_PLAN_BOX_F32 16   /* ... fp16 plan whose head kernels also write the four box rows as fp32 (see RVA_PLAN_BOX_F32 above); RVA_ERR_ARG with RVA_PLAN_F32 */
typedef struct rva_yolov8_plan rva_yolov8_plan;
typedef struct rva_yolov8_desc {
    int32_t batch, height, width;     /* input tensor; height and width multiples of 32 */
    int32_t widths[5];                /* c1..c5 (YOLOv8s: 32 64 128 256 512) */
    int32_t depth_backbone[4];        /* bottlenecks of the C2f blocks b2, b4, b6, b8 (YOLOv8s: 1 2 2 1) */
    int32_t depth_head;               /* bottlenecks of h12, h15, h18, h21 (YOLOv8s: 1) */
    int32_t nc, reg_max;              /* classes (1..1024, see "Class count" above), DFL bins (16) */
    int32_t n_convs;                  /* length of `convs` */
    int32_t flags;
} rva_yolov8_desc;
typedef struct rva_conv_weights {
    const float *weight;              /* [cout][cin][k][k] */
    const float *bias;                /* [cout] or NULL */
    int32_t cout, cin, k, stride;
} rva_conv_weights;
int rva_yolov8_plan_create(rva_ctx *ctx, const rva_yolov8_desc *desc, const rva_conv_weights *convs, rva_yolov8_plan **out);
void rva_yolov8_plan_destroy(rva_yolov8_plan *plan);
int rva_yolov8_plan_info(const rva_yolov8_plan *plan, int32_t *anchors, int32_t *out_rows, int32_t *n_steps, int32_t *n_tunable,
                         int32_t *quiet_step);
int rva_yolov8_plan_output_layout(const rva_yolov8_plan *plan, int64_t *total_bytes, int64_t *boxes_offset);
int rva_yolov8_plan_run(rva_yolov8_plan *plan, const void *input, void *output, rva_stream_t stream);
int rva_yolov8_plan_run_lanes(rva_yolov8_plan *plan, const void *input, void *output, rva_stream_t stream, rva_stream_t side1,
                              rva_stream_t side2);
int rva_yolov8_plan_run_range(rva_yolov8_plan *plan, const void *input, void *output, int first, int last, rva_stream_t stream);
int rva_yolov8_plan_tunable_desc(const rva_yolov8_plan *plan, int index, char *buf, int len);
int rva_yolov8_plan_launch_tunable(rva_yolov8_plan *plan, int index, int variant, void *output, rva_stream_t stream);
int rva_yolov8_plan_set_variant(rva_yolov8_plan *plan, int index, int variant);
int rva_yolov8_plan_get_variant(const rva_yolov8_plan *plan, int index);
int rva_yolov8_plan_set_static_rows(rva_yolov8_plan *plan, int top, int bottom);
int rva_yolov8_plan_run_n(rva_yolov8_plan *plan, const void *input, void *output, int n, rva_stream_t stream);
int rva_yolov8_plan_run_lanes_n(rva_yolov8_plan *plan, const void *input, void *output, int n, rva_stream_t stream, rva_stream_t side1,
                                rva_stream_t side2);
int rva_yolov8_plan_run_range_n(rva_yolov8_plan *plan, const void *input, void *output, int n, int first, int last, rva_stream_t stream);
int rva_yolov8_plan_primed_images(const rva_yolov8_plan *plan);
int rva_yolov8_plan_step_rows(const rva_yolov8_plan *plan, int step, int32_t *y0, int32_t *y1);
/* What step `step` (0 .. n_steps - 1) of the launch list is, for reports and tests: the tunable description of a convolution
 * step ("64->128 k3s2 80x80", with its row window), else the kernel and its shape: "attention heads 2 tokens 400",
 * "dwconv3x3 64 act1 80x80", "sppf pool3 128 20x20", "stem 3->16 k3s2 640x640", "head3 decode". */
int rva_yolov8_plan_step_desc(const rva_yolov8_plan *plan, int step, char *buf, int len);

/* ----------------------------------------------------------------------------------------------
 * YOLOv5 (v6.0 - v7.0 architecture, n / s / m / l; `model_type: yolov5`, whose objectness rule the reference's post-process
 * applies, detector.py:294-305) as a second graph builder for the SAME plan object: every rva_yolov8_plan_* entry point above
 * works on a plan made by rva_yolov5_plan_create unchanged.  fp16 only (RVA_PLAN_F32: RVA_ERR_ARG); RVA_PLAN_BOX_F32 and
 * RVA_PLAN_NO_CIN_PAD as above; the other flags have no effect.  There are no detect lanes: _run_lanes is _run.
 * Output: fp16 [batch, 5+nc, anchors], anchors = 3 * (H/8*W/8 + H/16*W/16 + H/32*W/32), anchor index = level offset +
 * a * h * w + y * w + x -- the transpose of the exported graph's [batch, anchors, 5+nc], which rva_postprocess_batch reads
 * through its strides.  _info reports out_rows = 5 + nc.
 *
 * Graph: b0 stem 6x6 s2 p2 | b1 3x3 s2 | b2 C3 | b3 3x3 s2 | b4 C3 | b5 3x3 s2 | b6 C3 | b7 3x3 s2 | b8 C3 | b9 SPPF | h10 1x1 |
 *   h13 C3(cat[up(h10), p4]) | h14 1x1 | h17 C3(cat[up(h14), p3]) | h18 3x3 s2 | h20 C3(cat[h18, h14]) | h21 3x3 s2 |
 *   h23 C3(cat[h21, h10]) | per level Conv2d(ch, 3 * (5 + nc), 1) fused with the anchor decode (rva_conv1x1_head5_f16).
 * Module order of `convs`: b0, b1, C3(b2), b3, C3(b4), b5, C3(b6), b7, C3(b8), SPPF cv1 cv2, h10, C3(h13), h14, C3(h17), h18,
 *   C3(h20), h21, C3(h23), detect.m[0..2];  C3(x) = cv1, cv2, cv3, then cv1 (1x1) cv2 (3x3) of every bottleneck.
 * C3 inside the plan: cv1 and cv2 read the same input and run as ONE launch that writes [cv1 out | cv2 out]; the last
 *   bottleneck writes behind them, and cv3 reads [cv2 out | m out] with its input channels swapped half for half on the host --
 *   the concatenation never materialises, and only the summation order of cv3 differs from the module's.
 *
 * rva_stem6_conv_f16: the stem, 6x6 stride 2 pad 2 + bias + SiLU on the PLANAR tensor K1 writes ([batch,3,H,W] fp16), NHWC fp16
 *   out [batch, H/2, W/2, Cout] with row stride ldo.  weights fp16 [64][128]: row = output channel (zero beyond Cout), column
 *   k = (c*6 + ky)*6 + kx -- the checkpoint's own [Cout][3][6][6] order -- zero for k >= 108; bias fp32 [Cout].  Cout % 8 == 0,
 *   8 <= Cout <= 64, W % 8 == 0, H even, ldo % 8 == 0.  fp32 accumulation of the 108 products in four MFMA steps of 32, one
 *   rounding to fp16 after SiLU.  _rows: output rows [y0, y1) only (y1 < 0 = the last row), bit-identical to them; output row r
 *   reads input rows 2r-2 .. 2r+3 (rva_conv_rows_through_pad(6, 2, 2, ...)).
 * rva_conv_rows_through_pad: rva_conv_rows_through for any k >= 1, stride >= 1 and 0 <= pad < k.
 * rva_conv1x1_head5_f16: one level's Conv2d(Cin, 3 * (5 + nc), 1) fused with the decode, written straight into
 *   out[batch, 5+nc, anchors_total] at anchors [anchor_offset, anchor_offset + 3*H*W).  weights fp16
 *   [rva_conv_cout_pad(Cout)][1][Cin] and bias fp32 [rva_conv_cout_pad(Cout)] with Cout = roundup(3 * (5 + nc), 8), rows >=
 *   3 * (5 + nc) zero (never stored); channel a * (5 + nc) + j = anchor a, entry j.  anchors_px: DEVICE float [6], the level's
 *   three (w, h) pairs in pixels.  Rounding points: the logit z (fp32 accumulator + bias) is rounded to fp16 once; then in fp32,
 *   in this order, y = 1 / (1 + exp(-z)) (v_exp_f32 / v_rcp_f32); entry 0: ((y * 2 - 0.5) + x) * stride_px, entry 1 the same with
 *   y of the grid; entries 2 / 3: t = y * 2, (t * t) * anchor w / h; entries >= 4: y; each rounded once to fp16.  boxes32 (NULL =
 *   none): fp32 [batch, 4, anchors_total] receives the fp32 values of entries 0-3 before that last rounding, so (half)boxes32 ==
 *   rows 0-3 bit for bit; nothing outside the level's anchor range is written in either tensor.  1 <= nc <= 1024,
 *   Cin % 64 == 0; variant 0 or 33..39.  No split-K, no atomics: bit-identical across batch sizes.
 * -------------------------------------------------------------------------------------------- */
typedef struct rva_yolov5_desc {
    int32_t batch, height, width;     /* input tensor; height and width multiples of 32 */
    int32_t widths[5];                /* c1..c5 (YOLOv5s: 32 64 128 256 512); c1 <= 64, c3 and c4 multiples of 64 */
    int32_t depth_backbone[4];        /* bottlenecks of the C3 blocks b2, b4, b6, b8 (YOLOv5s: 1 2 3 1) */
    int32_t depth_head;               /* bottlenecks of h13, h17, h20, h23 (YOLOv5s: 1) */
    int32_t nc;                       /* classes, 1..1024 */
    float anchors[18];                /* [level][anchor][(w, h)] in input pixels */
    int32_t n_convs;                  /* length of `convs` */
    int32_t flags;
} rva_yolov5_desc;
int rva_yolov5_plan_create(rva_ctx *ctx, const rva_yolov5_desc *desc, const rva_conv_weights *convs, rva_yolov8_plan **out);
int rva_stem6_conv_f16(rva_ctx *ctx, const void *in_planar, const void *weights, const float *bias, void *out, int ldo,
                       int batch, int H, int W, int Cout, rva_stream_t stream);
int rva_stem6_conv_f16_rows(rva_ctx *ctx, const void *in_planar, const void *weights, const float *bias, void *out, int ldo,
                            int batch, int H, int W, int Cout, int y0, int y1, rva_stream_t stream);
int rva_conv_rows_through_pad(int k, int stride, int pad, int H_in, int lo, int hi, int32_t *out_lo, int32_t *out_hi);
int rva_conv1x1_head5_f16(rva_ctx *ctx, const void *in, int ldi, const void *weights, const float *bias, int batch, int H, int W,
                          int Cin, int nc, const float *anchors_px, void *out, float *boxes32, int anchors_total, int anchor_offset,
                          float stride_px, int variant, rva_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * YOLO11 (n / s / m / l of Ultralytics 8.3, the `yolo11<scale>` file names; there is no model_type of its own) as a third graph
 * builder for the SAME plan object: every rva_yolov8_plan_* entry point above works on a plan made by rva_yolo11_plan_create
 * unchanged.  fp16 only (RVA_PLAN_F32: RVA_ERR_ARG); RVA_PLAN_BOX_F32, RVA_PLAN_NO_STEM2 and RVA_PLAN_NO_CIN_PAD as above; the
 * other flags have no effect.  There are no detect lanes: _run_lanes is _run.  Output: YOLOv8's fp16 [batch, 4+nc, anchors].
 *
 * Graph (layer numbers of yolo11.yaml; w1..w5 = widths):
 *   0 stem 3x3 s2 w1 | 1 3x3 s2 w2 | 2 C3k2 w3 (e 0.25) | 3 3x3 s2 w3 | 4 C3k2 w4 (e 0.25) | 5 3x3 s2 w4 | 6 C3k2 w4 | 7 3x3 s2 w5 |
 *   8 C3k2 w5 | 9 SPPF | 10 C2PSA | 13 C3k2(cat[up(10), 6]) w4 | 16 C3k2(cat[up(13), 4]) w3 | 17 3x3 s2 | 19 C3k2(cat[17, 13]) w4 |
 *   20 3x3 s2 | 22 C3k2(cat[20, 10]) w5 | detect(16, 19, 22): box = 3x3, 3x3, 1x1 (64) as YOLOv8; cls = dw3x3, 1x1, dw3x3, 1x1, 1x1 (nc).
 *   C3k2(c2, e): c = c2 * e; cv1 1x1 -> 2c; n inner blocks on the last chunk; cv2 1x1 (2 + n) c -> c2.  Inner block: a
 *   bottleneck 3x3 c -> c/2, 3x3 c/2 -> c, or with c3k a C3 at width c/2 with two bottlenecks 3x3, 3x3 (it writes its cv3 into the
 *   outer concat slice).  The shortcut is added in layers 2-8 and not behind them.
 *   C2PSA: cv1 1x1 w5 -> [a | b] (two launches: `a` goes into cv2's input buffer, `b` into its own), psa_blocks times
 *   b <- b + proj(attention(qkv(b)) + pe(v)); b <- b + ffn1(ffn0(b)), the last one into cv2's input buffer; cv2 1x1.
 *   qkv / proj / ffn are rva_conv2d_nhwc_f16 (proj and ffn1 with act 0 and the residual); attention is rva_psa_attention_f16 on
 *   the qkv buffer as the convolution wrote it; pe is rva_dwconv3x3_nhwc_f16 once per head on the head's v slice with the head's
 *   attention output as the residual (a head's 64 v channels are contiguous, the heads' are not).
 * Module order of `convs`: layers 0..22 in order, then per level box[l][0..2], then per level cls[l] = dw, 1x1, dw, 1x1, 1x1;
 *   C3k2(x) = cv1, cv2, then per inner block cv1, cv2 (bottleneck) or cv1, cv2, cv3, m0.cv1, m0.cv2, m1.cv1, m1.cv2 (C3k);
 *   SPPF = cv1, cv2; C2PSA = cv1, cv2, then per block qkv, proj, pe, ffn0, ffn1.  A depthwise convolution is an
 *   rva_conv_weights with cin = 1: weight [C][1][3][3].
 * Refused (RVA_ERR_ARG): height or width not a multiple of 32, nc outside 1..1024, widths not multiples of 8, RVA_PLAN_F32,
 *   psa_heads * 64 != w5 / 2, w1 > 64 ("stem wider than 64 channels": scale x).
 *
 * rva_dwconv3x3_nhwc_f16: out[n,y,x,c] = [SiLU](sum_{ky,kx} in[n,y+ky-1,x+kx-1,c] * w[c][ky][kx] + bias[c]) [+ residual[n,y,x,c]]
 *   on NHWC fp16 channel slices (row strides ldi, ldo, ldr in elements), stride 1, zero padding.  weights: fp16 [9][C], tap
 *   ky * 3 + kx major (the transpose of the checkpoint's [C][1][3][3]: a lane's 8 channels of a tap are one 16-byte load);
 *   bias fp32 [C]; residual NULL = none; act 1 = SiLU, 0 = none.  The nine products are added in fp32 from zero in the order
 *   (ky, kx), then the bias, SiLU, the residual; one rounding to fp16.  RVA_ERR_ARG before any launch unless batch, H, W > 0,
 *   C % 8 == 0, ldi / ldo / ldr >= C and multiples of 8, and every pointer 16-byte aligned.  `out` may not overlap `in`.
 * rva_psa_attention_f16: multi-head self-attention over `tokens` positions.  qkv fp16 [batch, tokens, ld]: head h owns channels
 *   [128 h, 128 h + 128) = q 32 | k 32 | v 64 -- what the qkv 1x1 convolution writes in NHWC.  out fp16 [batch, tokens, ldo], head
 *   h at channels [64 h, 64 h + 64).  Per (image, head, query): S = q . k (v_mfma_f32_32x32x16_f16, fp32), * 32^-0.5 in fp32,
 *   max-subtracted softmax in fp32 (online over key tiles of 32 in order; keys >= tokens are masked and never read), P rounded
 *   to fp16, O = P V with fp32 accumulators, O / (fp32 row sum), one rounding to fp16.  The order of every sum depends on
 *   `tokens` alone: an image's result does not depend on batch.  RVA_ERR_ARG before any launch unless batch, tokens, heads >= 1,
 *   ld >= 128 heads, ldo >= 64 heads, ld and ldo multiples of 8, and both pointers 16-byte aligned.
 * -------------------------------------------------------------------------------------------- */
typedef struct rva_yolo11_desc {
    int32_t batch, height, width;     /* input tensor; height and width multiples of 32 */
    int32_t widths[5];                /* w1..w5 (YOLO11n: 16 32 64 128 256); w1 <= 64 */
    int32_t repeats[8];               /* inner blocks of the C3k2 layers 2, 4, 6, 8, 13, 16, 19, 22 (YOLO11n: all 1) */
    int32_t c3k[8];                   /* ... and whether they are C3k (YOLO11n / s: 0 0 1 1 0 0 0 1; m / l: all 1) */
    int32_t psa_blocks, psa_heads;    /* C2PSA: blocks (1; l: 2) and heads = w5 / 128 */
    int32_t nc;                       /* classes, 1..1024 */
    int32_t n_convs;                  /* length of `convs` */
    int32_t flags;
} rva_yolo11_desc;
int rva_yolo11_plan_create(rva_ctx *ctx, const rva_yolo11_desc *desc, const rva_conv_weights *convs, rva_yolov8_plan **out);
int rva_dwconv3x3_nhwc_f16(rva_ctx *ctx, const void *in, int ldi, const void *weights, const float *bias, void *out, int ldo,
                           const void *residual, int ldr, int batch, int H, int W, int C, int act, rva_stream_t stream);
int rva_psa_attention_f16(rva_ctx *ctx, const void *qkv, int ld, void *out, int ldo, int batch, int tokens, int heads,
                          rva_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * The CNN-LSTM clip network as ONE fp32 object -- replaces the network call of the reference's CNN-LSTM head
 * (the inference call of CNNLSTMDetector._predict_sequence, temporal_detector.py:382-388; the network is
 * DummyCNNLSTM of scripts/convert_temporal_model_to_onnx.py:34-88) and its top-5 (temporal_detector.py:392-424), for `half:
 * false`.  Per frame: Conv2d(3,64,7,s2,p3)+BN+ReLU -> MaxPool(3,s2,p1) -> Conv2d(64,128,3,p1)+BN+ReLU -> mean over H,W; per
 * clip: 2-layer LSTM(128 -> hidden, gates i,f,g,o) -> Linear(hidden -> classes) on the last step.
 *
 * rva_cnnlstm_plan_create: `weights` = the module's tensors in the field order of rva_cnnlstm_weights as fp32 host arrays (all
 *   required): conv1 weight [64][3][7][7] and bias [64], conv2 weight [128][64][3][3] and bias [128], each with its BatchNorm folded in; LSTM layer 1
 *   weight_ih [4h][128], bias_ih + bias_hh [4h], weight_hh [4h][h]; layer 2 weight_ih [4h][h], weight_hh [4h][h], bias_ih +
 *   bias_hh [4h]; head weight [classes][h] and bias [classes] (gate rows in PyTorch's order i, f, g, o).  The plan copies and
 *   packs them, and allocates its whole workspace for desc.max_clips clips (frames 1..64, hidden 1..1024, classes 1..16384).
 * rva_cnnlstm_plan_run: frames = a device ring of planar fp32 frames [3][height][width] (what rva_preprocess_frames_* writes
 *   with RVA_NORM_IMAGENET_F32); frame_index = device int32 [n_clips * frames]: frame t of clip b is ring + frame_index[b*T+t] *
 *   3*height*width (no gathered copy).  logits = device fp32 [n_clips][classes], the raw outputs (no softmax).  Every launch
 *   goes to `stream`; no host synchronisation, no allocation: capturable.  Each sum runs in one fixed order (no split-K that
 *   follows the grid, no atomics): a clip's logits are bit-identical for every batch size, position in the batch and launch
 *   mode.
 * rva_cnnlstm_plan_run_post: one result row per stream of the tick.  rows = device int32 [n_rows][3]: (clip of the row or -1,
 *   frame width, frame height).  A row with a clip gets the top k = min(5, classes) of its logits in the reference's order
 *   (ascending stable sort, last k reversed: exact ties rank the larger class index first, NaN ranks above every number as in torch.sort) in scores[row][0..k) / cls, boxes
 *   (0, 0, w, h) and counts[row] = k; a row without one gets counts[row] = 0.  scores / boxes / cls have row stride max_det
 *   (>= k) as in the post-process buffers of rva_postprocess_batch.
 * rva_cnnlstm_plan_info: pooled map size (height / width after the max pool), conv2 tiles per frame, launches per _run.
 * rva_cnnlstm_plan_stage: a read-only tap on the workspace for tests and tools: ONE device-to-device copy on `stream` of the
 *   first n_clips clips' worth of one intermediate tensor into dst (device fp32, dst_floats elements of room), the element
 *   count in *n_floats (may be NULL).  Valid after a _run of at least n_clips clips on the same stream, until the next _run.
 *   dst == NULL only reports the count.  RVA_ERR_ARG (and no copy) for a null plan, an unknown stage, n_clips outside
 *   1..max_clips or dst_floats below the count.  _run neither changes nor gains a launch.  With n = n_clips, T = frames,
 *   h = hidden, Hp x Wp the pooled map and P = Hp * Wp:
 *     RVA_CNNLSTM_STAGE_POOLED   [n*T][Hp][Wp][64]          stem output: conv1 + BN + ReLU + max pool, channels last
 *     RVA_CNNLSTM_STAGE_PARTIAL  [n*T][conv2_tiles][128]    per-tile channel sums of ReLU(conv2 + BN); tile k holds pixels
 *                                                           256k .. min(256k + 255, P - 1) of the raster [Hp][Wp]
 *     RVA_CNNLSTM_STAGE_FEAT     [n*T][128]                 the spatial mean: tile sums in tile order, divided by P
 *     RVA_CNNLSTM_STAGE_GX       [n][T][4h]                 layer 1's input projection feat . W_ih1^T + (b_ih1 + b_hh1)
 *     RVA_CNNLSTM_STAGE_H1 / H2  [T][n][h]                  hidden state of LSTM layer 1 / 2 at every step (the workspace
 *                                                           keeps max_clips rows per step; the tap copies n of them)
 * -------------------------------------------------------------------------------------------- */
typedef struct rva_cnnlstm_plan rva_cnnlstm_plan;
typedef struct rva_cnnlstm_desc {
    int32_t height, width;            /* frame size of the clip (224 x 224 by default) */
    int32_t frames;                   /* T = sequence_length */
    int32_t hidden, classes;
    int32_t max_clips;                /* capacity: the most clips one _run may take */
} rva_cnnlstm_desc;
typedef struct rva_cnnlstm_weights {
    const float *conv1_w, *conv1_b, *conv2_w, *conv2_b;
    const float *w_ih1, *b1, *w_hh1;
    const float *w_ih2, *w_hh2, *b2;
    const float *head_w, *head_b;
} rva_cnnlstm_weights;
int rva_cnnlstm_plan_create(rva_ctx *ctx, const rva_cnnlstm_desc *desc, const rva_cnnlstm_weights *weights, rva_cnnlstm_plan **out);
void rva_cnnlstm_plan_destroy(rva_cnnlstm_plan *plan);
int rva_cnnlstm_plan_info(const rva_cnnlstm_plan *plan, int32_t *pooled_h, int32_t *pooled_w, int32_t *conv2_tiles,
                          int32_t *n_launches);
int rva_cnnlstm_plan_run(rva_cnnlstm_plan *plan, const void *frames, const int32_t *frame_index, int n_clips, void *logits,
                         rva_stream_t stream);
int rva_cnnlstm_plan_run_post(rva_cnnlstm_plan *plan, const void *logits, const int32_t *rows, int n_rows, int max_det,
                              void *scores, void *cls, void *boxes, void *counts, rva_stream_t stream);
enum rva_cnnlstm_stage {
    RVA_CNNLSTM_STAGE_POOLED = 0, RVA_CNNLSTM_STAGE_PARTIAL = 1, RVA_CNNLSTM_STAGE_FEAT = 2, RVA_CNNLSTM_STAGE_GX = 3,
    RVA_CNNLSTM_STAGE_H1 = 4, RVA_CNNLSTM_STAGE_H2 = 5
};
int rva_cnnlstm_plan_stage(rva_cnnlstm_plan *plan, int stage, int n_clips, void *dst, int64_t dst_floats, int64_t *n_floats,
                           rva_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * The same CNN-LSTM clip network for `half: true` (engine "clip-f16"): fp16 frames, fp16 convolution and LSTM weights and an
 * fp16 stored stem output, conv1 and conv2 on the fp16-input MFMA, every sum in fp32.  Network, launches and the
 * reproducibility contract are those of rva_cnnlstm_plan_*; the entries have the same signatures and reuse rva_cnnlstm_desc,
 * rva_cnnlstm_weights and enum rva_cnnlstm_stage.
 *
 * rva_cnnlstm_f16_plan_create: `weights` = fp32 host arrays in the layouts of rva_cnnlstm_plan_create (BatchNorm folded by the
 *   caller).  conv1_w, conv2_w, w_ih1, w_hh1, w_ih2 and w_hh2 are rounded ONCE to fp16, round to nearest even; RVA_ERR_ARG,
 *   naming the array, if a value does not stay finite in fp16.  b1, b2, the conv biases, head weight and head bias stay fp32.
 *   The descriptor limits are those of rva_cnnlstm_plan_create and max_clips * frames <= 65535; a workspace larger than the
 *   free device memory is refused with RVA_ERR_CAPACITY.
 * rva_cnnlstm_f16_plan_run: frames = a device ring of planar fp16 frames [3][height][width] (what rva_preprocess_frames_* writes
 *   for RVA_F16 with RVA_NORM_IMAGENET_F32; no alignment of a frame row is assumed), read through frame_index as in
 *   rva_cnnlstm_plan_run.  logits = device fp32 [n_clips][classes].  Arithmetic: every sum accumulates in fp32 (products of two
 *   fp16 values are exact in fp32) in one fixed order; the stem output gets ONE rounding to fp16, of ReLU(max of the raw sums +
 *   bias); conv2's tile partials, the mean, the LSTM's gates, hidden and cell states, the head and the logits are fp32.  Every
 *   launch goes to `stream`; no host synchronisation, no allocation: capturable.  A clip's logits are bit-identical for every
 *   batch size, position in the batch, index-table permutation of the ring and launch mode.
 * rva_cnnlstm_f16_plan_run_post / _info: as rva_cnnlstm_plan_run_post / _info.
 * rva_cnnlstm_f16_plan_stage: the tap of rva_cnnlstm_plan_stage, one device-to-device copy and no kernel, with the same
 *   layouts, rules and errors; dst_elems / *n_elems count ELEMENTS of the stage's type:
 *     RVA_CNNLSTM_STAGE_POOLED                          fp16 elements
 *     RVA_CNNLSTM_STAGE_PARTIAL / FEAT / GX / H1 / H2   fp32 elements
 * -------------------------------------------------------------------------------------------- */
typedef struct rva_cnnlstm_f16_plan rva_cnnlstm_f16_plan;
int rva_cnnlstm_f16_plan_create(rva_ctx *ctx, const rva_cnnlstm_desc *desc, const rva_cnnlstm_weights *weights,
                                rva_cnnlstm_f16_plan **out);
void rva_cnnlstm_f16_plan_destroy(rva_cnnlstm_f16_plan *plan);
int rva_cnnlstm_f16_plan_info(const rva_cnnlstm_f16_plan *plan, int32_t *pooled_h, int32_t *pooled_w, int32_t *conv2_tiles,
                              int32_t *n_launches);
int rva_cnnlstm_f16_plan_run(rva_cnnlstm_f16_plan *plan, const void *frames, const int32_t *frame_index, int n_clips, void *logits,
                             rva_stream_t stream);
int rva_cnnlstm_f16_plan_run_post(rva_cnnlstm_f16_plan *plan, const void *logits, const int32_t *rows, int n_rows, int max_det,
                                  void *scores, void *cls, void *boxes, void *counts, rva_stream_t stream);
int rva_cnnlstm_f16_plan_stage(rva_cnnlstm_f16_plan *plan, int stage, int n_clips, void *dst, int64_t dst_elems, int64_t *n_elems,
                               rva_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * The 3D-CNN clip network as ONE fp32 object -- replaces the network call of the reference's 3D-CNN head and its top-5
 * (CNN3DDetector._predict_sequence, temporal_detector.py:596-641; the network is Dummy3DCNN of
 * scripts/convert_temporal_model_to_onnx.py:91-121), for `half: false`.  Per clip [3][T][H][W]: Conv3d(3,64,3,p1)+BN+ReLU ->
 * MaxPool3d((1,2,2)) -> Conv3d(64,128,3,p1)+BN+ReLU -> MaxPool3d(2) -> Conv3d(128,256,3,p1)+BN+ReLU -> mean over T,H,W ->
 * Linear(256 -> classes).  The pools floor as torch's do (trailing odd rows, columns and frames are dropped).
 *
 * rva_cnn3d_plan_create: `weights` = fp32 host arrays in the field order of rva_cnn3d_weights (all required), each conv with
 *   its BatchNorm folded in: conv1 weight [64][3][3][3][3] = [co][ci][kt][ky][kx] (the checkpoint's layout) and bias [64];
 *   conv2 weight [128][27][64] and conv3 weight [256][27][128] = [co][tap = (kt*3 + ky)*3 + kx][ci] (channels innermost: what
 *   the kernels read) with biases [128] / [256]; head weight [classes][256] and bias [classes].  The plan copies them and
 *   allocates its whole workspace for desc.max_clips clips (height, width >= 4, frames >= 2, classes 1..16384, max_clips *
 *   frames <= 65535); a workspace larger than the free device memory is refused with RVA_ERR_CAPACITY.
 * rva_cnn3d_plan_run: frames = a device ring of planar fp32 frames [3][height][width] (what rva_preprocess_frames_* writes
 *   with RVA_NORM_VIDEO_F32); frame_index = device int32 [n_clips * frames]: frame t of clip b is ring + frame_index[b*T+t] *
 *   3*height*width, and its temporal neighbours are entries b*T+t-1 and b*T+t+1 (zero padding at the clip's ends; no gathered
 *   or permuted copy).  logits = device fp32 [n_clips][classes], the raw outputs.  Every launch goes to `stream`; no host
 *   synchronisation, no allocation: capturable.  Each sum runs in one fixed order (no split-K that follows the grid, no
 *   atomics): a clip's logits are bit-identical for every batch size, position in the batch and launch mode.
 * rva_cnn3d_plan_run_post: the arguments and the rule of rva_cnnlstm_plan_run_post (the same kernel).
 * rva_cnn3d_plan_info: pool1[3] = (T, H/2, W/2) after the first pool, pool2[3] = (T/2, H/4, W/4) after the second, tiles[3] =
 *   blocks per frame of conv1 and blocks per clip of conv2 and conv3 (per channel half), launches per _run.  Any may be NULL.
 * rva_cnn3d_plan_stage: the read-only workspace tap of rva_cnnlstm_plan_stage (same arguments, rules and errors).  With n =
 *   n_clips, (T, H1, W1) = pool1 and (T2, H2, W2) = pool2 of _info:
 *     RVA_CNN3D_STAGE_ACT1     [n][T][H1][W1][64]       conv1 + BN + ReLU + (1,2,2) max pool, channels last
 *     RVA_CNN3D_STAGE_ACT2     [n][T2*H2*W2][128]       conv2 + BN + ReLU + (2,2,2) max pool, positions linear over [T2][H2][W2]
 *     RVA_CNN3D_STAGE_PARTIAL  [n][conv3_tiles][256]    per-tile channel sums of ReLU(conv3 + BN); tile k holds positions
 *                                                       256k .. min(256k + 255, T2*H2*W2 - 1), linear over [T2][H2][W2]
 *     RVA_CNN3D_STAGE_FEAT     [n][256]                 the mean over T2, H2, W2: tile sums in tile order, divided by T2*H2*W2
 * -------------------------------------------------------------------------------------------- */
typedef struct rva_cnn3d_plan rva_cnn3d_plan;
typedef struct rva_cnn3d_desc {
    int32_t height, width;            /* frame size of the clip (112 x 112 by default) */
    int32_t frames;                   /* T = sequence_length */
    int32_t classes;
    int32_t max_clips;                /* capacity: the most clips one _run may take */
} rva_cnn3d_desc;
typedef struct rva_cnn3d_weights {
    const float *conv1_w, *conv1_b, *conv2_w, *conv2_b, *conv3_w, *conv3_b;
    const float *head_w, *head_b;
} rva_cnn3d_weights;
int rva_cnn3d_plan_create(rva_ctx *ctx, const rva_cnn3d_desc *desc, const rva_cnn3d_weights *weights, rva_cnn3d_plan **out);
void rva_cnn3d_plan_destroy(rva_cnn3d_plan *plan);
int rva_cnn3d_plan_info(const rva_cnn3d_plan *plan, int32_t *pool1, int32_t *pool2, int32_t *tiles, int32_t *n_launches);
int rva_cnn3d_plan_run(rva_cnn3d_plan *plan, const void *frames, const int32_t *frame_index, int n_clips, void *logits,
                       rva_stream_t stream);
int rva_cnn3d_plan_run_post(rva_cnn3d_plan *plan, const void *logits, const int32_t *rows, int n_rows, int max_det,
                            void *scores, void *cls, void *boxes, void *counts, rva_stream_t stream);
enum rva_cnn3d_stage { RVA_CNN3D_STAGE_ACT1 = 0, RVA_CNN3D_STAGE_ACT2 = 1, RVA_CNN3D_STAGE_PARTIAL = 2, RVA_CNN3D_STAGE_FEAT = 3 };
int rva_cnn3d_plan_stage(rva_cnn3d_plan *plan, int stage, int n_clips, void *dst, int64_t dst_floats, int64_t *n_floats,
                         rva_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * The same 3D-CNN clip network for `half: true` (engine "clip3d-f16"): fp16 frames, fp16 convolution weights and fp16 stored
 * activations on the fp16-input MFMA, every sum in fp32.  The reference honours `half` on this head by making the clip tensor
 * float16 (temporal_detector.py:590-591).  Network, launches, pools and the reproducibility contract are those of
 * rva_cnn3d_plan_*; the entries have the same signatures and reuse rva_cnn3d_desc, rva_cnn3d_weights and enum rva_cnn3d_stage.
 *
 * rva_cnn3d_f16_plan_create: `weights` = fp32 host arrays in the layouts of rva_cnn3d_plan_create (BatchNorm folded by the
 *   caller).  The three convolution weights are rounded ONCE to fp16, round to nearest even; RVA_ERR_ARG, naming the array, if
 *   a value does not stay finite in fp16.  Biases, head weight and head bias stay fp32.  The descriptor limits are those of
 *   rva_cnn3d_plan_create, and a workspace (fp16 activations) larger than the free device memory is refused with
 *   RVA_ERR_CAPACITY.
 * rva_cnn3d_f16_plan_run: frames = a device ring of planar fp16 frames [3][height][width] (what rva_preprocess_frames_* writes
 *   for RVA_F16 with RVA_NORM_VIDEO_F32; no alignment of a frame row is assumed), read through frame_index as in
 *   rva_cnn3d_plan_run, zero padding at the clip's ends.  logits = device fp32 [n_clips][classes].  Arithmetic: every
 *   convolution sum accumulates in fp32 (products of two fp16 values are exact in fp32) in one fixed order; the max pools take the
 *   max of the raw fp32 sums, then + bias, ReLU, and ONE rounding to fp16 for the two stored activations; conv3's tile partials,
 *   the mean, the head and the logits are fp32.  Every launch goes to `stream`; no host synchronisation, no allocation:
 *   capturable.  A clip's logits are bit-identical for every batch size, position in the batch, index-table permutation of the
 *   ring and launch mode.
 * rva_cnn3d_f16_plan_run_post / _info: as rva_cnn3d_plan_run_post / _info.
 * rva_cnn3d_f16_plan_stage: the tap of rva_cnn3d_plan_stage, one device-to-device copy and no kernel, with the same layouts,
 *   rules and errors; dst_elems / *n_elems count ELEMENTS of the stage's type:
 *     RVA_CNN3D_STAGE_ACT1 / ACT2      fp16 elements
 *     RVA_CNN3D_STAGE_PARTIAL / FEAT   fp32 elements
 * -------------------------------------------------------------------------------------------- */
typedef struct rva_cnn3d_f16_plan rva_cnn3d_f16_plan;
int rva_cnn3d_f16_plan_create(rva_ctx *ctx, const rva_cnn3d_desc *desc, const rva_cnn3d_weights *weights, rva_cnn3d_f16_plan **out);
void rva_cnn3d_f16_plan_destroy(rva_cnn3d_f16_plan *plan);
int rva_cnn3d_f16_plan_info(const rva_cnn3d_f16_plan *plan, int32_t *pool1, int32_t *pool2, int32_t *tiles, int32_t *n_launches);
int rva_cnn3d_f16_plan_run(rva_cnn3d_f16_plan *plan, const void *frames, const int32_t *frame_index, int n_clips, void *logits,
                           rva_stream_t stream);
int rva_cnn3d_f16_plan_run_post(rva_cnn3d_f16_plan *plan, const void *logits, const int32_t *rows, int n_rows, int max_det,
                                void *scores, void *cls, void *boxes, void *counts, rva_stream_t stream);
int rva_cnn3d_f16_plan_stage(rva_cnn3d_f16_plan *plan, int stage, int n_clips, void *dst, int64_t dst_elems, int64_t *n_elems,
                             rva_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * The ResNet-18 classifier as ONE fp32 object -- replaces the network call of the reference's ResNet head and its top-K
 * (detector.py:870-1001) for a batch of frames.  Per frame [3][H][W]: Conv 7x7 s2 p3 + BN + ReLU -> MaxPool 3x3 s2 p1 -> eight
 * BasicBlocks (widths 64, 64, 128, 128, 256, 256, 512, 512; blocks 2, 4 and 6 have stride 2 and a 1x1 stride-2 shortcut
 * convolution) -> mean over H,W -> Linear(512 -> classes).
 *
 * rva_resnet_plan_create: `weights` = fp32 host arrays (all required), every convolution with its BatchNorm folded in (by the
 *   caller, in float64, rounded once): stem weight [64][3][7][7] (the checkpoint's layout) and bias [64]; conv[19] = the block
 *   convolutions as [Cout][k*k][Cin] (tap = ky*k + kx, channels innermost: what the kernel reads) with bias [Cout], block by
 *   block in the order conv1 (3x3), conv2 (3x3), then the block's shortcut (1x1) where it has one -- so conv[6], conv[11] and
 *   conv[16] are the shortcuts of blocks 2, 4 and 6; head weight [classes][512] and bias [classes].  The plan copies them and
 *   allocates its whole workspace for desc.max_frames frames (height, width >= 1, classes 1..16384, top_k >= 1, max_frames
 *   1..65535); a workspace larger than the free device memory is refused with RVA_ERR_CAPACITY.
 * rva_resnet_plan_run: frames = device planar fp32 frames [3][height][width] (what rva_preprocess_frames_* writes with
 *   RVA_NORM_IMAGENET_F32); frame_index = device int32 [n]: frame b is frames + frame_index[b] * 3*height*width (no gathered
 *   copy).  logits = device fp32 [n][classes], the raw outputs (no softmax).  Every launch goes to `stream`; no host
 *   synchronisation, no allocation: capturable.  Each sum runs in one fixed order (no split-K, no atomics): a frame's logits
 *   are bit-identical for every batch size, position in the batch and launch mode.
 * rva_resnet_plan_run_post: the arguments and the rule of rva_cnnlstm_plan_run_post (the same kernel) with k = min(desc.top_k,
 *   classes); the row table's first column is the batch row of the result row or -1.
 * rva_resnet_plan_info: maps[5][2] = (height, width) of the pooled map and of the four stages' maps, the workspace size in
 *   bytes (activations of max_frames frames), launches per _run.  Any may be NULL.
 * rva_resnet_plan_stage: the read-only workspace tap of rva_cnnlstm_plan_stage (same arguments, rules and errors; n_clips =
 *   frames).  Every tensor is [n][h][w][C] (channels last) with (h, w) the map of the block's stage and C its width:
 *     RVA_RESNET_STAGE_POOLED         [n][Hp][Wp][64]   stem output: conv1 + BN + ReLU + max pool
 *     RVA_RESNET_STAGE_MID0 + b       b = 0..7: ReLU(conv1 + BN) of block b
 *     RVA_RESNET_STAGE_DOWN2 / 4 / 6  shortcut convolution + BN of blocks 2, 4, 6
 *     RVA_RESNET_STAGE_OUT0 + b       b = 0..7: ReLU((conv2 + BN) + shortcut) of block b
 *     RVA_RESNET_STAGE_FEAT           [n][512]          the spatial mean: pixels in raster order from zero, divided by h*w
 * -------------------------------------------------------------------------------------------- */
typedef struct rva_resnet_plan rva_resnet_plan;
typedef struct rva_resnet_desc {
    int32_t height, width;            /* frame size (224 x 224 by default) */
    int32_t classes, top_k;
    int32_t max_frames;               /* capacity: the most frames one _run may take */
} rva_resnet_desc;
typedef struct rva_resnet_conv {
    const float *w, *b;
} rva_resnet_conv;
typedef struct rva_resnet_weights {
    const float *stem_w, *stem_b;
    rva_resnet_conv conv[19];
    const float *head_w, *head_b;
} rva_resnet_weights;
int rva_resnet_plan_create(rva_ctx *ctx, const rva_resnet_desc *desc, const rva_resnet_weights *weights, rva_resnet_plan **out);
void rva_resnet_plan_destroy(rva_resnet_plan *plan);
int rva_resnet_plan_info(const rva_resnet_plan *plan, int32_t *maps, int64_t *workspace_bytes, int32_t *n_launches);
int rva_resnet_plan_run(rva_resnet_plan *plan, const void *frames, const int32_t *frame_index, int n, void *logits,
                        rva_stream_t stream);
int rva_resnet_plan_run_post(rva_resnet_plan *plan, const void *logits, const int32_t *rows, int n_rows, int max_det,
                             void *scores, void *cls, void *boxes, void *counts, rva_stream_t stream);
enum rva_resnet_stage {
    RVA_RESNET_STAGE_POOLED = 0, RVA_RESNET_STAGE_MID0 = 1, RVA_RESNET_STAGE_DOWN2 = 9, RVA_RESNET_STAGE_DOWN4 = 10,
    RVA_RESNET_STAGE_DOWN6 = 11, RVA_RESNET_STAGE_OUT0 = 12, RVA_RESNET_STAGE_FEAT = 20
};
int rva_resnet_plan_stage(rva_resnet_plan *plan, int stage, int n, void *dst, int64_t dst_floats, int64_t *n_floats,
                          rva_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The fp16 ResNet-18 plan (csrc/rva_resnet_f16.hip): the network of rva_resnet_plan for `half: true` -- fp16 frames, fp16
 * convolution weights and fp16 stored activations on v_mfma_f32_32x32x16_f16, every sum in fp32.  It shares rva_resnet_desc,
 * rva_resnet_weights and enum rva_resnet_stage.  These entries are a front door of the one fp16 ResNet plan (rva_resnetx_f16_plan
 * below): BasicBlocks 2, 2, 2, 2 with RVA_RESX_SPLIT_SHORTCUT, conv[19] passed on as `convs`, every stage code translated.
 *
 * rva_resnet_f16_plan_create: `weights` = fp32 host arrays in the layouts of rva_resnet_plan_create (BatchNorm folded by the
 *   caller).  stem_w and the 19 conv[i].w are rounded ONCE to fp16, round to nearest even; RVA_ERR_ARG, naming the array
 *   ("stem_w", "conv[i].w"), if a value does not stay finite in fp16.  All biases, head weight and head bias stay fp32.  The
 *   descriptor limits are those of rva_resnet_plan_create; a workspace larger than the free device memory is refused with
 *   RVA_ERR_CAPACITY before anything is allocated.
 * rva_resnet_f16_plan_run: frames = a device array of planar fp16 frames [3][height][width] (what rva_preprocess_frames_* writes
 *   for RVA_F16 with RVA_NORM_IMAGENET_F32; no alignment of a frame row is assumed), read through frame_index as in
 *   rva_resnet_plan_run.  logits = device fp32 [n][classes].  Arithmetic: every sum accumulates in fp32 (products of two fp16
 *   values are exact in fp32) in one fixed order per layer; the stored activations are fp16 with one rounding of the fp32 epilogue
 *   value, except the last block's output, the spatial mean and the logits, which are fp32.  Every launch goes to `stream`; no
 *   host synchronisation, no allocation: capturable.  A frame's logits are bit-identical for every batch size, position in the
 *   batch, index-table permutation and launch mode.
 * rva_resnet_f16_plan_run_post / _info: as rva_resnet_plan_run_post / _info (the workspace is about half the fp32 plan's).
 * rva_resnet_f16_plan_stage: the tap of rva_resnet_plan_stage, one device-to-device copy and no kernel, with the same layouts,
 *   rules and errors; dst_elems / *n_elems count ELEMENTS of the stage's type:
 *     RVA_RESNET_STAGE_POOLED, MID0 + b, DOWN2 / 4 / 6, OUT0 + b for b = 0..6   fp16 elements
 *     RVA_RESNET_STAGE_OUT0 + 7, RVA_RESNET_STAGE_FEAT                          fp32 elements
 * -------------------------------------------------------------------------------------------- */
typedef struct rva_resnet_f16_plan rva_resnet_f16_plan;
int rva_resnet_f16_plan_create(rva_ctx *ctx, const rva_resnet_desc *desc, const rva_resnet_weights *weights,
                               rva_resnet_f16_plan **out);
void rva_resnet_f16_plan_destroy(rva_resnet_f16_plan *plan);
int rva_resnet_f16_plan_info(const rva_resnet_f16_plan *plan, int32_t *maps, int64_t *workspace_bytes, int32_t *n_launches);
int rva_resnet_f16_plan_run(rva_resnet_f16_plan *plan, const void *frames, const int32_t *frame_index, int n, void *logits,
                            rva_stream_t stream);
int rva_resnet_f16_plan_run_post(rva_resnet_f16_plan *plan, const void *logits, const int32_t *rows, int n_rows, int max_det,
                                 void *scores, void *cls, void *boxes, void *counts, rva_stream_t stream);
int rva_resnet_f16_plan_stage(rva_resnet_f16_plan *plan, int stage, int n, void *dst, int64_t dst_elems, int64_t *n_elems,
                              rva_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The fp16 plan for any ResNet of the torchvision family (csrc/rva_resnet_f16.hip): the stem of rva_resnet_plan, then four
 * stages of desc.blocks[s] blocks of width 64 << s -- BasicBlocks (3x3, 3x3: ResNet-18 / 34) or Bottlenecks (1x1, 3x3, 1x1 with
 * expansion 4 and the stride on the 3x3: ResNet-50 / 101 / 152) --, the mean over H,W and Linear(512 * expansion -> classes).  The
 * first block of stages 1..3 has stride 2.  A block whose stride is not 1 or whose input width differs from its output width has a
 * 1x1 shortcut convolution (the first block of stage 0 of a Bottleneck net has one with stride 1).  Numeric contract, kernels and
 * tile table are those of rva_resnet_f16_plan: both sets of entries run the same plan code over one description of the network,
 * which the fp32 rva_resnet_plan walks too.
 *
 * rva_resnetx_f16_plan_create: weights as for rva_resnet_f16_plan_create; `convs` holds desc.n_convs convolutions, block by block
 *   in the order conv1, conv2[, conv3], then the block's shortcut where it has one, each [Cout][k*k][Cin] with bias [Cout];
 *   head_w is [classes][512 * expansion].  desc.n_convs is checked against the topology (RVA_ERR_ARG).  Limits: those of
 *   rva_resnet_desc, bottleneck 0 or 1, blocks[s] 1..64, flags 0 or RVA_RESX_SPLIT_SHORTCUT.  stem_w and every convs[i].w are
 *   rounded once to fp16; RVA_ERR_ARG naming "stem_w" / "conv[i].w" if a value does not stay finite.  RVA_ERR_CAPACITY before
 *   anything is allocated.
 *   Without RVA_RESX_SPLIT_SHORTCUT a block's shortcut convolution runs inside the launch of its closing convolution, as further
 *   steps of the same fp32 sum (taps of the closing convolution in order, then the shortcut's input channels in order):
 *   out = ReLU(conv_close(mid) + conv_short(x) + b), and the CLOSING convolution's `b` must hold b_close + b_short (added by the
 *   caller in float64, rounded once to fp32); the shortcut's own `b` is not read.  With the flag the shortcut is a launch of its
 *   own into its own fp16 stage and the closing convolution adds it as the residual: the launches and the order of
 *   rva_resnet_f16_plan, and every `b` is the convolution's own.
 * rva_resnetx_f16_plan_run / _run_post / _info: as rva_resnet_f16_plan_*.
 * rva_resnetx_f16_plan_stage: the tap of rva_resnet_f16_plan_stage with these stage codes, b = the block's index over all stages:
 *     RVA_RESX_POOLED                       [n][Hp][Wp][64]
 *     RVA_RESX_FEAT                         [n][512 * expansion], fp32
 *     RVA_RESX_BLOCK0 + 4 b + 0             after conv1 (a Bottleneck's is on the block's INPUT map: the stride is on the 3x3)
 *     RVA_RESX_BLOCK0 + 4 b + 1             after conv2, Bottleneck only
 *     RVA_RESX_BLOCK0 + 4 b + 2             the shortcut convolution, split plans only
 *     RVA_RESX_BLOCK0 + 4 b + 3             the block's output; fp32 for the last block, fp16 otherwise
 *   A stage the plan does not have is RVA_ERR_ARG.  Every stage keeps its own buffer.
 * -------------------------------------------------------------------------------------------- */
#define RVA_RESX_SPLIT_SHORTCUT 1     /* flags: shortcut convolutions as launches of their own (A/B and cross-check) */
typedef struct rva_resnetx_f16_plan rva_resnetx_f16_plan;
typedef struct rva_resnetx_desc {
    int32_t height, width, classes, top_k, max_frames;   /* limits of rva_resnet_desc */
    int32_t bottleneck;                                   /* 0 BasicBlock, 1 Bottleneck */
    int32_t blocks[4];                                    /* 1..64 each */
    int32_t n_convs;                                      /* length of convs: checked against the topology */
    int32_t flags;
} rva_resnetx_desc;
typedef struct rva_resnetx_weights {
    const float *stem_w, *stem_b;
    const rva_resnet_conv *convs;    /* per block conv1, conv2[, conv3], then its shortcut where it has one; [Cout][k*k][Cin] */
    const float *head_w, *head_b;    /* [classes][512 * expansion] */
} rva_resnetx_weights;
enum rva_resx_stage { RVA_RESX_POOLED = 0, RVA_RESX_FEAT = 1, RVA_RESX_BLOCK0 = 2 };
int rva_resnetx_f16_plan_create(rva_ctx *ctx, const rva_resnetx_desc *desc, const rva_resnetx_weights *weights,
                                rva_resnetx_f16_plan **out);
void rva_resnetx_f16_plan_destroy(rva_resnetx_f16_plan *plan);
int rva_resnetx_f16_plan_info(const rva_resnetx_f16_plan *plan, int32_t *maps, int64_t *workspace_bytes, int32_t *n_launches);
int rva_resnetx_f16_plan_run(rva_resnetx_f16_plan *plan, const void *frames, const int32_t *frame_index, int n, void *logits,
                             rva_stream_t stream);
int rva_resnetx_f16_plan_run_post(rva_resnetx_f16_plan *plan, const void *logits, const int32_t *rows, int n_rows, int max_det,
                                  void *scores, void *cls, void *boxes, void *counts, rva_stream_t stream);
int rva_resnetx_f16_plan_stage(rva_resnetx_f16_plan *plan, int stage, int n, void *dst, int64_t dst_elems, int64_t *n_elems,
                               rva_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * K5 motion gate -- replaces MotionFilter.should_process (utils/frame_filter.py:26-40)
 * for a tick of NV12 surfaces: gray -> 5x5 Gaussian -> |diff| against prev_blur[i] -> counts[i] = number of
 * pixels with diff > 25 (device int32[n]; -1 where prev_blur[i] is NULL = first frame of that stream).
 * blur_out[i] (device uint8 [h][w]) receives the new blurred frame; pass it as prev_blur next tick.
 * The caller compares counts[i] / (w*h) >= motion_threshold (frame_filter.py:38-40).
 * -------------------------------------------------------------------------------------------- */
int rva_motion_nv12_batch(rva_ctx *ctx, const void *const *y_ptrs, const void *const *uv_ptrs,
                          const int32_t *pitches, const void *const *prev_blur, void *const *blur_out, int n,
                          int w, int h, int32_t *counts, rva_stream_t stream);
/* Same with per-stream ROI masks (uint8 [h][w], 0 = outside; entries may be NULL) applied first, and for uint8 BGR
 * device images (the downsampled frames): the gate sees what the reference's frame_for_detection holds. */
int rva_motion_nv12_masked_batch(rva_ctx *ctx, const void *const *y_ptrs, const void *const *uv_ptrs,
                                 const int32_t *pitches, const void *const *masks, const void *const *prev_blur,
                                 void *const *blur_out, int n, int w, int h, int32_t *counts, rva_stream_t stream);
int rva_motion_bgr_batch(rva_ctx *ctx, const void *const *frames, const int32_t *row_bytes,
                         const void *const *prev_blur, void *const *blur_out, int n, int w, int h, int32_t *counts,
                         rva_stream_t stream);

/* ROI + downsample in front of the detector (utils/frame_filter.py:43-57, pipeline.py:149-154):
 * rva_preprocess_nv12_masked_batch = rva_preprocess_nv12_batch with apply_roi (pixels whose mask byte is 0
 * become BGR 0,0,0 before the resize); rva_resize_nv12_to_bgr_batch = apply_roi + downsample: cv2.resize
 * INTER_LINEAR to (dst_w, dst_h) as uint8 BGR images out_bgr[n][dst_h][dst_w][3] (feed rva_preprocess_bgr_batch). */
int rva_preprocess_nv12_masked_batch(rva_ctx *ctx, const void *const *y_ptrs, const void *const *uv_ptrs,
                                     const int32_t *pitches, const void *const *masks, int n, int src_w, int src_h,
                                     void *out, int out_dtype, int dst_w, int dst_h, rva_letterbox *meta_out,
                                     rva_stream_t stream);
int rva_resize_nv12_to_bgr_batch(rva_ctx *ctx, const void *const *y_ptrs, const void *const *uv_ptrs,
                                 const int32_t *pitches, const void *const *masks, int n, int src_w, int src_h,
                                 void *out_bgr, int dst_w, int dst_h, rva_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * K6 annotated preview -- replaces the pixel work of KafkaSink._render_frame (sinks/kafka_sink.py:200-294) and of
 * StreamWorker._maybe_save_snapshot (pipeline.py:264-290): uint8 BGR image out_bgr[dst_h][dst_w][3] (device) =
 * the NV12 surface converted (BT.601 as in K1), box-averaged down by the integer `ratio` (1 = same size; 0 = out_bgr
 * already holds the base image, draw only), then `n_rects` filled rectangles (device int32[n][4] x0,y0,x1,y1
 * inclusive, device uint8[n][4] b,g,r,-) in painter's order and `n_glyphs` characters of a built-in 5x7 font (device
 * int32[m][3] x, y, code; digits, 'I', 'D', space) in white at `glyph_scale`.  WHAT is drawn is decided by the host
 * (preview.py, pinned against a call-level recording of the reference); how OpenCV rasterises lines and glyphs is unpinned.
 * -------------------------------------------------------------------------------------------- */
int rva_preview_nv12(rva_ctx *ctx, const void *y, const void *uv, int pitch, int src_w, int src_h, int ratio,
                     void *out_bgr, int dst_w, int dst_h, const int32_t *rects, const uint8_t *colors, int n_rects,
                     const int32_t *glyphs, int n_glyphs, int glyph_scale, rva_stream_t stream);

/* K6 for n surfaces in ONE launch (the previews of a tick, kafka_sink.py:134-146): the same per-pixel arithmetic as
 * rva_preview_nv12 for every item.  `table_host` (pinned host memory, so that the copy is asynchronous; untouched until it has
 * run) holds, back to back: rva_preview_item[n]; int32 rects[n_rects][4]; int32 glyphs[n_glyphs][3]; uint8 colors[n_rects][4] --
 * an item draws rects / colors [rect_first, rect_first + n_rects) and glyphs [glyph_first, glyph_first + n_glyphs) of the packed
 * arrays.  The call checks every item, copies the table to `table_dev` (device, table_bytes >= the table's size) with one
 * asynchronous copy and launches once.  ratio per item as above (0: out_bgr already holds the base image, y / uv unused). */
typedef struct rva_preview_item {
    const void *y, *uv;
    void *out_bgr;
    int32_t pitch, src_w, src_h, ratio, dst_w, dst_h;
    int32_t rect_first, n_rects, glyph_first, n_glyphs;
} rva_preview_item;
int rva_preview_nv12_batch(rva_ctx *ctx, const void *table_host, void *table_dev, int64_t table_bytes, int n, int n_rects,
                           int n_glyphs, int glyph_scale, rva_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * D1 decode -- stands where VideoStream.open()/frames() sit on cv2.VideoCapture(url, CAP_FFMPEG) (video_stream.py:76,
 * 173): an H.264 / H.265 Annex-B elementary stream goes to the VCN decoder through rocDecode and comes back as NV12
 * surfaces in HBM (device pointers + pitch, the input form of rva_preprocess_nv12_batch); no frame visits the host.
 * librocdecode is looked up with dlopen at run time: rva_decode_available() / rva_decoder_create() report
 * RVA_ERR_UNAVAILABLE on a machine that does not have it (the demuxer and the retry / back-off / reconnect policy of
 * video_stream.py:155-243 live on the host side: mp4.py, video_stream.py of this package).
 * -------------------------------------------------------------------------------------------- */
typedef struct rva_decoder rva_decoder;
enum rva_codec { RVA_CODEC_H264 = 0, RVA_CODEC_HEVC = 1 };

int rva_decode_available(char *detail, int detail_len);

/* One decode session (parser + decoder) on ctx's device.  num_surfaces: decode surfaces to ask for (the stream's own
 * minimum wins when larger; <= 0: 8).  8-bit 4:2:0 streams only (what maps onto NV12). */
int rva_decoder_create(rva_ctx *ctx, int codec, int num_surfaces, rva_decoder **out);
void rva_decoder_destroy(rva_decoder *dec);

/* Feed ONE access unit (host memory, Annex-B start codes, parameter sets in band in front of sync samples); pts in
 * 10 MHz units.  end_of_stream != 0 flushes the decoder (data may be NULL / size 0).  Decoding is submitted from inside
 * this call (parser callbacks); decoded pictures queue up for rva_decoder_next_frame. */
int rva_decoder_feed(rva_decoder *dec, const uint8_t *data, int size, int64_t pts, int end_of_stream);

/* Next picture in display order: *pic_index >= 0 and device pointers *y / *uv (interleaved) with a common *pitch, the
 * display size *width x *height (cropped to whole chroma pairs), or *pic_index == -1 when nothing is displayable yet
 * (feed more data).  Waits for that picture's decode to finish.  *pic_index is a ticket (decoder generation << 10 | the
 * library's picture index): the surface stays valid until rva_decoder_release(dec, that ticket) hands it back -- also
 * across a change of picture size mid-stream, where the previous decoder lives on until its last picture is released.
 * The library probed first is the one RVA_ROCDECODE_LIB names (then librocdecode.so on the default search path). */
int rva_decoder_next_frame(rva_decoder *dec, void **y, void **uv, int32_t *pitch, int32_t *width, int32_t *height,
                           int64_t *pts, int32_t *pic_index);
int rva_decoder_release(rva_decoder *dec, int pic_index);

/* ----------------------------------------------------------------------------------------------
 * K7 device JPEG encoder (round 4) -- replaces cv2.imencode('.jpg', frame, [IMWRITE_JPEG_QUALITY, q, ...]) of
 * KafkaSink._render_frame (/root/reference/src/realtime_analytics/sinks/kafka_sink.py:260-284) and of
 * StreamWorker._maybe_save_snapshot (pipeline.py:264-290): a uint8 BGR image in HBM ([height] rows of `pitch` bytes, 3 bytes per
 * pixel: what rva_preview_nv12 writes) -> a baseline JFIF stream in `out` (device), its length in *out_size (device or mapped
 * host int32), both written asynchronously on `stream`.  libjpeg's arithmetic step by step (colour conversion, 4:2:0 downsampling,
 * edge rules, islow DCT, quantisation tables of `quality`), Annex-K Huffman tables, one restart interval per MCU row: a decoder
 * reconstructs exactly the picture it reconstructs from libjpeg's own file of the same quality (the reference asks for the
 * progressive, Huffman-optimised form of the same coefficients).  rva_jpeg_max_bytes: a capacity that fits photographic content
 * (128 B per 8x8 block); rva_jpeg_status (host-synchronous): bit 0 = a stream did not fit since the last call (*out_size is -1
 * for such a picture).
 * CONCURRENCY: the scratch of rva_jpeg_encode_bgr belongs to the context -- ONE stream and one thread at a time per context
 * (calls on the same stream queue up safely; a larger picture than any before regrows the scratch behind a device
 * synchronisation).  Concurrent encodes take one rva_jpeg_batch each.
 * -------------------------------------------------------------------------------------------- */
int rva_jpeg_max_bytes(int width, int height);
int rva_jpeg_encode_bgr(rva_ctx *ctx, const void *bgr, int pitch, int width, int height, int quality, void *out,
                        int out_capacity, int32_t *out_size, rva_stream_t stream);
int rva_jpeg_status(rva_ctx *ctx, rva_stream_t stream, int *flags);

/* Batched K7: KafkaSink.send_tracks renders and encodes one preview per due stream (sinks/kafka_sink.py:134-146, 200-294); the
 * rate limit of 0.1 s (kafka_sink.py:49) makes every stream of a 30 fps pipeline due on the same tick.  An rva_jpeg_batch owns
 * every buffer an encode touches (coefficients, interval staging, sizes, flags, the descriptor table and its pinned staging),
 * allocated once by _create for up to max_images pictures of up to max_width x max_height each: _encode allocates nothing,
 * never synchronises the device and never regrows -- a batch outside those bounds is RVA_ERR_ARG and launches nothing.
 * _encode: n BGR images in HBM (HOST arrays of n device pointers / pitches / widths / heights / qualities, mixed freely) ->
 * their JFIF streams back to back in `out` (device, out_capacity bytes), in order; out_sizes[n] (device or mapped host int32):
 * the length of each stream, or -1 for a picture that failed (an interval overflowed its 128 B per block, or `out` had no room
 * left for it) -- it takes no bytes and the pictures after it pack on.  A fixed number of launches whatever n (one table copy,
 * transform, entropy coding, size scan, gather), all asynchronous on `stream`; every byte is what rva_jpeg_encode_bgr writes for
 * that picture alone.
 * CONCURRENCY: one object serves one stream at a time (consecutive calls on that stream queue up safely; the pinned staging is
 * guarded by an event).  Distinct objects share nothing and are independent on distinct streams and threads. */
typedef struct rva_jpeg_batch rva_jpeg_batch;
int rva_jpeg_batch_create(rva_ctx *ctx, int max_images, int max_width, int max_height, rva_jpeg_batch **out);
void rva_jpeg_batch_destroy(rva_jpeg_batch *enc);
int rva_jpeg_batch_encode(rva_jpeg_batch *enc, int n, const void *const *bgr, const int32_t *pitch, const int32_t *width,
                          const int32_t *height, const int32_t *quality, void *out, int64_t out_capacity, int32_t *out_sizes,
                          rva_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * K8 device JPEG decoder -- stands where VideoStream.open() / frames() sit on cv2.VideoCapture(url) (video_stream.py:76,173)
 * for Motion-JPEG sources: baseline JPEG pictures in HOST memory -> frames in HBM.  Accepted: SOF0, 8-bit samples, Huffman
 * coding, one interleaved scan; 1 component, or Y/Cb/Cr with chroma 1x1 and luma 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0);
 * 8-bit DQT, any DHT, optional DRI; JFIF, Adobe APP14 with transform 1 or neither -- three components are YCbCr as libjpeg
 * decides it: RGB samples (ids 'R','G','B' without JFIF or Adobe; Adobe transform 0) are refused.  Everything else is refused on the
 * host by the marker walk, before anything is launched, with a message that names what was found.
 * Output formats: RVA_JPEG_DEC_BGR -- uint8 [h][w][3] with the given pitch, libjpeg's own picture (islow IDCT, fancy
 * upsampling, jdcolor.c), bit for bit what cv2.imdecode and Pillow's libjpeg-turbo give for streams a real encoder made (where
 * libjpeg's range-limit table wraps for sums far outside 0..255, this decoder saturates).  RVA_JPEG_DEC_NV12 -- dst0 a
 * pitch-linear Y plane, dst1 an interleaved CbCr plane of the same pitch, in the BT.601 limited range that
 * rva_preprocess_nv12_batch assumes: Y' = 16 + (219 Y + 127) / 255, C' = 128 + (224 (C - 128) +- 127) / 255 (the sign of the 127
 * follows C - 128, the division truncates); the chroma pair is the decoded 4:2:0 sample, (a + b + 1) >> 1 of the two 4:2:2 rows,
 * (a + b + c + d + 2) >> 2 of the 4:4:4 group, 128 for grayscale.  Even width and height only in this format.
 * One lane decodes one restart interval: a stream without DRI is decoded by ONE lane per picture.
 * -------------------------------------------------------------------------------------------- */
typedef struct rva_jpeg_dec rva_jpeg_dec;
enum rva_jpeg_dec_format { RVA_JPEG_DEC_BGR = 0, RVA_JPEG_DEC_NV12 = 1 };
enum rva_jpeg_dec_result { RVA_JPEG_DEC_OK = 0, RVA_JPEG_DEC_REFUSED = -1, RVA_JPEG_DEC_FAILED = -2 };
typedef struct rva_jpeg_dec_info {
    int32_t width, height, components;
    int32_t h_samp, v_samp;          /* luma sampling factors (chroma is 1x1): 1 1 = 4:4:4 or grayscale, 2 1 = 4:2:2, 2 2 = 4:2:0 */
    int32_t restart_interval;        /* MCUs per restart interval (DRI), 0: none */
    int32_t intervals;               /* restart intervals of the scan: the lanes that decode it */
    int32_t mcus;
} rva_jpeg_dec_info;

/* video_stream.py:76,173 (what cap.isOpened() / cap.read() find out about a source): host only, no context.  RVA_OK and *info,
 * or RVA_ERR_ARG and the refusal in msg (msg_len bytes, always terminated). */
int rva_jpeg_dec_probe(const uint8_t *data, int64_t len, rva_jpeg_dec_info *info, char *msg, int msg_len);

/* video_stream.py:76,173: the decoder object owns every buffer a decode touches, device and pinned, for up to max_images
 * pictures of up to max_width x max_height whose entropy segments hold up to max_bytes_per_image bytes each.  After _create
 * nothing allocates. */
int rva_jpeg_dec_create(rva_ctx *ctx, int max_images, int max_width, int max_height, int max_bytes_per_image, rva_jpeg_dec **out);
void rva_jpeg_dec_destroy(rva_jpeg_dec *dec);

/* video_stream.py:76,173: n streams (HOST arrays of n host pointers / lengths) -> dst0[i] (and dst1[i] for NV12), device
 * pointers with pitch[i] bytes per row; sizes and sampling mixed freely.  One async copy of a pinned blob (descriptors,
 * restart-interval table, entropy segments) and a fixed number of launches whatever n, all on `stream`; the host memory is
 * free to reuse on return.  RVA_ERR_ARG (nothing launched): n outside 1..max_images, a missing destination or a short pitch
 * for a picture the parser accepts, an odd size with NV12.  A stream the parser refuses, or one beyond the object's limits,
 * does not fail the call: that picture is skipped (its destination may be NULL), rva_jpeg_dec_status reports it, and
 * rva_last_error holds the first such refusal. */
int rva_jpeg_dec_decode(rva_jpeg_dec *dec, int n, const uint8_t *const *data, const int64_t *len, int format, void *const *dst0,
                        void *const *dst1, const int32_t *pitch, rva_stream_t stream);

/* video_stream.py:76,173 (the `ok` of cap.read()): waits for the stream of the last _decode, then status[i] of its n pictures:
 * RVA_JPEG_DEC_OK, RVA_JPEG_DEC_REFUSED (by the parser, nothing was launched for it) or RVA_JPEG_DEC_FAILED (on the device:
 * a code in no table, a run past coefficient 63, broken byte stuffing, an interval that ran dry or had bytes left over).  A
 * failed picture's destination holds nothing a caller may rely on; its neighbours are intact. */
int rva_jpeg_dec_status(rva_jpeg_dec *dec, int32_t *status);

/* video_stream.py:76,173 (where the time of a cap.read() goes): device time of the last _decode's four steps in milliseconds,
 * from events the call records on its stream -- ms[0] the blob's copy, ms[1] entropy decoding, ms[2] IDCT, ms[3] the output
 * kernel.  Waits for that call.  RVA_ERR_ARG if it launched nothing (every picture refused). */
int rva_jpeg_dec_times(rva_jpeg_dec *dec, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* RVA_H */
