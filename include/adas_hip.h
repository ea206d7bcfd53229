/* adas_hip.h -- C ABI of libadas_hip.so: the MI355X-native per-frame ADAS inference path.
 *
 * The reference (jason-li-831202/Vehicle-CV-ADAS @ 2024_10_08) has no FFI: its engine seam is the
 * Python class protocol of coreEngine.py.  Each entry point below names the reference interface it
 * replaces (file:line, relative to the reference repo).  The ctypes stubs a reference maintainer
 * would add are shown in INTEGRATION.md; the in-tree host mirror is vehicle-cv-adas_amd/.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a negative
 * adas_status; adas_last_error() gives the message of the calling thread's last failure.
 * `stream` is a hipStream_t passed as void* (NULL = the library's own stream).  Pointers named d_*
 * are device (HBM) pointers, h_* host pointers.  All objects are single-threaded like the
 * reference engines (coreEngine.py:94-116): one caller at a time per handle.
 */
#ifndef ADAS_HIP_H
#define ADAS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    ADAS_OK = 0,
    ADAS_ERR_INVALID = -1,   /* bad argument */
    ADAS_ERR_IO = -2,        /* model file missing / unreadable (coreEngine.py:12-13) */
    ADAS_ERR_FORMAT = -3,    /* not a model container this library understands (coreEngine.py:14) */
    ADAS_ERR_HIP = -4,       /* HIP runtime failure */
    ADAS_ERR_CAPACITY = -5,  /* a fixed capacity (candidates, tracks, detections) was exceeded */
    ADAS_ERR_NO_DEVICE = -6  /* no gfx950 device visible: the library never falls back to the CPU */
} adas_status;

const char* adas_last_error(void);
int adas_version(void);
/* Number of visible HIP devices (<=0: none) and selection of the device subsequent handles live on
 * (reference: cuda.Device(0) hard-coded at coreEngine.py:47). */
int adas_device_count(void);
int adas_set_device(int index);
/* PCI address ("0000:c1:00.0") of device `index`, so that a one-process-per-GPU launcher can pin its launching thread to the GPU's
 * NUMA node (sharding.pin_rank; the reference is one process on cuda.Device(0), coreEngine.py:47). */
int adas_device_pci_bus_id(int index, char* out, int out_len);
/* Plain device-memory helpers so a ctypes/cgo caller can stage buffers without another runtime. */
int adas_malloc(void** d_ptr, size_t bytes);
int adas_free(void* d_ptr);
int adas_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes);
int adas_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes);
int adas_synchronize(void);
/* Page-locked host memory for frames that adas_pipeline_step_frames_host uploads asynchronously. */
int adas_host_alloc(void** h_ptr, size_t bytes);
int adas_host_free(void* h_ptr);
/* A pair of timing events for measuring a stretch of work ON THE STREAM IT IS LAUNCHED ON (bench.py's roofline / post_hbm legs:
 * no reference counterpart; the reference times with time.time() around synchronous calls, demo.py:262-281).
 * start/stop record on `stream`; elapsed_ms waits for the stop event. */
typedef struct adas_timer adas_timer;
int adas_timer_create(adas_timer** out);
int adas_timer_destroy(adas_timer* t);
int adas_timer_start(adas_timer* t, void* stream);
int adas_timer_stop(adas_timer* t, void* stream);
int adas_timer_elapsed_ms(adas_timer* t, float* ms);

/* ===================================================================================
 * Engine: replaces EngineBase / OnnxEngine / TensorRTEngine (coreEngine.py:7-39,120-186)
 * =================================================================================== */
typedef struct adas_engine adas_engine;

#define ADAS_PREC_BF16 0 /* bf16 storage + bf16 MFMA, fp32 accumulate (bench precision) */
#define ADAS_PREC_FP32 1 /* fp32 storage + fp32 MFMA (parity precision, 1e-3 vs the fp32 oracle) */
#define ADAS_PREC_FP16 2 /* IEEE half storage + f16 MFMA (bf16's rate, 11 significant bits), fp32 accumulate: the precision the
                          * reference ships (demo.py:18-29 *_fp16.trt; coreEngine.py:168 fp16 engine_dtype) */
#define ADAS_PREC_FP16X3 3 /* split precision: every activation and weight is a pair of halves (hi, lo * 2^11) = 22 significant
                            * bits, every product three f16 MFMAs (hi*hi + 2^-11 (hi*lo + lo*hi)), fp32 accumulate: f32-class results
                            * (the discrete decisions of the fp32 oracle chain) at a third of the 16-bit MFMA rate instead of
                            * the f32 MFMA's sixteenth */

/* OnnxEngine.__init__(path) / TensorRTEngine.__init__(path) (coreEngine.py:122-126,161-170).
 * `max_batch` frames per call are planned in HBM (the reference is fixed at 1). */
int adas_engine_create(const char* model_path, int precision, int max_batch, adas_engine** out);
int adas_engine_destroy(adas_engine* e);
/* get_engine_input_shape() -> [1,3,H,W] (coreEngine.py:144-145,178-179) */
int adas_engine_input_shape(const adas_engine* e, int64_t dims[4]);
/* get_engine_output_shape() -> (shapes, names) (coreEngine.py:147-148,181-182) */
int adas_engine_num_outputs(const adas_engine* e);
int adas_engine_output_shape(const adas_engine* e, int index, int64_t dims[4], int* ndim);
const char* adas_engine_output_name(const adas_engine* e, int index);
/* engine_inference(input_tensor) (coreEngine.py:150-157,184-186): NCHW fp32 host tensor in, fp32 host
 * tensors out in graph output order.  h_outputs[i] must hold batch * prod(dims[1:]) floats. */
int adas_engine_infer_host(adas_engine* e, const float* h_input_nchw, int batch, float* const* h_outputs);
/* Device-resident form ("frames never round-trip to host"): input is NCHW fp32 already in HBM;
 * outputs stay in HBM and are read through adas_engine_output_device(). Asynchronous on `stream`. */
int adas_engine_infer_device(adas_engine* e, const float* d_input_nchw, int batch, void* stream);
/* 1 when the engine's first layer is the fused stem (bf16 mode) and so can read the packed tensor of adas_preprocess_*_packed */
int adas_engine_accepts_packed_input(const adas_engine* e);
/* ADAS_PREC_* the engine was created with */
int adas_engine_precision(const adas_engine* e);
/* 1 when the model file declared float16 graph inputs (an fp16 ONNX export): the reference's OnnxEngine then reports
 * engine_dtype float16 and exchanges float16 arrays (coreEngine.py:168); the C seam stays fp32 either way. */
int adas_engine_model_io_half(const adas_engine* e);
int adas_engine_infer_device_packed(adas_engine* e, const uint16_t* d_input_nhwc4, int batch, void* stream);
const float* adas_engine_output_device(const adas_engine* e, int index);
/* Algorithmic work of one frame: 2*MACs over conv+linear layers and weight bytes. */
int adas_engine_stats(const adas_engine* e, double* flops_per_frame, double* weight_bytes, int* num_layers);
/* Per-layer device timing: `iters` forwards with one hipEvent behind every launch of the schedule (the null stream).  A launch's time,
 * less the cost of the marker itself, goes to the layer that carries its label (adas_engine_layer_kernel); a layer that rides in another
 * layer's launch, or that nothing computes, reads exactly 0. */
int adas_engine_profile(adas_engine* e, const float* d_input_nchw, int batch, int iters, float* ms_per_layer,
                        int max_layers, int* num_layers);
/* Pipeline-internal fast path of a v8-layout detector whose Detect head runs as the fused kernel (16-bit precisions): while a sink is
 * set, inference writes per anchor the best class probability and its first arg-max class ([batch][num_anchors] each) plus the four
 * box rows of the head, and NOT the head's class rows -- exactly what adas_yolo_post_run derives from them (yoloDetector.py:120-127).
 * Pass the arrays of adas_yolo_post_scan_views and run adas_yolo_post_run_prescanned afterwards; pass NULL, NULL to restore the full
 * head.  adas_pipeline_* does this around its own detector launches; engine_inference callers never see it. */
int adas_engine_detect_sink_supported(const adas_engine* e);
/* Layout (ADAS_HEAD_V8 | ADAS_HEAD_V5), anchor and class count of the head the sink describes: the arrays handed to
 * adas_engine_set_detect_sink hold [max_batch][num_anchors] entries. */
int adas_engine_detect_sink_shape(const adas_engine* e, int32_t* layout, int32_t* num_anchors, int32_t* num_classes);
int adas_engine_set_detect_sink(adas_engine* e, float* d_best_conf, int32_t* d_best_cls);
int adas_engine_layer_info(const adas_engine* e, int layer, char* name, int name_cap, double* flops, int* kind);
/* Which kernel instantiation layer `layer` launches at `batch` frames (matches the rocprofv3 kernel name). */
int adas_engine_layer_kernel(const adas_engine* e, int layer, int batch, char* name, int name_cap);
/* The launch schedule.  What one forward launches depends on the batch size (the kernel a conv resolves to does), so the engine decides
 * it once per batch size: which layers launch on their own, which ride in another layer's launch (the load-time fusions, a projection
 * shortcut folded at this batch), and which layers share a launch.  16-bit engines share launches in one of two ways, chosen by the
 * environment when the engine is created:
 *   grouped (the default; ADAS_NO_GROUP=1 keeps every layer its own launch): a run of consecutive 3x3 convs is launched level by
 *     dependency level, the independent layers of a level (at most 8) as ONE plain launch -- bit-identical to the per-layer launches;
 *   multi-layer (csrc/conv_ml.hip; OPT-IN, ADAS_ML=1 -- at 64 frames the per-layer launches measured faster): maximal runs
 *     of consecutive convolution layers that conv_halo / conv_pw would take run as ONE persistent launch each -- a table of (layer,
 *     tile, channel block) items behind per-layer, per-frame arrival counters -- bit-identical to the per-layer launches too.
 * adas_engine_prepare decides the schedule of a batch size and builds its device tables (adas_engine_create does it for max_batch;
 * adas_engine_infer_* and adas_pipeline_* call it themselves, outside stream captures; at most 16 batch sizes get shared launches, later
 * ones one launch per layer).  At a batch size nothing was prepared for, a forward inside a stream capture and the queries below use the
 * plain schedule (no shared launches).  adas_engine_launch_count = launches of one forward = steps of the schedule;
 * adas_engine_ml_info reports the multi-layer launches; adas_engine_ml_status synchronises and returns ADAS_ERR_HIP when a dependency
 * wait of the last launch timed out (every wait is bounded: a launch can fail, never hang). */
int adas_engine_prepare(adas_engine* e, int batch);
int adas_engine_ml_info(const adas_engine* e, int batch, int32_t* n_launches, int32_t* n_layers, int32_t* n_items);
int adas_engine_ml_status(const adas_engine* e, int batch, uint32_t* error_word);
int adas_engine_launch_count(adas_engine* e, int batch);
/* first 16 words of launch `launch`'s control block after its last run: ticket, error word, and (builds with -DADAS_ML_PROF only) the
 * per-phase cycle counters of the item loop (tools/ml_debug.py prof) */
int adas_engine_ml_counters(const adas_engine* e, int batch, int launch, uint32_t head16[16]);
/* The planner of those launches on descriptions alone (no device: tests/test_ml_plan.py).  A layer: kernel (1 = 3x3 halo conv, 4 = 1x1
 * pointwise: CONV_HALO / CONV_PW), stride, activation, residual mode, and its views as (buffer id, pixel stride, channel offset,
 * channels, h, w); `up_c` > 0: the first up_c input channels are read from the half-resolution view `up`.  Outputs: per layer its
 * producer layers after transitive reduction (deps[layer * 6 + k], -1 padded) and the arrivals per frame that complete them
 * (targets[...]); the item table in ticket order (low word: tile or chunk, high word: layer | channel block << 8 | frame << 16);
 * summary = {items, grid, LDS bytes, order mode}.  Returns ADAS_OK or ADAS_ERR_INVALID with the reason in adas_last_error(). */
typedef struct adas_ml_view {
    uint64_t buf;
    int32_t cs, coff, c, h, w;
} adas_ml_view;
typedef struct adas_ml_layer_desc {
    int32_t kernel, stride, act, res_mode, up_c, halo_bn;
    adas_ml_view x, y, res, up;   /* input, output, residual, half-resolution source */
} adas_ml_layer_desc;
int adas_debug_ml_plan(const adas_ml_layer_desc* layers, int n_layers, int batch, int precision, int32_t* deps, int32_t* targets,
                       uint64_t* items, int items_cap, int32_t summary[4]);
/* Which conv kernel one such layer launches on at `batch` frames in `precision` (ADAS_PREC_*), on the description alone: the label
 * adas_engine_layer_kernel gives the layer in an engine whose max_batch is `batch` (no device: tests/test_conv_route_cpu.py).  `kernel`
 * only tells 1x1 (4) from 3x3 (any other value); the kernel class comes from the plan. */
int adas_debug_conv_route(const adas_ml_layer_desc* layer, int batch, int precision, char* name, int name_cap);
/* Which body of conv_h8x3_kernel such a layer runs at `batch` frames in ADAS_PREC_FP16X3: 1 the one-pass body (each 32-channel chunk
 * streamed once, hi and lo together), 0 the two-pass body or another kernel altogether (adas_debug_conv_route names it), -1 a bad
 * argument.  Decided by the tile plan's window size and ADAS_H8X_ONEPASS (read once); no device. */
int adas_debug_h8x3_onepass(const adas_ml_layer_desc* layer, int batch);
/* The load-time plan of an engine: what adas_engine_create decided before it touched a weight.  One row of ADAS_PLAN_COLS int64 per
 * layer (rows[layer * ADAS_PLAN_COLS + column]); a link column holds a layer index or -1, an offset column bytes into the weight arena:
 *    0 kernel (weight packing, CONV_* of csrc/kernels.h)   1 skip (launches nothing: fused into a neighbour)
 *    2 fuse_pool   3 fuse_conv2 (stem: the max-pool / second conv in its launch)
 *    4 ds_src   5 ds_user (3x3 conv <-> the 1x1 stride-2 projection shortcut it can carry)
 *    6 up_src (1x1 conv: the upsample folded into its loads)   7..8 pool3 (max-pool: the two pools chained into its launch)
 *    9 pair_b (first conv of a 3x3 pair: the second)   10..12 c2f (cv1 of a fused C2f block: conv A, conv B, cv2)
 *   13..18 det_src (Detect: the 1x1 convs folded into the decode)   19 halo_bn   20 has_x3h8 (second fp16x3 packing)
 *   21 k   22 kpad   23 cin_pad   24 cout_pad (0 for layers without packed conv weights)
 *   25 w_off   26 b_off   27 ds_w_off   28 x3h8_w_off
 * adas_engine_plan reads a live engine.  adas_debug_engine_plan needs no device: `tables` are the first `weights_off` bytes of a model
 * container (header and the three tables), which it reads, validates and plans exactly as adas_engine_create does -- the same error codes
 * and texts for a container that is refused -- without touching a weight (tests/test_engine_plan_cpu.py).  `rows` may be NULL to ask for
 * n_ops alone; ADAS_ERR_CAPACITY when rows_cap (in rows) is too small. */
#define ADAS_PLAN_COLS 29
int adas_engine_plan(const adas_engine* e, int64_t* rows, int rows_cap, int32_t* n_ops, uint64_t* weight_bytes);
int adas_debug_engine_plan(const void* tables, size_t bytes, int precision, int max_batch, int64_t* rows, int rows_cap, int32_t* n_ops,
                           uint64_t* weight_bytes);
/* The schedule of one batch size, layer by layer: step_of[layer] = the launch (0 .. n_steps - 1, in launch order) that computes the
 * layer, or -1 where nothing does; role[layer] = what the layer is to the forward:
 *    0 launches on its own                                 1 / 2 leads / rides in a grouped launch
 *    3 / 4 leads / rides in a multi-layer launch           5 projection shortcut computed inside the conv that adds it
 *    6 upsample folded into its consumer's loads           7 second / third pool of the SPPF pool launch
 *    8 / 9 / 10 fused C2f block: cv1 (launches it), the Bottleneck's convs (stay in LDS), cv2 (materialised)
 *   11 / 12 3x3 pair: first conv (launches it, stays in LDS), second conv
 *   13 1x1 conv computed inside the Detect launch          14 / 15 / 16 fused stem: the conv (launches it), the input conversion, the pool / second conv
 * A launch's first layer by role (0, 1, 3, 8, 11, 14) carries its label and its profiled time.  adas_engine_schedule reads a live engine
 * (the prepared schedule, else the plain one).  adas_debug_engine_schedule needs no device: it reads, validates and plans `tables` as
 * adas_debug_engine_plan does, decides the schedule with the mode the environment selects (ADAS_ML, ADAS_NO_GROUP) and also writes the
 * labels adas_engine_layer_kernel would give (labels[layer * ADAS_LABEL_CAP], may be NULL) -- tests/test_engine_schedule_cpu.py.  All
 * arrays may be NULL to ask for the counts alone; ADAS_ERR_CAPACITY when cap (in layers) is too small. */
#define ADAS_LABEL_CAP 96
int adas_engine_schedule(const adas_engine* e, int batch, int32_t* step_of, int32_t* role, int cap, int32_t* n_ops, int32_t* n_steps);
int adas_debug_engine_schedule(const void* tables, size_t bytes, int precision, int max_batch, int batch, int32_t* step_of, int32_t* role,
                               char* labels, int cap, int32_t* n_ops, int32_t* n_steps);
/* Debug/parity tap: copy an intermediate activation (by layer index) to the host as NCHW fp32.  ADAS_ERR_INVALID for a layer whose
 * role (above) leaves it no activation in memory: 5, 6, 8, 9, 11, 13, 14, 15. */
int adas_engine_fetch_activation(adas_engine* e, int layer, int batch, float* h_out_nchw, int64_t dims[4]);

/* ===================================================================================
 * Frame pre-processing on the device (the layer in front of the engine seam): `n` BGR u8 frames
 * (H x W x 3, tightly packed, back to back) in HBM -> the (n,3,h,w) fp32 tensor engine_inference takes.
 * adas_preprocess_yolo replaces YoloDetector.__prepare_input (yoloDetector.py:96-102) =
 * Scaler.process_image (utils.py:42-63) + cv2.dnn.blobFromImage(1/255, swapRB);
 * adas_preprocess_ufld replaces UltrafastLaneDetectorV2.__prepare_input (ultrafastLaneDetectorV2.py:96-112).
 * cv2.resize INTER_LINEAR is restated from OpenCV's 8-bit fixed-point path (parity with cv2 unpinned).
 * =================================================================================== */
int adas_preprocess_yolo(const uint8_t* d_frames_bgr, int n, int src_h, int src_w, float* d_out_nchw, int dst_h,
                         int dst_w, int keep_ratio, void* stream);
int adas_preprocess_ufld(const uint8_t* d_frames_bgr, int n, int src_h, int src_w, float* d_out_nchw, int in_h,
                         int in_w, double crop_ratio, void* stream);
/* The same two conversions into the layout the fused first layer stages anyway: (c0, c1, c2, 0) bf16 pixels, NHWC, 8 bytes per
 * pixel, rounded exactly as the engine rounds the fp32 tensor -- for adas_engine_infer_device_packed (device-resident path:
 * the tensor between pre-processing and the first conv shrinks from 12 to 8 bytes per pixel, same network values). */
int adas_preprocess_yolo_packed(const uint8_t* d_frames_bgr, int n, int src_h, int src_w, uint16_t* d_out_nhwc4, int dst_h,
                                int dst_w, int keep_ratio, void* stream);
int adas_preprocess_ufld_packed(const uint8_t* d_frames_bgr, int n, int src_h, int src_w, uint16_t* d_out_nhwc4, int in_h,
                                int in_w, double crop_ratio, void* stream);
/* The packed form in the 16-bit type of the engine that will consume it: precision = ADAS_PREC_BF16 (what the two calls above
 * write) or ADAS_PREC_FP16. */
int adas_preprocess_yolo_packed_prec(const uint8_t* d_frames_bgr, int n, int src_h, int src_w, uint16_t* d_out_nhwc4, int dst_h,
                                     int dst_w, int keep_ratio, int precision, void* stream);
int adas_preprocess_ufld_packed_prec(const uint8_t* d_frames_bgr, int n, int src_h, int src_w, uint16_t* d_out_nhwc4, int in_h,
                                     int in_w, double crop_ratio, int precision, void* stream);

/* ===================================================================================
 * YOLO post-processing: replaces YoloDetector.__process_output (yoloDetector.py:104-133),
 * Scaler.convert_boxes_coordinate (utils.py:70-87), NMS.fast_soft_nms / NMS.fast_nms
 * (utils.py:161-256 / 105-159), get_nms_results + RectInfo.tolist (yoloDetector.py:135-157,
 * core.py:18-23).  fp64 from the box corners onward; survivor indices bit-exact.
 * =================================================================================== */
typedef struct adas_yolo_post adas_yolo_post;

#define ADAS_HEAD_V8 0 /* (4+nc, A) channel-major: YOLOv8/9/10 (yoloDetector.py:114-115,121-122) */
#define ADAS_HEAD_V5 1 /* (A, 5+nc) row-major, conf = cls*obj in fp32: YOLOv5/6/7 (yoloDetector.py:123-124) */
#define ADAS_HEAD_V5_LITE 2 /* V5 layout holding raw grid offsets: adds YoloLiteParameters.lite_postprocess (yoloDetector.py:35-49) */
#define ADAS_NMS_REFERENCE 0 /* production call yoloDetector.py:139, bug-compatible (SURVEY finding 1) */
#define ADAS_NMS_GREEDY 1    /* NMS.fast_nms, the commented alternative yoloDetector.py:138 */

typedef struct {
    int32_t layout;         /* ADAS_HEAD_V8 | ADAS_HEAD_V5 | ADAS_HEAD_V5_LITE */
    int32_t num_anchors;    /* 8400 | 25200 */
    int32_t num_classes;    /* 80 */
    int32_t nms_mode;       /* ADAS_NMS_* */
    double box_score;       /* keep if conf > box_score (strict), >= 0 */
    double iou_thr;         /* box_nms_iou */
    int32_t pad_h, pad_w;   /* Scaler._pad_shape (utils.py:62) */
    double ratio_h, ratio_w; /* Scaler.get_scale_ratio() (utils.py:65-68) */
    int32_t max_candidates; /* capacity per frame; exceeding it sets ADAS_ERR_CAPACITY on fetch */
    int32_t reserved;
} adas_yolo_post_params;

/* Scaler.process_image geometry without the pixels (utils.py:42-63): fills pad_* and ratio_*. */
int adas_letterbox_params(int src_h, int src_w, int dst_h, int dst_w, int keep_ratio, adas_yolo_post_params* p);

int adas_yolo_post_create(const adas_yolo_post_params* p, int max_batch, adas_yolo_post** out);
int adas_yolo_post_destroy(adas_yolo_post* h);
/* Network input size (YoloLiteParameters.input_shape, yoloDetector.py:30): the v5-lite grid decode derives its three
 * grids from it; required before the first run of an ADAS_HEAD_V5_LITE handle, ignored by the other layouts. */
int adas_yolo_post_set_input_size(adas_yolo_post* h, int in_h, int in_w);
/* d_head: batch head tensors back to back in the reference layout, fp32, in HBM. Asynchronous. */
int adas_yolo_post_run(adas_yolo_post* h, const float* d_head, int batch, void* stream);
/* The same two launches `iters` times on the null stream with events between them: ms[0] = the head scan (per-anchor best class,
 * HBM-bound: the whole head tensor is read once), ms[1] = candidate compaction + inverse letterbox + NMS + RectInfo (latency-bound),
 * averaged per run.  Measurement only (bench.py `post_hbm`). */
/* The post-processing without its class scan: per-anchor (best probability, class) were written into the arrays of
 * adas_yolo_post_scan_views by the producer of the head (adas_engine_set_detect_sink); d_head supplies the box rows. */
int adas_yolo_post_scan_views(adas_yolo_post* h, float** d_best_conf, int32_t** d_best_cls);
int adas_yolo_post_run_prescanned(adas_yolo_post* h, const float* d_head, int batch, void* stream);
int adas_yolo_post_profile(adas_yolo_post* h, const float* d_head, int batch, int iters, float ms[2]);

typedef struct {
    int32_t n_found;       /* anchors over threshold (may exceed capacity) */
    int32_t n_candidates;  /* stored */
    int32_t n_keep;        /* survivors */
    int32_t flags;         /* bit0: capacity overflow */
} adas_yolo_counts;
/* Synchronises, then copies frame `frame`'s results.  Any pointer may be NULL.  Arrays must hold
 * max_candidates entries (x4 for boxes).  cand_*: thresholded rows in anchor order after the inverse
 * letterbox (xywh fp64); keep: NMS result as indices into the candidates, in the reference's order;
 * det_*: RectInfo fields of the survivors; det_xyxy_int = RectInfo.tolist(). */
int adas_yolo_post_fetch(adas_yolo_post* h, int frame, adas_yolo_counts* counts, int32_t* cand_anchor,
                         double* cand_xywh, double* cand_conf, int32_t* cand_cls, int32_t* keep, double* det_xywh,
                         double* det_conf, int32_t* det_cls, int32_t* det_xyxy_int);
/* The survivors only (what yoloDetector.py:141-157 turns into RectInfo), as ONE device-to-host message: a pack kernel behind the NMS
 * writes [counts][n_keep x 64-byte record] and one copy brings it over (a second one past 62 survivors).  Same values, same error
 * behaviour as adas_yolo_post_fetch's keep / det_* arrays; arrays hold max_candidates entries, any pointer may be NULL. */
int adas_yolo_post_fetch_dets(adas_yolo_post* h, int frame, adas_yolo_counts* counts, int32_t* keep, double* det_xywh,
                              double* det_conf, int32_t* det_cls, int32_t* det_xyxy_int);
/* Device views of the survivors for GPU-resident consumers (the tracker): per-frame strides are
 * max_candidates entries.  xyxy as fp64 of the int-truncated corners, scores fp64, classes, counts[4]. */
int adas_yolo_post_device_views(adas_yolo_post* h, const double** d_xyxy, const double** d_score,
                                const int32_t** d_cls, const int32_t** d_counts);
int adas_yolo_post_capacity(const adas_yolo_post* h, int* max_candidates);
/* The head tensor this handle reads: layout (ADAS_HEAD_*), anchors A, classes nc -- (1, 4+nc, A) for V8, (1, A, 5+nc) for V5 /
 * V5_LITE (yoloDetector.py:110-124).  adas_pipeline_create checks the detector engine's output against it. */
int adas_yolo_post_head_shape(const adas_yolo_post* h, int32_t* layout, int32_t* num_anchors, int32_t* num_classes);

/* ===================================================================================
 * EfficientDet post-processing: replaces EfficientdetDetector.__process_output (efficientdetDetector.py:67-85) with
 * Scaler.convert_boxes_coordinate (utils.py:70-87).  Inputs are the exported graph's three outputs (decode and NMS live inside
 * it): boxes (n, 4) xyxy float32 in input pixels, class ids (n) int32, confidences (n) float32.  float32 arithmetic, as in the
 * reference; order kept; a detection is dropped iff conf < box_score.
 * =================================================================================== */
typedef struct adas_effdet_post adas_effdet_post;
typedef struct {
    double box_score;        /* 0.6 in the reference's defaults */
    int32_t pad_h, pad_w;    /* Scaler._pad_shape (fill with adas_letterbox_params) */
    double ratio_h, ratio_w; /* Scaler.get_scale_ratio() */
    int32_t max_boxes;       /* per frame, <= 4096 */
    int32_t reserved;
} adas_effdet_post_params;
int adas_effdet_post_create(const adas_effdet_post_params* p, int max_batch, adas_effdet_post** out);
int adas_effdet_post_destroy(adas_effdet_post* h);
/* Frame b reads h_counts[b] detections at row offset b * max_boxes of the three device arrays. */
int adas_effdet_post_run(adas_effdet_post* h, const float* d_boxes, const int32_t* d_ids, const float* d_confs,
                         const int32_t* h_counts, int batch, void* stream);
/* Synchronises.  xywh [k][4] float32 (RectInfo x, y, width, height), conf [k], class_id [k], xyxy_int [k][4]; returns k in *n_keep. */
int adas_effdet_post_fetch(adas_effdet_post* h, int frame, int32_t* n_keep, float* xywh, float* conf, int32_t* class_id,
                           int32_t* xyxy_int);
/* The in-graph tail of the exported EfficientDet-D0 the reference loads (efficientdetDetector.py:38 OnnxEngine(model_path); its three
 * outputs are read at :68-70): anchor decode, score threshold and per-class NMS over the network's raw head tensors (per pyramid
 * level l = 0..4, stride 8 << l: box regression [batch][cells_l * 9][4] as (dy, dx, dh, dw) and class logits
 * [batch][cells_l * 9][num_classes], rows ordered (y, x, anchor) -- the ten outputs of the "efficientdet-d0" engine graph).  The
 * reference holds no such graph or weights: the steps restate the published post-processing of the architecture (csrc/post_core.h
 * effdet_tail_frame).  Output per frame: boxes (n, 4) xyxy float32 in input pixels, class ids, confidences, by descending
 * confidence -- what adas_effdet_post_run consumes. */
typedef struct adas_effdet_tail adas_effdet_tail;
typedef struct {
    int32_t in_h, in_w;          /* network input (multiples of 128) */
    int32_t num_classes;         /* 90 for the COCO export */
    int32_t max_candidates;      /* anchors over score_thr per frame, <= 3072 (more: ADAS_ERR_CAPACITY at fetch) */
    int32_t max_det;             /* survivors per frame */
    int32_t reserved;
    double score_thr, iou_thr;   /* score > score_thr is a candidate; IoU > iou_thr suppresses within a class */
    double anchor_scale;         /* 4.0 */
} adas_effdet_tail_params;
int adas_effdet_tail_create(const adas_effdet_tail_params* p, int max_batch, adas_effdet_tail** out);
int adas_effdet_tail_destroy(adas_effdet_tail* h);
int adas_effdet_tail_run(adas_effdet_tail* h, const float* const* d_reg /* [5] */, const float* const* d_cls /* [5] */, int batch, void* stream);
/* Synchronises.  boxes_xyxy [n][4], class_id [n], conf [n]; n_candidates (optional) = anchors over the threshold. */
int adas_effdet_tail_fetch(adas_effdet_tail* h, int frame, int32_t* n_det, float* boxes_xyxy, int32_t* class_id, float* conf,
                           int32_t* n_candidates);
/* Device-resident results: boxes [max_batch][max_det][4], ids / confs [max_batch][max_det], counts [max_batch][2] (survivors, candidates). */
int adas_effdet_tail_device_views(adas_effdet_tail* h, const float** d_boxes, const int32_t** d_ids, const float** d_confs,
                                  const int32_t** d_counts);
/* EfficientdetDetector.__prepare_input (efficientdetDetector.py:57-65): Scaler.process_image letterbox (canvas 114), then
 * (pixel / 255 - mean) / std per BGR channel -- NO channel swap -- with mean (0.406, 0.456, 0.485), std (0.225, 0.224, 0.229),
 * evaluated in double and cast to float32; NCHW. */
int adas_preprocess_effdet(const uint8_t* d_frames_bgr, int n, int src_h, int src_w, float* d_out_nchw, int dst_h, int dst_w,
                           int keep_ratio, void* stream);

/* ===================================================================================
 * UFLDv2 lane decode: replaces UltrafastLaneDetectorV2.__process_output
 * (ultrafastLaneDetectorV2.py:114-181, _softmax :15-19, ModelConfig :21-55)
 * =================================================================================== */
typedef struct adas_ufld_decode adas_ufld_decode;
#define ADAS_UFLD_MAX_POINTS 128

typedef struct {
    int32_t grid_row, cls_row, grid_col, cls_col; /* 200,72,100,81 (CULane) */
    int32_t img_w, img_h;                         /* source image size the points are scaled to */
    int32_t local_width;                          /* 1 */
    int32_t num_lanes;                            /* last tensor dimension: 4 (CULane / Tusimple), 10 (CurveLanes configs,
                                                   * configs/curvelanes_res18.py:25); 0 = 4.  Lanes 1,2 (rows) and 0,3 (columns)
                                                   * are decoded whatever the count (ultrafastLaneDetectorV2.py:141-142) */
    const double* h_row_anchor;                   /* [cls_row] cfg.row_anchor (host) */
    const double* h_col_anchor;                   /* [cls_col] cfg.col_anchor (host) */
} adas_ufld_params;

int adas_ufld_decode_create(const adas_ufld_params* p, int max_batch, adas_ufld_decode** out);
int adas_ufld_decode_destroy(adas_ufld_decode* h);
/* Four device tensors in the engine's output layout (1,G,K,4); frame b is at ptr + b*batch_stride_* */
int adas_ufld_decode_run(adas_ufld_decode* h, const float* d_loc_row, const float* d_loc_col,
                         const float* d_exist_row, const float* d_exist_col, size_t stride_loc_row,
                         size_t stride_loc_col, size_t stride_exist_row, size_t stride_exist_col, int batch,
                         void* stream);
/* lane order: left-side, left-ego, right-ego, right-side (ultrafastLaneDetectorV2.py:143-145).
 * points: [4][ADAS_UFLD_MAX_POINTS][2] (x,y) int32; counts[4]; detected[4]. */
int adas_ufld_decode_fetch(adas_ufld_decode* h, int frame, int32_t* points, int32_t* counts, int32_t* detected);
/* The inverse of fetch: places lane points decoded elsewhere into frame `frame`'s slot (same array shapes), e.g. to run
 * adas_lane_geometry on them. */
int adas_ufld_decode_upload(adas_ufld_decode* h, int frame, const int32_t* points, const int32_t* counts, const int32_t* detected);

/* -----------------------------------------------------------------------------------
 * UFLD (v1) lane decode: replaces UltrafastLaneDetector.__process_output (ultrafastLaneDetector.py:96-139,
 * ModelConfig :16-40).  One (1, griding_num+1, cls_num_per_lane, 4) tensor per frame; the handle type, fetch and
 * destroy are shared with the v2 decoder (lane index = the tensor's lane axis, points in the reference's order).
 * ----------------------------------------------------------------------------------- */
typedef struct {
    int32_t griding_num, cls_num_per_lane; /* 100,56 (Tusimple) | 200,18 (CULane) */
    int32_t cfg_img_w, cfg_img_h;          /* ModelConfig.img_w/img_h: 1280x720 | 1640x590 */
    int32_t input_w, input_h;              /* network input, 800x288 */
    int32_t src_w, src_h;                  /* source frame size: w_ratio/h_ratio of ultrafastLaneDetector.py:80 */
    const double* h_row_anchor;            /* [cls_num_per_lane] cfg.row_anchor (host) */
} adas_ufld1_params;
int adas_ufld1_decode_create(const adas_ufld1_params* p, int max_batch, adas_ufld_decode** out);
int adas_ufld1_decode_set_source_size(adas_ufld_decode* h, int src_w, int src_h);
/* 1: handle made by adas_ufld1_decode_create (UFLD v1), 2: by adas_ufld_decode_create (UFLDv2), 0: NULL */
int adas_ufld_decode_kind(const adas_ufld_decode* h);
/* The tensors this handle decodes, in engine output order: returns their number (4 for UFLDv2: loc_row, loc_col, exist_row,
 * exist_col, ultrafastLaneDetectorV2.py:118; 1 for UFLD v1) and fills dims[i] = (1, G, K, 4).  < 0: error. */
int adas_ufld_decode_expected_outputs(const adas_ufld_decode* h, int64_t dims[4][4]);
int adas_ufld1_decode_run(adas_ufld_decode* h, const float* d_out, size_t batch_stride, int batch, void* stream);

/* -----------------------------------------------------------------------------------
 * Ego-lane geometry on the decoder's device-resident points: replaces
 * LaneDetectBase.__update_lanes_status / __update_lanes_area / __adjust_lanes_points (ufldDetector/core.py:102-158),
 * PerspectiveTransformation.transformToBirdViewPoints and .calcCurveAndOffset (perspectiveTransformation.py:120-214,
 * without the drawing calls).  One homography for the whole batch (create / set_matrix), or one per frame from a device table
 * (run_matrices: adas_birdview keeps updateTransformParams, :39-86, on the device per stream).
 * ----------------------------------------------------------------------------------- */
typedef struct adas_lane_geometry adas_lane_geometry;
typedef struct {
    int32_t img_h;         /* source frame height = resampling count of __adjust_lanes_points (core.py:130) */
    int32_t bird_w, bird_h; /* PerspectiveTransformation.img_size (bird-view image); bird_h must exceed 719 for the curvature
                              (the reference reads row 719, perspectiveTransformation.py:196-199) */
    int32_t adjust_lanes;  /* default for run() */
    double M[9];           /* frontal -> bird-view homography, row-major (cv2.getPerspectiveTransform, :33) */
} adas_lane_geometry_params;
typedef struct {
    int32_t area_status;          /* both ego lanes detected (core.py:143-148) */
    int32_t n_area_left, n_area_right; /* area_points = left points then the reversed right points (core.py:158) */
    int32_t direction;            /* 0: no curve estimate, 1 "L", 2 "R", 3 "F" (perspectiveTransformation.py:170-175) */
    int32_t bird_counts[4];       /* points per lane in the bird view */
    double curvature;             /* metres (:193) */
    double offset;                /* metres from the lane centre (:201-202) */
} adas_lane_geometry_result;
int adas_lane_geometry_create(const adas_lane_geometry_params* p, int max_batch, adas_lane_geometry** out);
int adas_lane_geometry_destroy(adas_lane_geometry* h);
int adas_lane_geometry_set_matrix(adas_lane_geometry* h, const double* M9);
/* Reads the lane points the decoder (v1 or v2 handle) left in HBM for frames [0, batch). Asynchronous.
 * adjust_lanes < 0: the value given at create. */
int adas_lane_geometry_run(adas_lane_geometry* h, const adas_ufld_decode* decode, int adjust_lanes, int batch, void* stream);
/* The same kernel text with frame f reading its homography from d_M + 9 f (device, [batch][9] row-major, e.g. the first table of
 * adas_birdview_device_views) instead of the handle's matrix.  A plain launch: capturable, and a changed matrix needs no re-capture. */
int adas_lane_geometry_run_matrices(adas_lane_geometry* h, const adas_ufld_decode* decode, int adjust_lanes, int batch, const double* d_M,
                                    void* stream);
/* area_points: room for [2*img_h][2] int32 (x,y); bird_points: [4][ADAS_UFLD_MAX_POINTS][2]; either may be NULL. */
int adas_lane_geometry_fetch(adas_lane_geometry* h, int frame, adas_lane_geometry_result* res, int32_t* area_points,
                             int32_t* bird_points);
/* Device views of the results for GPU-resident consumers (adas_analysis_run): per frame 8 header words (area_status, n_area_left,
 * n_area_right, direction, bird_counts[4]: the int32 fields of adas_lane_geometry_result in order), 2 doubles (curvature, offset) and
 * the area polygon, frame f's (x, y) pairs at d_area + f * area_stride int32 (room for 2 * img_h points). */
int adas_lane_geometry_device_views(adas_lane_geometry* h, const int32_t** d_header, const double** d_values, const int32_t** d_area,
                                    int32_t* area_stride);
/* veh_pos of frame `frame`: the vehicle's bird-view column (lx + rx) / 2 that the offset is measured from (perspectiveTransformation.py:198),
 * kept per frame in an fp64 device array of its own beside the results above; 0.0 when the frame has no curve (direction NONE).  The
 * overlay's readouts stage draws its arrow there.  Waits for the handle's last run. */
int adas_lane_geometry_fetch_veh_pos(adas_lane_geometry* h, int frame, double* veh_pos);

/* -----------------------------------------------------------------------------------
 * Bird-view image: replaces the cv2.warpPerspective calls of PerspectiveTransformation.transformToBirdView /
 * .transformToFrontalView (perspectiveTransformation.py:89-117) for 8-bit BGR frames, INTER_LINEAR, BORDER_CONSTANT 0, on frames
 * that already sit in HBM.  The arithmetic restates OpenCV 4.5's reference path (csrc/warp_core.h); parity with a real cv2
 * build is UNPINNED.  One matrix per frame of a batch; matrices may change between runs.
 * ----------------------------------------------------------------------------------- */
typedef struct adas_warp adas_warp;
typedef struct {
    int32_t src_h, src_w; /* source frames: [batch][src_h][src_w][3] u8 */
    int32_t dst_h, dst_w; /* warped frames: [batch][dst_h][dst_w][3] u8; all four: 1..4320 rows, 1..16384 columns */
} adas_warp_params;
/* Host state only (every matrix starts as the identity); device memory is allocated by the first run / device_view. */
int adas_warp_create(const adas_warp_params* p, int max_batch, adas_warp** out);
int adas_warp_destroy(adas_warp* h);
/* M9: row-major 3x3.  inverse_map = 0: M maps source to destination (the cv2 default) and is inverted here, a singular
 * matrix is ADAS_ERR_INVALID; inverse_map != 0: M maps destination to source (cv2.WARP_INVERSE_MAP).  frame = -1 sets the
 * matrix of every frame.  Takes effect with the next run. */
int adas_warp_set_matrix(adas_warp* h, int frame, const double* M9, int inverse_map);
/* Warps frames [0, batch) of d_src_bgr, frame f with matrix f.  Asynchronous on `stream`; matrices changed since the last run
 * are copied to the device on that stream ahead of the kernel, from pageable host memory: such a run may block the host until the
 * copy is staged, and is not capturable into a graph (a run with no matrix changed since the last one is a plain launch).
 * d_dst_bgr may be NULL: the handle's own [max_batch][dst_h][dst_w][3] buffer is written. */
int adas_warp_run(adas_warp* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, int batch, void* stream);
/* The same kernel with frame f's matrix read from d_M_warp + 9 f (device, [batch][9], destination -> source: what set_matrix forms
 * by inversion, e.g. the second table of adas_birdview_device_views).  The handle's host matrices are neither read nor copied: a plain
 * launch, capturable into a graph -- with d_dst_bgr = NULL once the handle's own buffer exists (adas_warp_device_view allocates it). */
int adas_warp_run_device_matrices(adas_warp* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, const double* d_M_warp, int batch, void* stream);
/* Frame `frame` of the handle's own buffer -> h_dst_bgr [dst_h][dst_w][3], after the last run's stream has drained.  A frame that no
 * run has written (frame >= the largest batch run with d_dst_bgr = NULL) is ADAS_ERR_INVALID. */
int adas_warp_fetch(adas_warp* h, int frame, uint8_t* h_dst_bgr);
int adas_warp_device_view(adas_warp* h, const uint8_t** d_dst_bgr);

/* -----------------------------------------------------------------------------------
 * Per-stream adaptive bird view: replaces PerspectiveTransformation.__init__ / .updateTransformParams
 * (perspectiveTransformation.py:21-86) with one trapezoid per video stream kept on the device.  The host (its TaskConditions state
 * machine, demo.py:287-292) only says WHICH re-anchoring rule a stream applies next; the kernel applies it if and only if the two ego
 * lanes of that frame are detected (area_status, core.py:143-148), consumes the request either way, solves
 * cv2.getPerspectiveTransform both ways in fp64 (csrc/birdview_core.h; agreement with LAPACK / cv2 to rounding, not bit for bit) and
 * leaves every frame's matrices in device tables for adas_lane_geometry_run_matrices and adas_warp_run_device_matrices.
 * An update whose trapezoid is degenerate (singular system, non-finite result, det M == 0) is REJECTED: the state stays bit for bit
 * what it was and n_rejected counts it -- the reference raises or goes on with garbage there.
 * ----------------------------------------------------------------------------------- */
typedef struct adas_birdview adas_birdview;
typedef struct {
    int32_t img_w, img_h;   /* PerspectiveTransformation.img_size: the initial trapezoid and the destination corners (:24-34) */
} adas_birdview_params;
#define ADAS_BIRDVIEW_NONE 0
#define ADAS_BIRDVIEW_DEFAULT 1  /* updateTransformParams(..., "Default") */
#define ADAS_BIRDVIEW_TOP 2      /* "Top": the bottom corners move by -10 / +10 from where they ARE, every time it is applied */
#define ADAS_BIRDVIEW_BOTTOM 3   /* "Bottom" */
typedef struct {
    float src[8];         /* frontal-view trapezoid, float32 as in the reference: tl, bl, br, tr as (x, y) */
    double M[9];          /* frontal -> bird view, row-major */
    double M_inv[9];      /* bird view -> frontal (transformToFrontalView) */
    double M_warp[9];     /* inverse of M by the warp's own 3x3 inversion: the destination -> source matrix of the bird-view image */
    int32_t n_updates;    /* requests applied */
    int32_t n_rejected;   /* requests rejected as degenerate */
} adas_birdview_state;
/* max_frames: frames of one run the per-frame tables hold (n_streams x frames per stream), >= n_streams. */
int adas_birdview_create(const adas_birdview_params* p, int n_streams, int max_frames, adas_birdview** out);
int adas_birdview_destroy(adas_birdview* h);
/* Back to PerspectiveTransformation(img_size); drops a queued request.  stream = -1: every stream.  Waits for the whole device. */
int adas_birdview_reset(adas_birdview* h, int stream);
/* Queues `mode` (ADAS_BIRDVIEW_*; any other value is consumed without effect, as the reference ignores an unknown type) for the
 * stream's NEXT run only: one word stored into a device table by a launch on hip_stream, so it must be the stream the next run is
 * ordered behind.  No configuration generation moves and no captured step is dropped.  A later request before the run replaces it. */
int adas_birdview_request(adas_birdview* h, int stream, int mode, void* hip_stream);
/* One launch, one wave per stream.  Frame b of stream s is frame b * n_streams + s of the decoder.  The queued mode meets frame 0 of
 * the stream; frames are walked in temporal order and every frame's matrices go to row b * n_streams + s of the tables, so later
 * frames of the run carry the updated state.  A plain launch: capturable. */
int adas_birdview_run(adas_birdview* h, const adas_ufld_decode* decode, int n_streams, int n_frames, void* hip_stream);
/* The live state of one stream.  Synchronises with the last run's stream. */
int adas_birdview_fetch_stream(adas_birdview* h, int stream, adas_birdview_state* state);
/* Row `frame` of the last run: M9, M_warp9 and applied (1: the request was applied on this frame, -1: rejected on it, 0: neither);
 * any of the three may be NULL.  Synchronises. */
int adas_birdview_fetch_frame(adas_birdview* h, int frame, double* M9, double* M_warp9, int32_t* applied);
/* The mode still queued for a stream (0: none).  Waits for the whole device. */
int adas_birdview_pending(adas_birdview* h, int stream, int32_t* mode);
/* The per-frame tables, [max_frames][9] doubles each; before the first run every row holds the initial matrices. */
int adas_birdview_device_views(adas_birdview* h, const double** d_M, const double** d_M_warp);

/* -----------------------------------------------------------------------------------
 * Distance, collision and warning state per stream: replaces the last block of the reference's loop (demo.py:284-296) --
 * SingleCamDistanceMeasure.updateDistance / calcCollisionPoint (ObjectDetector/distanceMeasure.py:50-93) and TaskConditions
 * .UpdateCollisionStatus / UpdateOffsetStatus / UpdateRouteStatus / CheckStatus (taskConditions.py:88-312) -- with one state machine
 * per video stream kept on the device (csrc/analysis_core.h).  Per frame: the three updates in the reference's order, then CheckStatus()
 * FOR THE NEXT FRAME (the reference calls it at the start of that frame; nothing in between touches what it reads); its result is the
 * stream's request word: the new transform_status (ADAS_BIRDVIEW_*) when it returned true, else ADAS_BIRDVIEW_NONE.  A new or reset
 * stream is TaskConditions() after its first CheckStatus(), which returns true with "Default": the owner of a bird view queues that one.
 * Defined where the reference leaves it to chance: a window that mixes directions picks R before L before F (what its
 * max(set(...), key=...) returns under PYTHONHASHSEED=0); a frame whose curvature is not finite (the reference raises) counts as a frame
 * without a curve estimate, in n_nonfinite.
 * ----------------------------------------------------------------------------------- */
typedef struct adas_analysis adas_analysis;
typedef struct {
    double focal;               /* SingleCamDistanceMeasure.f: 100 (distanceMeasure.py:21) */
    double y_limit;             /* boxes whose bottom lies below this row are not measured: 650 (:62) */
    double distance_thres;      /* UpdateCollisionStatus: 1.5 */
    double offset_thres;        /* UpdateOffsetStatus: 0.65 */
    double curvae_thres;        /* UpdateRouteStatus: 500 */
    double calib_curvae_thres;  /* _calibration_curve: 15000 */
    int32_t calib_frequency;    /* _calibration_curve: 3 */
    int32_t n_classes;          /* entries of h_ref_height */
    const double* h_ref_height; /* [n_classes] (host, copied): RefSizeDict[label][0] in inches for the detector's class ids, 0 for a class
                                 * outside object_list (the device never sees a label string) */
    int32_t max_points;         /* survivors read and distance points kept per frame, 1..2048 (512) */
    int32_t max_poly;           /* points of a frame's ego-lane polygon, 1..8640 (1440 = 2 x 720 rows) */
} adas_analysis_params;
#define ADAS_COLLISION_UNKNOWN 0 /* CollisionType (ObjectDetector/utils.py:8-12) */
#define ADAS_COLLISION_NORMAL 1
#define ADAS_COLLISION_PROMPT 2
#define ADAS_COLLISION_WARNING 3
#define ADAS_OFFSET_UNKNOWN 0    /* OffsetType (ufldDetector/utils.py:10-14) */
#define ADAS_OFFSET_RIGHT 1
#define ADAS_OFFSET_LEFT 2
#define ADAS_OFFSET_CENTER 3
#define ADAS_CURVATURE_UNKNOWN 0 /* CurvatureType (ufldDetector/utils.py:16-22) */
#define ADAS_CURVATURE_STRAIGHT 1
#define ADAS_CURVATURE_EASY_LEFT 2
#define ADAS_CURVATURE_HARD_LEFT 3
#define ADAS_CURVATURE_EASY_RIGHT 4
#define ADAS_CURVATURE_HARD_RIGHT 5
#define ADAS_ANALYSIS_OVERFLOW 1  /* frame flags: the detector frame reported a capacity overflow (adas_yolo_counts.flags bit0) */
#define ADAS_ANALYSIS_NONFINITE 2 /* the frame's curvature was not finite */
#define ADAS_ANALYSIS_TRUNCATED 4 /* more survivors than max_points: the rest was not read */
typedef struct {                  /* one stream's TaskConditions (taskConditions.py:90-101) */
    int32_t collision_msg, offset_msg, curvature_msg;  /* ADAS_COLLISION_* / ADAS_OFFSET_* / ADAS_CURVATURE_* */
    int32_t toggle_status, transform_status;           /* ADAS_BIRDVIEW_* (NONE = Python's None) */
    int32_t oscillator[2];                             /* toggle_oscillator_status */
    int32_t counter_offset, counter_curvae, counter_birdview; /* toggle_status_counter */
    int32_t n_collision, n_offset, n_curvature;        /* lengths of the three windows */
    int32_t n_nonfinite;                               /* frames whose curvature was not finite */
    double collision_record[5], offset_record[5];      /* the windows, oldest entry first */
    double curvature_record[10];
    int32_t direction_record[10];                      /* direction (adas_lane_geometry_result.direction) of each curvature entry */
} adas_analysis_state;
typedef struct {                  /* what one frame hands TaskConditions */
    int32_t has_point;            /* calcCollisionPoint returned a point ... */
    int32_t area;                 /* lane_info.area_status */
    int32_t has_offset;           /* vehicle_offset is not None */
    int32_t has_curvature;        /* vehicle_curvature is not None */
    int32_t direction;            /* 0: vehicle_direction is None, 1 "L", 2 "R", 3 "F" */
    int32_t reserved;
    double distance;              /* ... and its metres */
    double offset, curvature;
} adas_analysis_input;
typedef struct {                  /* one frame of the last run */
    int32_t n_points;             /* distance points (adas_analysis_fetch_points) */
    int32_t has_collision;        /* 0: calcCollisionPoint is None */
    int32_t collision_x, collision_y;
    double collision_d;
    int32_t collision_index;      /* the point's index among the frame's distance points, -1: none */
    int32_t collision_msg, offset_msg, curvature_msg;  /* after the frame's three updates */
    int32_t toggle_status, transform_status;           /* after the updates, before the next frame's CheckStatus() */
    int32_t oscillator[2];
    int32_t counters[3];          /* Offset, Curvae, BirdViewAngle */
    int32_t check;                /* CheckStatus() for the next frame */
    int32_t request;              /* the word written for it: the new transform_status if check, else ADAS_BIRDVIEW_NONE */
    int32_t flags;                /* ADAS_ANALYSIS_* */
} adas_analysis_frame;
/* The reference's constants; no classes (n_classes 0, h_ref_height NULL), max_points 512, max_poly 1440. */
int adas_analysis_default_params(adas_analysis_params* p);
/* max_frames: frames of one run the per-frame tables hold (n_streams x frames per stream), >= n_streams. */
int adas_analysis_create(const adas_analysis_params* p, int n_streams, int max_frames, adas_analysis** out);
int adas_analysis_destroy(adas_analysis* h);
/* Back to TaskConditions() after its first CheckStatus(); stream = -1: every stream.  Waits for the whole device.  In a pipeline with a
 * bird view (adas_pipeline_attach_analysis) it also queues that stream's "Default" request. */
int adas_analysis_reset(adas_analysis* h, int stream);
/* One launch, one workgroup per stream, on the handles' device arrays: the survivors of adas_yolo_post_device_views, the area polygon
 * and results of adas_lane_geometry_device_views.  Frame b of stream s is frame b * n_streams + s of both; the frames of a stream are
 * walked in temporal order.  bird may be NULL; otherwise each stream's request word is stored into that handle's pending table, where
 * its next adas_birdview_run consumes it (order the two launches on one stream, or by events).  A plain launch: capturable. */
int adas_analysis_run(adas_analysis* h, adas_yolo_post* post, adas_lane_geometry* geometry, adas_birdview* bird, int n_streams, int n_frames,
                      void* stream);
/* The same kernel on raw device arrays: d_xyxy [frames][det_stride][4] fp64 of the int-truncated corners, d_cls [frames][det_stride],
 * d_counts [frames][4] laid out as the adas_yolo_counts record: n_keep survivors are read, flags bit0 is reported; d_poly [frames][poly_cap][2] with
 * d_poly_counts [frames]; one adas_lane_geometry_result per frame (area_status, direction, curvature and offset are read); d_request
 * [n_streams] may be NULL. */
int adas_analysis_run_arrays(adas_analysis* h, const double* d_xyxy, const int32_t* d_cls, const int32_t* d_counts, int det_stride,
                             const int32_t* d_poly, int poly_cap, const int32_t* d_poly_counts, const adas_lane_geometry_result* d_geometry,
                             int32_t* d_request, int n_streams, int n_frames, void* stream);
/* The state machine alone, for replays and callers with their own geometry: h_inputs [n_streams * n_frames] (host), frame b of stream s at
 * b * n_streams + s.  Copied on `stream` ahead of the launch from the caller's memory: not capturable. */
int adas_analysis_run_inputs(adas_analysis* h, const adas_analysis_input* h_inputs, int n_streams, int n_frames, void* stream);
/* The live state of one stream.  Synchronises with the last run's stream. */
int adas_analysis_fetch_stream(adas_analysis* h, int stream, adas_analysis_state* state);
/* Row `frame` of the last run.  Synchronises. */
int adas_analysis_fetch_frame(adas_analysis* h, int frame, adas_analysis_frame* out);
/* The first n distance points of that frame in survivor order: xy [n][2] (x centre, y bottom), d [n] metres; either may be NULL.
 * ADAS_ERR_INVALID after adas_analysis_run_inputs (no points). */
int adas_analysis_fetch_points(adas_analysis* h, int frame, int32_t* xy, double* d, int n);

/* -----------------------------------------------------------------------------------
 * Lane overlay: the part of the reference's Draw* block (demo.py:300-305) that needs nothing but pixels, on frames that already sit
 * in HBM -- UltrafastLaneDetectorV2.DrawDetectedOnFrame / .DrawAreaOnFrame (ultrafastLaneDetectorV2.py:196-218, the same in v1), the
 * discs of SingleCamDistanceMeasure.DrawDetectedOnFrame (distanceMeasure.py:98) and PerspectiveTransformation.DrawDetectedOnBirdView
 * (perspectiveTransformation.py:217-226): two whole-frame cv2.addWeighted passes, a cv2.fillPoly and filled cv2.circles.
 * Text (putText / getTextSize) is adas_overlay_run_text below, from caller-supplied glyph atlases, with a mask of its own; the UI panels are adas_overlay_run_panels below, with a mask of their own; the boxes of the detector and the tracker are the object layer below, the
 * tracker's trajectories and direction marks (thick circles, arrowedLine) the trajectories stage below that.
 * The pixel rules are modelled on OpenCV 4.5's drawing.cpp / arithm and defined in csrc/overlay_core.h (restated in NumPy,
 * tests/overlay_ref.py); parity with a real cv2 build is UNPINNED, and lines are not clipped before they are walked (OpenCV clips the
 * segment first and restarts the error term).  Per frame f, S0 = the source frame:
 *   1 LANES     lanes 0..3 in order, each point a disc of lane_radius in lane_colors[lane] -- offset_color for lane 1 when the frame's
 *               offset type is RIGHT and for lane 2 when it is LEFT; the last disc over a pixel wins; S1 = blend(colour, lane_alpha, S0)
 *               on disc pixels.  Every decoded point is drawn, detected lane or not.
 *   2 AREA      if area_status and the polygon is not empty: S2 = blend(S1, area_alpha, area colour) on the polygon (edges + even-odd
 *               interior).  A vertex with |x| or |y| > 32767 skips the frame's fill and sets ADAS_OVERLAY_POLY_RANGE in its flags.
 *   3 DISTANCE  a disc of distance_radius in distance_color, written, at every distance point (needs an analysis handle).
 *   4 BIRD      on the bird-view image, in place: discs of bird_radius at the geometry's bird points, lane order and colours of 1, written.
 * With an analysis handle the offset type and the area colour (collision_colors[collision_msg]) are the frame's row after its three
 * updates; without one the offset type is UNKNOWN and the colour is area_color.  The frame goes to a buffer of its own
 * (frame_show = frame.copy()); every output byte depends on the same input byte and geometry only, so dst == src is legal.
 * Three launches for the frame (coverage, one streaming pass with 16-byte accesses, coverage clean-up; four with the object layer, two
 * more with the trajectories stage), two for the bird view; all plain:
 * capturable.  Nothing is capped: lanes hold at most ADAS_UFLD_MAX_POINTS points, polygons and distance points as many as their sources.
 *
 * The object layer: two more stages, off unless asked for, drawn between AREA and DISTANCE in the reference's order (demo.py:299-305).
 *   16 DETECTIONS  YoloDetector / EfficientdetDetector.DrawDetectedOnFrame's boxes (yoloDetector.py:170-191): per survivor, in _object_info
 *               order, ObjectDetectBase.cornerRect (ObjectDetector/core.py:94-113) on RectInfo.tolist() in the class colour -- the outline
 *               (rt = 1) and eight corner arms (t = 5) of length max(1, int(min(ymax - ymin, xmax - xmin) * 0.2)), written.
 *   32 TRACKS   the box part of BYTETracker.DrawTrackedOnFrame (byteTracker.py:202-215, plot_bbox, ObjectTracker/core.py:226-245): every
 *               track of tracked_stracks, in list order, that is activated and has tlwh[2] * tlwh[3] > min_box_area: tlwh.astype(int),
 *               clamped to the image (x1 = max(0, tx), x2 = min(W, tx + tw), the same in y), cv2.rectangle((x1, y1), (x2, y2), thickness 2)
 *               written, then addWeighted(region, 0.6, colour, 0.4, 1.0) on columns x1 .. x2 - 1, rows y1 .. y2 - 1.  One divergence: with
 *               x2 <= x1 or y2 <= y1 nothing is tinted (the reference slices from the end, or raises on the empty crop).
 * A class id outside the colour table is the reference's 'unknown': black.  Where boxes overlap the result is the sequential fold of the
 * reference's calls; the distance discs still lie over everything.  The pixel rules are D6-D9 of csrc/overlay_core.h (a thick axis-aligned
 * segment is a body plus two end discs; modelled on OpenCV 4.5's ThickLine, parity UNPINNED).  NOT drawn: text, the label's background
 * rectangle, key points, DrawTransformFrontalViewArea's slanted thick lines.  One more launch (the boxes' records) when one
 * of the two stages is on, none when both are off; nothing is capped below the sources' capacities (max_candidates per frame, max_tracks
 * per stream).
 *
 * The trajectories stage: what the reference's demo actually draws for a track -- DrawTrackedOnFrame(frame_show, False) (demo.py:304:
 * show_box = False, show_traject = True).  Off unless asked for; bit 128 (64 stays an unknown stage bit).
 *  128 TRAJECTORIES  per track of tracked_stracks, in list order, that is activated and has tlwh[2] * tlwh[3] > min_box_area (the gate and the
 *               min_box_area of TRACKS): plot_trajectories' circles (ObjectTracker/core.py:188-197) -- with more than one box in the
 *               trajectory, box i (oldest first) a circle at (int((x1 + x2) / 2), int(y2)) of radius int(sqrt(i + 1) * 0.5) and thickness
 *               int(sqrt(i + 1) * 1.2) in the class colour -- then plot_directions' indicator (core.py:132-171) from the boxes at least 10
 *               pixels inside the frame (strack.py:145-149): with n < 5 direction vectors the lock-on rectangle (thickness 2, class colour
 *               minus 10 per channel, saturated), else the shadowed arrow along the median direction (three arrowedLine calls:
 *               (100,100,100) t 5 tip 0.3 shifted by (-2, +2), white t 2 tip 0.3 - 0.1 ending one pixel short, white t 3 tip 0.3).
 * In the fold a track's circles and indicator come behind its own TRACKS outline and tint and ahead of the next track's; every primitive
 * writes its colour; the distance discs still lie over everything.  The arithmetic and the pixel rules D10-D12 (thick circle, thick segment
 * of any slope, arrow; modelled on OpenCV 4.5's EllipseEx / ThickLine / arrowedLine, the arrow's tips without trigonometry, parity
 * UNPINNED) are csrc/overlay_track_core.h.  A segment endpoint beyond +-32767 skips that primitive and sets ADAS_OVERLAY_TRACK_RANGE.
 * Colours are the TRACKS class colours.  NOT drawn: the 'ID: n' text and the label.  Two more launches when the stage is on (the tracks'
 * primitives; behind the streaming pass one pass per band of rows that lists the primitives meeting the band, builds their coverage in
 * LDS and writes the covered pixels), none when it is off: the other kernels are then the ones they were.  At most 30 circles + 9 segments per track, max_tracks tracks per stream: nothing is capped, nothing allocates at run time once
 * the first run (or adas_pipeline_set_overlay_stages) has sized the tables.
 * ----------------------------------------------------------------------------------- */
typedef struct adas_overlay adas_overlay;
typedef struct {
    int32_t src_h, src_w;      /* frames: [frames][src_h][src_w][3] u8 BGR; the warp's limits (1..4320 rows, 1..16384 columns) */
    int32_t bird_h, bird_w;    /* the bird-view image; 0, 0: no bird view */
    int32_t lane_radius, distance_radius, bird_radius; /* 3, 4, 10; each 0..64 */
    int32_t reserved;
    double lane_alpha, area_alpha;  /* 0.3, 0.85 */
    uint8_t lane_colors[4][3];      /* (255,0,0), (46,139,87), (50,205,50), (0,255,255): written to channels 0, 1, 2 as given */
    uint8_t offset_color[3];        /* (0,0,255) */
    uint8_t area_color[3];          /* DrawAreaOnFrame's default (255,191,0) */
    uint8_t collision_colors[4][3]; /* CollisionDict (demo.py:33-38) by ADAS_COLLISION_*: (0,255,255), (0,255,0), (0,102,255), (0,0,255) */
    uint8_t distance_color[3];      /* (255,255,255) */
    uint8_t pad[7];
} adas_overlay_params;
#define ADAS_OVERLAY_LANES 1
#define ADAS_OVERLAY_AREA 2
#define ADAS_OVERLAY_DISTANCE 4
#define ADAS_OVERLAY_BIRD 8
/* Every run entry point below is a stage mask over one path: adas_overlay_run and _run_arrays accept bits 1..8 (mask 15), _run_objects and
 * _run_arrays_objects also 16 and 32 (mask 63), _run_trajectories, _run_arrays_trajectories and adas_pipeline_set_overlay_stages also 128.
 * A bit outside an entry's mask is ADAS_ERR_INVALID ("<entry>: unknown stage bits"); inside it the entries draw the same bytes. */
#define ADAS_OVERLAY_DETECTIONS 16 /* the masks 63 and 63 | 128 */
#define ADAS_OVERLAY_TRACKS 32
#define ADAS_OVERLAY_TRAJECTORIES 128 /* the mask 63 | 128 only; 64 is no stage */
#define ADAS_OVERLAY_POLY_RANGE 1 /* frame flags: a polygon vertex outside +-32767, the frame's fill was skipped */
#define ADAS_OVERLAY_TRACK_RANGE 2 /* a segment of a track's indicator had an endpoint outside +-32767 and was skipped */
/* The reference's radii, alphas and colours; the four sizes are 0. */
int adas_overlay_default_params(adas_overlay_params* p);
/* max_batch frames per run.  Allocates the coverage planes (src_h x src_w / 8 bytes per frame, plus a detail plane of src_h x src_w
 * bytes that is read only where something is drawn; the same for the bird view). */
int adas_overlay_create(const adas_overlay_params* p, int max_batch, adas_overlay** out);
int adas_overlay_destroy(adas_overlay* h);
/* Radii, alphas and colours of `p` replace the handle's (its sizes are ignored); takes effect with the next run, and a captured
 * pipeline step is re-captured. */
int adas_overlay_set_style(adas_overlay* h, const adas_overlay_params* p);
/* Frames [0, n_streams * n_frames) of d_src_bgr -> d_dst_bgr (NULL: the handle's own buffer; d_src_bgr itself: in place) with the stages
 * of `stages` drawn from the handles' device arrays; frame b of stream s is frame b * n_streams + s of every handle.  LANES needs
 * `decode` (4 lanes: a decoder with num_lanes != 4 is ADAS_ERR_INVALID), AREA and BIRD need `geometry`, DISTANCE needs `analysis`,
 * BIRD needs d_bird_bgr ([frames][bird_h][bird_w][3], drawn in place).  With stages & 7 == 0 no frame is written.  Asynchronous. */
int adas_overlay_run(adas_overlay* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, const adas_ufld_decode* decode, adas_lane_geometry* geometry,
                     adas_analysis* analysis, uint8_t* d_bird_bgr, int stages, int n_streams, int n_frames, void* stream);
/* The same kernels on raw device arrays, any of which may be NULL with its stage off: d_lane_points [frames][4][ADAS_UFLD_MAX_POINTS][2]
 * int32 (x, y) + d_lane_counts [frames][4]; d_poly [frames][poly_cap][2] + d_poly_counts [frames] + d_area_status [frames];
 * d_offset_type [frames] (ADAS_OFFSET_*; NULL: UNKNOWN); d_area_bgr [frames][3] u8 (NULL: area_color); d_dist_points [frames][dist_cap][2]
 * + d_dist_counts [frames]; d_bird_points [frames][4][ADAS_UFLD_MAX_POINTS][2] + d_bird_counts [frames][4]. */
int adas_overlay_run_arrays(adas_overlay* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, const int32_t* d_lane_points, const int32_t* d_lane_counts,
                            const int32_t* d_poly, int poly_cap, const int32_t* d_poly_counts, const int32_t* d_area_status,
                            const int32_t* d_offset_type, const uint8_t* d_area_bgr, const int32_t* d_dist_points, int dist_cap,
                            const int32_t* d_dist_counts, const int32_t* d_bird_points, const int32_t* d_bird_counts, uint8_t* d_bird_bgr, int stages,
                            int n_frames, void* stream);
/* The object layer's run-time style; the tint's weights (0.6, 0.4, + 1.0) are plot_bbox's and fixed. */
typedef struct {
    double min_box_area;         /* BYTETracker.min_box_area, 10: a track is drawn when tlwh[2] * tlwh[3] > min_box_area */
    int32_t det_rect_thickness;  /* cornerRect's rt, 1 */
    int32_t det_arm_thickness;   /* cornerRect's t, 5 */
    int32_t track_thickness;     /* plot_bbox's rectangle, 2; each thickness 1 .. 127 */
    int32_t reserved;
} adas_overlay_object_style;
int adas_overlay_default_object_style(adas_overlay_object_style* p);
/* Takes effect with the next run; a captured pipeline step is re-captured. */
int adas_overlay_set_object_style(adas_overlay* h, const adas_overlay_object_style* p);
/* The class colours of one stage (which: ADAS_OVERLAY_DETECTIONS -- colors_dict by class id, yoloDetector.py:93-94 -- or ADAS_OVERLAY_TRACKS --
 * class_colors, ObjectTracker/core.py:83-93), n BGR triples written to channels 0, 1, 2 as given.  With no table set (or n = 0) every
 * object is 'unknown', black.  Takes effect with the next run; a captured pipeline step is re-captured.  Waits for the device. */
int adas_overlay_set_class_colors(adas_overlay* h, int which, const uint8_t (*bgr)[3], int n);
/* adas_overlay_run plus the two stages of the object layer: DETECTIONS reads `post`'s survivors (frame index as for the other handles),
 * TRACKS reads `tracker`'s live table, stream s for frame s -- the table holds the last frame only, so TRACKS needs n_frames == 1.  A stage
 * without its handle is ADAS_ERR_INVALID, by name.  post / tracker may be NULL with their stages off. */
int adas_overlay_run_objects(adas_overlay* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, const adas_ufld_decode* decode, adas_lane_geometry* geometry,
                             adas_analysis* analysis, adas_yolo_post* post, struct adas_bytetrack* tracker, uint8_t* d_bird_bgr, int stages, int n_streams,
                             int n_frames, void* stream);
/* adas_overlay_run_arrays plus: d_det_xyxy [frames][det_cap][4] int32 (xmin, ymin, xmax, ymax) + d_det_cls [frames][det_cap] + d_det_counts
 * [frames]; d_trk_tlwh [frames][trk_cap][4] fp64 + d_trk_cls [frames][trk_cap] + d_trk_counts [frames], rows already filtered to activated
 * tracked tracks in list order -- the area gate is applied on the device. */
int adas_overlay_run_arrays_objects(adas_overlay* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, const int32_t* d_lane_points,
                                    const int32_t* d_lane_counts, const int32_t* d_poly, int poly_cap, const int32_t* d_poly_counts,
                                    const int32_t* d_area_status, const int32_t* d_offset_type, const uint8_t* d_area_bgr, const int32_t* d_dist_points,
                                    int dist_cap, const int32_t* d_dist_counts, const int32_t* d_bird_points, const int32_t* d_bird_counts,
                                    uint8_t* d_bird_bgr, const int32_t* d_det_xyxy, int det_cap, const int32_t* d_det_cls, const int32_t* d_det_counts,
                                    const double* d_trk_tlwh, int trk_cap, const int32_t* d_trk_cls, const int32_t* d_trk_counts, int stages,
                                    int n_frames, void* stream);
/* adas_overlay_run_objects plus the trajectories stage, which reads `tracker`'s live state: the message rows for the order, tlwh, class and
 * is_activated, and each row's trajectory ring through the table slot the row names.  Like TRACKS it needs n_frames == 1 and a tracker
 * handle (ADAS_ERR_INVALID otherwise, by name). */
int adas_overlay_run_trajectories(adas_overlay* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, const adas_ufld_decode* decode,
                                  adas_lane_geometry* geometry, adas_analysis* analysis, adas_yolo_post* post, struct adas_bytetrack* tracker,
                                  uint8_t* d_bird_bgr, int stages, int n_streams, int n_frames, void* stream);
/* The arguments of adas_overlay_run_arrays_objects as one struct, plus the trajectories of the rows of d_trk_tlwh: d_traj_tlbr
 * [frames][trk_cap][ADAS_TRAJECTORY_LEN][4] fp64 (x1, y1, x2, y2), oldest first, and d_traj_len [frames][trk_cap], 0 .. 30. */
typedef struct {
    const uint8_t* d_src_bgr;
    uint8_t* d_dst_bgr;
    const int32_t *d_lane_points, *d_lane_counts;
    const int32_t *d_poly, *d_poly_counts, *d_area_status, *d_offset_type;
    const uint8_t* d_area_bgr;
    const int32_t *d_dist_points, *d_dist_counts;
    const int32_t *d_bird_points, *d_bird_counts;
    uint8_t* d_bird_bgr;
    const int32_t *d_det_xyxy, *d_det_cls, *d_det_counts;
    const double* d_trk_tlwh;
    const int32_t *d_trk_cls, *d_trk_counts;
    const double* d_traj_tlbr;
    const int32_t* d_traj_len;
    void* stream;
    int32_t poly_cap, dist_cap, det_cap, trk_cap;
    int32_t stages, n_frames;
} adas_overlay_arrays;
/* adas_overlay_run_arrays_objects plus the trajectories stage (TRAJECTORIES needs the four track arrays and the two trajectory arrays). */
int adas_overlay_run_arrays_trajectories(adas_overlay* h, const adas_overlay_arrays* a);
/* The primitives the device built for frame `frame` of the last run with the trajectories stage, in drawing order: per track row its
 * circles, then its rectangle or its three arrows.  Up to max_marks are stored, *n_marks is their total.  Synchronises. */
#define ADAS_TRACK_MARK_CIRCLE 1 /* centre (x1, y1), radius, thickness */
#define ADAS_TRACK_MARK_RECT 2   /* cv2.rectangle((x1, y1), (x2, y2), thickness) */
#define ADAS_TRACK_MARK_ARROW 3  /* cv2.arrowedLine((x1, y1), (x2, y2), thickness); tip: the two tip points (x, y), (x, y) */
typedef struct {
    int32_t kind, track;         /* ADAS_TRACK_MARK_*; the track's row */
    int32_t x1, y1, x2, y2;
    int32_t radius, thickness;
    int32_t tip[4];
    uint8_t color[3];            /* channels 0, 1, 2 */
    uint8_t skipped;             /* bit j: segment j of the mark was out of range and not drawn */
} adas_overlay_track_mark;
int adas_overlay_fetch_track_marks(adas_overlay* h, int frame, adas_overlay_track_mark* marks, int max_marks, int32_t* n_marks);
/* Frame `frame` of the handle's own buffer -> h_bgr [src_h][src_w][3], after the last run's stream has drained.  A frame that no run
 * has written is ADAS_ERR_INVALID. */
int adas_overlay_fetch(adas_overlay* h, int frame, uint8_t* h_bgr);
int adas_overlay_device_view(adas_overlay* h, const uint8_t** d_bgr);
/* ADAS_OVERLAY_* flags of frame `frame` of the last run.  Synchronises. */
int adas_overlay_fetch_flags(adas_overlay* h, int frame, int32_t* flags);

/* The bird view's readouts: what PerspectiveTransformation.calcCurveAndOffset draws on the bird-view image it is handed
 * (perspectiveTransformation.py:205-213) -- the white arrow at the vehicle's position, the grey arrow at the image centre and the red
 * strings 'Offset: %.1f m' and 'R : %.1f m' -- under the bird stage's discs (demo.py:292 before :299).  Stage bit 256, accepted only by
 * the two entries below and by adas_pipeline_set_overlay_readouts: every other entry keeps its mask and refuses it ("unknown stage bits").
 * The rules R0-R6 are csrc/overlay_readout_core.h (D11 / D12 segments and arrows, T1-T4 numbers and glyphs; the definitions are the
 * authority, parity with a real cv2 build UNPINNED).  Two stated divergences: a frame is drawn only when its direction is not NONE (the
 * reference draws whenever both ego lanes are non-empty; the geometry kernel fits only with 3 points each and bird_h > 719), and the
 * strings are the font of `slot` (adas_overlay_set_font) magnified by the integer `zoom` with nearest-neighbour glyph pixels (a Hershey face
 * at fontScale 3 is taller than a 64-row cell: the caller renders its atlas at fontScale 3 / zoom).  READOUTS needs BIRD's inputs -- a
 * handle with a bird size and d_bird_bgr -- and draws in place there, ahead of the discs; without BIRD it draws arrows and strings only.
 * Two launches (a layout of one wave per frame, a draw that touches only the 16-byte pieces inside the record's boxes), none with the
 * stage off. */
#define ADAS_OVERLAY_READOUTS 256
#define ADAS_OVERLAY_READOUT_RANGE 1 /* readout flags of a frame: an arrow segment beyond +-32767 or a value with |x| >= 2^30 was skipped */
typedef struct {
    int32_t slot, zoom;                 /* the font slot, 10; the magnification, 2 (1 .. 4) */
    int32_t offset_x, offset_y;         /* the origin of 'Offset: ...', (20, 80) */
    int32_t radius_x, radius_y;         /* the origin of 'R : ...', (20, 180) */
    uint8_t text_color[3];              /* (0, 0, 255) */
    uint8_t arrow_a_color[3];           /* the arrow at veh_pos, (255, 255, 255) */
    uint8_t arrow_b_color[3];           /* the arrow at the image centre, (150, 150, 150) */
    uint8_t pad[3];
} adas_overlay_readout_style;
int adas_overlay_default_readout_style(adas_overlay_readout_style* p);
/* Takes effect with the next run; a captured pipeline step is re-captured.  zoom outside 1 .. 4 or a slot outside the table is
 * ADAS_ERR_INVALID.  Allocates the per-frame records on first use: not inside a stream capture. */
int adas_overlay_set_readout_style(adas_overlay* h, const adas_overlay_readout_style* p);
/* adas_overlay_run_trajectories plus the readouts stage, which reads `geometry`'s direction (header word 3), curvature and offset and its
 * veh_pos array.  READOUTS without a bird image, with an empty font slot or without a geometry handle is ADAS_ERR_INVALID, by name. */
int adas_overlay_run_readouts(adas_overlay* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, const adas_ufld_decode* decode,
                              adas_lane_geometry* geometry, adas_analysis* analysis, adas_yolo_post* post, struct adas_bytetrack* tracker,
                              uint8_t* d_bird_bgr, int stages, int n_streams, int n_frames, void* stream);
typedef struct {
    const int32_t* d_direction;         /* [frames]: 0 is NONE, the frame is not drawn */
    const double *d_veh_pos, *d_curvature, *d_offset; /* [frames] each */
} adas_overlay_readout_arrays;
/* adas_overlay_run_arrays_trajectories plus the readouts stage from raw device arrays (r may be NULL with the stage off; with it on all
 * four arrays are needed). */
int adas_overlay_run_arrays_readouts(adas_overlay* h, const adas_overlay_arrays* a, const adas_overlay_readout_arrays* r);
typedef struct {
    int32_t x, y;                       /* the origin */
    int32_t box[4];                     /* x0, y0, x1, y1: every pixel it can touch, inside the bird image, half open; zeros: none */
    int32_t len;                        /* characters of text; 0: not drawn */
    int32_t skipped;                    /* 1: |value| >= 2^30 */
    char text[32];
} adas_overlay_readout_string;
typedef struct {
    int32_t drawn, flags;               /* R0's gate; ADAS_OVERLAY_READOUT_* */
    adas_overlay_track_mark arrows[2];  /* kind ADAS_TRACK_MARK_ARROW, track 0 / 1: at veh_pos, at the centre */
    adas_overlay_readout_string strings[2]; /* the offset, the radius */
} adas_overlay_readout_record;
/* What the device laid out for frame `frame` of the last run with the readouts stage.  Synchronises. */
int adas_overlay_fetch_readout(adas_overlay* h, int frame, adas_overlay_readout_record* rec);

/* The demo's three UI panels on frames that sit in HBM (ControlPanel.DisplayBirdViewPanel / DisplaySignsPanel / DisplayCollisionPanel,
 * demo.py:101-214, painted in that order as at demo.py:307-309), without their putText lines (ADAS_TEXT_PANELS and ADAS_TEXT_LINES of the text block below): the bird-view image
 * resized to W x H = int(src_w * ratio) x int(src_h * ratio) inside a black border in the top right corner; the dimmed, red-framed signs
 * widget in the top left corner with up to two sign sprites; the dimmed, red-framed collision widget below the bird panel with one FCWS
 * sprite.  The pixel and state rules P1-P6 are csrc/overlay_panel_core.h (the signs and collision panels and the bird panel's placement
 * restate the reference's NumPy lines; the resize is the rule of adas_preprocess_*, parity with a real cv2 build UNPINNED).
 * The panels are NOT stage bits of the masks above: they have a mask and calls of their own, in place on frames that have been drawn.
 * Two launches: one lane per stream walks that stream's frames in order and writes a record per frame (the sprites chosen and the
 * curve_status latch, which lives in the handle's device memory, so a replayed graph carries it), then one pass over the rows and column
 * spans of the panels writes every byte at most once with the whole sequence folded in (16-byte accesses; overlapping panels on narrow
 * frames need no second pass).  Both are plain launches: capturable. */
#define ADAS_PANEL_BIRD 1
#define ADAS_PANEL_SIGNS 2
#define ADAS_PANEL_COLLISION 4
#define ADAS_PANEL_SPRITES 9
#define ADAS_PANEL_SPRITE_FCWS_WARNING 0 /* assets/FCWS-warning.png at 100 x 100: mask = alpha */
#define ADAS_PANEL_SPRITE_FCWS_PROMPT 1
#define ADAS_PANEL_SPRITE_FCWS_NORMAL 2
#define ADAS_PANEL_SPRITE_LEFT 3         /* left_turn.png, 200 x 200: alpha */
#define ADAS_PANEL_SPRITE_RIGHT 4
#define ADAS_PANEL_SPRITE_STRAIGHT 5
#define ADAS_PANEL_SPRITE_WARN 6
#define ADAS_PANEL_SPRITE_LTA_LEFT 7     /* LTA-left_lanes.png, 300 x 200: mask = channel 2, as the reference tests [:, :, 2] */
#define ADAS_PANEL_SPRITE_LTA_RIGHT 8
#define ADAS_PANEL_LATCH_NONE 0          /* ControlPanel.curve_status: None / "Left" / "Right" / "Straight" */
#define ADAS_PANEL_LATCH_LEFT 1
#define ADAS_PANEL_LATCH_RIGHT 2
#define ADAS_PANEL_LATCH_STRAIGHT 3
typedef struct {
    double show_ratio;              /* 0.25 */
    int32_t border;                 /* 10: the bird panel's black border; the collision widget starts 2 * border below H */
    int32_t signs_w, signs_h;       /* 400 x 365 */
    int32_t signs_sprite_row;       /* 10: a sign sprite's row offset; its column is signs_w / 2 - sprite_w / 2 */
    int32_t collision_sprite_row;   /* 50: the FCWS sprite's first row is H + 50 */
    int32_t collision_sprite_col;   /* 5: its first column is src_w - W - 5 */
    uint8_t border_color[3];        /* (0, 0, 255) */
    uint8_t reserved;
} adas_overlay_panel_params;
typedef struct {
    const uint8_t* bgra;            /* host, [h][w][4] u8; NULL: an empty sprite, draws nothing */
    int32_t w, h;
} adas_overlay_sprite;
typedef struct {
    int32_t sign[2];                /* ADAS_PANEL_SPRITE_* of the first / second if-chain of DisplaySignsPanel in paint order, -1: none */
    int32_t collision;              /* ADAS_PANEL_SPRITE_FCWS_* or -1 */
    int32_t latch;                  /* ADAS_PANEL_LATCH_* after the frame */
    int32_t offset_type, curvature_type, collision_type; /* as read */
    int32_t reserved;
} adas_overlay_panel_record;
int adas_overlay_default_panel_params(adas_overlay_panel_params* p);
/* Geometry and sprites (copied into one BGRA atlas on the device; the mask channel is fixed by slot).  Checks once that every rectangle
 * and every sprite placement lies wholly inside the frame (e.g. W + collision_sprite_col >= the FCWS sprites' width, H > 2 * border):
 * anything else is ADAS_ERR_INVALID with a message naming the panel -- the reference would clip, wrap to the other edge or raise.
 * Allocates the latches (max_batch of them, all NONE) and the records.  Not inside a stream capture. */
int adas_overlay_set_panels(adas_overlay* h, const adas_overlay_panel_params* p, const adas_overlay_sprite sprites[ADAS_PANEL_SPRITES]);
/* The panels `panels` (ADAS_PANEL_*), in place on d_frames_bgr [n_streams * n_frames][src_h][src_w][3] (any alignment); NULL: the handle's
 * own buffer, what adas_overlay_run just wrote.  Frame b of stream s is frame b * n_streams + s; stream s uses latch s.  SIGNS and
 * COLLISION read `analysis`' frame rows (after its three updates); BIRD reads d_bird_bgr [frames][bird_h][bird_w][3] (after the bird
 * stage's discs) and needs a handle created with a bird size.  ADAS_ERR_INVALID, prefixed with the entry's name: unknown panel bits, a
 * call before adas_overlay_set_panels, n_streams * n_frames > max_batch, a panel without its input. */
int adas_overlay_run_panels(adas_overlay* h, uint8_t* d_frames_bgr, const adas_analysis* analysis, const uint8_t* d_bird_bgr, int panels,
                            int n_streams, int n_frames, void* stream);
/* The same kernels on raw [n_streams * n_frames] int32 arrays (ADAS_OFFSET_* / ADAS_CURVATURE_* / ADAS_COLLISION_*; a value outside its
 * enum is UNKNOWN).  SIGNS needs the first two, COLLISION the third. */
int adas_overlay_run_panels_arrays(adas_overlay* h, uint8_t* d_frames_bgr, const int32_t* d_offset_type, const int32_t* d_curvature_type,
                                   const int32_t* d_collision_type, const uint8_t* d_bird_bgr, int panels, int n_streams, int n_frames,
                                   void* stream);
/* Latch `stream_index` back to NONE; -1: all of them.  Synchronises with the last run. */
int adas_overlay_reset_panels(adas_overlay* h, int stream_index);
/* The record of frame `frame` of the last panel run.  Synchronises. */
int adas_overlay_fetch_panel_record(adas_overlay* h, int frame, adas_overlay_panel_record* rec);

/* The overlay's text on frames that sit in HBM, from glyph atlases the caller supplies: the class label on its filled background
 * (yoloDetector.py:180-191; EfficientDet's variant by the style's offsets), the tracker's "name : id" (ObjectTracker/core.py:235-239) and
 * shadowed "ID: n" (core.py:199-210), the shadowed " 12.34 m" of a distance point (distanceMeasure.py:97-115), the three strings of the
 * panels (demo.py:173-174, 212) and up to ADAS_TEXT_MAX_LINES caller lines (the FPS and inference-time strings are host timings of a
 * per-frame loop: the caller prints them as lines).  The font is DATA, like the panels' sprites: a u8 coverage atlas per slot with the
 * metrics of characters 32..126 -- on a machine with cv2 one putText per glyph renders it (tools/make_font_atlas.py); the repository
 * ships no font and OpenCV's Hershey tables exist nowhere here.  Which strings exist, where they go, their colours, '%.2f' of a distance
 * that only exists in HBM, ids and class names are decided on the device by the rules T1-T7 of csrc/overlay_text_core.h (restated in NumPy,
 * tests/text_ref.py).  Stated divergences: a bitmap font cannot scale, so the two continuously scaled strings pick the slot of a LADDER
 * (a run of consecutive slots) whose declared scale is nearest the reference's fontScale, the smaller on a tie, d == 0 as scale 1; glyphs
 * sit on whole pixels where cv2 strokes sub-pixel polylines; text lies over every stage where the reference lets a later box cover an
 * earlier label; parity with a real cv2 build is UNPINNED.
 * Text is NOT a stage bit: it has a mask and calls of its own, in place on frames that have been drawn.  Two launches: a layout kernel
 * (one wave per frame) writes the frame's item list -- rectangles and glyph runs with their clipped boxes, in paint order -- its count and
 * flags; a draw kernel folds the items over the aligned 16-byte pieces their boxes cover, in order, each byte written by one lane with the
 * whole sequence applied.  Both are plain launches: capturable. */
#define ADAS_TEXT_FONTS 16
#define ADAS_TEXT_MAX_LINES 8
#define ADAS_TEXT_DETECTIONS 1  /* the mask of adas_overlay_run_text*: painted in this order */
#define ADAS_TEXT_TRACKS 2
#define ADAS_TEXT_TRACK_IDS 4
#define ADAS_TEXT_DISTANCE 8
#define ADAS_TEXT_PANELS 16
#define ADAS_TEXT_LINES 32
#define ADAS_OVERLAY_TEXT_RANGE 1    /* text flags of a frame: a number with |x| >= 2^30, or an origin beyond +-2^30: the item was skipped */
#define ADAS_OVERLAY_TEXT_OVERFLOW 2 /* more than max_text_items items: the rest, in paint order, were dropped */
#define ADAS_TEXT_ITEM_RECT 1
#define ADAS_TEXT_ITEM_RUN 2
typedef struct {
    const uint8_t* atlas;        /* host, [cell_h][atlas_w] u8 coverage (0: nothing, 255: the colour); copied to the device */
    int32_t atlas_w, cell_h;     /* cell_h 1 .. 64 */
    int32_t baseline_row;        /* the cell's row that sits on the text origin's y */
    int32_t size_h;              /* what getTextSize returns as the height */
    int32_t size_w_extra;        /* 16.16: getTextSize's width is (sum of advances + size_w_extra + 0x8000) >> 16 (the thickness term) */
    int32_t reserved;
    double scale;                /* the declared fontScale: used by ladders only */
    int32_t glyph_x[95];         /* characters 32 .. 126: the glyph's first atlas column */
    int32_t glyph_w[95];         /* its columns, 0 .. 64 (0: draws nothing, e.g. the space) */
    int32_t bearing_x[95];       /* first column relative to the pen, may be negative */
    int32_t advance[95];         /* 16.16 */
} adas_overlay_font;
typedef struct {
    double show_ratio;           /* 0.25: the FCWS string starts at column src_w - int(src_w * show_ratio) + fcws_dx */
    double min_box_area;         /* 10: the gate of the tracks and their ids, as adas_overlay_object_style's */
    int32_t max_text_items;      /* 256 per frame, 1 .. 1024: a rectangle is one item, a shadowed string two */
    int32_t det_size_slot, det_label_slot; /* 0, 1: the font the label's box is sized by (face 0, tl / 3) and the one that is drawn */
    int32_t det_label_dx, det_label_dy;    /* (2, -7); EfficientDet's variant: (0, -5) */
    int32_t det_box_pad;         /* 3: the box is (xmin, ymin) .. (xmin + tw, ymin - th - 3) */
    int32_t track_slot, track_dy; /* 2, -10 */
    int32_t id_first, id_count, id_shadow_first, id_shadow_count; /* ladders: 3, 1 and 4, 1 */
    int32_t dist_size_first, dist_size_count, dist_first, dist_count, dist_shadow_first, dist_shadow_count; /* 5, 1; 6, 1; 7, 1 */
    int32_t shadow_dx, shadow_dy; /* (2, 2) */
    int32_t ldws_slot, lkas_slot, fcws_slot; /* 8, 8, 9 */
    int32_t ldws_x, ldws_y, lkas_x, lkas_y, fcws_dx, fcws_y; /* (10, 240), (10, 280), (100, 240) */
    int32_t id_shadow_sub;       /* 30: the id's shadow is the class colour minus 30 per channel, saturated at 0 */
    uint8_t label_color[3], dist_color[3], dist_shadow_color[3]; /* white, white, (150, 150, 150) */
    uint8_t offset_colors[4][3], curvature_colors[6][3], collision_colors[4][3]; /* OffsetDict, CurvatureDict, CollisionDict (demo.py:33-54) */
    uint8_t pad[5];
} adas_overlay_text_style;
typedef struct {
    int32_t kind;                /* ADAS_TEXT_ITEM_* */
    int32_t source;              /* the ADAS_TEXT_* bit it belongs to */
    int32_t x, y;                /* a run's origin (putText's org); a rectangle's first corner */
    int32_t x1, y1;              /* a rectangle's second corner, inclusive, in either order as cv2.rectangle takes them; 0 for a run */
    int32_t bx0, by0, bx1, by1;  /* every pixel the item can touch, clipped to the frame, half open; all 0: none */
    int32_t slot;                /* a run's font slot; -1 for a rectangle */
    uint8_t color[3];            /* channels 0, 1, 2 */
    uint8_t len;
    char text[48];
} adas_overlay_text_item;
typedef struct {
    int32_t x, y, slot;
    uint8_t color[3];
    uint8_t len;                 /* at most 47 */
    char text[48];
} adas_overlay_text_line;
/* What the layout reads, as raw device arrays, frame q of n_streams * n_frames: survivors d_det_xyxy [q][det_cap][4] + d_det_cls + d_det_counts
 * as adas_overlay_run_arrays_objects takes them; tracks d_trk_tlwh [q][trk_cap][4] fp64 + d_trk_cls + d_trk_ids + d_trk_counts, with the
 * newest box of each row's trajectory d_trk_last_tlbr [q][trk_cap][4] fp64 and the trajectory's length d_traj_len (an id is drawn when it
 * exceeds 1); distance points d_dist_points [q][dist_cap][2] with d_dist_d [q][dist_cap] fp64 and d_dist_counts; the three message types
 * [q].  Arrays of kinds that are off may be NULL. */
typedef struct {
    const int32_t *d_det_xyxy, *d_det_cls, *d_det_counts;
    const double* d_trk_tlwh;
    const int32_t *d_trk_cls, *d_trk_ids, *d_trk_counts;
    const double* d_trk_last_tlbr;
    const int32_t* d_traj_len;
    const int32_t* d_dist_points;
    const double* d_dist_d;
    const int32_t* d_dist_counts;
    const int32_t *d_offset_type, *d_curvature_type, *d_collision_type;
    int32_t det_cap, trk_cap, dist_cap, reserved;
} adas_overlay_text_arrays;
int adas_overlay_default_text_style(adas_overlay_text_style* p);
/* Takes effect with the next run; a captured pipeline step is re-captured.  Waits for the device. */
int adas_overlay_set_text_style(adas_overlay* h, const adas_overlay_text_style* p);
/* Font `slot` (0 .. ADAS_TEXT_FONTS - 1), validated once: glyph rectangles inside the atlas, cell_h <= 64, glyph_w <= 64; anything else is
 * ADAS_ERR_INVALID with a message naming the field.  A character outside 32..126 draws as '?'.  Waits for the device. */
int adas_overlay_set_font(adas_overlay* h, int slot, const adas_overlay_font* font);
/* Class names by id for which = ADAS_OVERLAY_DETECTIONS or ADAS_OVERLAY_TRACKS, at most 31 bytes each (longer: ADAS_ERR_INVALID).  An id
 * outside the table prints 'unknown' (in black on the detections' label box), as get_nms_results does.  The colours are the class colours of
 * adas_overlay_set_class_colors. */
int adas_overlay_set_text_labels(adas_overlay* h, int which, const char* const* names, int n);
/* Up to ADAS_TEXT_MAX_LINES caller strings, drawn last on every frame (ADAS_TEXT_LINES). */
int adas_overlay_set_text_lines(adas_overlay* h, const adas_overlay_text_line* lines, int n);
/* The text `mask` (ADAS_TEXT_*) in place on d_frames_bgr [n_streams * n_frames][src_h][src_w][3] (any alignment); NULL: the handle's own
 * buffer.  ADAS_ERR_INVALID, prefixed with the entry's name: unknown mask bits, a run before any font is set, a bit whose font slot is
 * empty, a bit whose source is missing, n_streams * n_frames > max_batch. */
int adas_overlay_run_text_arrays(adas_overlay* h, uint8_t* d_frames_bgr, const adas_overlay_text_arrays* a, int mask, int n_streams, int n_frames,
                                 void* stream);
/* The same kernels on the handles' device arrays, where they already sit: DETECTIONS reads `post`'s survivors; TRACKS and TRACK_IDS read
 * `tracker`'s live table (activated tracked rows over the area gate; the id's origin comes from the newest box of the row's trajectory ring)
 * -- the table holds the last frame only, so they need n_frames == 1; DISTANCE reads `analysis`' distance points and their metres, PANELS
 * its frame rows after the three updates.  A bit whose handle is NULL is ADAS_ERR_INVALID, by name; a handle whose bits are off may be NULL. */
int adas_overlay_run_text(adas_overlay* h, uint8_t* d_frames_bgr, adas_yolo_post* post, struct adas_bytetrack* tracker, const adas_analysis* analysis,
                          int mask, int n_streams, int n_frames, void* stream);
/* The item list of frame `frame` of the last text run, in paint order: up to max_items are stored, *n_items is their number.  Synchronises. */
int adas_overlay_fetch_text_items(adas_overlay* h, int frame, adas_overlay_text_item* items, int max_items, int32_t* n_items);
/* ADAS_OVERLAY_TEXT_* of frame `frame` of the last text run.  Synchronises. */
int adas_overlay_fetch_text_flags(adas_overlay* h, int frame, int32_t* flags);

/* ===================================================================================
 * Baseline JPEG on the device: what the demo's loop ends with, vout.write(frame_show) (demo.py:314), as one compressed stream per
 * frame -- a finished frame leaves the device as a few hundred KB instead of width x height x 3 bytes (adas_overlay_fetch).
 * Baseline sequential DCT (SOF0), 8 bit, 4:2:0, the Annex K tables of ITU-T T.81 scaled by a quality of 1..100, one restart interval per
 * MCU row, no APP0; any width and height in 1..65535 (edges are replicated).  The rules J1-J9 are csrc/jpeg_core.h, all of them integer
 * arithmetic.  Three plain launches (transform and quantise per block; entropy-code per restart segment; lay the segments out per
 * frame): capturable, no allocation and no host synchronisation in adas_jpeg_run.
 * =================================================================================== */
typedef struct adas_jpeg adas_jpeg;
#define ADAS_JPEG_OVERFLOW 1      /* flags: the frame's stream would not fit the capacity; its length is 0 and no byte of it was written */
#define ADAS_JPEG_SRC_OVERLAY 0   /* adas_pipeline_attach_jpeg: the attached overlay's own buffer, behind its stages and panels */
#define ADAS_JPEG_SRC_FRAMES 1    /* the u8 frames adas_pipeline_step_frames* was given */
typedef struct {
    int32_t width, height;
    int32_t quality;              /* 1..100 (90) */
    int32_t reserved;
    int64_t capacity;             /* bytes per frame of the handle's stream buffer; 0: width * height * 3 */
} adas_jpeg_params;
int adas_jpeg_default_params(adas_jpeg_params* p);
/* The most bytes a width x height frame can take at any quality: header + blocks * 416 + markers (0 for a size outside 1..65535). */
int64_t adas_jpeg_bound(int width, int height);
/* ADAS_ERR_INVALID by name: a size outside 1..65535, a quality outside 1..100, max_batch < 1, a capacity below the 611 header bytes.
 * Allocates every table, the level arena, the segment arena (worst case: 416 bytes per block) and max_batch streams of `capacity` bytes. */
int adas_jpeg_create(const adas_jpeg_params* p, int max_batch, adas_jpeg** out);
int adas_jpeg_destroy(adas_jpeg* h);
/* New quantisation tables and header bytes from the next run on, at the old addresses (a captured run picks them up).  Synchronises; not
 * inside a stream capture. */
int adas_jpeg_set_quality(adas_jpeg* h, int quality);
/* d_frames_bgr [batch][height][width][3] u8, starting on any byte -> the handle's streams, lengths and flags.  Every byte below a frame's
 * length is written once, the bytes from there to the capacity are left alone; a frame that would not fit gets length 0 and
 * ADAS_JPEG_OVERFLOW, the other frames are unaffected.  A frame's bytes depend on its pixels, its size and the quality alone. */
int adas_jpeg_run(adas_jpeg* h, const uint8_t* d_frames_bgr, int batch, void* stream);
/* Frame `frame` of the last run -> h_buf, after that run's stream has drained; *n_bytes is its length.  ADAS_ERR_INVALID when h_cap is
 * below the length (*n_bytes is set all the same) or the frame was not part of the last run. */
int adas_jpeg_fetch(adas_jpeg* h, int frame, uint8_t* h_buf, int64_t h_cap, int64_t* n_bytes, int32_t* flags);
int adas_jpeg_fetch_lengths(adas_jpeg* h, int batch, int64_t* n_bytes, int32_t* flags);
/* The streams on the device: frame f at d_streams + f * stride, d_lengths[f] bytes long. */
int adas_jpeg_device_view(adas_jpeg* h, const uint8_t** d_streams, const int64_t** d_lengths, int64_t* stride);

/* ===================================================================================
 * Baseline JPEG decoding on the device: what the demo's loop starts with, cap.read() (demo.py:261), for a camera or file that delivers
 * MJPEG -- a frame crosses the bus as a few hundred KB instead of width x height x 3 bytes and is decoded where the step reads it.
 * Baseline sequential DCT (SOF0), 8 bit, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0, the stream's own tables, any restart interval (a restart
 * segment is the unit of parallelism: a stream without restart markers decodes on one lane).  The rules D1-D9 are csrc/jpegdec_core.h, all
 * of them integer arithmetic.  A memset and five plain launches (header per frame; restart markers per frame; entropy-decode per
 * segment; inverse transform per block; upsample and convert per 16 output bytes): capturable, no allocation and no host
 * synchronisation in adas_jpegdec_run.
 * Stream CONTENT never produces an error code: every frame gets a flag word, and a frame flagged UNSUPPORTED, FORMAT or SIZE has every
 * pixel 0; the other frames of the batch are unaffected.  For any bytes whatever the decoder reads only the words that hold the
 * stream's bytes and writes only its own arenas and the destination frame.
 * =================================================================================== */
typedef struct adas_jpegdec adas_jpegdec;
#define ADAS_JPEGDEC_UNSUPPORTED 1   /* a valid JPEG outside the accepted kind: progressive, 12 bit, four components, other sampling, ... */
#define ADAS_JPEGDEC_FORMAT 2        /* not a JPEG stream, a damaged header, a missing table, a length of 0 or above the capacity */
#define ADAS_JPEGDEC_SIZE 4          /* the stream's width or height differ from the handle's */
#define ADAS_JPEGDEC_CORRUPT 8       /* an error in the entropy data: the blocks from there to the segment's end are zero coefficients */
typedef struct {
    int32_t width, height;
    int32_t reserved[2];
    int64_t capacity;             /* most bytes per stream; 0: adas_jpeg_bound(width, height) */
} adas_jpegdec_params;
int adas_jpegdec_default_params(adas_jpegdec_params* p);
/* ADAS_ERR_INVALID by name: a size outside 1..65535, max_batch < 1, a capacity outside 1..2^31-1.  Allocates every arena, max_batch
 * frames and the two staging buffers of adas_jpegdec_run_host, pinned on the host and mirrored on the device, max_batch x capacity bytes
 * each: with the default capacity (9 MB per 1280x720 stream) that is the handle's largest part, so give the capacity the source needs. */
int adas_jpegdec_create(const adas_jpegdec_params* p, int max_batch, adas_jpegdec** out);
int adas_jpegdec_destroy(adas_jpegdec* h);
/* Streams on the device: frame f at d_streams + f * stride, d_lengths[f] bytes, starting on any byte (adas_jpeg_device_view's triple fits).
 * d_dst_bgr [batch][height][width][3] u8, any alignment; NULL: the handle's own frames.  Every byte of the batch's frames is written,
 * nothing behind them. */
int adas_jpegdec_run(adas_jpegdec* h, const uint8_t* d_streams, const int64_t* d_lengths, int64_t stride, int batch, uint8_t* d_dst_bgr, void* stream);
/* Streams on the host: packed into one of two pinned staging buffers of the handle, copied asynchronously on `stream`, then the run
 * above.  A length above the capacity flags that frame FORMAT and copies nothing of it.  The host bytes are free again on return.  Calls may use
 * different streams: a staging buffer is refilled only behind the run that last read it.  (adas_pipeline_step_jpeg_host shares the two
 * buffers: do not mix it with calls of this entry point on the attached handle.) */
int adas_jpegdec_run_host(adas_jpegdec* h, const uint8_t* const* h_streams, const int64_t* h_lengths, int batch, uint8_t* d_dst_bgr, void* stream);
/* Frame `frame` of the handle's own buffer -> h_bgr [height][width][3], after the last run's stream has drained.  ADAS_ERR_INVALID for a
 * frame the last run did not write there. */
int adas_jpegdec_fetch(adas_jpegdec* h, int frame, uint8_t* h_bgr);
int adas_jpegdec_fetch_flags(adas_jpegdec* h, int batch, int32_t* flags);
int adas_jpegdec_device_view(adas_jpegdec* h, const uint8_t** d_frames_bgr, const int32_t** d_flags);

/* ===================================================================================
 * Uncompressed camera formats into BGR on the device: the other thing cap.read() (demo.py:261) hides.  A UVC camera delivers YUYV, an
 * ISP, a hardware video decoder or `ffmpeg -pix_fmt nv12 / yuv420p` NV12 or I420; the frame crosses the bus as 1.5 or 2 bytes per pixel
 * instead of 3 and is converted where the step reads it.  The rules C1-C7 are csrc/yuv_core.h: chroma by replication, BT.601 limited
 * range in OpenCV's 20-bit integers (ADAS_YUV_MATRIX_VIDEO, what cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420 / _YUY2 / _UYVY) computes) or
 * JFIF full range (ADAS_YUV_MATRIX_FULL, the JPEG decoder's rule D8).  One plain launch: capturable, no allocation and no host
 * synchronisation in adas_yuv_run.
 * =================================================================================== */
typedef struct adas_yuv adas_yuv;
#define ADAS_YUV_NV12 0   /* Y plane, then interleaved U,V pairs (4:2:0) */
#define ADAS_YUV_NV21 1   /* Y plane, then interleaved V,U pairs */
#define ADAS_YUV_I420 2   /* Y plane, U plane, V plane; YV12: swap u_offset and v_offset */
#define ADAS_YUV_YUYV 3   /* packed 4:2:2, bytes Y0 U Y1 V */
#define ADAS_YUV_UYVY 4   /* packed 4:2:2, bytes U Y0 V Y1 */
#define ADAS_YUV_MATRIX_VIDEO 0
#define ADAS_YUV_MATRIX_FULL 1
typedef struct {
    int32_t format, matrix;
    int32_t width, height;        /* width even; height even for the 4:2:0 formats */
    int64_t frame_stride;         /* bytes from one frame of a batch to the next */
    int64_t y_offset, y_pitch;    /* the Y plane (the only plane of a packed format): bytes from the frame's start, bytes from row to row */
    int64_t u_offset, u_pitch;    /* the U plane of I420, the interleaved plane of NV12 / NV21 */
    int64_t v_offset, v_pitch;    /* the V plane of I420 */
} adas_yuv_params;
/* The tight layout of a width x height frame, matrix VIDEO.  Hardware decoders and V4L2 pad rows and plane heights: overwrite the
 * layout fields with what the source reports. */
int adas_yuv_default_params(adas_yuv_params* p, int format, int width, int height);
/* Bytes of one source frame that are read (the end of its last plane); a batch is read up to (batch - 1) * frame_stride + this.  0 for
 * parameters adas_yuv_create would refuse. */
int64_t adas_yuv_frame_bytes(const adas_yuv_params* p);
/* ADAS_ERR_INVALID by name: odd width, odd height for a 4:2:0 format, pitch shorter than a row, plane outside the frame, planes overlap,
 * max_batch < 1.  Allocates max_batch BGR frames; the two staging buffers of adas_yuv_run_host (max_batch x frame_stride bytes each)
 * with its first calls. */
int adas_yuv_create(const adas_yuv_params* p, int max_batch, adas_yuv** out);
int adas_yuv_destroy(adas_yuv* h);
/* Frames on the device, frame f at d_src + f * frame_stride, any alignment (a decoder's surface as it is: nothing is padded or copied).
 * d_dst_bgr [batch][height][width][3] u8, any alignment; NULL: the handle's own frames.  Every byte of the batch's frames is written,
 * nothing behind them.  When width, the pitches, the offsets, frame_stride and both pointers are multiples of 16 every access is 16
 * bytes wide; any other geometry goes byte by byte and gives the same pixels. */
int adas_yuv_run(adas_yuv* h, const uint8_t* d_src, int batch, uint8_t* d_dst_bgr, void* stream);
/* Frames on the host (pinned for an asynchronous copy: adas_host_alloc): copied on `stream` into one of two device buffers of the
 * handle, then the run above.  h_src must stay as it is until the stream has passed the copy.  Calls may use different streams: a
 * buffer is refilled only behind the run that last read it. */
int adas_yuv_run_host(adas_yuv* h, const uint8_t* h_src, int batch, uint8_t* d_dst_bgr, void* stream);
/* Frame `frame` of the handle's own buffer -> h_bgr [height][width][3], after the last run's stream has drained.  ADAS_ERR_INVALID for a
 * frame the last run did not write there. */
int adas_yuv_fetch(adas_yuv* h, int frame, uint8_t* h_bgr);
int adas_yuv_device_view(adas_yuv* h, const uint8_t** d_frames_bgr);

/* ===================================================================================
 * BGR frames into uncompressed video formats on the device: the way out that mirrors the way in above.  What cv2.VideoWriter.write(frame_show)
 * (demo.py:314) does in front of its encoder, for every encoder that is not MJPEG (x264, SVT, `ffmpeg -f rawvideo -pix_fmt yuv420p`, a
 * V4L2 loopback, a hardware encoder on another box): the frame leaves the device as 1.5 or 2 bytes per pixel instead of 3, a whole step's
 * frames in one copy.  The same five formats, the same description of pitches and plane offsets -- adas_yuv_params now describes a
 * destination.  The rules E1-E7 are csrc/yuvout_core.h: BT.601 limited range in OpenCV's 20-bit integers (ADAS_YUV_MATRIX_VIDEO) or JFIF full
 * range (ADAS_YUV_MATRIX_FULL, the JPEG encoder's rule J2); a chroma sample is the rounded mean of its cell's pixels
 * (ADAS_YUVOUT_CHROMA_MEAN, what encoders' scalers do) or its first pixel's (ADAS_YUVOUT_CHROMA_FIRST).  One plain launch: capturable, no
 * allocation and no host synchronisation in adas_yuvout_run.
 * =================================================================================== */
typedef struct adas_yuvout adas_yuvout;
#define ADAS_YUVOUT_CHROMA_MEAN 0    /* (a + b + c + d + 2) >> 2 over a 2x2 cell (4:2:0), (a + b + 1) >> 1 over a 2x1 cell (4:2:2) */
#define ADAS_YUVOUT_CHROMA_FIRST 1   /* U and V of the cell's first pixel */
#define ADAS_YUVOUT_SRC_OVERLAY 0    /* adas_pipeline_attach_yuvout: the attached overlay's own buffer, behind its stages, text and panels */
#define ADAS_YUVOUT_SRC_FRAMES 1     /* the u8 frames adas_pipeline_step_frames* was given */
typedef struct {                  /* adas_yuv_params, then chroma */
    int32_t format, matrix;
    int32_t width, height;
    int64_t frame_stride;
    int64_t y_offset, y_pitch;
    int64_t u_offset, u_pitch;
    int64_t v_offset, v_pitch;
    int32_t chroma;
} adas_yuvout_params;
/* The tight layout of a width x height frame, matrix VIDEO, chroma MEAN. */
int adas_yuvout_default_params(adas_yuvout_params* p, int format, int width, int height);
/* Bytes of one destination frame up to the end of its last plane; a batch ends (batch - 1) * frame_stride + this behind its start.  0 for
 * parameters adas_yuvout_create would refuse. */
int64_t adas_yuvout_frame_bytes(const adas_yuvout_params* p);
/* ADAS_ERR_INVALID by name, with adas_yuv_create's words: odd width, odd height for a 4:2:0 format, pitch shorter than a row, plane
 * outside the frame, planes overlap, max_batch < 1; and unknown chroma mode.  Allocates (max_batch - 1) * frame_stride + frame_bytes bytes,
 * zeroed. */
int adas_yuvout_create(const adas_yuvout_params* p, int max_batch, adas_yuvout** out);
int adas_yuvout_destroy(adas_yuvout* h);
/* d_bgr [batch][height][width][3] u8 on the device, any alignment.  d_dst: frame f at d_dst + f * frame_stride, any alignment; NULL: the
 * handle's own buffer.  Every byte of every plane row is written and no other byte: pitch padding and the gaps between planes and frames
 * keep what they held.  When width, the pitches, the offsets, frame_stride and both pointers are multiples of 16 every access is 16 (I420's
 * chroma: 8) bytes wide; any other geometry goes byte by byte and gives the same bytes.  Asynchronous on `stream`. */
int adas_yuvout_run(adas_yuvout* h, const uint8_t* d_bgr, int batch, uint8_t* d_dst, void* stream);
/* Frame `frame` of the handle's own buffer -> h_dst [frame_bytes], after the last run's stream has drained.  ADAS_ERR_INVALID for a frame
 * the last run did not write there. */
int adas_yuvout_fetch(adas_yuvout* h, int frame, uint8_t* h_dst);
/* The first `batch` frames of the last run in ONE copy: (batch - 1) * frame_stride + frame_bytes bytes, frame f at h_dst + f * frame_stride.
 * Meant for a pinned buffer (adas_host_alloc). */
int adas_yuvout_fetch_all(adas_yuvout* h, int batch, uint8_t* h_dst);
int adas_yuvout_device_view(adas_yuvout* h, const uint8_t** d_frames);

/* ===================================================================================
 * Finished BGR frames reduced on the device: a preview per frame, or a mosaic in which every frame of a step is a tile -- a video wall.  What
 * a caller's cv2.resize(frame_show, size) and NumPy slice assignments do on host cores after fetching every full frame: here one canvas, or a
 * reduced frame per stream, leaves instead.  The rules S1-S8 are csrc/scale_core.h: a tile is dst_w x dst_h, a canvas is cols x rows tiles,
 * frame f goes to canvas f / (cols * rows), cell f % (cols * rows) in row-major order; ADAS_SCALE_AREA is an exact integer box filter
 * (reduction only, round to nearest with ties up, (a + b + c + d + 2) >> 2 at a ratio of 2), ADAS_SCALE_LINEAR the project's 8-bit
 * INTER_LINEAR (the bird panel's rule P5).  A tile can wear its frame's collision state as a border.  One plain launch: capturable, no
 * allocation and no host synchronisation in adas_scale_run.
 * =================================================================================== */
typedef struct adas_scale adas_scale;
#define ADAS_SCALE_AREA 0          /* exact box filter, dst <= src on both axes */
#define ADAS_SCALE_LINEAR 1        /* rule P5, any sizes */
#define ADAS_SCALE_SRC_OVERLAY 0   /* adas_pipeline_attach_scale: the attached overlay's own buffer, behind its stages, text and panels */
#define ADAS_SCALE_SRC_FRAMES 1    /* the u8 frames adas_pipeline_step_frames* was given */
typedef struct {
    int32_t src_w, src_h;           /* a source frame */
    int32_t dst_w, dst_h;           /* a tile */
    int32_t mode;                   /* ADAS_SCALE_* */
    int32_t cols, rows;             /* tiles of a canvas; 1, 1: one reduced frame per frame */
    int32_t border;                 /* pixel rings that take border_bgr[state]; 0: none */
    uint8_t background[4];          /* B, G, R of a cell without a frame; [3] unused */
    uint8_t border_bgr[4][4];       /* [ANA_COLLISION_*] B, G, R; [3] unused */
} adas_scale_params;
/* mode AREA, one tile per canvas, no border, a black background, border colours demo.py's ControlPanel.CollisionDict: UNKNOWN (0,255,255),
 * NORMAL (0,255,0), PROMPT (0,102,255), WARNING (0,0,255). */
int adas_scale_default_params(adas_scale_params* p, int src_w, int src_h, int dst_w, int dst_h);
/* Bytes of one canvas, rows * dst_h * cols * dst_w * 3, and the canvases a run of `batch` frames writes, ceil(batch / (cols * rows)); 0
 * for parameters adas_scale_create would refuse. */
int64_t adas_scale_canvas_bytes(const adas_scale_params* p);
int adas_scale_canvases(const adas_scale_params* p, int batch);
/* ADAS_ERR_INVALID by name: unknown mode; source and tile sides must be in 1..16383; mosaic columns and rows must be in 1..16383; area does
 * not enlarge; area needs src_w * src_h <= 8388608; border must be >= 0 and 2 * border < min(dst_w, dst_h); a canvas must stay below 2^31
 * bytes; max_batch < 1.  Allocates adas_scale_canvases(max_batch) canvases, zeroed. */
int adas_scale_create(const adas_scale_params* p, int max_batch, adas_scale** out);
int adas_scale_destroy(adas_scale* h);
/* d_bgr [batch][src_h][src_w][3] u8 on the device, any alignment.  d_state: NULL, or frame f's int32 state (ANA_COLLISION_*; anything else
 * counts as UNKNOWN) at d_state + f * state_stride bytes, read only when border > 0.  d_dst: canvas k at d_dst + k * canvas_bytes, any
 * alignment; NULL: the handle's own buffer.  Every byte of the adas_scale_canvases(batch) canvases is written exactly once, cells without a
 * frame with `background`, and no other byte.  When dst_w * 3 and both pointers are multiples of 16 every store is 16 bytes wide; anything
 * else goes byte by byte and gives the same bytes.  ADAS_ERR_INVALID for batch > max_batch.  Asynchronous on `stream`. */
int adas_scale_run(adas_scale* h, const uint8_t* d_bgr, int batch, const void* d_state, int64_t state_stride, uint8_t* d_dst, void* stream);
/* Canvas `canvas` of the handle's own buffer -> h_dst [canvas_bytes], after the last run's stream has drained.  ADAS_ERR_INVALID for a
 * canvas the last run did not write there. */
int adas_scale_fetch(adas_scale* h, int canvas, uint8_t* h_dst);
/* The first `canvases` canvases of the last run in ONE copy.  Meant for a pinned buffer (adas_host_alloc). */
int adas_scale_fetch_all(adas_scale* h, int canvases, uint8_t* h_dst);
int adas_scale_device_view(adas_scale* h, const uint8_t** d_canvases);

/* ===================================================================================
 * Camera frames rectified on the device, in FRONT of the step: cv2.remap(frame, map1, map2, INTER_LINEAR, BORDER_CONSTANT 0) of BGR u8 frames
 * in HBM through a fixed-point map per stream -- what a caller's cv2.undistort / cv2.remap does on host cores before the upload.  A map is
 * cv2's CV_16SC2 + CV_16UC1 pair: (sx, sy) int16 per destination pixel and a fraction word ay * 32 + ax (ax, ay in 0..31; the top 6 bits are
 * ignored).  It is either built here from a lens model as cv2.initUndistortRectifyMap(K, D, R, new_K, size, CV_16SC2) writes it (Brown-Conrady
 * / rational: k1 k2 p1 p2 k3 k4 k5 k6), or the caller's own table, which covers fisheye lenses, stereo rectification and anything else cv2
 * can tabulate.  The rules U1-U6 are csrc/remap_core.h; OpenCV's arithmetic restated, parity with a real cv2 build unpinned.  Frame f of a
 * batch belongs to stream f % n_streams and reads the map assigned to that stream; several streams may share one map.
 * =================================================================================== */
typedef struct adas_remap adas_remap;
typedef struct {
    int src_h, src_w;               /* a camera frame */
    int dst_h, dst_w;               /* a rectified frame: rectification often crops */
    int n_streams, n_maps;          /* streams of a batch; maps the handle holds */
} adas_remap_params;
typedef struct {
    double K[4];                    /* fx, fy, cx, cy of the camera */
    double D[8];                    /* k1, k2, p1, p2, k3, k4, k5, k6; a shorter list is zero-padded */
    double new_K[4];                /* fx, fy, cx, cy of the rectified image (cv2.undistort's default: K) */
    double R[9];                    /* rectifying rotation, row-major (default: identity) */
} adas_remap_camera;
/* ADAS_ERR_INVALID by name: "size outside 1..4320 rows x 1..16384 columns"; n_streams, n_maps or max_batch outside 1..65535.  The handle is
 * host state until the first set call (or adas_remap_device_view) allocates n_maps maps and max_batch BGR frames. */
int adas_remap_create(const adas_remap_params* p, int max_batch, adas_remap** out);
int adas_remap_destroy(adas_remap* h);
/* Builds map `map` (-1: every map) from a lens model on the device.  ADAS_ERR_INVALID by name: "non-finite parameter", "zero focal length"
 * (fx, fy of K or new_K), "singular new_K * R", "map index outside the handle's table".  Ordered behind the handle's last run on that run's
 * stream, and finished on return. */
int adas_remap_set_camera(adas_remap* h, int map, const adas_remap_camera* cam);
/* Map `map` from the caller: h_xy [dst_h][dst_w][2] int16, h_frac [dst_h][dst_w] uint16.  Ordered as adas_remap_set_camera. */
int adas_remap_set_map(adas_remap* h, int map, const int16_t* h_xy, const uint16_t* h_frac);
/* Stream `stream` reads map `map` from the next run on.  Default: stream s reads map min(s, n_maps - 1). */
int adas_remap_assign(adas_remap* h, int stream, int map);
/* Map `map` as the runs read it, in adas_remap_set_map's layout.  ADAS_ERR_INVALID for a map that was never set. */
int adas_remap_fetch_map(adas_remap* h, int map, int16_t* h_xy, uint16_t* h_frac);
/* d_src_bgr [batch][src_h][src_w][3] u8 on the device, any alignment.  d_dst_bgr [batch][dst_h][dst_w][3], any alignment; NULL: the handle's
 * own buffer.  Every byte of frames [0, batch) is written exactly once and no other byte.  ADAS_ERR_INVALID for batch > max_batch and for a
 * stream whose map was never set.  One plain launch, asynchronous on `stream`, capturable. */
int adas_remap_run(adas_remap* h, const uint8_t* d_src_bgr, int batch, uint8_t* d_dst_bgr, void* stream);
/* Frame `frame` of the handle's own buffer -> h_bgr [dst_h][dst_w][3], after the last run's stream has drained.  The set calls, the fetches and
 * this call use the stream of the handle's last run: that stream must still exist (a caller who destroys it first runs the handle once more
 * on another stream, or detaches it from its pipeline). */
int adas_remap_fetch(adas_remap* h, int frame, uint8_t* h_bgr);
int adas_remap_device_view(adas_remap* h, const uint8_t** d_frames_bgr);

/* ===================================================================================
 * ByteTrack: replaces BYTETracker.__init__/update/reset (byteTracker.py:30-51,62-185,187-200)
 * with matching.py, kalman_filter.py, strack.py, base_track.py, byteTrack/utils.py underneath.
 * One independent tracker (own id counter) per stream; the whole update runs on the GPU.
 * =================================================================================== */
typedef struct adas_bytetrack adas_bytetrack;

typedef struct {
    double track_thresh;  /* 0.5 */
    double match_thresh;  /* 0.8 */
    double frame_rate;    /* 30 */
    int32_t track_buffer; /* 30 */
    int32_t max_tracks;   /* track-table capacity per stream (tracked + lost) */
    int32_t max_dets;     /* detections per frame capacity */
    int32_t reserved;
} adas_bytetrack_params;

typedef struct {          /* base_track.py:61-72 + strack.py:207-215 (crops stay on the host; trajectories: adas_bytetrack_fetch_trajectories) */
    double tlwh[4];       /* STrack.tlwh (Kalman-filtered) */
    double score;
    int32_t track_id, state, is_activated, class_id;
    int32_t frame_id, start_frame, tracklet_len;
    int32_t trajectory_len;   /* len(STrack.trajectories), 0 .. 30 (strack.py:53,115); the boxes: adas_bytetrack_fetch_trajectories */
} adas_track;
#define ADAS_TRAJECTORY_LEN 30   /* LimitedList(30), strack.py:53 */

typedef struct {
    int32_t frame_id, id_count, n_tracked, n_lost, err, pad[3];
} adas_track_header;

int adas_bytetrack_create(const adas_bytetrack_params* p, int n_streams, adas_bytetrack** out);
int adas_bytetrack_destroy(adas_bytetrack* h);
int adas_bytetrack_reset(adas_bytetrack* h, int stream_index /* -1 = all */);
/* BYTETracker.update(bboxes, scores, class_ids, frame) for one stream from host arrays
 * (xyxy fp64 [n][4], scores fp64, integer class ids). */
int adas_bytetrack_update_host(adas_bytetrack* h, int stream_index, const double* h_xyxy, const double* h_scores,
                               const int32_t* h_cls, int n);
/* All streams at once from device-resident detections (e.g. adas_yolo_post_device_views):
 * stream s reads n = d_counts[s*count_stride + count_index] rows at row offset s*det_stride. */
int adas_bytetrack_update_device(adas_bytetrack* h, const double* d_xyxy, const double* d_scores,
                                 const int32_t* d_cls, const int32_t* d_counts, int det_stride, int count_stride,
                                 int count_index, int n_streams, void* stream);
/* The same for n_frames CONSECUTIVE frames of every stream in one launch (temporal micro-batching, adas_pipeline_desc.micro_batch):
 * frame f of stream s reads detection slab f * n_streams + s; the updates of a stream run in temporal order inside its workgroup,
 * exactly as n_frames calls of adas_bytetrack_update_device would (BYTETracker.update once per frame, byteTracker.py:62). */
int adas_bytetrack_update_device_frames(adas_bytetrack* h, const double* d_xyxy, const double* d_scores,
                                        const int32_t* d_cls, const int32_t* d_counts, int det_stride, int count_stride,
                                        int count_index, int n_streams, int n_frames, void* stream);
/* Sizes the per-frame message store of adas_bytetrack_update_device_frames ahead of time (needed before such a launch is captured into
 * a hipGraph: adas_pipeline_create does it for micro-batched pipelines; eager launches size it on demand). */
int adas_bytetrack_reserve_frames(adas_bytetrack* h, int n_frames, int n_streams);
/* The message of frame `frame` (0 .. n_frames - 1) of the LAST adas_bytetrack_update_device_frames launch: what BYTETracker.update returned
 * for that frame (byteTracker.py:185) -- the live state (adas_bytetrack_fetch) only holds the last frame's.  Same layout as fetch. */
int adas_bytetrack_fetch_frame(adas_bytetrack* h, int stream_index, int frame, adas_track_header* hdr, adas_track* tracks, int max_tracks);
/* Synchronises; tracks[0..n_tracked) are tracked_stracks, then n_lost lost_stracks, list order kept. */
int adas_bytetrack_fetch(adas_bytetrack* h, int stream_index, adas_track_header* hdr, adas_track* tracks,
                         int max_tracks);

/* STrack.trajectories of the LIVE state (the last 30 detection boxes a track was updated with, strack.py:115 -- what DrawTrackedOnFrame
 * draws and filter_trajectories / plot_directions read, byteTracker.py:202-215), for the tracks in the order of adas_bytetrack_fetch
 * (tracked, then lost): lens[k] = len(trajectories) and tlbr[k][i][0..4) = trajectories[i] (x1, y1, x2, y2 fp64, oldest first) for
 * i < lens[k].  lens holds max_tracks entries, tlbr max_tracks x ADAS_TRAJECTORY_LEN x 4; *n_tracks = n_tracked + n_lost.  Synchronises. */
int adas_bytetrack_fetch_trajectories(adas_bytetrack* h, int stream_index, int32_t* lens, double* tlbr, int max_tracks, int32_t* n_tracks);

/* ===================================================================================
 * Fused per-frame pipeline (the path demo.py:261-281 drives): detector forward + decode/NMS,
 * lane forward + decode, tracker update, for `n_streams` independent video streams per step,
 * captured in a hipGraph.  Inputs are the two pre-processed NCHW fp32 tensors per stream in HBM.
 * =================================================================================== */
typedef struct adas_pipeline adas_pipeline;
typedef struct {
    adas_engine* detector;      /* may be NULL */
    adas_engine* lane;          /* may be NULL */
    adas_yolo_post* post;       /* required with detector */
    adas_ufld_decode* decode;   /* required with lane */
    adas_bytetrack* tracker;    /* may be NULL */
    int32_t n_streams;
    int32_t use_graph;          /* bit0: capture the step in a hipGraph (the lane branch is then forked onto a second
                                 * stream so the two nets overlap); bit1: keep both nets on one stream */
    adas_lane_geometry* geometry; /* may be NULL; with lane: area polygon / bird view / curvature right behind the decode */
    int32_t micro_batch;        /* 0 / 1: one frame of every stream per step.  B > 1: temporal micro-batching -- a step takes B
                                 * CONSECUTIVE frames of every stream (frame b of stream s at index b * n_streams + s of the input),
                                 * the pre-processing / networks / decode / NMS run on all n_streams * B frames at once (no
                                 * cross-frame dependency there) and the tracker then consumes each stream's B frames in order
                                 * (B update launches).  Engines, post and decode handles need max_batch >= n_streams * B; results of
                                 * frame b of stream s are fetched at frame index b * n_streams + s, tracker state per stream.
                                 * Throughput mode for few streams per GPU (adds B - 1 frames of latency). */
    int32_t reserved;
} adas_pipeline_desc;
int adas_pipeline_create(const adas_pipeline_desc* d, adas_pipeline** out);
/* 1 when the steps feed the post-processing's per-anchor scan arrays from the fused Detect kernel (adas_engine_set_detect_sink). */
int adas_pipeline_detect_sink(const adas_pipeline* p);
int adas_pipeline_destroy(adas_pipeline* p);
/* Optional stages on the lane branch, right behind the decode and inside the capture: adas_birdview_run, then
 * adas_lane_geometry_run_matrices on its per-frame matrices (in place of the geometry handle's single matrix), then -- with a warp
 * handle -- adas_warp_run_device_matrices from the step's u8 frames into the warp handle's own buffer.  Call before the first step
 * (cached graphs are dropped).  Needs a lane engine, a decode and a geometry handle; the bird-view handle must hold n_streams streams
 * and n_streams x micro_batch frames, the warp handle as many frames and the step's camera geometry as its source size.  With a warp
 * attached the seam-tensor step is ADAS_ERR_INVALID (no frame to warp).  `warp` may be NULL.  The handles stay the caller's. */
int adas_pipeline_attach_birdview(adas_pipeline* p, adas_birdview* bird, adas_warp* warp);
/* adas_birdview_request on the pipeline's own stream: lands on the next step, which replays the same graph.  ADAS_ERR_INVALID while an
 * analysis handle is attached: the device then owns the requests. */
int adas_pipeline_request_transform(adas_pipeline* p, int stream, int mode);
/* Optional last stage of the step: adas_analysis_run on the pipeline's main stream behind the join of the two branches, inside the
 * capture.  Needs a detector with its post handle and a lane engine with decode and geometry handles; the analysis handle must hold
 * n_streams streams and n_streams x micro_batch frames.  With a bird-view handle attached (in either order) the stage stores each stream's
 * request word into that handle's pending table, the next step's adas_birdview_run consumes it (ordered through that step's own fork),
 * every stream's initial "Default" is queued now and again by adas_analysis_reset, and adas_pipeline_request_transform is refused; that
 * combination needs micro_batch <= 1 (frame b's request could not reach frame b + 1 inside one step).  Call before the first step (cached
 * graphs are dropped).  Without it the step, its graph and its launch count are unchanged.  The handle stays the caller's and must outlive
 * the pipeline. */
int adas_pipeline_attach_analysis(adas_pipeline* p, adas_analysis* analysis);
/* Optional drawing stage, last on the pipeline's main stream (behind adas_analysis_run, or behind the join of the two branches when no
 * analysis handle is attached) and inside the capture: adas_overlay_run from the step's u8 frames into the overlay handle's own buffer
 * (adas_overlay_fetch), with the attached analysis handle if there is one.  Needs a lane engine with decode (4 lanes) and geometry
 * handles.  The stages drawn are LANES and AREA, DISTANCE when an analysis handle is attached by the time of the step, and BIRD when a
 * bird view with its warp is (the discs land on the warp handle's own buffer, behind adas_warp_run_device_matrices; the overlay's bird
 * size must then be the warp's destination size); adas_pipeline_set_overlay_stages narrows them.  The overlay handle must hold
 * n_streams x micro_batch frames and the step's camera geometry as its source size.  With an overlay attached the seam-tensor step is
 * ADAS_ERR_INVALID (no frame to draw on).  Call before the first step (cached graphs are dropped).  Without it the step, its graph and
 * its launch count are unchanged.  The handle stays the caller's. */
int adas_pipeline_attach_overlay(adas_pipeline* p, adas_overlay* overlay);
/* The stages (ADAS_OVERLAY_*) the attached overlay draws; one that lacks its handle (DISTANCE without an analysis handle, BIRD without a
 * warp, DETECTIONS without a detector, TRACKS or TRAJECTORIES without a tracker) is ADAS_ERR_INVALID at the step.  The default set holds
 * none of DETECTIONS, TRACKS, TRAJECTORIES.  DETECTIONS draws the step's survivors, TRACKS and TRAJECTORIES the tracker's table after this
 * step's update; either with micro_batch > 1 is ADAS_ERR_INVALID at the step (the live table holds the last frame only).  Accepts
 * 63 | ADAS_OVERLAY_TRAJECTORIES; bit 64 is refused.  Cached graphs are dropped. */
int adas_pipeline_set_overlay_stages(adas_pipeline* p, int stages);
/* The panels (ADAS_PANEL_*) the step paints on the overlay's frames: adas_overlay_run_panels on the overlay handle's own buffer, recorded
 * directly behind the attached overlay's run and inside the capture (two more launches; 0: none, the step is what it was).  Needs
 * adas_overlay_set_panels on the attached handle.  BIRD needs a bird view with its warp attached, SIGNS and COLLISION an analysis handle:
 * a missing one is ADAS_ERR_INVALID at the step, by name.  micro_batch > 1 is allowed (the latch walks a stream's frames in order).
 * Cached graphs are dropped. */
int adas_pipeline_set_overlay_panels(adas_pipeline* p, int panels);
/* The text (ADAS_TEXT_*) the step paints on the overlay's frames, inside the capture (0: none, the step is what it was): one layout launch
 * behind the overlay's run (adas_overlay_run_text on the step's post, tracker and analysis handles), a draw of the scene's text -- detections,
 * tracks, ids, distances -- over the stages and under the panels, and a draw of the panel strings and the caller's lines behind the panels;
 * all of it ahead of the JPEG stage.  Stated divergence: in the reference a label can be covered by a box drawn later; here text lies over
 * all stages.  Needs adas_overlay_set_font on the attached handle; TRACKS and TRACK_IDS need micro_batch <= 1; a bit without its handle is
 * refused at the step, by name.  Cached graphs are dropped. */
int adas_pipeline_set_overlay_text(adas_pipeline* p, int mask);
/* on != 0: the step draws the bird view's readouts (ADAS_OVERLAY_READOUTS) on the attached warp's image, inside the capture and ahead of the
 * bird stage's discs -- two more launches; 0 (the default): none, the step is what it was.  The bit has this entry of its own because
 * adas_pipeline_set_overlay_stages keeps its mask.  Needs a font in the readout style's slot on the attached overlay handle (checked
 * here) and a bird view with its warp (ADAS_ERR_INVALID at the step, by name).  The bird panel then shows them.  Cached graphs are dropped. */
int adas_pipeline_set_overlay_readouts(adas_pipeline* p, int on);
/* Optional encoding stage, the step's last launch group on the pipeline's main stream and inside the capture: adas_jpeg_run on all
 * n_streams x micro_batch frames of the step (frames are independent: any micro_batch).  source ADAS_JPEG_SRC_OVERLAY: the attached
 * overlay's own buffer, behind its stages and panels (needs adas_pipeline_attach_overlay first); ADAS_JPEG_SRC_FRAMES: the camera frames
 * the step was given.  Either needs adas_pipeline_step_frames* (the seam-tensor step is then ADAS_ERR_INVALID).  The handle must hold
 * n_streams x micro_batch frames; its size must be the overlay's (checked here) and the step's camera geometry (checked at the step).
 * jpeg == NULL detaches.  Cached graphs are dropped.  Without it the step, its graph and its launch count are unchanged.  The handle
 * stays the caller's; adas_jpeg_fetch after adas_pipeline_sync. */
int adas_pipeline_attach_jpeg(adas_pipeline* p, adas_jpeg* jpeg, int source);
/* Optional raw-video stage on the pipeline's main stream and inside the capture, behind the overlay's stages, text and panels: adas_yuvout_run
 * on all n_streams x micro_batch frames of the step into the handle's own buffer -- one more launch.  source ADAS_YUVOUT_SRC_OVERLAY: the
 * attached overlay's own buffer (needs adas_pipeline_attach_overlay first); ADAS_YUVOUT_SRC_FRAMES: the camera frames the step was given.
 * Independent of an attached JPEG stage: both may be on.  Needs adas_pipeline_step_frames* (the seam-tensor step is then
 * ADAS_ERR_INVALID).  The handle must hold n_streams x micro_batch frames; its size must be the overlay's (checked here) and the step's
 * camera geometry (checked at the step).  yuvout == NULL detaches.  Cached graphs are dropped.  Without it the step, its graph and its
 * launch count are unchanged.  The handle stays the caller's; adas_yuvout_fetch / _fetch_all after adas_pipeline_sync. */
int adas_pipeline_attach_yuvout(adas_pipeline* p, adas_yuvout* yuvout, int source);
/* Optional scaling stage on the pipeline's main stream and inside the capture, behind the overlay's stages, text and panels and in front of
 * the JPEG and YUV stages: adas_scale_run on all n_streams x micro_batch frames of the step, in frame-index order, into the handle's own
 * canvases -- one more launch.  source as for adas_pipeline_attach_yuvout, with the same checks: the overlay source needs an attached overlay
 * whose frame geometry equals the handle's source, the handle must hold a step's frames.  With border > 0 the step passes the attached
 * analysis handle's collision column as the states; the attach is refused when border > 0 and no analysis handle is attached.  The stage
 * needs adas_pipeline_step_frames*.  scale == NULL detaches.  Every call detaches the two consumers below, which were checked against the
 * handle that leaves: attach them again behind a new one.  Cached graphs are dropped.  Without it the step, its graph and its launch count
 * are unchanged. */
int adas_pipeline_attach_scale(adas_pipeline* p, adas_scale* scale, int source);
/* A second JPEG encoder and a second YUV writer, created by the caller at the canvas size (cols * dst_w x rows * dst_h) for at least the
 * step's canvas count, that consume the scaling stage's canvases directly behind it: adas_jpeg_run's launches, one launch of
 * adas_yuvout_run.  Independent of adas_pipeline_attach_jpeg / _yuvout, so the full-size feed and the preview can leave the same step.
 * Refused by name: no scale handle attached first, a handle of another width or height than the canvas, a handle that holds fewer frames
 * than the step has canvases.  NULL detaches.  Cached graphs are dropped. */
int adas_pipeline_attach_scale_jpeg(adas_pipeline* p, adas_jpeg* jpeg);
int adas_pipeline_attach_scale_yuvout(adas_pipeline* p, adas_yuvout* yuvout);
/* Kernel nodes of the captured step the last graph-mode step replayed.  ADAS_ERR_INVALID before the first such step. */
int adas_pipeline_graph_kernels(adas_pipeline* p, int32_t* n_kernels);
/* One step = one frame of every stream (micro_batch frames with temporal micro-batching).  Asynchronous; adas_pipeline_sync() waits. */
int adas_pipeline_step(adas_pipeline* p, const float* d_det_input_nchw, const float* d_lane_input_nchw);
/* The same step from camera frames: n_streams BGR u8 frames (src_h x src_w x 3, back to back) in HBM; each branch runs its
 * pre-processing (adas_preprocess_yolo / adas_preprocess_ufld with lane_crop_ratio = ModelConfig.crop_ratio) into seam
 * tensors the pipeline owns, so one upload per stream and frame feeds both nets (yoloDetector.py:96-102,
 * ultrafastLaneDetectorV2.py:96-112 + the body of demo.py:261-281). */
int adas_pipeline_step_frames(adas_pipeline* p, const uint8_t* d_frames_bgr, int src_h, int src_w, double lane_crop_ratio);
/* The same step from HOST frames (what a capture thread hands over, demo.py:261-270): the frames of this step are copied to one
 * of two device staging buffers on a dedicated copy stream while the previous step still computes (double buffering: copy k+1
 * overlaps compute k; the compute stream waits for its copy, the copy stream for the step that last read its buffer).
 * h_frames_bgr should come from adas_host_alloc (pinned): pageable memory works but the copy then cannot overlap. */
int adas_pipeline_step_frames_host(adas_pipeline* p, const uint8_t* h_frames_bgr, int src_h, int src_w, double lane_crop_ratio);
/* The call above returns when the upload is ENQUEUED: the host buffer must not be rewritten before the copy has read it.  This waits
 * for exactly that (the copy stream only, not the compute): call it before refilling a host buffer that the last step was given. */
int adas_pipeline_wait_upload(adas_pipeline* p);
/* Optional decoding stage in FRONT of the step, outside the capture: the handle adas_pipeline_step_jpeg_host decodes with.  It must hold
 * n_streams x micro_batch frames; its size is the step's camera geometry and must be that of an attached warp, overlay or JPEG stage
 * (checked at the step).  jpegdec == NULL detaches.  Nothing inside the captured step changes; the handle stays the caller's. */
int adas_pipeline_attach_jpegdec(adas_pipeline* p, adas_jpegdec* jpegdec);
/* The step from COMPRESSED host frames, n_streams x micro_batch baseline JPEG streams: their bytes are packed into one of the decoder's
 * two staging buffers and copied on the pipeline's copy stream while the previous step still computes (the double buffering of
 * adas_pipeline_step_frames_host, on a few hundred KB per frame), decoded on the main stream into the decoder's own frames, and those go
 * through adas_pipeline_step_frames: one address, so one captured step.  The host bytes are free again on return;
 * adas_pipeline_wait_upload keeps its meaning.  Each frame's flag word: adas_jpegdec_fetch_flags on the attached handle after
 * adas_pipeline_sync; a rejected frame is a black frame to the step. */
int adas_pipeline_step_jpeg_host(adas_pipeline* p, const uint8_t* const* h_streams, const int64_t* h_lengths, double lane_crop_ratio);
/* Optional conversion stage in FRONT of the step, outside the capture: the handle adas_pipeline_step_yuv* converts with.  It must hold
 * n_streams x micro_batch frames; its size is the step's camera geometry and must be that of an attached warp, overlay or JPEG stage
 * (checked at the step).  yuv == NULL detaches.  Nothing inside the captured step changes; the handle stays the caller's. */
int adas_pipeline_attach_yuv(adas_pipeline* p, adas_yuv* yuv);
/* The step from n_streams x micro_batch camera frames in the attached handle's format ALREADY ON THE DEVICE (a decoder's surface): they
 * are converted on the main stream into the handle's own BGR frames, and those go through adas_pipeline_step_frames: one address, so
 * one captured step. */
int adas_pipeline_step_yuv(adas_pipeline* p, const uint8_t* d_src, double lane_crop_ratio);
/* The same from HOST frames (pinned: adas_host_alloc), (frames - 1) * frame_stride + adas_yuv_frame_bytes bytes: the double buffering
 * of adas_pipeline_step_frames_host on 1.5 or 2 bytes per pixel -- the copy runs on the copy stream into one of two device buffers
 * while the previous step still computes, the conversion waits for it.  adas_pipeline_wait_upload keeps its meaning. */
int adas_pipeline_step_yuv_host(adas_pipeline* p, const uint8_t* h_src, double lane_crop_ratio);
/* Optional rectification stage in FRONT of the step, outside the capture, behind every way in (adas_pipeline_step_frames, _frames_host,
 * _jpeg_host, _yuv, _yuv_host): adas_pipeline_step_frames first runs adas_remap_run on the main stream from the frames it was given into the
 * handle's own buffer, and the whole step -- pre-processing, the bird-view warp, the overlay, the *_SRC_FRAMES sources -- reads that buffer:
 * one address, so one captured step.  The handle's source and destination sizes must both equal the step's camera geometry (checked at the
 * step), its n_streams the pipeline's, and it must hold n_streams x micro_batch frames.  remap == NULL detaches.  Cached graphs are dropped.
 * Without it no line of the step's path changes.  The handle stays the caller's; adas_remap_fetch after adas_pipeline_sync.  The handle
 * remembers the pipeline's stream as that of its last run; detaching it and adas_pipeline_destroy synchronise that stream and hand the
 * handle back with no stream remembered, so it must outlive the pipeline or be detached first. */
int adas_pipeline_attach_remap(adas_pipeline* p, adas_remap* remap);
int adas_pipeline_sync(adas_pipeline* p);
/* Device time of the last `n` steps' sections in ms (hipEvents on the pipeline stream):
 * [0] detector net, [1] yolo post, [2] lane net, [3] lane decode, [4] tracker, [5] whole step.  The stages in FRONT of the step -- an attached
 * decoder, converter or remap handle -- are launched before the step's first event and are not part of any of the six figures. */
int adas_pipeline_timings(adas_pipeline* p, float ms[6]);

#ifdef __cplusplus
}
#endif
#endif /* ADAS_HIP_H */
