"""ctypes binding of libadas_hip.so -- the only way the Python host side reaches the GPU.

Fails loudly: a missing/unloadable library is an ImportError-like RuntimeError, a missing device is
reported by the library itself (ADAS_ERR_NO_DEVICE); nothing here computes on the CPU.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ADAS_LIB") or os.path.join(HERE, "libadas_hip.so")   # ADAS_LIB: an instrumented scratch build (tools/)

UFLD_MAX_POINTS = 128
HEAD_V8, HEAD_V5, HEAD_V5_LITE = 0, 1, 2
NMS_REFERENCE, NMS_GREEDY = 0, 1
PREC_BF16, PREC_FP32, PREC_FP16, PREC_FP16X3 = 0, 1, 2, 3
# "fp16x3": split precision -- (hi, lo) half pairs, three f16 MFMAs per product, fp32 accumulate: the fp32 mode's results at speed
PRECISIONS = {"bf16": PREC_BF16, "fp32": PREC_FP32, "fp16": PREC_FP16, "fp16x3": PREC_FP16X3}


class AdasError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libadas_hip error {code}: {msg}")
        self.code = code


class YoloPostParams(C.Structure):
    _fields_ = [("layout", C.c_int32), ("num_anchors", C.c_int32), ("num_classes", C.c_int32), ("nms_mode", C.c_int32),
                ("box_score", C.c_double), ("iou_thr", C.c_double), ("pad_h", C.c_int32), ("pad_w", C.c_int32),
                ("ratio_h", C.c_double), ("ratio_w", C.c_double), ("max_candidates", C.c_int32), ("reserved", C.c_int32)]


class YoloCounts(C.Structure):
    _fields_ = [("n_found", C.c_int32), ("n_candidates", C.c_int32), ("n_keep", C.c_int32), ("flags", C.c_int32)]


class EffdetPostParams(C.Structure):
    _fields_ = [("box_score", C.c_double), ("pad_h", C.c_int32), ("pad_w", C.c_int32), ("ratio_h", C.c_double), ("ratio_w", C.c_double),
                ("max_boxes", C.c_int32), ("reserved", C.c_int32)]


class EffdetTailParams(C.Structure):
    _fields_ = [("in_h", C.c_int32), ("in_w", C.c_int32), ("num_classes", C.c_int32), ("max_candidates", C.c_int32), ("max_det", C.c_int32),
                ("reserved", C.c_int32), ("score_thr", C.c_double), ("iou_thr", C.c_double), ("anchor_scale", C.c_double)]


class UfldParams(C.Structure):
    _fields_ = [("grid_row", C.c_int32), ("cls_row", C.c_int32), ("grid_col", C.c_int32), ("cls_col", C.c_int32),
                ("img_w", C.c_int32), ("img_h", C.c_int32), ("local_width", C.c_int32), ("num_lanes", C.c_int32),
                ("h_row_anchor", C.c_void_p), ("h_col_anchor", C.c_void_p)]


class Ufld1Params(C.Structure):
    _fields_ = [("griding_num", C.c_int32), ("cls_num_per_lane", C.c_int32), ("cfg_img_w", C.c_int32), ("cfg_img_h", C.c_int32),
                ("input_w", C.c_int32), ("input_h", C.c_int32), ("src_w", C.c_int32), ("src_h", C.c_int32),
                ("h_row_anchor", C.c_void_p)]


class LaneGeometryParams(C.Structure):
    _fields_ = [("img_h", C.c_int32), ("bird_w", C.c_int32), ("bird_h", C.c_int32), ("adjust_lanes", C.c_int32), ("M", C.c_double * 9)]


class LaneGeometryResult(C.Structure):
    _fields_ = [("area_status", C.c_int32), ("n_area_left", C.c_int32), ("n_area_right", C.c_int32), ("direction", C.c_int32),
                ("bird_counts", C.c_int32 * 4), ("curvature", C.c_double), ("offset", C.c_double)]


class WarpParams(C.Structure):
    _fields_ = [("src_h", C.c_int32), ("src_w", C.c_int32), ("dst_h", C.c_int32), ("dst_w", C.c_int32)]


class BirdviewParams(C.Structure):
    _fields_ = [("img_w", C.c_int32), ("img_h", C.c_int32)]


class BirdviewState(C.Structure):
    _fields_ = [("src", C.c_float * 8), ("M", C.c_double * 9), ("M_inv", C.c_double * 9), ("M_warp", C.c_double * 9),
                ("n_updates", C.c_int32), ("n_rejected", C.c_int32)]


BIRDVIEW_MODES = {"Default": 1, "Top": 2, "Bottom": 3}     # ADAS_BIRDVIEW_*: updateTransformParams' type strings


class AnalysisParams(C.Structure):
    _fields_ = [("focal", C.c_double), ("y_limit", C.c_double), ("distance_thres", C.c_double), ("offset_thres", C.c_double),
                ("curvae_thres", C.c_double), ("calib_curvae_thres", C.c_double), ("calib_frequency", C.c_int32), ("n_classes", C.c_int32),
                ("h_ref_height", C.c_void_p), ("max_points", C.c_int32), ("max_poly", C.c_int32)]


class AnalysisState(C.Structure):
    _fields_ = [("collision_msg", C.c_int32), ("offset_msg", C.c_int32), ("curvature_msg", C.c_int32), ("toggle_status", C.c_int32),
                ("transform_status", C.c_int32), ("oscillator", C.c_int32 * 2), ("counter_offset", C.c_int32), ("counter_curvae", C.c_int32),
                ("counter_birdview", C.c_int32), ("n_collision", C.c_int32), ("n_offset", C.c_int32), ("n_curvature", C.c_int32),
                ("n_nonfinite", C.c_int32), ("collision_record", C.c_double * 5), ("offset_record", C.c_double * 5),
                ("curvature_record", C.c_double * 10), ("direction_record", C.c_int32 * 10)]


class AnalysisInput(C.Structure):
    _fields_ = [("has_point", C.c_int32), ("area", C.c_int32), ("has_offset", C.c_int32), ("has_curvature", C.c_int32), ("direction", C.c_int32),
                ("reserved", C.c_int32), ("distance", C.c_double), ("offset", C.c_double), ("curvature", C.c_double)]


class AnalysisFrame(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("has_collision", C.c_int32), ("collision_x", C.c_int32), ("collision_y", C.c_int32),
                ("collision_d", C.c_double), ("collision_index", C.c_int32), ("collision_msg", C.c_int32), ("offset_msg", C.c_int32),
                ("curvature_msg", C.c_int32), ("toggle_status", C.c_int32), ("transform_status", C.c_int32), ("oscillator", C.c_int32 * 2),
                ("counters", C.c_int32 * 3), ("check", C.c_int32), ("request", C.c_int32), ("flags", C.c_int32)]


ANALYSIS_INPUT_DTYPE = np.dtype([("has_point", "i4"), ("area", "i4"), ("has_offset", "i4"), ("has_curvature", "i4"), ("direction", "i4"),
                                 ("reserved", "i4"), ("distance", "f8"), ("offset", "f8"), ("curvature", "f8")])
ANALYSIS_OVERFLOW, ANALYSIS_NONFINITE, ANALYSIS_TRUNCATED = 1, 2, 4     # adas_analysis_frame.flags


class OverlayParams(C.Structure):
    _fields_ = [("src_h", C.c_int32), ("src_w", C.c_int32), ("bird_h", C.c_int32), ("bird_w", C.c_int32), ("lane_radius", C.c_int32),
                ("distance_radius", C.c_int32), ("bird_radius", C.c_int32), ("reserved", C.c_int32), ("lane_alpha", C.c_double),
                ("area_alpha", C.c_double), ("lane_colors", (C.c_uint8 * 3) * 4), ("offset_color", C.c_uint8 * 3), ("area_color", C.c_uint8 * 3),
                ("collision_colors", (C.c_uint8 * 3) * 4), ("distance_color", C.c_uint8 * 3), ("pad", C.c_uint8 * 7)]


class OverlayObjectStyle(C.Structure):
    _fields_ = [("min_box_area", C.c_double), ("det_rect_thickness", C.c_int32), ("det_arm_thickness", C.c_int32), ("track_thickness", C.c_int32),
                ("reserved", C.c_int32)]


OVERLAY_LANES, OVERLAY_AREA, OVERLAY_DISTANCE, OVERLAY_BIRD = 1, 2, 4, 8     # adas_overlay_run's stages
OVERLAY_DETECTIONS, OVERLAY_TRACKS = 16, 32                                  # the object layer: adas_overlay_run_objects / _run_arrays_objects
OVERLAY_TRAJECTORIES = 128                                                   # adas_overlay_run_trajectories / _run_arrays_trajectories (64 is no stage)
OVERLAY_STAGES = {"lanes": OVERLAY_LANES, "area": OVERLAY_AREA, "distance": OVERLAY_DISTANCE, "bird": OVERLAY_BIRD,
                  "detections": OVERLAY_DETECTIONS, "tracks": OVERLAY_TRACKS, "trajectories": OVERLAY_TRAJECTORIES}
OVERLAY_POLY_RANGE, OVERLAY_TRACK_RANGE = 1, 2                               # adas_overlay_fetch_flags
TRAJECTORY_LEN = 30
TRACK_MARK_CIRCLE, TRACK_MARK_RECT, TRACK_MARK_ARROW = 1, 2, 3


class OverlayArrays(C.Structure):                                            # adas_overlay_arrays
    _fields_ = [(n, C.c_void_p) for n in ("d_src_bgr", "d_dst_bgr", "d_lane_points", "d_lane_counts", "d_poly", "d_poly_counts", "d_area_status",
                                          "d_offset_type", "d_area_bgr", "d_dist_points", "d_dist_counts", "d_bird_points", "d_bird_counts",
                                          "d_bird_bgr", "d_det_xyxy", "d_det_cls", "d_det_counts", "d_trk_tlwh", "d_trk_cls", "d_trk_counts",
                                          "d_traj_tlbr", "d_traj_len", "stream")] + \
               [(n, C.c_int32) for n in ("poly_cap", "dist_cap", "det_cap", "trk_cap", "stages", "n_frames")]


TRACK_MARK_DTYPE = np.dtype([("kind", "i4"), ("track", "i4"), ("x1", "i4"), ("y1", "i4"), ("x2", "i4"), ("y2", "i4"), ("radius", "i4"),
                             ("thickness", "i4"), ("tip", "i4", (4,)), ("color", "u1", (3,)), ("skipped", "u1")])   # adas_overlay_track_mark


OVERLAY_READOUTS = 256                                                       # adas_overlay_run_readouts / _run_arrays_readouts / adas_pipeline_set_overlay_readouts only
OVERLAY_STAGES["readouts"] = OVERLAY_READOUTS
OVERLAY_READOUT_RANGE = 1                                                    # the readout flags of a frame


class OverlayReadoutStyle(C.Structure):                                      # adas_overlay_readout_style
    _fields_ = [("slot", C.c_int32), ("zoom", C.c_int32), ("offset_x", C.c_int32), ("offset_y", C.c_int32), ("radius_x", C.c_int32), ("radius_y", C.c_int32),
                ("text_color", C.c_uint8 * 3), ("arrow_a_color", C.c_uint8 * 3), ("arrow_b_color", C.c_uint8 * 3), ("pad", C.c_uint8 * 3)]


class OverlayReadoutArrays(C.Structure):                                     # adas_overlay_readout_arrays
    _fields_ = [(n, C.c_void_p) for n in ("d_direction", "d_veh_pos", "d_curvature", "d_offset")]


READOUT_STRING_DTYPE = np.dtype([("x", "i4"), ("y", "i4"), ("box", "i4", (4,)), ("len", "i4"), ("skipped", "i4"), ("text", "S32")])   # adas_overlay_readout_string
READOUT_RECORD_DTYPE = np.dtype([("drawn", "i4"), ("flags", "i4"), ("arrows", TRACK_MARK_DTYPE, (2,)), ("strings", READOUT_STRING_DTYPE, (2,))])   # adas_overlay_readout_record


PANEL_BIRD, PANEL_SIGNS, PANEL_COLLISION = 1, 2, 4                        # adas_overlay_run_panels' mask (no stage bits: a mask of their own)
PANELS = {"bird": PANEL_BIRD, "signs": PANEL_SIGNS, "collision": PANEL_COLLISION}
PANEL_SPRITES = ("fcws_warning", "fcws_prompt", "fcws_normal", "left", "right", "straight", "warn", "lta_left", "lta_right")   # ADAS_PANEL_SPRITE_*
PANEL_LATCHES = (None, "Left", "Right", "Straight")                          # ADAS_PANEL_LATCH_*: ControlPanel.curve_status


class OverlayPanelParams(C.Structure):                                       # adas_overlay_panel_params
    _fields_ = [("show_ratio", C.c_double), ("border", C.c_int32), ("signs_w", C.c_int32), ("signs_h", C.c_int32), ("signs_sprite_row", C.c_int32),
                ("collision_sprite_row", C.c_int32), ("collision_sprite_col", C.c_int32), ("border_color", C.c_uint8 * 3), ("reserved", C.c_uint8)]


class OverlaySprite(C.Structure):                                            # adas_overlay_sprite
    _fields_ = [("bgra", C.c_void_p), ("w", C.c_int32), ("h", C.c_int32)]


class OverlayPanelRecord(C.Structure):                                       # adas_overlay_panel_record
    _fields_ = [("sign", C.c_int32 * 2), ("collision", C.c_int32), ("latch", C.c_int32), ("offset_type", C.c_int32), ("curvature_type", C.c_int32),
                ("collision_type", C.c_int32), ("reserved", C.c_int32)]


TEXT_FONTS, TEXT_MAX_LINES = 16, 8                                           # ADAS_TEXT_FONTS, ADAS_TEXT_MAX_LINES
TEXT = {"detections": 1, "tracks": 2, "track_ids": 4, "distance": 8, "panels": 16, "lines": 32}   # ADAS_TEXT_*: a mask of its own, painted in this order
OVERLAY_TEXT_RANGE, OVERLAY_TEXT_OVERFLOW = 1, 2                             # the text flags of a frame
TEXT_ITEM_RECT, TEXT_ITEM_RUN = 1, 2


class OverlayFont(C.Structure):                                              # adas_overlay_font
    _fields_ = [("atlas", C.c_void_p), ("atlas_w", C.c_int32), ("cell_h", C.c_int32), ("baseline_row", C.c_int32), ("size_h", C.c_int32),
                ("size_w_extra", C.c_int32), ("reserved", C.c_int32), ("scale", C.c_double), ("glyph_x", C.c_int32 * 95), ("glyph_w", C.c_int32 * 95),
                ("bearing_x", C.c_int32 * 95), ("advance", C.c_int32 * 95)]


TEXT_STYLE_INTS = ("max_text_items", "det_size_slot", "det_label_slot", "det_label_dx", "det_label_dy", "det_box_pad", "track_slot", "track_dy", "id_first",
                   "id_count", "id_shadow_first", "id_shadow_count", "dist_size_first", "dist_size_count", "dist_first", "dist_count", "dist_shadow_first",
                   "dist_shadow_count", "shadow_dx", "shadow_dy", "ldws_slot", "lkas_slot", "fcws_slot", "ldws_x", "ldws_y", "lkas_x", "lkas_y", "fcws_dx",
                   "fcws_y", "id_shadow_sub")


class OverlayTextStyle(C.Structure):                                         # adas_overlay_text_style
    _fields_ = [("show_ratio", C.c_double), ("min_box_area", C.c_double)] + [(n, C.c_int32) for n in TEXT_STYLE_INTS] + \
               [("label_color", C.c_uint8 * 3), ("dist_color", C.c_uint8 * 3), ("dist_shadow_color", C.c_uint8 * 3), ("offset_colors", (C.c_uint8 * 3) * 4),
                ("curvature_colors", (C.c_uint8 * 3) * 6), ("collision_colors", (C.c_uint8 * 3) * 4), ("pad", C.c_uint8 * 5)]


class OverlayTextLine(C.Structure):                                          # adas_overlay_text_line
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("slot", C.c_int32), ("color", C.c_uint8 * 3), ("len", C.c_uint8), ("text", C.c_char * 48)]


class OverlayTextArrays(C.Structure):                                        # adas_overlay_text_arrays
    _fields_ = [(n, C.c_void_p) for n in ("d_det_xyxy", "d_det_cls", "d_det_counts", "d_trk_tlwh", "d_trk_cls", "d_trk_ids", "d_trk_counts", "d_trk_last_tlbr",
                                          "d_traj_len", "d_dist_points", "d_dist_d", "d_dist_counts", "d_offset_type", "d_curvature_type",
                                          "d_collision_type")] + \
               [(n, C.c_int32) for n in ("det_cap", "trk_cap", "dist_cap", "reserved")]


TEXT_ITEM_DTYPE = np.dtype([("kind", "i4"), ("source", "i4"), ("x", "i4"), ("y", "i4"), ("x1", "i4"), ("y1", "i4"), ("box", "i4", (4,)), ("slot", "i4"),
                            ("color", "u1", (3,)), ("len", "u1"), ("text", "S48")])   # adas_overlay_text_item


class JpegParams(C.Structure):                                               # adas_jpeg_params
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("quality", C.c_int32), ("reserved", C.c_int32), ("capacity", C.c_int64)]


JPEG_OVERFLOW = 1                                                            # ADAS_JPEG_OVERFLOW
JPEG_SOURCES = {"overlay": 0, "frames": 1}                                   # ADAS_JPEG_SRC_*


class JpegDecParams(C.Structure):                                            # adas_jpegdec_params
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("reserved", C.c_int32 * 2), ("capacity", C.c_int64)]


JPEGDEC_UNSUPPORTED, JPEGDEC_FORMAT, JPEGDEC_SIZE, JPEGDEC_CORRUPT = 1, 2, 4, 8   # ADAS_JPEGDEC_*


class YuvParams(C.Structure):                                                # adas_yuv_params
    _fields_ = [("format", C.c_int32), ("matrix", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("frame_stride", C.c_int64),
                ("y_offset", C.c_int64), ("y_pitch", C.c_int64), ("u_offset", C.c_int64), ("u_pitch", C.c_int64), ("v_offset", C.c_int64),
                ("v_pitch", C.c_int64)]


YUV_FORMATS = {"nv12": 0, "nv21": 1, "i420": 2, "yuyv": 3, "uyvy": 4}             # ADAS_YUV_*
YUV_MATRICES = {"video": 0, "full": 1}                                       # ADAS_YUV_MATRIX_*
YUV_LAYOUT_FIELDS = ("frame_stride", "y_offset", "y_pitch", "u_offset", "u_pitch", "v_offset", "v_pitch")


class YuvOutParams(C.Structure):                                             # adas_yuvout_params: adas_yuv_params, then chroma
    _fields_ = list(YuvParams._fields_) + [("chroma", C.c_int32)]


YUVOUT_CHROMA = {"mean": 0, "first": 1}                                      # ADAS_YUVOUT_CHROMA_*
YUVOUT_SOURCES = {"overlay": 0, "frames": 1}                                 # ADAS_YUVOUT_SRC_*


class ScaleParams(C.Structure):                                              # adas_scale_params
    _fields_ = [("src_w", C.c_int32), ("src_h", C.c_int32), ("dst_w", C.c_int32), ("dst_h", C.c_int32), ("mode", C.c_int32), ("cols", C.c_int32),
                ("rows", C.c_int32), ("border", C.c_int32), ("background", C.c_uint8 * 4), ("border_bgr", (C.c_uint8 * 4) * 4)]


SCALE_MODES = {"area": 0, "linear": 1}                                       # ADAS_SCALE_*
SCALE_SOURCES = {"overlay": 0, "frames": 1}                                  # ADAS_SCALE_SRC_*


class RemapParams(C.Structure):                                              # adas_remap_params
    _fields_ = [("src_h", C.c_int), ("src_w", C.c_int), ("dst_h", C.c_int), ("dst_w", C.c_int), ("n_streams", C.c_int), ("n_maps", C.c_int)]


class RemapCamera(C.Structure):                                              # adas_remap_camera
    _fields_ = [("K", C.c_double * 4), ("D", C.c_double * 8), ("new_K", C.c_double * 4), ("R", C.c_double * 9)]


class BytetrackParams(C.Structure):
    _fields_ = [("track_thresh", C.c_double), ("match_thresh", C.c_double), ("frame_rate", C.c_double),
                ("track_buffer", C.c_int32), ("max_tracks", C.c_int32), ("max_dets", C.c_int32), ("reserved", C.c_int32)]


class TrackHeader(C.Structure):
    _fields_ = [("frame_id", C.c_int32), ("id_count", C.c_int32), ("n_tracked", C.c_int32), ("n_lost", C.c_int32),
                ("err", C.c_int32), ("pad", C.c_int32 * 3)]


class PipelineDesc(C.Structure):
    _fields_ = [("detector", C.c_void_p), ("lane", C.c_void_p), ("post", C.c_void_p), ("decode", C.c_void_p),
                ("tracker", C.c_void_p), ("n_streams", C.c_int32), ("use_graph", C.c_int32), ("geometry", C.c_void_p),
                ("micro_batch", C.c_int32), ("reserved", C.c_int32)]


class MlView(C.Structure):
    _fields_ = [("buf", C.c_uint64), ("cs", C.c_int32), ("coff", C.c_int32), ("c", C.c_int32), ("h", C.c_int32), ("w", C.c_int32)]


class MlLayerDesc(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("stride", C.c_int32), ("act", C.c_int32), ("res_mode", C.c_int32), ("up_c", C.c_int32), ("halo_bn", C.c_int32),
                ("x", MlView), ("y", MlView), ("res", MlView), ("up", MlView)]


TRACK_DTYPE = np.dtype([("tlwh", "f8", 4), ("score", "f8"), ("track_id", "i4"), ("state", "i4"), ("is_activated", "i4"),
                        ("class_id", "i4"), ("frame_id", "i4"), ("start_frame", "i4"), ("tracklet_len", "i4"), ("traj_len", "i4")])
TRAJECTORY_LEN = 30        # ADAS_TRAJECTORY_LEN

_P = C.c_void_p
_SIGS = {
    "adas_last_error": (C.c_char_p, []),
    "adas_version": (C.c_int, []),
    "adas_device_count": (C.c_int, []),
    "adas_set_device": (C.c_int, [C.c_int]),
    "adas_device_pci_bus_id": (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    "adas_malloc": (C.c_int, [C.POINTER(_P), C.c_size_t]),
    "adas_free": (C.c_int, [_P]),
    "adas_memcpy_h2d": (C.c_int, [_P, _P, C.c_size_t]),
    "adas_memcpy_d2h": (C.c_int, [_P, _P, C.c_size_t]),
    "adas_synchronize": (C.c_int, []),
    "adas_host_alloc": (C.c_int, [C.POINTER(_P), C.c_size_t]),
    "adas_host_free": (C.c_int, [_P]),
    "adas_timer_create": (C.c_int, [C.POINTER(_P)]),
    "adas_timer_destroy": (C.c_int, [_P]),
    "adas_timer_start": (C.c_int, [_P, _P]),
    "adas_timer_stop": (C.c_int, [_P, _P]),
    "adas_timer_elapsed_ms": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "adas_engine_create": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(_P)]),
    "adas_engine_destroy": (C.c_int, [_P]),
    "adas_engine_input_shape": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "adas_engine_num_outputs": (C.c_int, [_P]),
    "adas_engine_output_shape": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "adas_engine_output_name": (C.c_char_p, [_P, C.c_int]),
    "adas_engine_infer_host": (C.c_int, [_P, _P, C.c_int, C.POINTER(_P)]),
    "adas_engine_infer_device": (C.c_int, [_P, _P, C.c_int, _P]),
    "adas_engine_accepts_packed_input": (C.c_int, [_P]),
    "adas_engine_precision": (C.c_int, [_P]),
    "adas_engine_prepare": (C.c_int, [_P, C.c_int]),
    "adas_engine_ml_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "adas_engine_ml_status": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint32)]),
    "adas_engine_launch_count": (C.c_int, [_P, C.c_int]),
    "adas_engine_ml_counters": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_uint32)]),
    "adas_debug_ml_plan": (C.c_int, [C.POINTER(MlLayerDesc), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64),
                                     C.c_int, C.POINTER(C.c_int32)]),
    "adas_debug_conv_route": (C.c_int, [C.POINTER(MlLayerDesc), C.c_int, C.c_int, C.c_char_p, C.c_int]),
    "adas_debug_h8x3_onepass": (C.c_int, [C.POINTER(MlLayerDesc), C.c_int]),
    "adas_engine_plan": (C.c_int, [_P, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "adas_debug_engine_plan": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "adas_engine_schedule": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "adas_debug_engine_schedule": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_char_p,
                                             C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "adas_engine_model_io_half": (C.c_int, [_P]),
    "adas_engine_infer_device_packed": (C.c_int, [_P, _P, C.c_int, _P]),
    "adas_engine_output_device": (_P, [_P, C.c_int]),
    "adas_engine_stats": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "adas_engine_profile": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.POINTER(C.c_int)]),
    "adas_engine_layer_info": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "adas_engine_layer_kernel": (C.c_int, [_P, C.c_int, C.c_int, C.c_char_p, C.c_int]),
    "adas_engine_fetch_activation": (C.c_int, [_P, C.c_int, C.c_int, _P, C.POINTER(C.c_int64)]),
    "adas_preprocess_yolo": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
    "adas_preprocess_ufld": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_double, _P]),
    "adas_preprocess_yolo_packed": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
    "adas_preprocess_ufld_packed": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_double, _P]),
    "adas_preprocess_yolo_packed_prec": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "adas_preprocess_ufld_packed_prec": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_double, C.c_int, _P]),
    "adas_letterbox_params": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(YoloPostParams)]),
    "adas_yolo_post_create": (C.c_int, [C.POINTER(YoloPostParams), C.c_int, C.POINTER(_P)]),
    "adas_yolo_post_destroy": (C.c_int, [_P]),
    "adas_yolo_post_set_input_size": (C.c_int, [_P, C.c_int, C.c_int]),
    "adas_yolo_post_run": (C.c_int, [_P, _P, C.c_int, _P]),
    "adas_yolo_post_profile": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "adas_yolo_post_fetch": (C.c_int, [_P, C.c_int, C.POINTER(YoloCounts)] + [_P] * 9),
    "adas_yolo_post_fetch_dets": (C.c_int, [_P, C.c_int, C.POINTER(YoloCounts)] + [_P] * 5),
    "adas_yolo_post_device_views": (C.c_int, [_P] + [C.POINTER(_P)] * 4),
    "adas_yolo_post_scan_views": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "adas_yolo_post_run_prescanned": (C.c_int, [_P, _P, C.c_int, _P]),
    "adas_engine_detect_sink_supported": (C.c_int, [_P]),
    "adas_engine_detect_sink_shape": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "adas_engine_set_detect_sink": (C.c_int, [_P, _P, _P]),
    "adas_pipeline_detect_sink": (C.c_int, [_P]),
    "adas_yolo_post_capacity": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "adas_yolo_post_head_shape": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "adas_effdet_post_create": (C.c_int, [C.POINTER(EffdetPostParams), C.c_int, C.POINTER(_P)]),
    "adas_effdet_post_destroy": (C.c_int, [_P]),
    "adas_effdet_post_run": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _P]),
    "adas_effdet_post_fetch": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32), _P, _P, _P, _P]),
    "adas_effdet_tail_create": (C.c_int, [C.POINTER(EffdetTailParams), C.c_int, C.POINTER(_P)]),
    "adas_effdet_tail_destroy": (C.c_int, [_P]),
    "adas_effdet_tail_run": (C.c_int, [_P, _P, _P, C.c_int, _P]),
    "adas_effdet_tail_fetch": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32), _P, _P, _P, C.POINTER(C.c_int32)]),
    "adas_effdet_tail_device_views": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    "adas_preprocess_effdet": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
    "adas_ufld_decode_create": (C.c_int, [C.POINTER(UfldParams), C.c_int, C.POINTER(_P)]),
    "adas_ufld_decode_destroy": (C.c_int, [_P]),
    "adas_ufld_decode_run": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, _P]),
    "adas_ufld_decode_fetch": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "adas_ufld_decode_upload": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "adas_ufld1_decode_create": (C.c_int, [C.POINTER(Ufld1Params), C.c_int, C.POINTER(_P)]),
    "adas_ufld1_decode_set_source_size": (C.c_int, [_P, C.c_int, C.c_int]),
    "adas_ufld_decode_kind": (C.c_int, [_P]),
    "adas_ufld_decode_expected_outputs": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "adas_ufld1_decode_run": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P]),
    "adas_lane_geometry_create": (C.c_int, [C.POINTER(LaneGeometryParams), C.c_int, C.POINTER(_P)]),
    "adas_lane_geometry_destroy": (C.c_int, [_P]),
    "adas_lane_geometry_set_matrix": (C.c_int, [_P, _P]),
    "adas_lane_geometry_run": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "adas_lane_geometry_fetch": (C.c_int, [_P, C.c_int, C.POINTER(LaneGeometryResult), _P, _P]),
    "adas_lane_geometry_run_matrices": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "adas_warp_run_device_matrices": (C.c_int, [_P, _P, _P, _P, C.c_int, _P]),
    "adas_birdview_create": (C.c_int, [C.POINTER(BirdviewParams), C.c_int, C.c_int, C.POINTER(_P)]),
    "adas_birdview_destroy": (C.c_int, [_P]),
    "adas_birdview_reset": (C.c_int, [_P, C.c_int]),
    "adas_birdview_request": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "adas_birdview_run": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "adas_birdview_fetch_stream": (C.c_int, [_P, C.c_int, C.POINTER(BirdviewState)]),
    "adas_birdview_fetch_frame": (C.c_int, [_P, C.c_int, _P, _P, C.POINTER(C.c_int32)]),
    "adas_birdview_pending": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32)]),
    "adas_birdview_device_views": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "adas_pipeline_attach_birdview": (C.c_int, [_P, _P, _P]),
    "adas_pipeline_attach_analysis": (C.c_int, [_P, _P]),
    "adas_lane_geometry_device_views": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int32)]),
    "adas_analysis_default_params": (C.c_int, [C.POINTER(AnalysisParams)]),
    "adas_analysis_create": (C.c_int, [C.POINTER(AnalysisParams), C.c_int, C.c_int, C.POINTER(_P)]),
    "adas_analysis_destroy": (C.c_int, [_P]),
    "adas_analysis_reset": (C.c_int, [_P, C.c_int]),
    "adas_analysis_run": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "adas_analysis_run_arrays": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P]),
    "adas_analysis_run_inputs": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "adas_analysis_fetch_stream": (C.c_int, [_P, C.c_int, C.POINTER(AnalysisState)]),
    "adas_analysis_fetch_frame": (C.c_int, [_P, C.c_int, C.POINTER(AnalysisFrame)]),
    "adas_analysis_fetch_points": (C.c_int, [_P, C.c_int, _P, _P, C.c_int]),
    "adas_pipeline_request_transform": (C.c_int, [_P, C.c_int, C.c_int]),
    "adas_overlay_default_params": (C.c_int, [C.POINTER(OverlayParams)]),
    "adas_overlay_create": (C.c_int, [C.POINTER(OverlayParams), C.c_int, C.POINTER(_P)]),
    "adas_overlay_destroy": (C.c_int, [_P]),
    "adas_overlay_set_style": (C.c_int, [_P, C.POINTER(OverlayParams)]),
    "adas_overlay_run": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "adas_overlay_run_arrays": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "adas_overlay_run_objects": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "adas_overlay_run_arrays_objects": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P,
                                                  _P, C.c_int, _P, _P, _P, C.c_int, _P, _P, C.c_int, C.c_int, _P]),
    "adas_overlay_run_trajectories": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "adas_overlay_run_arrays_trajectories": (C.c_int, [_P, C.POINTER(OverlayArrays)]),
    "adas_overlay_fetch_track_marks": (C.c_int, [_P, C.c_int, _P, C.c_int, C.POINTER(C.c_int32)]),
    "adas_overlay_default_object_style": (C.c_int, [C.POINTER(OverlayObjectStyle)]),
    "adas_overlay_set_object_style": (C.c_int, [_P, C.POINTER(OverlayObjectStyle)]),
    "adas_overlay_set_class_colors": (C.c_int, [_P, C.c_int, _P, C.c_int]),
    "adas_overlay_fetch": (C.c_int, [_P, C.c_int, _P]),
    "adas_overlay_device_view": (C.c_int, [_P, C.POINTER(_P)]),
    "adas_overlay_fetch_flags": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32)]),
    "adas_overlay_default_panel_params": (C.c_int, [C.POINTER(OverlayPanelParams)]),
    "adas_overlay_set_panels": (C.c_int, [_P, C.POINTER(OverlayPanelParams), C.POINTER(OverlaySprite)]),
    "adas_overlay_run_panels": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "adas_overlay_run_panels_arrays": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "adas_overlay_reset_panels": (C.c_int, [_P, C.c_int]),
    "adas_overlay_fetch_panel_record": (C.c_int, [_P, C.c_int, C.POINTER(OverlayPanelRecord)]),
    "adas_pipeline_set_overlay_panels": (C.c_int, [_P, C.c_int]),
    "adas_overlay_default_text_style": (C.c_int, [C.POINTER(OverlayTextStyle)]),
    "adas_overlay_set_text_style": (C.c_int, [_P, C.POINTER(OverlayTextStyle)]),
    "adas_overlay_set_font": (C.c_int, [_P, C.c_int, C.POINTER(OverlayFont)]),
    "adas_overlay_set_text_labels": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.c_int]),
    "adas_overlay_set_text_lines": (C.c_int, [_P, C.POINTER(OverlayTextLine), C.c_int]),
    "adas_overlay_run_text_arrays": (C.c_int, [_P, _P, C.POINTER(OverlayTextArrays), C.c_int, C.c_int, C.c_int, _P]),
    "adas_overlay_run_text": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "adas_pipeline_set_overlay_text": (C.c_int, [_P, C.c_int]),
    "adas_overlay_fetch_text_items": (C.c_int, [_P, C.c_int, _P, C.c_int, C.POINTER(C.c_int32)]),
    "adas_overlay_fetch_text_flags": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32)]),
    "adas_overlay_default_readout_style": (C.c_int, [C.POINTER(OverlayReadoutStyle)]),
    "adas_overlay_set_readout_style": (C.c_int, [_P, C.POINTER(OverlayReadoutStyle)]),
    "adas_overlay_run_readouts": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "adas_overlay_run_arrays_readouts": (C.c_int, [_P, C.POINTER(OverlayArrays), C.POINTER(OverlayReadoutArrays)]),
    "adas_overlay_fetch_readout": (C.c_int, [_P, C.c_int, _P]),
    "adas_pipeline_set_overlay_readouts": (C.c_int, [_P, C.c_int]),
    "adas_lane_geometry_fetch_veh_pos": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double)]),
    "adas_jpeg_default_params": (C.c_int, [C.POINTER(JpegParams)]),
    "adas_jpeg_bound": (C.c_int64, [C.c_int, C.c_int]),
    "adas_jpeg_create": (C.c_int, [C.POINTER(JpegParams), C.c_int, C.POINTER(_P)]),
    "adas_jpeg_destroy": (C.c_int, [_P]),
    "adas_jpeg_set_quality": (C.c_int, [_P, C.c_int]),
    "adas_jpeg_run": (C.c_int, [_P, _P, C.c_int, _P]),
    "adas_jpeg_fetch": (C.c_int, [_P, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "adas_jpeg_fetch_lengths": (C.c_int, [_P, C.c_int, _P, _P]),
    "adas_jpeg_device_view": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int64)]),
    "adas_pipeline_attach_jpeg": (C.c_int, [_P, _P, C.c_int]),
    "adas_jpegdec_default_params": (C.c_int, [C.POINTER(JpegDecParams)]),
    "adas_jpegdec_create": (C.c_int, [C.POINTER(JpegDecParams), C.c_int, C.POINTER(_P)]),
    "adas_jpegdec_destroy": (C.c_int, [_P]),
    "adas_jpegdec_run": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P]),
    "adas_jpegdec_run_host": (C.c_int, [_P, _P, _P, C.c_int, _P, _P]),
    "adas_jpegdec_fetch": (C.c_int, [_P, C.c_int, _P]),
    "adas_jpegdec_fetch_flags": (C.c_int, [_P, C.c_int, _P]),
    "adas_jpegdec_device_view": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "adas_pipeline_attach_jpegdec": (C.c_int, [_P, _P]),
    "adas_yuv_default_params": (C.c_int, [C.POINTER(YuvParams), C.c_int, C.c_int, C.c_int]),
    "adas_yuv_frame_bytes": (C.c_int64, [C.POINTER(YuvParams)]),
    "adas_yuv_create": (C.c_int, [C.POINTER(YuvParams), C.c_int, C.POINTER(_P)]),
    "adas_yuv_destroy": (C.c_int, [_P]),
    "adas_yuv_run": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "adas_yuv_run_host": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "adas_yuv_fetch": (C.c_int, [_P, C.c_int, _P]),
    "adas_yuv_device_view": (C.c_int, [_P, C.POINTER(_P)]),
    "adas_yuvout_default_params": (C.c_int, [C.POINTER(YuvOutParams), C.c_int, C.c_int, C.c_int]),
    "adas_yuvout_frame_bytes": (C.c_int64, [C.POINTER(YuvOutParams)]),
    "adas_yuvout_create": (C.c_int, [C.POINTER(YuvOutParams), C.c_int, C.POINTER(_P)]),
    "adas_yuvout_destroy": (C.c_int, [_P]),
    "adas_yuvout_run": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "adas_yuvout_fetch": (C.c_int, [_P, C.c_int, _P]),
    "adas_yuvout_fetch_all": (C.c_int, [_P, C.c_int, _P]),
    "adas_yuvout_device_view": (C.c_int, [_P, C.POINTER(_P)]),
    "adas_pipeline_attach_yuvout": (C.c_int, [_P, _P, C.c_int]),
    "adas_scale_default_params": (C.c_int, [C.POINTER(ScaleParams), C.c_int, C.c_int, C.c_int, C.c_int]),
    "adas_scale_canvas_bytes": (C.c_int64, [C.POINTER(ScaleParams)]),
    "adas_scale_canvases": (C.c_int, [C.POINTER(ScaleParams), C.c_int]),
    "adas_scale_create": (C.c_int, [C.POINTER(ScaleParams), C.c_int, C.POINTER(_P)]),
    "adas_scale_destroy": (C.c_int, [_P]),
    "adas_scale_run": (C.c_int, [_P, _P, C.c_int, _P, C.c_int64, _P, _P]),
    "adas_scale_fetch": (C.c_int, [_P, C.c_int, _P]),
    "adas_scale_fetch_all": (C.c_int, [_P, C.c_int, _P]),
    "adas_scale_device_view": (C.c_int, [_P, C.POINTER(_P)]),
    "adas_pipeline_attach_scale": (C.c_int, [_P, _P, C.c_int]),
    "adas_pipeline_attach_scale_jpeg": (C.c_int, [_P, _P]),
    "adas_pipeline_attach_scale_yuvout": (C.c_int, [_P, _P]),
    "adas_remap_create": (C.c_int, [C.POINTER(RemapParams), C.c_int, C.POINTER(_P)]),
    "adas_remap_destroy": (C.c_int, [_P]),
    "adas_remap_set_camera": (C.c_int, [_P, C.c_int, C.POINTER(RemapCamera)]),
    "adas_remap_set_map": (C.c_int, [_P, C.c_int, _P, _P]),
    "adas_remap_assign": (C.c_int, [_P, C.c_int, C.c_int]),
    "adas_remap_fetch_map": (C.c_int, [_P, C.c_int, _P, _P]),
    "adas_remap_run": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "adas_remap_fetch": (C.c_int, [_P, C.c_int, _P]),
    "adas_remap_device_view": (C.c_int, [_P, C.POINTER(_P)]),
    "adas_pipeline_attach_remap": (C.c_int, [_P, _P]),
    "adas_pipeline_attach_yuv": (C.c_int, [_P, _P]),
    "adas_pipeline_step_yuv": (C.c_int, [_P, _P, C.c_double]),
    "adas_pipeline_step_yuv_host": (C.c_int, [_P, _P, C.c_double]),
    "adas_pipeline_step_jpeg_host": (C.c_int, [_P, _P, _P, C.c_double]),
    "adas_pipeline_graph_kernels": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "adas_pipeline_attach_overlay": (C.c_int, [_P, _P]),
    "adas_pipeline_set_overlay_stages": (C.c_int, [_P, C.c_int]),
    "adas_warp_create": (C.c_int, [C.POINTER(WarpParams), C.c_int, C.POINTER(_P)]),
    "adas_warp_destroy": (C.c_int, [_P]),
    "adas_warp_set_matrix": (C.c_int, [_P, C.c_int, _P, C.c_int]),
    "adas_warp_run": (C.c_int, [_P, _P, _P, C.c_int, _P]),
    "adas_warp_fetch": (C.c_int, [_P, C.c_int, _P]),
    "adas_warp_device_view": (C.c_int, [_P, C.POINTER(_P)]),
    "adas_bytetrack_create": (C.c_int, [C.POINTER(BytetrackParams), C.c_int, C.POINTER(_P)]),
    "adas_bytetrack_destroy": (C.c_int, [_P]),
    "adas_bytetrack_reset": (C.c_int, [_P, C.c_int]),
    "adas_bytetrack_update_host": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int]),
    "adas_bytetrack_update_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "adas_bytetrack_update_device_frames": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "adas_bytetrack_fetch": (C.c_int, [_P, C.c_int, C.POINTER(TrackHeader), _P, C.c_int]),
    "adas_bytetrack_fetch_trajectories": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.POINTER(C.c_int32)]),
    "adas_bytetrack_reserve_frames": (C.c_int, [_P, C.c_int, C.c_int]),
    "adas_bytetrack_fetch_frame": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(TrackHeader), _P, C.c_int]),
    "adas_pipeline_create": (C.c_int, [C.POINTER(PipelineDesc), C.POINTER(_P)]),
    "adas_pipeline_destroy": (C.c_int, [_P]),
    "adas_pipeline_step": (C.c_int, [_P, _P, _P]),
    "adas_pipeline_step_frames": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_double]),
    "adas_pipeline_step_frames_host": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_double]),
    "adas_pipeline_wait_upload": (C.c_int, [_P]),
    "adas_pipeline_sync": (C.c_int, [_P]),
    "adas_pipeline_timings": (C.c_int, [_P, C.POINTER(C.c_float)]),
}

_lib = None


def exported_symbols():
    return sorted(_SIGS)


def lib():
    """Load libadas_hip.so once and type its entry points.  Raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is not built; run `python vehicle-cv-adas_amd/build.py` "
                               "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)          # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(code):
    if code != 0:
        raise AdasError(code, lib().adas_last_error().decode("utf-8", "replace"))
    return code


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class DeviceBuffer:
    """A raw HBM allocation owned by Python (adas_malloc / adas_free)."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(lib().adas_malloc(C.byref(p), self.nbytes))
        self.ptr = p.value

    @classmethod
    def from_array(cls, arr):
        arr = np.ascontiguousarray(arr)
        b = cls(arr.nbytes)
        b.upload(arr)
        return b

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        check(lib().adas_memcpy_h2d(self.ptr, ptr(arr), arr.nbytes))

    def download(self, shape, dtype):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        check(lib().adas_memcpy_d2h(ptr(out), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().adas_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class StreamTimer:
    """hipEvents around work launched on `stream` (adas_timer_*): `with StreamTimer() as t: ...launches...; t.ms`."""

    def __init__(self, stream=None):
        self.stream = stream
        h = C.c_void_p()
        check(lib().adas_timer_create(C.byref(h)))
        self.h = h.value

    def __enter__(self):
        check(lib().adas_timer_start(self.h, self.stream))
        return self

    def __exit__(self, *exc):
        check(lib().adas_timer_stop(self.h, self.stream))
        return False

    @property
    def ms(self):
        v = C.c_float()
        check(lib().adas_timer_elapsed_ms(self.h, C.byref(v)))
        return float(v.value)

    def close(self):
        if getattr(self, "h", None):
            lib().adas_timer_destroy(self.h)
            self.h = None

    __del__ = close


class PinnedBuffer:
    """Page-locked host memory (adas_host_alloc) viewed as a NumPy array: frames that adas_pipeline_step_frames_host uploads
    asynchronously must live here for the copy to overlap the previous step."""

    def __init__(self, shape, dtype=np.uint8):
        self.shape, self.dtype = tuple(int(x) for x in shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        check(lib().adas_host_alloc(C.byref(p), self.nbytes))
        self.ptr = p.value
        self.array = np.ctypeslib.as_array((C.c_uint8 * self.nbytes).from_address(self.ptr)).view(self.dtype).reshape(self.shape)

    def free(self):
        if getattr(self, "ptr", None):
            self.array = None
            lib().adas_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
