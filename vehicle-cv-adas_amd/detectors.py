"""Drop-in equivalents of the reference's three per-frame task wrappers, GPU-resident end to end.

    YoloDetector              <- ObjectDetector/yoloDetector.py:53-157 (+ core.py RectInfo/ObjectDetectBase, utils.py Scaler/NMS)
    UltrafastLaneDetectorV2   <- TrafficLaneDetector/ufldDetector/ultrafastLaneDetectorV2.py:56-194 (+ core.py LaneInfo/LaneDetectBase)
    BYTETracker               <- ObjectTracker/byteTrack/byteTracker.py:10-200
    EfficientdetDetector      <- ObjectDetector/efficientdetDetector.py:18-111 (pre- and post-processing; the EfficientDet graph itself is
                                 not one of HipEngine's architectures: the class takes any EngineBase-conforming engine)

Same public surface (`_defaults` / `set_defaults`, `DetectFrame(frame)`, `.object_info`, `.lane_info`,
`update(bboxes, scores, class_ids, frame)`, `reset()`), but a frame makes one trip to the GPU: the BGR u8
frame is uploaded, letterbox/normalise (pre_kernels.hip), the network (MFMA conv engine), decode + NMS /
lane decode (post_kernels.hip) all run in HBM, and only the survivors (<= 2 KB) come back.
Of the reference's drawing, the lane detectors' `DrawDetectedOnFrame` / `DrawAreaOnFrame` run on the device (csrc/overlay_kernels.hip:
filled discs, the ego-lane polygon and the alpha blends, restated from OpenCV 4.5 with parity unpinned), and so do the BOXES of
`YoloDetector.DrawDetectedOnFrame` / `EfficientdetDetector.DrawDetectedOnFrame` (cornerRect: outline and corner arms in the class colour)
and of `BYTETracker.DrawTrackedOnFrame` (plot_bbox's rectangle and tint) and, with `BYTETracker(draw_trajectories=True)`, its trajectories
and direction marks (plot_trajectories' circles, plot_directions' lock-on rectangle or shadowed arrow).  Text, the label's background
rectangle, key points, DrawTransformFrontalViewArea's lines, the UI panels and everything else cv2 stay out of scope.

What stays on the host is what the reference keeps there and SURVEY 8a marks "host": RectInfo construction and
LaneDetectBase.__update_lanes_status/__update_lanes_area (core.py:102-158: ego-lane polyfit, <1 ms).
There is no CPU fallback for the compute path.
"""
import abc
import ctypes as C
import os
from dataclasses import dataclass, field
from enum import Enum
from typing import Any, Dict, List, Tuple

import numpy as np

from . import _lib as L
from .coreEngine import OnnxEngine, TensorRTEngine, EfficientdetEngine
from .postproc import YoloPost, EffdetPost, UfldDecode, Ufld1Decode, LaneGeometry, DeviceTracker, OverlayPainter, letterbox


class ObjectModelType(Enum):       # ObjectDetector/utils.py:15-23
    YOLOV5 = 0
    YOLOV5_LITE = 1
    YOLOV6 = 2
    YOLOV7 = 3
    YOLOV8 = 4
    YOLOV9 = 5
    YOLOV10 = 6
    EfficientDet = 7


class LaneModelType(Enum):         # ufldDetector/utils.py:3-8
    UFLD_TUSIMPLE = 0
    UFLD_CULANE = 1
    UFLDV2_TUSIMPLE = 2
    UFLDV2_CULANE = 3
    UFLDV2_CURVELANES = 4


@dataclass
class RectInfo:                    # ObjectDetector/core.py:8-33
    x: float
    y: float
    width: float
    height: float
    conf: float
    label: str
    kpss: List[Tuple[int, int]] = field(default_factory=list)

    def tolist(self, dtype=int, format_type: str = "xyxy"):
        if format_type == "xyxy":
            temp = [self.x, self.y, self.x + self.width, self.y + self.height]
        else:
            temp = [self.x, self.y, self.width, self.height]
        return list(map(dtype, temp))

    def pad(self, padding: int) -> "RectInfo":
        return RectInfo(x=self.x - padding, y=self.y - padding, width=self.width + 2 * padding,
                        height=self.height + 2 * padding, conf=self.conf, label=self.label, kpss=self.kpss)


class _Defaults:
    """set_defaults / check_defaults / get_defaults of ObjectDetectBase and LaneDetectBase (core.py:36-55)."""
    _defaults: Dict[str, Any] = {}

    @classmethod
    def set_defaults(cls, config):
        cls._defaults = config

    @classmethod
    def check_defaults(cls):
        return cls._defaults

    @classmethod
    def get_defaults(cls, n):
        if n in cls._defaults:
            return cls._defaults[n]
        return "Unrecognized attribute name '" + n + "'"


def _engine_for(model_path, **kw):
    """Suffix dispatch of yoloDetector.py:74-77 / ultrafastLaneDetectorV2.py:82-85 (both names are HipEngine here)."""
    model_path = os.path.expanduser(model_path)
    return TensorRTEngine(model_path, **kw) if model_path.endswith('.trt') else OnnxEngine(model_path, **kw)


def _colors_dict(class_names):
    """label -> colour, what yoloDetector.py:93-94 ends up with: one 24-bit random number per label, its three bytes from the top down."""
    import random
    out = {}
    for label in class_names:
        v = random.randint(0, 0xFFFFFF)
        out[label] = ((v >> 16) & 0xFF, (v >> 8) & 0xFF, v & 0xFF)
    return out


class _DrawsBoxes:
    """DrawDetectedOnFrame of the two object detectors (yoloDetector.py:170-191, the same in efficientdetDetector.py) on the device: the
    cornerRect of every RectInfo, in _object_info order, in colors_dict[label] -- (0, 0, 0) for 'unknown'.  The label and its background
    rectangle are drawn once set_text_fonts has been given glyph atlases (none: the boxes only); the key points are NOT drawn.  `frame_show` is an HxWx3 uint8 ndarray (uploaded, drawn, copied
    back into frame_show[:]) or a StagedFrame (drawn where it sits).  OpenCV's thick line restated (csrc/overlay_core.h D6), parity unpinned."""

    def DrawDetectedOnFrame(self, frame_show) -> None:
        if len(self._object_info) == 0:
            return
        if getattr(self, "_painter", None) is None:
            self._painter = OverlayPainter()
        boxes = [info.tolist() for info in self._object_info]
        colors = [self.colors_dict[info.label] if info.label != 'unknown' else (0, 0, 0) for info in self._object_info]
        self._painter.detections(frame_show, boxes, list(range(len(boxes))), colors)
        if getattr(self, "text_fonts", None):      # set_text_fonts: the label on its filled background, over the boxes
            self._painter.text(frame_show, "detections", self.text_fonts, self.text_style, det_boxes=boxes,
                               det_names=[info.label for info in self._object_info], det_colors=colors)

    def set_text_fonts(self, fonts, **style):
        """fonts: {slot: atlas} (postproc.LaneOverlay.set_fonts; tools/make_font_atlas.py) -- DrawDetectedOnFrame then also draws every
        label on its filled background (yoloDetector.py:180-191) from the style's det_size_slot / det_label_slot; None: the boxes only, as
        before.  style: fields of adas_overlay_text_style (EfficientDet's offsets are its class default)."""
        self.text_fonts = fonts
        self.text_style = dict(getattr(self, "TEXT_STYLE", {}), **style)

    def _close_painter(self):
        if getattr(self, "_painter", None) is not None:
            self._painter.close()
            self._painter = None


class StagedFrame:
    """A BGR u8 frame that already sits in HBM: what `detector.staged_frame` hands out after a DetectFrame, so that the next task class
    of the same loop iteration (demo.py:269,280 pass the SAME frame to the object and the lane detector) does not upload its 2.7 MB
    again: `lane.DetectFrame(det.staged_frame)`.  Valid until the owning detector's next DetectFrame (or close)."""
    __slots__ = ("ptr", "height", "width", "serial")

    def __init__(self, ptr, height, width, serial):
        self.ptr, self.height, self.width, self.serial = ptr, int(height), int(width), serial

    @property
    def shape(self):
        return (self.height, self.width, 3)


class _FrameStage:
    """Device staging of one BGR u8 frame + the network input tensor it is turned into."""
    _serial = 0

    def __init__(self):
        self.frame = None
        self.tensor = None
        self.staged = None

    def upload(self, img):
        """-> (device pointer of the frame, height, width).  A StagedFrame (another detector's upload of this frame) is used in place."""
        if isinstance(img, StagedFrame):
            self.staged = img
            return img.ptr, img.height, img.width
        img = np.ascontiguousarray(img, dtype=np.uint8)
        if img.ndim != 3 or img.shape[2] != 3:
            raise Exception("frame must be an HxWx3 uint8 BGR image, got %s" % (img.shape,))
        if self.frame is None or self.frame.nbytes < img.nbytes:
            if self.frame is not None:
                self.frame.free()
            self.frame = L.DeviceBuffer(img.nbytes)
        self.frame.upload(img)
        _FrameStage._serial += 1
        self.staged = StagedFrame(self.frame.ptr, img.shape[0], img.shape[1], _FrameStage._serial)
        return self.frame.ptr, img.shape[0], img.shape[1]

    def tensor_for(self, shape):
        n = int(np.prod(shape)) * 4
        if self.tensor is None or self.tensor.nbytes < n:
            if self.tensor is not None:
                self.tensor.free()
            self.tensor = L.DeviceBuffer(n)
        return self.tensor

    def close(self):
        for b in (self.frame, self.tensor):
            if b is not None:
                b.free()
        self.frame = self.tensor = self.staged = None


# =====================================================================================
MAX_LDS_CANDIDATES = 2048      # candidate arenas up to this size live in LDS; larger ones (up to one per anchor) in HBM (post_kernels.hip)


class YoloDetector(_Defaults, _DrawsBoxes):
    _defaults = {
        "model_path": './models/yolov5n-coco.onnx',
        "model_type": ObjectModelType.YOLOV5,
        "classes_path": './models/coco_label.txt',
        "box_score": 0.4,
        "box_nms_iou": 0.45,
    }
    V8_LIKE = (ObjectModelType.YOLOV8, ObjectModelType.YOLOV9, ObjectModelType.YOLOV10)   # yoloDetector.py:114,121

    def __init__(self, logger=None, **kwargs):
        self.__dict__.update(self._defaults)
        self.logger = logger
        self.precision = None                    # None -> coreEngine.DEFAULT_PRECISION: the exact mode (fp16x3); "fp16" = throughput mode
        self.nms_mode = L.NMS_REFERENCE          # the production call (yoloDetector.py:139); NMS_GREEDY = fast_nms (:138)
        self.max_candidates = 1024
        self.__dict__.update(kwargs)
        if self.model_type == ObjectModelType.EfficientDet:
            raise Exception("%s heads are not implemented by HipEngine (SURVEY.md 8f row f4)" % self.model_type.name)
        self._initialize_class(self.classes_path)
        self._initialize_model(self.model_path)
        self._stage = _FrameStage()
        self._post = None
        self._post_key = None
        self._object_info = []
        self._last_full = None

    @property
    def staged_frame(self):
        """The last frame's device copy (StagedFrame), to hand to the other task classes of the same loop iteration."""
        return self._stage.staged

    def _initialize_model(self, model_path: str) -> None:
        self.engine = _engine_for(model_path, precision=self.precision)
        if self.logger:
            self.logger.info(f'YoloDetector Type : [{self.engine.framework_type}] || Version : [{self.engine.providers}]')
        self.input_shapes = self.engine.get_engine_input_shape()                 # core.py:73-82
        self.input_types = self.engine.engine_dtype
        self.channes, self.input_height, self.input_width = self.input_shapes[1:]
        self.output_shapes, self.output_names = self.engine.get_engine_output_shape()

    def _initialize_class(self, classes_path: str) -> None:
        classes_path = os.path.expanduser(classes_path)
        assert os.path.isfile(classes_path), Exception("%s is not exist." % classes_path)
        with open(classes_path) as f:
            self.class_names = [c.strip() for c in f.readlines()]
        self.colors_dict = _colors_dict(self.class_names)

    @property
    def object_info(self):
        return self._object_info

    @property
    def _last(self):
        """Everything the post-processor holds for the last frame (candidates too; the tests compare them with the oracle): fetched on
        demand, once per frame -- DetectFrame itself only brings the survivors over."""
        if self._post is None:
            raise Exception("YoloDetector: no frame has been processed yet")
        if self._last_full is None:
            self._last_full = self._post.fetch(0)
        return self._last_full

    def _post_for(self, src_hw):
        key = (int(src_hw[0]), int(src_hw[1]))
        if self._post_key != key:
            if self._post is not None:
                self._post.close()
            shp = self.output_shapes[0]
            v8 = self.model_type in self.V8_LIKE
            A, no = (shp[2], shp[1]) if v8 else (shp[1], shp[2])
            nc = no - 4 if v8 else no - 5
            lb = letterbox(key, self.input_shapes[-2:])
            lite = self.model_type == ObjectModelType.YOLOV5_LITE      # yoloDetector.py:21-22,116
            layout = L.HEAD_V8 if v8 else (L.HEAD_V5_LITE if lite else L.HEAD_V5)
            self._post = YoloPost(layout, A, nc, float(self.box_score), float(self.box_nms_iou), lb, self.nms_mode,
                                  self.max_candidates, 1, input_hw=tuple(self.input_shapes[-2:]) if lite else None)
            self._post_key = key
        return self._post

    def DetectFrame(self, srcimg) -> None:
        """yoloDetector.py:159-168 with every step on the device."""
        fptr, h, w = self._stage.upload(srcimg)
        self._last_full = None
        t = self._stage.tensor_for(self.input_shapes)
        L.check(L.lib().adas_preprocess_yolo(fptr, 1, h, w, t.ptr, self.input_height, self.input_width, 1, None))
        self.engine.infer_device(t.ptr, 1, None)
        post = self._post_for((h, w))
        post.run_device(self.engine.output_device_ptr(0), 1, None)
        r = post.fetch_dets(0)                 # one packed message: counts + survivors
        # The reference's candidate lists are unbounded (yoloDetector.py:120-133).  A frame with more anchors over box_score than the
        # arena holds is re-run with a larger arena (the head tensor is still in HBM): up to one slot per anchor, at which point nothing
        # can overflow -- arenas past MAX_LDS_CANDIDATES work out of an HBM workspace (slower, same results).
        limit = int(post.params.num_anchors)
        while r["overflow"] and self.max_candidates < limit:
            self.max_candidates = min(limit, max(2 * self.max_candidates, int(r["n_found"])))
            self._post_key = None
            post = self._post_for((h, w))
            post.run_device(self.engine.output_device_ptr(0), 1, None)
            r = post.fetch_dets(0)
        if r["overflow"]:
            raise RuntimeError("YoloDetector: %d anchors over box_score with a %d-candidate arena of %d anchors" % (r["n_found"], self.max_candidates, limit))
        elif r["rc"] != 0:
            L.check(r["rc"])
        self._last_dets = r
        out = []
        for (x, y, bw, bh), conf, cid in zip(r["xywh"], r["conf"], r["class_id"]):     # get_nms_results (:141-157)
            label = self.class_names[cid] if 0 <= cid < len(self.class_names) else "unknown"
            out.append(RectInfo(np.float64(x), np.float64(y), np.float64(bw), np.float64(bh), conf=float(conf), label=label, kpss=[]))
        self._object_info = out

    def close(self):
        self._close_painter()
        if getattr(self, "_post", None) is not None:
            self._post.close()
            self._post = None
        if getattr(self, "_stage", None) is not None:
            self._stage.close()
        if getattr(self, "engine", None) is not None:
            self.engine.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# =====================================================================================
class EfficientdetDetector(_Defaults, _DrawsBoxes):
    """efficientdetDetector.py:18-111.  The exported EfficientDet graph carries its own decode + NMS; around it the reference does
    letterbox + BGR mean/std normalisation (:57-65) and inverse letterbox + score filter + label lookup (:67-85).  Both run on the
    device here (adas_preprocess_effdet, adas_effdet_post_*).  The graph itself is coreEngine.EfficientdetEngine: an EfficientDet-D0 .. D3
    network (models.efficientdet: EfficientNet-B0 .. B3 MBConv + squeeze-and-excitation, BiFPN, separable-conv heads -- the reference's
    "efficientDet b0/b1/b2/b3") and the in-graph tail (anchor decode + per-class NMS, adas_effdet_tail_*) on the device -- `model_path` is
    an "efficientdet-d0" .. "efficientdet-d3" .hipm container, whose input size (512 / 640 / 768 / 896) the detector takes over; or pass
    `engine=`, any object with the EngineBase surface (get_engine_input_shape / get_engine_output_shape / engine_inference /
    engine_dtype).  An EfficientDet .onnx with its NMS baked in is not importable (onnx_import fails loudly), which is why the default
    `model_path` names a .hipm container and not the reference's './models/efficientdet-d0-coco_fp32.onnx' (efficientdetDetector.py:22).

    PADDING CAVEAT: models.efficientdet builds the PyTorch-native variant of the architecture -- symmetric k // 2 padding on every
    stride-2 conv, depth-wise conv and BiFPN max-pool.  The public TF-derived checkpoints / exports use static 'same' padding (stride 2 pads
    right and bottom only); pouring THOSE weights into this graph would shift every feature map by about a pixel per stride-2 stage against
    the anchor grid.  Valid weights for this container are the seeded synthetic ones (models.py) or a network trained with symmetric
    padding; no importer for the public checkpoint exists."""
    TEXT_STYLE = dict(det_label_dx=0, det_label_dy=-5)      # efficientdetDetector.py:110

    _defaults = {
        "model_path": './models/efficientdet-d0.hipm',
        "model_type": ObjectModelType.EfficientDet,
        "classes_path": './models/coco_label.txt',
        "box_score": 0.6,
    }

    def __init__(self, logger=None, engine=None, **kwargs):
        self.__dict__.update(self._defaults)
        self.logger = logger
        self.max_boxes = 256
        self.__dict__.update(kwargs)
        classes_path = os.path.expanduser(self.classes_path)
        assert os.path.isfile(classes_path), Exception("%s is not exist." % classes_path)
        with open(classes_path) as f:
            self.class_names = [c.strip() for c in f.readlines()]
        self.colors_dict = _colors_dict(self.class_names)
        # the in-graph tail's own parameters (what an exporter bakes into the graph): overridable like any other default
        self.engine = engine if engine is not None else EfficientdetEngine(
            os.path.expanduser(self.model_path), precision=getattr(self, "precision", None), score_thr=float(getattr(self, "graph_score_thr", 0.05)),
            iou_thr=float(getattr(self, "graph_nms_iou", 0.5)), max_det=int(getattr(self, "graph_max_det", 100)),
            max_candidates=int(getattr(self, "graph_max_candidates", 2048)))
        self.input_shapes = self.engine.get_engine_input_shape()                 # core.py:73-82
        self.input_types = self.engine.engine_dtype
        self.channes, self.input_height, self.input_width = self.input_shapes[1:]
        self.output_shapes, self.output_names = self.engine.get_engine_output_shape()
        self._stage = _FrameStage()
        self._post = None
        self._post_key = None
        self._object_info = []

    @property
    def object_info(self):
        return self._object_info

    @property
    def staged_frame(self):
        """The last frame's device copy (StagedFrame), to hand to the other task classes of the same loop iteration."""
        return self._stage.staged

    def DetectFrame(self, srcimg) -> None:
        fptr, h, w = self._stage.upload(srcimg)
        t = self._stage.tensor_for(self.input_shapes)
        L.check(L.lib().adas_preprocess_effdet(fptr, 1, h, w, t.ptr, self.input_height, self.input_width, 1, None))
        x = t.download((1, 3, self.input_height, self.input_width), np.float32).astype(self.input_types)
        out = self.engine.engine_inference(x)                                    # boxes, class ids, confidences (:68-70)
        key = (h, w)
        if self._post_key != key:
            if self._post is not None:
                self._post.close()
            self._post = EffdetPost(float(self.box_score), letterbox(key, self.input_shapes[-2:]), self.max_boxes, 1)
            self._post_key = key
        r = self._post.run_host([(np.asarray(out[0]).reshape(-1, 4), np.asarray(out[1]).reshape(-1), np.asarray(out[2]).reshape(-1))])[0]
        self._last = r
        info = []
        for (x0, y0, bw, bh), conf, cid in zip(r["xywh"], r["conf"], r["class_id"]):
            try:
                label = self.class_names[int(cid)]        # Python indexing, as there: a negative id wraps, one past the end is "unknown"
            except Exception:
                label = "unknown"
            info.append(RectInfo(np.float32(x0), np.float32(y0), np.float32(bw), np.float32(bh), conf=np.float32(conf), label=label))
        self._object_info = info

    def close(self):
        self._close_painter()
        if getattr(self, "_post", None) is not None:
            self._post.close()
            self._post = None
        if getattr(self, "_stage", None) is not None:
            self._stage.close()
        eng = getattr(self, "engine", None)
        if eng is not None and hasattr(eng, "close"):
            eng.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# =====================================================================================
@dataclass
class LaneInfo:                    # ufldDetector/core.py:7-50
    _lanes_points: np.ndarray
    _lanes_status: Any
    _area_points: np.ndarray
    _area_status: bool

    @property
    def lanes_points(self):
        return self._lanes_points

    @lanes_points.setter
    def lanes_points(self, arr):
        if isinstance(arr, np.ndarray):
            self._lanes_points = arr
        else:
            raise Exception("The 'lanes_points' must be np.array[List[Tuple[x, y], ...], ...].")

    @property
    def lanes_status(self):
        return self._lanes_status

    @lanes_status.setter
    def lanes_status(self, value):
        for v in value:
            if type(v) != bool:
                raise Exception("The elements of 'lanes_status' must be of type bool List[bool, ...].")
        self._lanes_status = value

    @property
    def area_status(self):
        return self._area_status

    @area_status.setter
    def area_status(self, value):
        raise Exception("You need to use the '__update_lanes_status' API to modify it.")

    @property
    def area_points(self):
        return self._area_points

    @area_points.setter
    def area_points(self, value):
        raise Exception("You need to use the '__update_lanes_area' API to modify it.")


class ModelConfig:                 # ultrafastLaneDetectorV2.py:21-55
    def __init__(self, model_type):
        if model_type == LaneModelType.UFLDV2_TUSIMPLE:
            self.img_w, self.img_h, self.griding_num, self.crop_ratio = 800, 320, 100, 0.8
            self.row_anchor = np.linspace(160, 710, 56) / 720
            self.col_anchor = np.linspace(0, 1, 41)
        elif model_type == LaneModelType.UFLDV2_CURVELANES:
            self.img_w, self.img_h, self.griding_num, self.crop_ratio = 1600, 800, 200, 0.8
            self.row_anchor = np.linspace(0.4, 1, 72)
            self.col_anchor = np.linspace(0, 1, 81)
        else:
            self.img_w, self.img_h, self.griding_num, self.crop_ratio = 1600, 320, 200, 0.6
            self.row_anchor = np.linspace(0.42, 1, 72)
            self.col_anchor = np.linspace(0, 1, 81)
        self.num_lanes = 4


def _ego_lane_fit(points, min_points=10):
    """(quadratic x(y) coefficients, y samples) of one ego lane, or None when the lane carries too few points to refit."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    if pts.shape[0] <= min_points:
        return None
    return np.polyfit(pts[:, 1], pts[:, 0], 2), pts[:, 1]


def adjust_lanes_points(left_lanes_points, right_lanes_points, image_height):
    """Ego-lane smoothing of the drivable-area polygon: each ego lane is replaced by its least-squares parabola x(y),
    sampled at `image_height` rows spanning both lanes.  Same results as LaneDetectBase.__adjust_lanes_points
    (ufldDetector/core.py:102-141): either lane with <= 10 points leaves both untouched; the common row range starts at
    min(H // 3, lowest lane row) and ends at max(H - 1, highest lane row); a sample is kept from the lane's first row down and
    only while x >= 0; coordinates are truncated.  (The device path is lane_core.h; this is the host form.)"""
    fits = [_ego_lane_fit(left_lanes_points), _ego_lane_fit(right_lanes_points)]
    if fits[0] is None or fits[1] is None:
        return left_lanes_points, right_lanes_points
    rows = np.concatenate([fits[0][1], fits[1][1]])
    lo = min(image_height // 3, rows.min())
    hi = max(image_height - 1, rows.max())
    ys = np.linspace(lo, hi, image_height)
    resampled = []
    for (c2, c1, c0), lane_rows in fits:
        xs = c2 * ys ** 2 + c1 * ys + c0
        sel = (ys >= lane_rows.min()) & (xs >= 0)
        # int() truncation of the reference == astype toward zero for these magnitudes
        resampled.append(list(zip(xs[sel].astype(np.int64).tolist(), ys[sel].astype(np.int64).tolist())))
    return resampled[0], resampled[1]


class UltrafastLaneDetectorV2(_Defaults):
    _defaults = {
        "model_path": "models/culane_res18.onnx",
        "model_type": LaneModelType.UFLDV2_TUSIMPLE,
    }

    def __init__(self, model_path: str = None, model_type: LaneModelType = None, logger=None, precision=None):
        self.__dict__.update(self._defaults)
        self.logger = logger
        self.adjust_lanes = False
        self.lane_info = LaneInfo(np.array([], dtype=object), np.array([], dtype=object), np.array([], dtype=object), False)
        if None not in [model_path, model_type]:
            self.model_path, self.model_type = model_path, model_type
        # The reference class rejects everything but Tusimple / CULane (ultrafastLaneDetectorV2.py:69-72) although its ModelConfig
        # carries a CurveLanes entry (:41-47) and exportLib ships the CurveLanes configs; that model type is accepted here (a
        # superset: the engine + decoder handle its 800x1600 input and 10-lane heads), any other type fails as in the reference.
        if self.model_type not in [LaneModelType.UFLDV2_TUSIMPLE, LaneModelType.UFLDV2_CULANE, LaneModelType.UFLDV2_CURVELANES]:
            raise Exception("UltrafastLaneDetectorV2 can't use %s type." % self.model_type.name)
        self.cfg = ModelConfig(self.model_type)
        self.precision = precision
        self._initialize_model(self.model_path)
        self._stage = _FrameStage()
        self._decode = None
        self._decode_key = None

    def _initialize_model(self, model_path: str) -> None:
        self.engine = _engine_for(model_path, precision=self.precision)
        if self.logger:
            self.logger.info(f'UfldDetectorV2 Type : [{self.engine.framework_type}] || Version : [{self.engine.providers}]')
        self.input_shape = self.engine.get_engine_input_shape()
        self.input_types = self.engine.engine_dtype
        self.channes, self.input_height, self.input_width = self.input_shape[1:]
        self.output_shape, self.output_names = self.engine.get_engine_output_shape()
        if len(self.output_names) != 4:
            raise Exception("Output dims is error, please check model. load %d channels not match 4." % len(self.output_names))

    @property
    def staged_frame(self):
        """The last frame's device copy (StagedFrame), to hand to the other task classes of the same loop iteration."""
        return self._stage.staged

    def _decode_for(self, img_hw):
        key = (int(img_hw[0]), int(img_hw[1]))
        if self._decode_key != key:
            if self._decode is not None:
                self._decode.close()
            lr, lc = self.output_shape[0], self.output_shape[1]
            self._decode = UfldDecode(lr[1], lr[2], lc[1], lc[2], key[1], key[0], self.cfg.row_anchor, self.cfg.col_anchor, 1, 1,
                                      num_lanes=lr[3])
            self._decode_key = key
        return self._decode

    def DetectFrame(self, image, adjust_lanes: bool = True) -> None:
        """ultrafastLaneDetectorV2.py:183-194."""
        fptr, h, w = self._stage.upload(image)
        self.img_height, self.img_width, self.img_channels = h, w, 3
        t = self._stage.tensor_for(self.input_shape)
        L.check(L.lib().adas_preprocess_ufld(fptr, 1, h, w, t.ptr, self.input_height, self.input_width,
                                             float(self.cfg.crop_ratio), None))
        self.engine.infer_device(t.ptr, 1, None)
        dec = self._decode_for((h, w))
        ptrs = [self.engine.output_device_ptr(i) for i in range(4)]
        strides = [int(np.prod(s[1:])) for s in self.output_shape]
        dec.run_device(ptrs, strides, 1, None)
        lanes, status = dec.fetch(0)
        self.lane_info.lanes_points = np.array(lanes + [None], dtype=object)[:4]      # ragged-safe object array of 4 lists
        self.lane_info.lanes_status = [bool(s) for s in status]
        self.adjust_lanes = adjust_lanes
        if self._device_geometry(dec, h, w):
            return
        self.__update_lanes_status(self.lane_info.lanes_status)
        self.__update_lanes_area(self.lane_info.lanes_points, self.img_height)

    # ---- optional: area polygon, bird-view points, curvature and offset straight from the decoder's device buffers
    def enable_device_geometry(self, transform_view) -> None:
        """transform_view: a PerspectiveTransformation (analysis.py); its current M is read at every DetectFrame.  After
        DetectFrame, `lane_info.area_*` come from the device and `birdview_lanes_points` / `curve_and_offset` hold what
        demo.py:290-291 computes with transformToBirdViewPoints / calcCurveAndOffset."""
        self._transform_view = transform_view
        self._geometry = None
        self._geometry_key = None
        self.birdview_lanes_points = [[], [], [], []]
        self.curve_and_offset = ((None, None), None)

    def _device_geometry(self, dec, h, w) -> bool:
        tv = getattr(self, "_transform_view", None)
        if tv is None:
            return False
        key = (h, tuple(tv.img_size))
        if self._geometry_key != key:
            if self._geometry is not None:
                self._geometry.close()
            self._geometry = LaneGeometry(h, tv.img_size, tv.M, self.adjust_lanes, 1)
            self._geometry_key = key
        self._geometry.set_matrix(tv.M)
        self._geometry.run(dec, self.adjust_lanes, 1, None)
        r = self._geometry.fetch(0)
        self.lane_info._area_status = r["area_status"]
        self.lane_info._area_points = r["area_points"].astype(np.int64) if r["area_status"] else np.array([], dtype=object)
        self.birdview_lanes_points = [p if len(p) else [] for p in r["bird_points"]]
        self.curve_and_offset = ((r["direction"], r["curvature"]), r["offset"])
        return True

    def __update_lanes_status(self, lanes_status) -> None:          # core.py:143-148
        self.lane_info._area_status = False
        if lanes_status != [] and len(lanes_status) % 2 == 0:
            index = len(lanes_status) // 2
            if lanes_status[index - 1] and lanes_status[index]:
                self.lane_info._area_status = True

    def __update_lanes_area(self, lanes_points, img_height) -> None:  # core.py:150-158
        self.lane_info._area_points = np.array([], dtype=object)
        if self.lane_info._area_status:
            index = len(lanes_points) // 2
            if self.adjust_lanes:
                l, r = adjust_lanes_points(lanes_points[index - 1], lanes_points[index], img_height)
            else:
                l, r = lanes_points[index - 1], lanes_points[index]
            self.lane_info._area_points = np.vstack((l, np.flipud(r)))

    # ---- drawing: the reference's two methods on the device (postproc.LaneOverlay), in place on `image` as the reference writes image[:]
    def DrawDetectedOnFrame(self, image, type=None, alpha: float = 0.3) -> None:
        """ultrafastLaneDetectorV2.py:196-209: a disc of radius 3 on every point of lane_info.lanes_points, lane by lane in lane_colors
        (lane 1 red when `type` is OffsetType.RIGHT, lane 2 when LEFT), blended over the image at `alpha`.  image: HxWx3 uint8 ndarray
        (written in place) or a StagedFrame (drawn where it sits in HBM)."""
        if getattr(self, "_painter", None) is None:
            self._painter = OverlayPainter()
        self._painter.lanes(image, self.lane_info.lanes_points, type, alpha)

    def DrawAreaOnFrame(self, image, color: tuple = (255, 191, 0), alpha: float = 0.85) -> None:
        """ultrafastLaneDetectorV2.py:211-218: lane_info.area_points filled (cv2.fillPoly) in `color` and blended at `alpha`, when
        lane_info.area_status."""
        if not self.lane_info.area_status:
            return
        if getattr(self, "_painter", None) is None:
            self._painter = OverlayPainter()
        self._painter.area(image, self.lane_info.area_points, color, alpha)

    def close(self):
        if getattr(self, "_painter", None) is not None:
            self._painter.close()
            self._painter = None
        if getattr(self, "_geometry", None) is not None:
            self._geometry.close()
            self._geometry = None
        if getattr(self, "_decode", None) is not None:
            self._decode.close()
            self._decode = None
        if getattr(self, "_stage", None) is not None:
            self._stage.close()
        if getattr(self, "engine", None) is not None:
            self.engine.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ModelConfigV1:               # ultrafastLaneDetector.py:16-40
    def __init__(self, model_type):
        if model_type == LaneModelType.UFLD_TUSIMPLE:
            self.img_w, self.img_h, self.griding_num, self.cls_num_per_lane = 1280, 720, 100, 56
            self.row_anchor = np.linspace(64, 284, self.cls_num_per_lane)
        else:
            self.img_w, self.img_h, self.griding_num, self.cls_num_per_lane = 1640, 590, 200, 18
            self.row_anchor = [round(value) for value in np.linspace(121, 287, self.cls_num_per_lane)]
        self.num_lanes = 4


class UltrafastLaneDetector(UltrafastLaneDetectorV2):
    """UFLD (v1) drop-in: ultrafastLaneDetector.py:42-139 with pre-processing, network and decode on the device.
    Pre-processing is the v2 kernel with crop_ratio 1 (plain resize to 800x288 + ImageNet normalisation, :79-94)."""
    _defaults = {
        "model_path": "models/tusimple_18.onnx",
        "model_type": LaneModelType.UFLD_TUSIMPLE,
    }

    def __init__(self, model_path: str = None, model_type: LaneModelType = None, logger=None, precision=None):
        self.__dict__.update(self._defaults)
        self.logger = logger
        self.adjust_lanes = False
        self.lane_info = LaneInfo(np.array([], dtype=object), np.array([], dtype=object), np.array([], dtype=object), False)
        if None not in [model_path, model_type]:
            self.model_path, self.model_type = model_path, model_type
        if self.model_type not in [LaneModelType.UFLD_TUSIMPLE, LaneModelType.UFLD_CULANE]:
            raise Exception("UltrafastLaneDetector can't use %s type." % self.model_type.name)
        self.cfg = ModelConfigV1(self.model_type)
        self.precision = precision
        self._initialize_model(self.model_path)
        self._stage = _FrameStage()
        self._decode = None
        self._decode_key = None

    def _initialize_model(self, model_path: str) -> None:
        self.engine = _engine_for(model_path, precision=self.precision)
        if self.logger:
            self.logger.info(f'UfldDetector Type : [{self.engine.framework_type}] || Version : {self.engine.providers}')
        self.input_shape = self.engine.get_engine_input_shape()
        self.input_types = self.engine.engine_dtype
        self.channes, self.input_height, self.input_width = self.input_shape[1:]
        self.output_shape, self.output_names = self.engine.get_engine_output_shape()
        if len(self.output_names) != 1:
            raise Exception("Output dims is error, please check model. load %d channels not match 1." % len(self.output_names))
        o = self.output_shape[0]
        if list(o[1:3]) != [self.cfg.griding_num + 1, self.cfg.cls_num_per_lane]:
            raise Exception("model output %s does not fit the %s configuration" % (o, self.model_type.name))

    def _decode_for(self, img_hw):
        key = (int(img_hw[0]), int(img_hw[1]))
        if self._decode is None:
            c = self.cfg
            self._decode = Ufld1Decode(c.griding_num, c.cls_num_per_lane, c.img_w, c.img_h, self.input_width, self.input_height,
                                       key[1], key[0], c.row_anchor, 1)
        elif self._decode_key != key:
            self._decode.set_source_size(key[1], key[0])
        self._decode_key = key
        return self._decode

    def DetectFrame(self, image, adjust_lanes: bool = True) -> None:
        """ultrafastLaneDetector.py:141-153."""
        fptr, h, w = self._stage.upload(image)
        self.img_height, self.img_width, self.img_channels = h, w, 3
        self.h_ratio, self.w_ratio = h / self.cfg.img_h, w / self.cfg.img_w
        t = self._stage.tensor_for(self.input_shape)
        L.check(L.lib().adas_preprocess_ufld(fptr, 1, h, w, t.ptr, self.input_height, self.input_width, 1.0, None))
        self.engine.infer_device(t.ptr, 1, None)
        dec = self._decode_for((h, w))
        dec.run_device(self.engine.output_device_ptr(0), int(np.prod(self.output_shape[0][1:])), 1, None)
        lanes, status = dec.fetch(0)
        self.lane_info.lanes_points = np.array(lanes + [None], dtype=object)[:4]
        self.lane_info.lanes_status = [bool(s) for s in status]
        self.adjust_lanes = adjust_lanes
        if self._device_geometry(dec, h, w):
            return
        self._UltrafastLaneDetectorV2__update_lanes_status(self.lane_info.lanes_status)
        self._UltrafastLaneDetectorV2__update_lanes_area(self.lane_info.lanes_points, self.img_height)


# =====================================================================================
class TrackState:                  # dtypes/base_track.py:5-9
    New = 0
    Tracked = 1
    Lost = 2
    Removed = 3


class BYTETracker:
    """byteTracker.py:30-51,62-200.  `class_ids` may be ints or the label strings demo.py:273-275 passes; strings are
    numbered in order of first appearance (identity is all STrack.update's class vote needs, strack.py:122-129).
    Each instance owns its id counter (the reference's BaseTrack._count is process-global, base_track.py:12)."""

    def __init__(self, track_thresh: float = 0.5, track_buffer: int = 30, match_thresh: float = 0.8, frame_rate: int = 30,
                 min_box_area: int = 10, max_tracks: int = 256, max_dets: int = 512, names=None, draw_trajectories: bool = False, **kwargs: Any):
        """names: the reference's ObjectTrackBase argument (ObjectTracker/core.py:83-93) -- a dict label -> colour (the class colours
        themselves) or a list of labels (one random colour each); None: no colours, every box is drawn black.
        draw_trajectories (also a plain attribute): False -- DrawTrackedOnFrame draws the boxes only, whatever show_traject says; True --
        show_box and show_traject select the boxes and the trajectories with their direction marks, as in the reference."""
        self.track_thresh, self.match_thresh, self.min_box_area = track_thresh, match_thresh, min_box_area
        self.draw_trajectories = bool(draw_trajectories)
        # what ObjectTrackBase keeps (ObjectTracker/core.py:83-93): a dict is the colour table itself and every label names itself; a list
        # of labels gets one random colour per entry, channels in 0 .. 254
        if names is None:
            self.names, self.class_colors = None, {}
        elif isinstance(names, dict):
            self.names, self.class_colors = {label: label for label in names}, names
        else:
            draw = np.random.default_rng()
            self.names, self.class_colors = names, [[int(c) for c in draw.integers(0, 255, 3)] for _ in range(len(names))]
        self._painter = None
        self.det_thresh = track_thresh + 0.1
        self.buffer_size = int(frame_rate / 30.0 * track_buffer)
        self.max_time_lost = self.buffer_size
        self.frame_id = 0
        self._labels: List[Any] = []
        self._dev = DeviceTracker(1, track_thresh, track_buffer, match_thresh, frame_rate, max_tracks, max_dets)
        self._tracked: List[Dict[str, Any]] = []
        self._lost: List[Dict[str, Any]] = []
        self._crops: Dict[int, list] = {}      # track id -> [crop]: strack.py:46,131-143 (filled once, when the track is activated)
        self._traj_cache = None                # (frame_id, {track id -> boxes}): one device fetch per frame however many tracks are drawn

    def _cls_index(self, c):
        if isinstance(c, (int, np.integer)):
            return int(c)
        if c not in self._labels:
            self._labels.append(c)
        return 1_000_000 + self._labels.index(c)

    def _cls_value(self, i):
        return self._labels[i - 1_000_000] if i >= 1_000_000 else i

    def _messages(self, recs, count):
        out = []
        for r in recs:
            out.append({"track_id": int(r["track_id"]), "count": int(count), "is_activated": bool(r["is_activated"]),
                        "state": int(r["state"]), "score": float(r["score"]), "start_frame_number": int(r["start_frame"]),
                        "curr_frame_number": int(r["frame_id"]),
                        "time_since_update": int(self.frame_id - r["frame_id"]), "location": str((np.inf, np.inf)),
                        "crops": self._crops.get(int(r["track_id"]), []), "class_id": self._cls_value(int(r["class_id"])),
                        "tlwh": [float(v) for v in r["tlwh"]]})
        return out

    def update(self, bboxes, scores, class_ids, frame=None):
        self.frame_id += 1
        b = np.asarray(bboxes, np.float64).reshape(-1, 4)
        s = np.asarray(scores, np.float64).reshape(-1)
        c = np.asarray([self._cls_index(x) for x in class_ids], np.int32)
        self._dev.update_host(0, b, s, c)
        hdr, tracked, lost = self._dev.fetch(0)
        self._traj_cache = None
        self._last_ids = [int(r["track_id"]) for r in tracked] + [int(r["track_id"]) for r in lost]
        if frame is not None:
            # byteTracker.py:161-168: a NEW track (unmatched detection over det_thresh) is activated and takes one crop of the frame at
            # its box (strack.py:131-143: tlwh truncated to int, clipped to the frame, copied); older tracks keep theirs
            fr = np.asarray(frame)
            for r in tracked:
                tid = int(r["track_id"])
                if int(r["start_frame"]) == self.frame_id and tid not in self._crops:
                    # astype(int) truncates toward zero (strack.py:131-143); a new track's filtered tlwh IS its detection's up to the
                    # tlwh -> xyah -> tlwh round trip's last ulp, which the 1e-9 guard absorbs on either side of zero
                    tx1, ty1, tw, th = (int(np.trunc(float(v) + (1e-9 if float(v) >= 0 else -1e-9))) for v in r["tlwh"])
                    x1, y1 = max(0, tx1), max(0, ty1)
                    x2, y2 = min(fr.shape[1], tx1 + tw), min(fr.shape[0], ty1 + th)
                    self._crops[tid] = [fr[y1:y2, x1:x2, :].copy()]
        live = {int(r["track_id"]) for r in tracked} | {int(r["track_id"]) for r in lost}
        for tid in [t for t in self._crops if t not in live]:
            del self._crops[tid]                       # removed tracks: their crops go with them
        self._tracked = self._messages(tracked, hdr.id_count)
        self._lost = self._messages(lost, hdr.id_count)
        return self._tracked

    def trajectories(self) -> Dict[int, list]:
        """track id -> STrack.trajectories (strack.py:53,115): the last 30 detection boxes (tlbr, fp64) the track was updated with,
        oldest first, for every tracked and lost track -- what DrawTrackedOnFrame hands to plot_trajectories (byteTracker.py:202-215).
        Fetched from the device on demand (update() does not pay for it), once per frame: drawing N tracks costs one fetch, not N."""
        if self._traj_cache is None or self._traj_cache[0] != self.frame_id:
            ids = getattr(self, "_last_ids", None)
            if ids is None:
                hdr, tracked, lost = self._dev.fetch(0)
                ids = [int(r["track_id"]) for r in tracked] + [int(r["track_id"]) for r in lost]
            traj = self._dev.fetch_trajectories(0)
            self._traj_cache = (self.frame_id, {tid: list(t) for tid, t in zip(ids, traj)})
        return {tid: [b.copy() for b in t] for tid, t in self._traj_cache[1].items()}

    def filter_trajectories(self, track_id: int, frame, pad: tuple = (0, 0)) -> list:
        """STrack.filter_trajectories (strack.py:145-149) of one track: the boxes that lie inside the frame shrunk by `pad`."""
        padh, padw = pad
        fh, fw = np.asarray(frame).shape[:2]
        return [b for b in self.trajectories().get(int(track_id), [])
                if b[0] >= 0 + padw and b[1] >= 0 + padh and b[2] <= fw - padw and b[3] <= fh - padh]

    def DrawTrackedOnFrame(self, frame, show_box: bool = True, show_traject: bool = True) -> None:
        """byteTracker.py:202-215 on the device: for every activated track of tracked_stracks, in list order, with tlwh[2] * tlwh[3] >
        min_box_area, plot_bbox's thickness-2 rectangle and its 0.6 / 0.4 / + 1 tint in class_colors[class_id] (a class without a colour is
        drawn black).  With draw_trajectories False (the default) that is all: show_traject is accepted and ignored.  With draw_trajectories
        True show_traject adds plot_trajectories' circles and plot_directions' lock-on rectangle or shadowed arrow behind each track's box
        -- DrawTrackedOnFrame(frame, False) is then the demo's call (demo.py:304) -- drawn from the device tracker's live state: rows, boxes
        and trajectory rings are read where they lie in HBM, nothing is fetched.  The text is drawn once set_text_fonts has been given atlases.  `frame` is an HxWx3 uint8 ndarray
        (drawn and copied back into frame[:]) or a StagedFrame."""
        self._draw_tracked(frame, show_box, show_traject)
        if getattr(self, "text_fonts", None) and self._tracked:      # set_text_fonts: "name : id" with the boxes, "ID: n" with the trajectories
            online = [t for t in self._tracked if t["is_activated"]]
            kinds = (["tracks"] if show_box else []) + (["track_ids"] if show_traject and self.draw_trajectories else [])
            if online and kinds:
                traj = self.trajectories()
                self._painter = self._painter or OverlayPainter()
                self._painter.text(frame, kinds, self.text_fonts, dict(self.text_style, min_box_area=float(self.min_box_area)),
                                   tlwhs=[t["tlwh"] for t in online], trk_names=[self._name_of(t["class_id"]) for t in online],
                                   trk_colors=[self._color_of(t["class_id"]) for t in online], trk_ids=[t["track_id"] for t in online],
                                   trajectories=[traj.get(int(t["track_id"]), []) for t in online])

    def set_text_fonts(self, fonts, **style):
        """fonts: {slot: atlas} -- DrawTrackedOnFrame then also draws plot_bbox's "name : id" (with the boxes) and, with
        draw_trajectories, plot_trajectories' shadowed "ID: n" (core.py:199-210, 235-239); None: as before."""
        self.text_fonts, self.text_style = fonts, dict(style)

    def _name_of(self, class_id):
        try:
            return str(self.names[class_id])
        except (KeyError, IndexError, TypeError):
            return None

    def _color_of(self, class_id):
        try:
            return tuple(int(v) for v in self.class_colors[class_id])
        except (KeyError, IndexError, TypeError):
            return (0, 0, 0)

    def _draw_tracked(self, frame, show_box, show_traject):
        if self.draw_trajectories:
            if (show_box or show_traject) and self._tracked:
                if self._painter is None:
                    self._painter = OverlayPainter()
                self._painter.live_tracks(frame, self._dev, self._live_colors(), min_box_area=self.min_box_area, boxes=bool(show_box),
                                          trajectories=bool(show_traject))
            return
        if not show_box:
            return
        online = [t for t in self._tracked if t["is_activated"]]
        if not online:
            return
        colors = []
        for t in online:
            try:
                colors.append(tuple(int(v) for v in self.class_colors[t["class_id"]]))
            except (KeyError, IndexError, TypeError):
                colors.append((0, 0, 0))
        if self._painter is None:
            self._painter = OverlayPainter()
        self._painter.tracks(frame, [t["tlwh"] for t in online], list(range(len(online))), colors, min_box_area=self.min_box_area)

    def _live_colors(self):
        """class_colors as the table the device indexes with ITS class ids: an int id is itself, label k is 1_000_000 + k (_cls_index).
        With labels the table is that long (4 MB in HBM, rebuilt only when a label is added); ids without a colour are black."""
        cc = self.class_colors
        ints = {k: v for k, v in (cc.items() if isinstance(cc, dict) else enumerate(cc)) if isinstance(k, (int, np.integer)) and 0 <= k < 1_000_000}
        labelled = [cc.get(lab) if isinstance(cc, dict) else None for lab in self._labels]
        key = (tuple(sorted((int(k), tuple(int(c) for c in v)) for k, v in ints.items())), tuple(None if v is None else tuple(int(c) for c in v) for v in labelled))
        if getattr(self, "_live_key", None) != key:
            n = (1_000_000 + len(labelled)) if any(v is not None for v in labelled) else (max(ints) + 1 if ints else 0)
            tab = np.zeros((n, 3), np.uint8)
            for k, v in ints.items():
                tab[int(k)] = [int(c) for c in v]
            for i, v in enumerate(labelled):
                if v is not None:
                    tab[1_000_000 + i] = [int(c) for c in v]
            self._live_key, self._live_tab = key, tab
        return self._live_tab

    @property
    def tracked_stracks(self):
        return self._tracked

    @property
    def lost_stracks(self):
        return self._lost

    def reset(self):
        self.frame_id = 0
        self._tracked, self._lost = [], []
        self._crops = {}
        self._traj_cache, self._last_ids = None, None
        self._dev.reset(0)

    def close(self):
        if getattr(self, "_painter", None) is not None:
            self._painter.close()
            self._painter = None
        if getattr(self, "_dev", None) is not None:
            self._dev.close()
            self._dev = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
