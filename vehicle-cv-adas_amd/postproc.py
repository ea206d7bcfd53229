"""Thin object wrappers over the post-processing entry points of the C ABI.

YoloPost      <- YoloDetector.__process_output + Scaler.convert_boxes_coordinate + NMS + get_nms_results
                 (ObjectDetector/yoloDetector.py:104-157, utils.py:70-87,105-256)
UfldDecode    <- UltrafastLaneDetectorV2.__process_output (ultrafastLaneDetectorV2.py:114-181)
DeviceTracker <- BYTETracker.update/reset (ObjectTracker/byteTrack/byteTracker.py:62-200)
PerspectiveWarp <- cv2.warpPerspective in PerspectiveTransformation.transformToBirdView / transformToFrontalView
                 (ufldDetector/perspectiveTransformation.py:89-117)
BirdView      <- PerspectiveTransformation.__init__ / updateTransformParams (perspectiveTransformation.py:21-86), one per stream
"""
import ctypes as C

import numpy as np

from . import _lib as L


def letterbox(src_hw, dst_hw, keep_ratio=True):
    """Scaler.process_image geometry (utils.py:42-68) -> dict(pad=(h,w), ratio=(h,w))."""
    p = L.YoloPostParams()
    L.check(L.lib().adas_letterbox_params(int(src_hw[0]), int(src_hw[1]), int(dst_hw[0]), int(dst_hw[1]),
                                          1 if keep_ratio else 0, C.byref(p)))
    return dict(pad=(p.pad_h, p.pad_w), ratio=(p.ratio_h, p.ratio_w))


class YoloPost:
    def __init__(self, layout, num_anchors, num_classes, box_score, iou_thr, lb, nms_mode=L.NMS_REFERENCE,
                 max_candidates=1024, max_batch=1, input_hw=None):
        """input_hw: network input size; required for HEAD_V5_LITE (the grid decode of yoloDetector.py:35-49)."""
        p = L.YoloPostParams(layout, num_anchors, num_classes, nms_mode, box_score, iou_thr, int(lb["pad"][0]),
                             int(lb["pad"][1]), float(lb["ratio"][0]), float(lb["ratio"][1]), max_candidates, 0)
        self.params, self.max_batch, self.cap = p, max_batch, max_candidates
        h = C.c_void_p()
        L.check(L.lib().adas_yolo_post_create(C.byref(p), max_batch, C.byref(h)))
        self.h = h.value
        if input_hw is not None:
            try:
                L.check(L.lib().adas_yolo_post_set_input_size(self.h, int(input_hw[0]), int(input_hw[1])))
            except Exception:
                self.close()
                raise
        self.head_elems = (4 + num_classes) * num_anchors if layout == L.HEAD_V8 else (5 + num_classes) * num_anchors

    def run_device(self, d_head_ptr, batch=1, stream=None):
        L.check(L.lib().adas_yolo_post_run(self.h, d_head_ptr, batch, stream))

    def run_host(self, heads):
        """heads: [batch, ...] fp32 in the reference layout; uploaded, processed on the GPU."""
        heads = np.ascontiguousarray(heads, np.float32)
        batch = heads.shape[0]
        assert heads[0].size == self.head_elems
        buf = L.DeviceBuffer.from_array(heads)
        try:
            self.run_device(buf.ptr, batch)
            return [self.fetch(b) for b in range(batch)]
        finally:
            buf.free()

    def fetch(self, frame=0):
        cap = self.cap
        cnt = L.YoloCounts()
        o = dict(cand_anchor=np.zeros(cap, np.int32), cand_xywh=np.zeros((cap, 4)), cand_conf=np.zeros(cap),
                 cand_cls=np.zeros(cap, np.int32), keep=np.zeros(cap, np.int32), xywh=np.zeros((cap, 4)),
                 conf=np.zeros(cap), class_id=np.zeros(cap, np.int32), xyxy_int=np.zeros((cap, 4), np.int32))
        rc = L.lib().adas_yolo_post_fetch(self.h, frame, C.byref(cnt), *[L.ptr(o[k]) for k in (
            "cand_anchor", "cand_xywh", "cand_conf", "cand_cls", "keep", "xywh", "conf", "class_id", "xyxy_int")])
        n, k = cnt.n_candidates, cnt.n_keep
        res = dict(n_found=cnt.n_found, overflow=bool(cnt.flags & 1))
        for key in ("cand_anchor", "cand_xywh", "cand_conf", "cand_cls"):
            res[key] = o[key][:n]
        for key in ("keep", "xywh", "conf", "class_id", "xyxy_int"):
            res[key] = o[key][:k]
        res["rc"] = rc
        return res

    def fetch_dets(self, frame=0):
        """The survivors only, as one packed device-to-host message (adas_yolo_post_fetch_dets): the keys of fetch() that
        get_nms_results reads (yoloDetector.py:141-157), same values."""
        cap = self.cap
        cnt = L.YoloCounts()
        o = dict(keep=np.zeros(cap, np.int32), xywh=np.zeros((cap, 4)), conf=np.zeros(cap), class_id=np.zeros(cap, np.int32),
                 xyxy_int=np.zeros((cap, 4), np.int32))
        rc = L.lib().adas_yolo_post_fetch_dets(self.h, frame, C.byref(cnt), *[L.ptr(o[k]) for k in ("keep", "xywh", "conf", "class_id", "xyxy_int")])
        res = dict(n_found=cnt.n_found, n_candidates=cnt.n_candidates, overflow=bool(cnt.flags & 1), rc=rc)
        for key, a in o.items():
            res[key] = a[:cnt.n_keep]
        return res

    def device_views(self):
        v = [C.c_void_p() for _ in range(4)]
        L.check(L.lib().adas_yolo_post_device_views(self.h, *[C.byref(x) for x in v]))
        return dict(xyxy=v[0].value, score=v[1].value, cls=v[2].value, counts=v[3].value)

    def close(self):
        if getattr(self, "h", None):
            L.lib().adas_yolo_post_destroy(self.h)
            self.h = None

    __del__ = close


class EffdetTail:
    """The in-graph tail of an exported EfficientDet (adas_effdet_tail_*): anchor decode + score threshold + per-class NMS over the ten
    raw head tensors of an "efficientdet-d0" .. "efficientdet-d3" engine graph -> (boxes xyxy float32, class ids, confidences) per frame,
    the three arrays EfficientdetDetector.__process_output reads (efficientdetDetector.py:68-70).  Two launches per run: a class-max pass
    over (anchor chunks x frames) workgroups, then one workgroup per frame for rank, decode and NMS; ADAS_EFFDET_TAIL_ONE_WG=1 in the
    environment when the object is created selects the older single-workgroup launch (same results, for comparisons)."""

    def __init__(self, in_hw, num_classes=90, score_thr=0.05, iou_thr=0.5, max_det=100, max_candidates=2048, max_batch=1, anchor_scale=4.0):
        p = L.EffdetTailParams(int(in_hw[0]), int(in_hw[1]), int(num_classes), int(max_candidates), int(max_det), 0, float(score_thr), float(iou_thr),
                               float(anchor_scale))
        self.max_det, self.max_batch = int(max_det), int(max_batch)
        h = C.c_void_p()
        L.check(L.lib().adas_effdet_tail_create(C.byref(p), max_batch, C.byref(h)))
        self.h = h.value

    def run(self, reg_ptrs, cls_ptrs, batch, stream=None):
        """reg_ptrs / cls_ptrs: five device pointers each (pyramid levels 3..7), [batch][cells * 9][4 | num_classes] float32."""
        reg = (C.c_void_p * 5)(*[int(p) for p in reg_ptrs])
        cls = (C.c_void_p * 5)(*[int(p) for p in cls_ptrs])
        L.check(L.lib().adas_effdet_tail_run(self.h, reg, cls, int(batch), stream))

    def fetch(self, frame=0):
        n, nc = C.c_int32(), C.c_int32()
        boxes = np.zeros((self.max_det, 4), np.float32); ids = np.zeros(self.max_det, np.int32); conf = np.zeros(self.max_det, np.float32)
        L.check(L.lib().adas_effdet_tail_fetch(self.h, frame, C.byref(n), L.ptr(boxes), L.ptr(ids), L.ptr(conf), C.byref(nc)))
        k = n.value
        return dict(boxes=boxes[:k].copy(), class_id=ids[:k].astype(np.int64), conf=conf[:k].copy(), n_candidates=nc.value)

    def close(self):
        if getattr(self, "h", None):
            L.lib().adas_effdet_tail_destroy(self.h)
            self.h = None

    __del__ = close


class EffdetPost:
    """EfficientdetDetector.__process_output on the device (adas_effdet_post_*): inverse letterbox in float32 + `conf < box_score`
    filter over the exported graph's (boxes, ids, confs) outputs."""

    def __init__(self, box_score, lb, max_boxes=256, max_batch=1):
        p = L.EffdetPostParams(float(box_score), int(lb["pad"][0]), int(lb["pad"][1]), float(lb["ratio"][0]), float(lb["ratio"][1]),
                               int(max_boxes), 0)
        self.cap, self.max_batch = int(max_boxes), int(max_batch)
        h = C.c_void_p()
        L.check(L.lib().adas_effdet_post_create(C.byref(p), max_batch, C.byref(h)))
        self.h = h.value

    def run_host(self, frames):
        """frames: list (<= max_batch) of (boxes (n,4), ids (n,), confs (n,)) host arrays -> list of result dicts."""
        B, cap = len(frames), self.cap
        boxes = np.zeros((B, cap, 4), np.float32); ids = np.zeros((B, cap), np.int32); confs = np.zeros((B, cap), np.float32)
        counts = np.zeros(B, np.int32)
        for b, (bx, i_, cf) in enumerate(frames):
            n = len(cf)
            if n > cap:
                raise L.AdasError(-1, "frame %d carries %d detections, max_boxes is %d" % (b, n, cap))
            counts[b] = n
            boxes[b, :n] = np.asarray(bx, np.float32).reshape(-1, 4); ids[b, :n] = np.asarray(i_).astype(np.int32); confs[b, :n] = cf
        bufs = [L.DeviceBuffer.from_array(a) for a in (boxes, ids, confs)]
        try:
            L.check(L.lib().adas_effdet_post_run(self.h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, L.ptr(counts), B, None))
            return [self.fetch(b) for b in range(B)]
        finally:
            for x in bufs:
                x.free()

    def fetch(self, frame=0):
        cap = self.cap
        k = C.c_int32()
        xywh = np.zeros((cap, 4), np.float32); conf = np.zeros(cap, np.float32); cls = np.zeros(cap, np.int32); xi = np.zeros((cap, 4), np.int32)
        L.check(L.lib().adas_effdet_post_fetch(self.h, frame, C.byref(k), L.ptr(xywh), L.ptr(conf), L.ptr(cls), L.ptr(xi)))
        n = k.value
        return dict(xywh=xywh[:n], conf=conf[:n], class_id=cls[:n].astype(np.int64), xyxy_int=xi[:n].astype(np.int64))

    def close(self):
        if getattr(self, "h", None):
            L.lib().adas_effdet_post_destroy(self.h)
            self.h = None

    __del__ = close


class UfldDecode:
    def __init__(self, grid_row, cls_row, grid_col, cls_col, img_w, img_h, row_anchor, col_anchor, local_width=1,
                 max_batch=1, num_lanes=4):
        """row_anchor / col_anchor: at least cls_row / cls_col entries; the first cls_* are used, as the reference indexes
        cfg.*_anchor[k] with the network's own k (ultrafastLaneDetectorV2.py:152,170 -- its CurveLanes ModelConfig carries 81
        column anchors for a 41-anchor head).  num_lanes: the tensors' last dimension (4; 10 for the CurveLanes configs)."""
        ra = np.ascontiguousarray(np.asarray(row_anchor, np.float64)[:cls_row])
        ca = np.ascontiguousarray(np.asarray(col_anchor, np.float64)[:cls_col])
        assert len(ra) == cls_row and len(ca) == cls_col, "anchor arrays shorter than the head's anchor counts"
        p = L.UfldParams(grid_row, cls_row, grid_col, cls_col, img_w, img_h, local_width, int(num_lanes), L.ptr(ra), L.ptr(ca))
        self.dims = (grid_row, cls_row, grid_col, cls_col)
        h = C.c_void_p()
        L.check(L.lib().adas_ufld_decode_create(C.byref(p), max_batch, C.byref(h)))
        self.h = h.value

    def run_device(self, ptrs, strides, batch=1, stream=None):
        L.check(L.lib().adas_ufld_decode_run(self.h, *ptrs, *strides, batch, stream))

    def run_host(self, outs):
        """outs = [loc_row (B,G,K,4), loc_col, exist_row, exist_col] fp32 arrays."""
        outs = [np.ascontiguousarray(o, np.float32) for o in outs]
        batch = outs[0].shape[0]
        bufs = [L.DeviceBuffer.from_array(o) for o in outs]
        try:
            self.run_device([b.ptr for b in bufs], [o[0].size for o in outs], batch)
            return [self.fetch(b) for b in range(batch)]
        finally:
            for b in bufs:
                b.free()

    def fetch(self, frame=0):
        pts = np.zeros((4, L.UFLD_MAX_POINTS, 2), np.int32)
        cnt = np.zeros(4, np.int32)
        det = np.zeros(4, np.int32)
        L.check(L.lib().adas_ufld_decode_fetch(self.h, frame, L.ptr(pts), L.ptr(cnt), L.ptr(det)))
        lanes = [[(int(x), int(y)) for x, y in pts[i, :cnt[i]]] for i in range(4)]
        return lanes, [bool(d) for d in det]

    def upload(self, lanes, detected, frame=0):
        """Place lane points decoded elsewhere into a frame slot (4 lists of (x, y), 4 bools)."""
        pts = np.zeros((4, L.UFLD_MAX_POINTS, 2), np.int32)
        cnt = np.asarray([len(l) for l in lanes], np.int32)
        for i, l in enumerate(lanes):
            if len(l):
                pts[i, :len(l)] = np.asarray(l, np.int32).reshape(-1, 2)
        det = np.asarray([1 if d else 0 for d in detected], np.int32)
        L.check(L.lib().adas_ufld_decode_upload(self.h, frame, L.ptr(pts), L.ptr(cnt), L.ptr(det)))

    def close(self):
        if getattr(self, "h", None):
            L.lib().adas_ufld_decode_destroy(self.h)
            self.h = None

    __del__ = close


class Ufld1Decode(UfldDecode):
    """UFLD (v1) decoder: UltrafastLaneDetector.__process_output (ultrafastLaneDetector.py:96-139) on the device."""

    def __init__(self, griding_num, cls_num_per_lane, cfg_img_w, cfg_img_h, input_w, input_h, src_w, src_h, row_anchor,
                 max_batch=1):
        ra = np.ascontiguousarray(row_anchor, np.float64)
        p = L.Ufld1Params(griding_num, cls_num_per_lane, cfg_img_w, cfg_img_h, input_w, input_h, src_w, src_h, L.ptr(ra))
        self.dims = (griding_num, cls_num_per_lane)
        h = C.c_void_p()
        L.check(L.lib().adas_ufld1_decode_create(C.byref(p), max_batch, C.byref(h)))
        self.h = h.value

    def set_source_size(self, src_w, src_h):
        L.check(L.lib().adas_ufld1_decode_set_source_size(self.h, int(src_w), int(src_h)))

    def run_device(self, ptr, stride, batch=1, stream=None):
        L.check(L.lib().adas_ufld1_decode_run(self.h, ptr, stride, batch, stream))

    def run_host(self, out):
        """out: (B, G+1, K, 4) fp32."""
        out = np.ascontiguousarray(out, np.float32)
        buf = L.DeviceBuffer.from_array(out)
        try:
            self.run_device(buf.ptr, out[0].size, out.shape[0])
            return [self.fetch(b) for b in range(out.shape[0])]
        finally:
            buf.free()


class LaneGeometry:
    """Ego-lane area polygon, bird-view points, curvature and offset computed on the device from a lane decoder's
    device-resident points (core.py:102-158, perspectiveTransformation.py:120-214)."""
    DIRECTIONS = (None, "L", "R", "F")

    def __init__(self, img_h, bird_wh, M, adjust_lanes=True, max_batch=1):
        p = L.LaneGeometryParams(int(img_h), int(bird_wh[0]), int(bird_wh[1]), 1 if adjust_lanes else 0,
                                 (C.c_double * 9)(*np.asarray(M, np.float64).reshape(9)))
        self.img_h = int(img_h)
        h = C.c_void_p()
        L.check(L.lib().adas_lane_geometry_create(C.byref(p), max_batch, C.byref(h)))
        self.h = h.value

    def set_matrix(self, M):
        m = np.ascontiguousarray(M, np.float64).reshape(9)
        L.check(L.lib().adas_lane_geometry_set_matrix(self.h, L.ptr(m)))

    def run(self, decode, adjust_lanes=True, batch=1, stream=None):
        L.check(L.lib().adas_lane_geometry_run(self.h, decode.h, 1 if adjust_lanes else 0, batch, stream))

    def run_matrices(self, decode, d_M_ptr, adjust_lanes=True, batch=1, stream=None):
        """run() with frame f reading its homography from the device table d_M_ptr [batch][9] (BirdView.device_views()[0])."""
        L.check(L.lib().adas_lane_geometry_run_matrices(self.h, decode.h, 1 if adjust_lanes else 0, batch, d_M_ptr, stream))

    def device_views(self):
        """(d_header, d_values, d_area, area_stride): per frame 8 int32 (area_status, n_left, n_right, direction, bird counts), 2 float64
        (curvature, offset) and the area polygon at d_area + frame * area_stride int32."""
        a, b, c, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int32()
        L.check(L.lib().adas_lane_geometry_device_views(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return a.value, b.value, c.value, int(n.value)

    def fetch(self, frame=0):
        res = L.LaneGeometryResult()
        area = np.zeros((2 * self.img_h, 2), np.int32)
        bird = np.zeros((4, L.UFLD_MAX_POINTS, 2), np.int32)
        L.check(L.lib().adas_lane_geometry_fetch(self.h, frame, C.byref(res), L.ptr(area), L.ptr(bird)))
        n = res.n_area_left + res.n_area_right
        return dict(area_status=bool(res.area_status), area_points=area[:n].copy(), n_left=res.n_area_left, n_right=res.n_area_right,
                    bird_points=[bird[i, :res.bird_counts[i]].copy() for i in range(4)],
                    direction=self.DIRECTIONS[res.direction], curvature=res.curvature if res.direction else None,
                    offset=res.offset if res.direction else None)

    def fetch_veh_pos(self, frame=0):
        """veh_pos of the frame: the bird-view column (lx + rx) / 2 the offset is measured from; 0.0 when the frame has no curve."""
        v = C.c_double()
        L.check(L.lib().adas_lane_geometry_fetch_veh_pos(self.h, int(frame), C.byref(v)))
        return float(v.value)

    def close(self):
        if getattr(self, "h", None):
            L.lib().adas_lane_geometry_destroy(self.h)
            self.h = None

    __del__ = close


class PerspectiveWarp:
    """cv2.warpPerspective(frame, M, dsize, INTER_LINEAR, BORDER_CONSTANT 0) of BGR u8 frames resident in HBM, one matrix per frame of a
    batch (perspectiveTransformation.py:89-117).  OpenCV's reference arithmetic restated (csrc/warp_core.h), parity with a real cv2
    build unpinned."""

    def __init__(self, src_hw, dst_hw, max_batch=1):
        p = L.WarpParams(int(src_hw[0]), int(src_hw[1]), int(dst_hw[0]), int(dst_hw[1]))
        self.src_hw, self.dst_hw, self.max_batch = (p.src_h, p.src_w), (p.dst_h, p.dst_w), int(max_batch)
        h = C.c_void_p()
        L.check(L.lib().adas_warp_create(C.byref(p), self.max_batch, C.byref(h)))
        self.h = h.value

    def set_matrix(self, M, frame=-1, inverse=False):
        """M maps source to destination (cv2's default); inverse=True: destination to source (cv2.WARP_INVERSE_MAP).
        frame=-1: every frame of the batch."""
        m = np.ascontiguousarray(M, np.float64).reshape(9)
        L.check(L.lib().adas_warp_set_matrix(self.h, int(frame), L.ptr(m), 1 if inverse else 0))

    def run(self, src_ptr, batch=1, dst_ptr=None, stream=None):
        """src_ptr: device pointer of [batch][src_h][src_w][3] u8.  dst_ptr=None writes the handle's own buffer (fetch / device_view)."""
        L.check(L.lib().adas_warp_run(self.h, src_ptr, dst_ptr, int(batch), stream))

    def run_device_matrices(self, src_ptr, d_M_warp_ptr, batch=1, dst_ptr=None, stream=None):
        """run() with frame f's destination -> source matrix read from the device table d_M_warp_ptr [batch][9]
        (BirdView.device_views()[1]); set_matrix plays no part.  A plain launch."""
        L.check(L.lib().adas_warp_run_device_matrices(self.h, src_ptr, dst_ptr, d_M_warp_ptr, int(batch), stream))

    def fetch(self, frame=0):
        out = np.empty((self.dst_hw[0], self.dst_hw[1], 3), np.uint8)
        L.check(L.lib().adas_warp_fetch(self.h, int(frame), L.ptr(out)))
        return out

    def device_view(self):
        p = C.c_void_p()
        L.check(L.lib().adas_warp_device_view(self.h, C.byref(p)))
        return p.value

    def close(self):
        if getattr(self, "h", None):
            L.lib().adas_warp_destroy(self.h)
            self.h = None

    __del__ = close


class BirdView:
    """One PerspectiveTransformation trapezoid per video stream kept on the device (perspectiveTransformation.py:21-86): request()
    queues updateTransformParams' type for a stream's next run, run() applies it where that frame's two ego lanes are detected and
    leaves every frame's matrices in device tables (device_views) for LaneGeometry.run_matrices / PerspectiveWarp.run_device_matrices."""
    MODES = L.BIRDVIEW_MODES

    def __init__(self, img_size, n_streams=1, max_frames=None):
        p = L.BirdviewParams(int(img_size[0]), int(img_size[1]))
        self.img_size, self.n_streams = (p.img_w, p.img_h), int(n_streams)
        self.max_frames = int(max_frames) if max_frames else self.n_streams
        h = C.c_void_p()
        L.check(L.lib().adas_birdview_create(C.byref(p), self.n_streams, self.max_frames, C.byref(h)))
        self.h = h.value

    def request(self, stream, mode, hip_stream=None):
        """mode: "Default" | "Top" | "Bottom" (or its number); anything else is consumed by the next run without effect, as the
        reference ignores an unknown type."""
        m = self.MODES.get(mode, -1) if (mode is None or isinstance(mode, str)) else int(mode)
        L.check(L.lib().adas_birdview_request(self.h, int(stream), m, hip_stream))

    def run(self, decode, n_streams=None, n_frames=1, stream=None):
        L.check(L.lib().adas_birdview_run(self.h, decode.h, int(n_streams or self.n_streams), int(n_frames), stream))

    def fetch_stream(self, stream=0):
        s = L.BirdviewState()
        L.check(L.lib().adas_birdview_fetch_stream(self.h, int(stream), C.byref(s)))
        return dict(src=np.array(s.src, np.float32).reshape(4, 2), M=np.array(s.M, np.float64).reshape(3, 3),
                    M_inv=np.array(s.M_inv, np.float64).reshape(3, 3), M_warp=np.array(s.M_warp, np.float64).reshape(3, 3),
                    n_updates=int(s.n_updates), n_rejected=int(s.n_rejected))

    def fetch_frame(self, frame=0):
        M, Mw, a = np.zeros(9, np.float64), np.zeros(9, np.float64), C.c_int32()
        L.check(L.lib().adas_birdview_fetch_frame(self.h, int(frame), L.ptr(M), L.ptr(Mw), C.byref(a)))
        return dict(M=M.reshape(3, 3), M_warp=Mw.reshape(3, 3), applied=int(a.value))

    def pending(self, stream=0):
        """The mode still queued for the stream (0: none)."""
        m = C.c_int32()
        L.check(L.lib().adas_birdview_pending(self.h, int(stream), C.byref(m)))
        return int(m.value)

    def device_views(self):
        """(d_M, d_M_warp): device pointers of the per-frame tables, [max_frames][9] float64 each."""
        a, b = C.c_void_p(), C.c_void_p()
        L.check(L.lib().adas_birdview_device_views(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def reset(self, stream=-1):
        L.check(L.lib().adas_birdview_reset(self.h, int(stream)))

    def close(self):
        if getattr(self, "h", None):
            L.lib().adas_birdview_destroy(self.h)
            self.h = None

    __del__ = close


class Analysis:
    """SingleCamDistanceMeasure + TaskConditions per video stream on the device (distanceMeasure.py:50-93, taskConditions.py:88-312;
    demo.py:284-296): distance points, the collision point inside the ego-lane polygon, the three warning messages and the bird view's
    re-anchoring toggle.  fetch_stream / fetch_frame return analysis.CollisionType / OffsetType / CurvatureType members and
    "Default" | "Top" | "Bottom" | None."""
    MODES = (None, "Default", "Top", "Bottom")
    DIRECTIONS = (None, "L", "R", "F")
    OBJECT_LIST = ("person", "bicycle", "car", "motorbike", "bus", "truck")     # SingleCamDistanceMeasure's default

    def __init__(self, class_names=(), object_list=None, n_streams=1, max_frames=None, max_points=512, max_poly=1440, ref_height=None, **constants):
        """class_names: the detector's label of every class id; object_list: the labels that are measured (default: the reference's six).
        A class gets RefSizeDict[label][0] inches when its label is in both, else 0 (not measured); ref_height= gives that per-class table
        directly instead.  constants: focal, y_limit, distance_thres, offset_thres, curvae_thres, calib_frequency, calib_curvae_thres."""
        from . import analysis as A
        self._A = A
        self._collision = (A.CollisionType.UNKNOWN, A.CollisionType.NORMAL, A.CollisionType.PROMPT, A.CollisionType.WARNING)
        self._offset = (A.OffsetType.UNKNOWN, A.OffsetType.RIGHT, A.OffsetType.LEFT, A.OffsetType.CENTER)
        self._curvature = (A.CurvatureType.UNKNOWN, A.CurvatureType.STRAIGHT, A.CurvatureType.EASY_LEFT, A.CurvatureType.HARD_LEFT,
                           A.CurvatureType.EASY_RIGHT, A.CurvatureType.HARD_RIGHT)
        objects = list(self.OBJECT_LIST if object_list is None else object_list)
        sizes = A.SingleCamDistanceMeasure.RefSizeDict
        if ref_height is None:
            ref_height = [float(sizes[n][0]) if (n in objects and n in sizes) else 0.0 for n in class_names]
        self.ref_height = np.ascontiguousarray(ref_height, np.float64).reshape(-1)
        p = L.AnalysisParams()
        L.check(L.lib().adas_analysis_default_params(C.byref(p)))
        for k, v in constants.items():
            if not hasattr(p, k) or k in ("n_classes", "h_ref_height", "max_points", "max_poly"):
                raise TypeError("unknown analysis constant %r" % k)
            setattr(p, k, v)
        p.n_classes, p.h_ref_height = len(self.ref_height), (self.ref_height.ctypes.data if len(self.ref_height) else None)
        p.max_points, p.max_poly = int(max_points), int(max_poly)
        self.n_streams, self.max_points = int(n_streams), int(max_points)
        self.max_frames = int(max_frames) if max_frames else self.n_streams
        h = C.c_void_p()
        L.check(L.lib().adas_analysis_create(C.byref(p), self.n_streams, self.max_frames, C.byref(h)))
        self.h = h.value

    def run(self, post, geometry, birdview=None, n_streams=None, n_frames=1, stream=None):
        """One launch on the handles' device arrays (YoloPost, LaneGeometry); with birdview= every stream's request lands in that BirdView's
        pending table for its next run."""
        L.check(L.lib().adas_analysis_run(self.h, post.h, geometry.h, birdview.h if birdview else None, int(n_streams or self.n_streams), int(n_frames),
                                          stream))

    def run_arrays(self, d_xyxy, d_cls, d_counts, det_stride, d_poly, poly_cap, d_poly_counts, d_geometry, d_request=None, n_streams=None, n_frames=1,
                   stream=None):
        """The same kernel on raw device pointers (adas_analysis_run_arrays)."""
        L.check(L.lib().adas_analysis_run_arrays(self.h, d_xyxy, d_cls, d_counts, int(det_stride), d_poly, int(poly_cap), d_poly_counts, d_geometry,
                                                 d_request, int(n_streams or self.n_streams), int(n_frames), stream))

    @staticmethod
    def make_inputs(frames):
        """[(collision point or its metres or None, area_status, offset or None, direction "L" | "R" | "F" | None, curvature or None), ...] ->
        the table run_inputs takes."""
        t = np.zeros(len(frames), L.ANALYSIS_INPUT_DTYPE)
        for r, (dist, area, off, direction, curv) in zip(t, frames):
            if dist is not None:
                r["has_point"], r["distance"] = 1, float(dist[2] if isinstance(dist, (list, tuple, np.ndarray)) else dist)
            r["area"] = 1 if area else 0
            if off is not None:
                r["has_offset"], r["offset"] = 1, float(off)
            if curv is not None:
                r["has_curvature"], r["curvature"] = 1, float(curv)
            r["direction"] = Analysis.DIRECTIONS.index(direction)
        return t

    def run_inputs(self, inputs, n_streams=None, n_frames=1, stream=None):
        """The state machine alone: inputs = make_inputs(...) (or that dtype), frame b of stream s at b * n_streams + s."""
        t = np.ascontiguousarray(inputs, L.ANALYSIS_INPUT_DTYPE)
        ns = int(n_streams or self.n_streams)
        if len(t) != ns * int(n_frames):
            raise ValueError("%d inputs for %d streams x %d frames" % (len(t), ns, n_frames))
        L.check(L.lib().adas_analysis_run_inputs(self.h, L.ptr(t), ns, int(n_frames), stream))

    def fetch_stream(self, stream=0):
        s = L.AnalysisState()
        L.check(L.lib().adas_analysis_fetch_stream(self.h, int(stream), C.byref(s)))
        nc = int(s.n_curvature)
        return dict(collision_msg=self._collision[s.collision_msg], offset_msg=self._offset[s.offset_msg], curvature_msg=self._curvature[s.curvature_msg],
                    toggle_status=self.MODES[s.toggle_status], transform_status=self.MODES[s.transform_status],
                    toggle_oscillator_status=[bool(v) for v in s.oscillator],
                    toggle_status_counter={"Offset": int(s.counter_offset), "Curvae": int(s.counter_curvae), "BirdViewAngle": int(s.counter_birdview)},
                    vehicle_collision_record=[float(v) for v in s.collision_record[:s.n_collision]],
                    vehicle_offset_record=[float(v) for v in s.offset_record[:s.n_offset]],
                    vehicle_curvature_record=[[self.DIRECTIONS[s.direction_record[k]], float(s.curvature_record[k])] for k in range(nc)],
                    n_nonfinite=int(s.n_nonfinite))

    def fetch_frame(self, frame=0):
        f = L.AnalysisFrame()
        L.check(L.lib().adas_analysis_fetch_frame(self.h, int(frame), C.byref(f)))
        return dict(n_points=int(f.n_points), collision_point=[int(f.collision_x), int(f.collision_y), float(f.collision_d)] if f.has_collision else None,
                    collision_index=int(f.collision_index), collision_msg=self._collision[f.collision_msg], offset_msg=self._offset[f.offset_msg],
                    curvature_msg=self._curvature[f.curvature_msg], toggle_status=self.MODES[f.toggle_status],
                    transform_status=self.MODES[f.transform_status], toggle_oscillator_status=[bool(v) for v in f.oscillator],
                    toggle_status_counter=dict(zip(("Offset", "Curvae", "BirdViewAngle"), (int(v) for v in f.counters))), check=bool(f.check),
                    request=self.MODES[f.request], flags=int(f.flags))

    def fetch_points(self, frame=0, n=None):
        """distance_points of the frame as the reference lists them: [[x, y, metres], ...] in survivor order."""
        if n is None:
            n = self.fetch_frame(frame)["n_points"]
        xy, d = np.zeros((n, 2), np.int32), np.zeros(n, np.float64)
        L.check(L.lib().adas_analysis_fetch_points(self.h, int(frame), L.ptr(xy), L.ptr(d), int(n)))
        return [[int(x), int(y), float(v)] for (x, y), v in zip(xy, d)]

    def reset(self, stream=-1):
        L.check(L.lib().adas_analysis_reset(self.h, int(stream)))

    def close(self):
        if getattr(self, "h", None):
            L.lib().adas_analysis_destroy(self.h)
            self.h = None

    __del__ = close


class LaneOverlay:
    """The pixel part of the reference's Draw* block on frames resident in HBM (adas_overlay_*): discs of radius 3 on every lane point
    blended at alpha 0.3 (UltrafastLaneDetectorV2.DrawDetectedOnFrame), the ego-lane polygon blended at 0.85 (DrawAreaOnFrame), white
    discs of radius 4 on the distance points (SingleCamDistanceMeasure.DrawDetectedOnFrame) and discs of radius 10 on the bird-view
    image (PerspectiveTransformation.DrawDetectedOnBirdView).  The object layer ("detections", "tracks"; off unless asked for) adds the
    boxes between the area blend and the distance discs: ObjectDetectBase.cornerRect per survivor (outline and eight corner arms in the
    class colour) and the box part of BYTETracker.DrawTrackedOnFrame (a thickness-2 rectangle, then the region tinted 0.6 / 0.4 / + 1) per
    activated tracked track over min_box_area.  The trajectories stage ("trajectories", bit 128; off unless asked for) adds what the demo's
    DrawTrackedOnFrame(frame_show, False) draws per such track, behind its box: plot_trajectories' growing circles over the track's last 30
    boxes and plot_directions' lock-on rectangle or shadowed arrow (csrc/overlay_track_core.h).  Text and the label's background rectangle are set_fonts /
    run_text below (a mask of their own).  Not drawn: key points, DrawTransformFrontalViewArea's slanted thick lines.  The demo's three UI panels are painted by set_panels /
    run_panels below (a mask of their own, not a stage).
    The pixel rules are csrc/overlay_core.h (modelled on OpenCV 4.5; parity with a real cv2 build is unpinned, lines are not clipped
    before they are walked)."""
    STAGES = L.OVERLAY_STAGES
    OBJECT_STYLE = ("min_box_area", "det_rect_thickness", "det_arm_thickness", "track_thickness")

    def __init__(self, src_hw, bird_hw=None, max_batch=1, **style):
        """style: lane_radius, distance_radius, bird_radius, lane_alpha, area_alpha, lane_colors (4 BGR tuples), offset_color,
        area_color, collision_colors (4), distance_color."""
        self.p = L.OverlayParams()
        L.check(L.lib().adas_overlay_default_params(C.byref(self.p)))
        self.p.src_h, self.p.src_w = int(src_hw[0]), int(src_hw[1])
        if bird_hw is not None:
            self.p.bird_h, self.p.bird_w = int(bird_hw[0]), int(bird_hw[1])
        self.os = L.OverlayObjectStyle()
        L.check(L.lib().adas_overlay_default_object_style(C.byref(self.os)))
        obj = {k: style.pop(k) for k in self.OBJECT_STYLE if k in style}
        self._apply(style)
        self.src_hw, self.bird_hw, self.max_batch = (self.p.src_h, self.p.src_w), (self.p.bird_h, self.p.bird_w), int(max_batch)
        h = C.c_void_p()
        L.check(L.lib().adas_overlay_create(C.byref(self.p), self.max_batch, C.byref(h)))
        self.h = h.value
        if obj:
            self.set_object_style(**obj)

    def set_object_style(self, **style):
        """min_box_area (10), det_rect_thickness (1), det_arm_thickness (5), track_thickness (2), from the next run on."""
        for k, v in style.items():
            if k not in self.OBJECT_STYLE:
                raise TypeError("unknown overlay object style %r" % k)
            setattr(self.os, k, v)
        L.check(L.lib().adas_overlay_set_object_style(self.h, C.byref(self.os)))

    def set_class_colors(self, which, colors):
        """The class colours of "detections" (colors_dict by class id) or "tracks" (class_colors): BGR triples, written as given.  A class id
        outside the table is 'unknown', black; so is every object while no table is set.  From the next run on."""
        which = self.stage_mask(which)
        tab = np.ascontiguousarray(np.asarray(list(colors), np.int64).reshape(-1, 3).astype(np.uint8))
        L.check(L.lib().adas_overlay_set_class_colors(self.h, which, L.ptr(tab) if len(tab) else None, len(tab)))

    def _apply(self, style):
        for k, v in style.items():
            if k in ("lane_colors", "collision_colors"):
                for i, c in enumerate(v):
                    for j in range(3):
                        getattr(self.p, k)[i][j] = int(c[j])
            elif k in ("offset_color", "area_color", "distance_color"):
                for j in range(3):
                    getattr(self.p, k)[j] = int(v[j])
            elif k in ("lane_radius", "distance_radius", "bird_radius", "lane_alpha", "area_alpha"):
                setattr(self.p, k, v)
            else:
                raise TypeError("unknown overlay style %r" % k)

    @classmethod
    def stage_mask(cls, stages):
        """An int, or names out of "lanes", "area", "distance", "bird", "detections", "tracks", "trajectories"."""
        if isinstance(stages, int):
            return stages
        names = [stages] if isinstance(stages, str) else list(stages)
        for n in names:
            if n not in cls.STAGES:
                raise ValueError("unknown overlay stage %r (one of %s)" % (n, ", ".join(cls.STAGES)))
        m = 0
        for n in names:
            m |= cls.STAGES[n]
        return m

    def set_style(self, **style):
        """Radii, alphas and colours from the next run on."""
        self._apply(style)
        L.check(L.lib().adas_overlay_set_style(self.h, C.byref(self.p)))

    def run(self, src_ptr, decode=None, geometry=None, analysis=None, bird_ptr=None, stages=None, n_streams=1, n_frames=1, dst_ptr=None, stream=None,
            post=None, tracker=None):
        """Frames [0, n_streams * n_frames) of the device pointer src_ptr -> dst_ptr (None: the handle's own buffer; src_ptr: in place), drawn
        from the handles' device arrays (UfldDecode / Ufld1Decode, LaneGeometry, Analysis; post=: a YoloPost, its survivors' boxes; tracker=: a
        DeviceTracker, its live tracked tracks -- n_frames must then be 1).  stages=None: every stage whose handle is given, except
        "trajectories", which is drawn only when named (it reads tracker='s live state: the rows and their trajectory rings)."""
        if stages is None:
            stages = ((L.OVERLAY_LANES if decode else 0) | (L.OVERLAY_AREA if geometry else 0) | (L.OVERLAY_DISTANCE if analysis else 0) |
                      (L.OVERLAY_BIRD if (geometry and bird_ptr) else 0) | (L.OVERLAY_DETECTIONS if post else 0) | (L.OVERLAY_TRACKS if tracker else 0))
        h = lambda x: x.h if x else None     # the widest entry of its family: the narrower ones are masks over the same path
        mask = self.stage_mask(stages)       # "readouts" (only by name) has entries of its own: the others keep refusing its bit
        run = L.lib().adas_overlay_run_readouts if mask & L.OVERLAY_READOUTS else L.lib().adas_overlay_run_trajectories
        L.check(run(self.h, src_ptr, dst_ptr, h(decode), h(geometry), h(analysis), h(post), h(tracker), bird_ptr, mask, int(n_streams), int(n_frames), stream))

    def run_arrays(self, src_ptr, n_frames=1, lane_points=None, lane_counts=None, poly=None, poly_cap=0, poly_counts=None, area_status=None,
                   offset_type=None, area_bgr=None, dist_points=None, dist_cap=0, dist_counts=None, bird_points=None, bird_counts=None,
                   bird_ptr=None, stages=None, dst_ptr=None, stream=None, det_xyxy=None, det_cap=0, det_cls=None, det_counts=None, trk_tlwh=None,
                   trk_cap=0, trk_cls=None, trk_counts=None, trajectories=None, readouts=None):
        """The same kernels on raw device pointers (adas_overlay_run_arrays; with boxes adas_overlay_run_arrays_objects: det_xyxy
        [frames][det_cap][4] int32 + det_cls + det_counts, trk_tlwh [frames][trk_cap][4] fp64 + trk_cls + trk_counts, rows of activated
        tracked tracks).  trajectories=(traj_tlbr, traj_len): device pointers to the rows' trajectories [frames][trk_cap][30][4] fp64, oldest
        first, and their lengths [frames][trk_cap] -- the "trajectories" stage (adas_overlay_run_arrays_trajectories), which also needs the
        four trk_ arrays.  stages=None: every stage whose arrays are given ("tracks" not by the trk_ arrays alone when trajectories= is).
        readouts=(direction, veh_pos, curvature, offset): device pointers to [frames] int32 and three [frames] fp64 -- the "readouts" stage
        (adas_overlay_run_arrays_readouts), drawn on bird_ptr ahead of the bird stage's discs."""
        if stages is None:
            stages = ((L.OVERLAY_LANES if lane_points else 0) | (L.OVERLAY_AREA if poly else 0) | (L.OVERLAY_DISTANCE if dist_points else 0) |
                      (L.OVERLAY_BIRD if (bird_points and bird_ptr) else 0) | (L.OVERLAY_DETECTIONS if det_xyxy else 0) |
                      (L.OVERLAY_TRACKS if (trk_tlwh and trajectories is None) else 0) | (L.OVERLAY_TRAJECTORIES if trajectories is not None else 0) |
                      (L.OVERLAY_READOUTS if readouts is not None else 0))
        tr = trajectories if trajectories is not None else (None, None)
        a = L.OverlayArrays(                # the widest entry of its family: the narrower ones are masks over the same path
            d_src_bgr=src_ptr, d_dst_bgr=dst_ptr, d_lane_points=lane_points, d_lane_counts=lane_counts, d_poly=poly, d_poly_counts=poly_counts,
            d_area_status=area_status, d_offset_type=offset_type, d_area_bgr=area_bgr, d_dist_points=dist_points, d_dist_counts=dist_counts,
            d_bird_points=bird_points, d_bird_counts=bird_counts, d_bird_bgr=bird_ptr, d_det_xyxy=det_xyxy, d_det_cls=det_cls, d_det_counts=det_counts,
            d_trk_tlwh=trk_tlwh, d_trk_cls=trk_cls, d_trk_counts=trk_counts, d_traj_tlbr=tr[0], d_traj_len=tr[1], stream=stream, poly_cap=int(poly_cap),
            dist_cap=int(dist_cap), det_cap=int(det_cap), trk_cap=int(trk_cap), stages=self.stage_mask(stages), n_frames=int(n_frames))
        if readouts is None and not a.stages & L.OVERLAY_READOUTS:
            L.check(L.lib().adas_overlay_run_arrays_trajectories(self.h, C.byref(a)))
            return
        r = L.OverlayReadoutArrays(*(readouts if readouts is not None else (None,) * 4))
        L.check(L.lib().adas_overlay_run_arrays_readouts(self.h, C.byref(a), C.byref(r)))

    READOUT_STYLE = ("slot", "zoom", "offset_x", "offset_y", "radius_x", "radius_y", "text_color", "arrow_a_color", "arrow_b_color")

    def set_readout_style(self, **style):
        """The "readouts" stage's style from the next run on: slot (10: the font the strings are drawn in, set_fonts), zoom (2; 1 .. 4: the
        atlas is rendered at fontScale 3 / zoom and magnified, nearest neighbour), offset_x / offset_y (20, 80) and radius_x / radius_y
        (20, 180): the strings' origins, text_color (0, 0, 255), arrow_a_color (255, 255, 255), arrow_b_color (150, 150, 150)."""
        if getattr(self, "rs", None) is None:
            self.rs = L.OverlayReadoutStyle()
            L.check(L.lib().adas_overlay_default_readout_style(C.byref(self.rs)))
        rs = L.OverlayReadoutStyle.from_buffer_copy(self.rs)
        for k, v in style.items():
            if k not in self.READOUT_STYLE:
                raise TypeError("unknown overlay readout style %r" % k)
            if k.endswith("_color"):
                getattr(rs, k)[:] = [int(c) for c in v]
            else:
                setattr(rs, k, int(v))
        L.check(L.lib().adas_overlay_set_readout_style(self.h, C.byref(rs)))
        self.rs = rs

    def readout_record(self, frame=0):
        """What the device laid out for the frame in the last run with the "readouts" stage: dict(drawn, flags (L.OVERLAY_READOUT_RANGE),
        arrows: two marks in track_marks' layout (at veh_pos, at the centre), strings: two dicts (x, y, box, text, skipped): the offset,
        the radius).  Synchronises."""
        rec = np.zeros(1, L.READOUT_RECORD_DTYPE)
        L.check(L.lib().adas_overlay_fetch_readout(self.h, int(frame), L.ptr(rec)))
        r = rec[0]
        return dict(drawn=bool(r["drawn"]), flags=int(r["flags"]), arrows=r["arrows"].copy(),
                    strings=[dict(x=int(s["x"]), y=int(s["y"]), box=tuple(int(v) for v in s["box"]), skipped=bool(s["skipped"]),
                                  text=bytes(s["text"])[:int(s["len"])].decode("latin-1")) for s in r["strings"]])

    def fetch(self, frame=0):
        out = np.empty((self.src_hw[0], self.src_hw[1], 3), np.uint8)
        L.check(L.lib().adas_overlay_fetch(self.h, int(frame), L.ptr(out)))
        return out

    def device_view(self):
        p = C.c_void_p()
        L.check(L.lib().adas_overlay_device_view(self.h, C.byref(p)))
        return p.value

    def flags(self, frame=0):
        """ADAS_OVERLAY_* flags of the frame in the last run (L.OVERLAY_POLY_RANGE: a polygon vertex outside +-32767, the fill was skipped)."""
        f = C.c_int32()
        L.check(L.lib().adas_overlay_fetch_flags(self.h, int(frame), C.byref(f)))
        return int(f.value)

    def track_marks(self, frame=0):
        """The primitives the device built for the frame in the last run with the "trajectories" stage, in drawing order: a structured
        array (L.TRACK_MARK_DTYPE: kind L.TRACK_MARK_CIRCLE / _RECT / _ARROW, track row, x1, y1, x2, y2, radius, thickness, tip, color,
        skipped).  Synchronises."""
        n = C.c_int32()
        L.check(L.lib().adas_overlay_fetch_track_marks(self.h, int(frame), None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), L.TRACK_MARK_DTYPE)
        L.check(L.lib().adas_overlay_fetch_track_marks(self.h, int(frame), L.ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    # ---- the demo's three UI panels (adas_overlay_*panel*; rules P1-P6 of csrc/overlay_panel_core.h), in place on drawn frames
    PANELS = L.PANELS
    PANEL_PARAMS = ("show_ratio", "border", "signs_w", "signs_h", "signs_sprite_row", "collision_sprite_row", "collision_sprite_col", "border_color")

    @classmethod
    def panel_mask(cls, names):
        """An int, or names out of "bird", "signs", "collision"."""
        if isinstance(names, int):
            return names
        names = [names] if isinstance(names, str) else list(names)
        for n in names:
            if n not in cls.PANELS:
                raise ValueError("unknown overlay panel %r (one of %s)" % (n, ", ".join(cls.PANELS)))
        m = 0
        for n in names:
            m |= cls.PANELS[n]
        return m

    def set_panels(self, sprites, **params):
        """sprites: {name: (h, w, 4) uint8 BGRA array} by L.PANEL_SPRITES name ("fcws_warning", "fcws_prompt", "fcws_normal", "left", "right",
        "straight", "warn", "lta_left", "lta_right") -- the arrays ControlPanel.__init__ builds (cv2.imread(..., IMREAD_UNCHANGED) + cv2.resize);
        a missing or None entry is empty and draws nothing.  params: show_ratio (0.25), border (10), signs_w / signs_h (400 x 365),
        signs_sprite_row (10), collision_sprite_row (50), collision_sprite_col (5), border_color ((0, 0, 255)).  Raises when a rectangle or a
        sprite placement would leave the frame.  Resets the latches."""
        for k in sprites:
            if k not in L.PANEL_SPRITES:
                raise ValueError("unknown panel sprite %r (one of %s)" % (k, ", ".join(L.PANEL_SPRITES)))
        p = L.OverlayPanelParams()
        L.check(L.lib().adas_overlay_default_panel_params(C.byref(p)))
        for k, v in params.items():
            if k not in self.PANEL_PARAMS:
                raise TypeError("unknown overlay panel parameter %r" % k)
            if k == "border_color":
                for j in range(3):
                    p.border_color[j] = int(v[j])
            else:
                setattr(p, k, v)
        table, keep = (L.OverlaySprite * len(L.PANEL_SPRITES))(), []
        for i, name in enumerate(L.PANEL_SPRITES):
            a = sprites.get(name)
            if a is None:
                continue
            a = np.asarray(a)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4:
                raise ValueError("panel sprite %r must be an (h, w, 4) uint8 BGRA array, got %s %s" % (name, a.dtype, a.shape))
            a = np.ascontiguousarray(a)
            keep.append(a)
            table[i].bgra, table[i].w, table[i].h = a.ctypes.data, a.shape[1], a.shape[0]
        L.check(L.lib().adas_overlay_set_panels(self.h, C.byref(p), table))

    def run_panels(self, frames_ptr=None, analysis=None, bird_ptr=None, panels=None, n_streams=1, n_frames=1, stream=None):
        """The panels in place on the device frames frames_ptr (None: the handle's own buffer, what run() just wrote), from an Analysis
        handle's frame rows ("signs", "collision") and the bird-view image bird_ptr ("bird").  Frame b of stream s is frame b * n_streams + s;
        the curve_status latch of stream s lives on the device and walks its frames in order.  panels=None: every panel whose input is given."""
        if panels is None:
            panels = (L.PANEL_BIRD if bird_ptr else 0) | ((L.PANEL_SIGNS | L.PANEL_COLLISION) if analysis else 0)
        L.check(L.lib().adas_overlay_run_panels(self.h, frames_ptr, analysis.h if analysis else None, bird_ptr, self.panel_mask(panels), int(n_streams),
                                                int(n_frames), stream))

    def run_panels_arrays(self, frames_ptr=None, offset_type=None, curvature_type=None, collision_type=None, bird_ptr=None, panels=None, n_streams=1,
                          n_frames=1, stream=None):
        """The same kernels on raw device pointers to [n_streams * n_frames] int32 types (ADAS_OFFSET_* / ADAS_CURVATURE_* / ADAS_COLLISION_*)."""
        if panels is None:
            panels = ((L.PANEL_BIRD if bird_ptr else 0) | (L.PANEL_SIGNS if (offset_type and curvature_type) else 0) |
                      (L.PANEL_COLLISION if collision_type else 0))
        L.check(L.lib().adas_overlay_run_panels_arrays(self.h, frames_ptr, offset_type, curvature_type, collision_type, bird_ptr, self.panel_mask(panels),
                                                       int(n_streams), int(n_frames), stream))

    def reset_panels(self, stream=-1):
        """curve_status of stream `stream` back to None; -1: every stream."""
        L.check(L.lib().adas_overlay_reset_panels(self.h, int(stream)))

    def panel_record(self, frame=0):
        """What the device chose for the frame in the last panel run: {"signs": [names in paint order], "collision": name or None, "latch":
        None / "Left" / "Right" / "Straight" after the frame, "offset_type", "curvature_type", "collision_type": as read}.  Synchronises."""
        r = L.OverlayPanelRecord()
        L.check(L.lib().adas_overlay_fetch_panel_record(self.h, int(frame), C.byref(r)))
        return {"signs": [L.PANEL_SPRITES[s] for s in r.sign if s >= 0], "collision": L.PANEL_SPRITES[r.collision] if r.collision >= 0 else None,
                "latch": L.PANEL_LATCHES[r.latch], "offset_type": int(r.offset_type), "curvature_type": int(r.curvature_type),
                "collision_type": int(r.collision_type)}

    # ---- the text (adas_overlay_*text*, adas_overlay_set_font; rules T1-T7 of csrc/overlay_text_core.h), in place on drawn frames
    TEXT = L.TEXT
    FONT_KEYS = ("atlas", "glyph_x", "glyph_w", "bearing_x", "advance", "baseline_row", "size_h", "size_w_extra", "scale")

    @classmethod
    def text_mask(cls, names):
        """An int, or names out of "detections", "tracks", "track_ids", "distance", "panels", "lines"."""
        if isinstance(names, int):
            return names
        names = [names] if isinstance(names, str) else list(names)
        for n in names:
            if n not in cls.TEXT:
                raise ValueError("unknown overlay text %r (one of %s)" % (n, ", ".join(cls.TEXT)))
        m = 0
        for n in names:
            m |= cls.TEXT[n]
        return m

    def set_fonts(self, fonts):
        """fonts: {slot: atlas}, an atlas a dict (or the .npz tools/make_font_atlas.py writes) of "atlas" (cell_h, atlas_w) uint8 coverage,
        "glyph_x", "glyph_w", "bearing_x", "advance" (95,) for characters 32..126 (advance in 16.16), "baseline_row", "size_h",
        "size_w_extra" (16.16) and "scale".  The font is the caller's data: the package ships none."""
        for slot, f in fonts.items():
            missing = [k for k in self.FONT_KEYS if k not in f]
            if missing:
                raise ValueError("font slot %r lacks %s" % (slot, ", ".join(missing)))
            a = np.asarray(f["atlas"])
            if a.dtype != np.uint8 or a.ndim != 2:
                raise ValueError("font slot %r: the atlas must be a (cell_h, atlas_w) uint8 array, got %s %s" % (slot, a.dtype, a.shape))
            a = np.ascontiguousarray(a)
            t = L.OverlayFont()
            t.atlas, t.atlas_w, t.cell_h = a.ctypes.data, a.shape[1], a.shape[0]
            t.baseline_row, t.size_h, t.size_w_extra, t.scale = int(f["baseline_row"]), int(f["size_h"]), int(f["size_w_extra"]), float(f["scale"])
            for k in ("glyph_x", "glyph_w", "bearing_x", "advance"):
                v = np.asarray(f[k]).reshape(-1)
                if v.shape != (95,):
                    raise ValueError("font slot %r: %s must hold 95 values (characters 32..126), got %d" % (slot, k, v.size))
                getattr(t, k)[:] = [int(x) for x in v]
            L.check(L.lib().adas_overlay_set_font(self.h, int(slot), C.byref(t)))

    def set_text_style(self, **style):
        """Fields of adas_overlay_text_style (slots, ladders as *_first / *_count, offsets, colours, max_text_items) over the last style set."""
        if not hasattr(self, "ts"):
            self.ts = L.OverlayTextStyle()
            L.check(L.lib().adas_overlay_default_text_style(C.byref(self.ts)))
        for k, v in style.items():
            if k in ("offset_colors", "curvature_colors", "collision_colors"):
                for i, c in enumerate(v):
                    getattr(self.ts, k)[i][:] = [int(x) for x in c]
            elif k in ("label_color", "dist_color", "dist_shadow_color"):
                getattr(self.ts, k)[:] = [int(x) for x in v]
            elif k in L.TEXT_STYLE_INTS or k in ("show_ratio", "min_box_area"):
                setattr(self.ts, k, v)
            else:
                raise TypeError("unknown overlay text style %r" % k)
        L.check(L.lib().adas_overlay_set_text_style(self.h, C.byref(self.ts)))

    def set_text_labels(self, which, names):
        """Class names by id for "detections" or "tracks", at most 31 bytes each; an id outside the table prints 'unknown'."""
        which = self.stage_mask(which)
        enc = [n.encode("latin-1") if isinstance(n, str) else bytes(n) for n in names]
        arr = (C.c_char_p * max(1, len(enc)))(*enc)
        L.check(L.lib().adas_overlay_set_text_labels(self.h, which, arr, len(enc)))

    def set_text_lines(self, lines):
        """Up to 8 caller strings [(x, y, slot, (b, g, r), text of at most 47 bytes)], drawn last on every frame ("lines")."""
        lines = list(lines)
        if len(lines) > L.TEXT_MAX_LINES:
            raise ValueError("%d text lines, at most %d" % (len(lines), L.TEXT_MAX_LINES))
        t = (L.OverlayTextLine * max(1, len(lines)))()
        for i, (x, y, slot, colour, text) in enumerate(lines):
            b = text.encode("latin-1") if isinstance(text, str) else bytes(text)
            if len(b) > 47:
                raise ValueError("text line %d holds %d bytes, at most 47" % (i, len(b)))
            t[i].x, t[i].y, t[i].slot, t[i].len, t[i].text = int(x), int(y), int(slot), len(b), b
            t[i].color[:] = [int(c) for c in colour]
        L.check(L.lib().adas_overlay_set_text_lines(self.h, t, len(lines)))

    def run_text(self, frames_ptr=None, post=None, tracker=None, analysis=None, text=None, n_streams=1, n_frames=1, stream=None):
        """The text `text` (names or a mask; None: every kind whose handle is given, and "lines") in place on the device frames frames_ptr
        (None: the handle's own buffer, what run() just wrote), from the handles' device arrays: post= a YoloPost ("detections"), tracker= a
        DeviceTracker ("tracks", "track_ids": n_frames must be 1), analysis= an Analysis ("distance", "panels")."""
        if text is None:
            T = L.TEXT
            text = ((T["detections"] if post else 0) | ((T["tracks"] | T["track_ids"]) if tracker else 0) |
                    ((T["distance"] | T["panels"]) if analysis else 0) | T["lines"])
        h = lambda x: x.h if x else None
        L.check(L.lib().adas_overlay_run_text(self.h, frames_ptr, h(post), h(tracker), h(analysis), self.text_mask(text), int(n_streams), int(n_frames),
                                              stream))

    def run_text_arrays(self, frames_ptr=None, text=0, n_streams=1, n_frames=1, stream=None, det_cap=0, trk_cap=0, dist_cap=0, **arrays):
        """The text `text` (names or a mask) in place on the device frames frames_ptr (None: the handle's own buffer) from raw device pointers,
        by the field names of adas_overlay_text_arrays without their d_ (det_xyxy, det_cls, det_counts, trk_tlwh, trk_cls, trk_ids, trk_counts,
        trk_last_tlbr, traj_len, dist_points, dist_d, dist_counts, offset_type, curvature_type, collision_type)."""
        a = L.OverlayTextArrays(det_cap=int(det_cap), trk_cap=int(trk_cap), dist_cap=int(dist_cap))
        for k, v in arrays.items():
            if not hasattr(a, "d_" + k):
                raise TypeError("unknown text array %r" % k)
            setattr(a, "d_" + k, v)
        L.check(L.lib().adas_overlay_run_text_arrays(self.h, frames_ptr, C.byref(a), self.text_mask(text), int(n_streams), int(n_frames), stream))

    def text_items(self, frame=0):
        """The frame's item list of the last text run, in paint order: a structured array (L.TEXT_ITEM_DTYPE: kind L.TEXT_ITEM_RECT / _RUN,
        source bit, x, y, x1, y1, box (clipped, half open), slot, color, len, text).  Synchronises."""
        n = C.c_int32()
        L.check(L.lib().adas_overlay_fetch_text_items(self.h, int(frame), None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), L.TEXT_ITEM_DTYPE)
        L.check(L.lib().adas_overlay_fetch_text_items(self.h, int(frame), L.ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    def text_flags(self, frame=0):
        """L.OVERLAY_TEXT_RANGE | L.OVERLAY_TEXT_OVERFLOW of the frame in the last text run.  Synchronises."""
        f = C.c_int32()
        L.check(L.lib().adas_overlay_fetch_text_flags(self.h, int(frame), C.byref(f)))
        return int(f.value)

    def close(self):
        if getattr(self, "h", None):
            L.lib().adas_overlay_destroy(self.h)
            self.h = None

    __del__ = close


class JpegEncoder:
    """Baseline JPEG of BGR u8 frames that sit in HBM (adas_jpeg_*): what the demo's vout.write(frame_show) gets, as one compressed stream per
    frame -- 4:2:0, the standard's Annex K tables scaled by `quality` (1..100), one restart interval per MCU row, any frame size.  The rules
    J1-J9 are csrc/jpeg_core.h; any JPEG decoder reads the streams, and concatenated they are a raw MJPEG file.
    capacity: bytes per frame of the stream buffer (None: width * height * 3; JpegEncoder.bound(width, height) always fits).  A frame whose
    stream would not fit comes back as b"" with the overflow flag in lengths(); the other frames of the run are unaffected."""
    OVERFLOW = L.JPEG_OVERFLOW

    @staticmethod
    def bound(width, height):
        """The most bytes a frame of this size can take at any quality."""
        return int(L.lib().adas_jpeg_bound(int(width), int(height)))

    def __init__(self, width, height, quality=90, max_batch=1, capacity=None):
        self.p = L.JpegParams(int(width), int(height), int(quality), 0, int(capacity or 0))
        self.width, self.height, self.max_batch = int(width), int(height), int(max_batch)
        self.capacity = int(capacity) if capacity else self.width * self.height * 3
        h = C.c_void_p()
        L.check(L.lib().adas_jpeg_create(C.byref(self.p), self.max_batch, C.byref(h)))
        self.h = h.value
        self._host = L.PinnedBuffer((self.capacity,))      # page-locked: a fetch is one small copy for the length and one for the bytes

    def set_quality(self, quality):
        """From the next run on; a captured run picks the new tables up.  Synchronises."""
        L.check(L.lib().adas_jpeg_set_quality(self.h, int(quality)))

    def run(self, d_frames, batch=1, stream=None):
        """d_frames: device pointer of [batch][height][width][3] u8, any alignment.  Asynchronous on `stream`."""
        L.check(L.lib().adas_jpeg_run(self.h, d_frames, int(batch), stream))

    def fetch(self, frame=0):
        """The stream of frame `frame` of the last run as bytes (b"" for a frame that overflowed).  Waits for that run."""
        n = C.c_int64()
        L.check(L.lib().adas_jpeg_fetch(self.h, int(frame), self._host.ptr, self.capacity, C.byref(n), None))
        return self._host.array[:n.value].tobytes()

    def lengths(self, batch=1):
        """(lengths [batch] int64, flags [batch] int32) of the last run.  Waits for that run."""
        n, f = np.zeros(int(batch), np.int64), np.zeros(int(batch), np.int32)
        L.check(L.lib().adas_jpeg_fetch_lengths(self.h, int(batch), L.ptr(n), L.ptr(f)))
        return n, f

    def device_view(self):
        """(device pointer of the streams, device pointer of the int64 lengths, bytes between two frames' streams)."""
        d, n, s = C.c_void_p(), C.c_void_p(), C.c_int64()
        L.check(L.lib().adas_jpeg_device_view(self.h, C.byref(d), C.byref(n), C.byref(s)))
        return d.value, n.value, int(s.value)

    def close(self):
        if getattr(self, "h", None):
            L.lib().adas_jpeg_destroy(self.h)
            self.h = None
            self._host.free()

    __del__ = close


def host_streams(streams):
    """A list of bytes-like objects -> (array of their addresses, int64 array of their lengths, what keeps them alive during the call)."""
    keep = [np.frombuffer(s, np.uint8) if len(s) else np.zeros(1, np.uint8) for s in streams]
    ptrs = (C.c_void_p * len(keep))(*[k.ctypes.data for k in keep])
    lengths = np.array([len(s) for s in streams], np.int64)
    return ptrs, lengths, keep


def split_mjpeg(data):
    """A raw MJPEG file (concatenated JPEG streams, what JpegEncoder's streams are when appended) -> [(stream bytes, (width, height) or None)].
    Every stream is walked marker by marker: the segments in front of the scan by their lengths, the entropy data up to the first marker
    that is neither a restart marker nor a stuffed 0xFF; a stream runs from its SOI to its EOI (or to the next SOI / the file's end when
    the EOI is missing).  The size is SOFn's; None when the stream has none in front of its scan."""
    data = bytes(data)
    out, i, n = [], 0, len(data)
    while True:
        a = data.find(b"\xff\xd8", i)
        if a < 0:
            return out
        p, size = a + 2, None
        while p + 4 <= n and data[p] == 0xFF:              # marker segments
            m = data[p + 1]
            if m == 0xFF:
                p += 1
                continue
            if m in (0xD8, 0xD9):
                break
            if m == 0x01 or 0xD0 <= m <= 0xD7:
                p += 2
                continue
            length = int.from_bytes(data[p + 2:p + 4], "big")
            if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC) and length >= 7:
                size = (int.from_bytes(data[p + 7:p + 9], "big"), int.from_bytes(data[p + 5:p + 7], "big"))
            p += 2 + length
            if m == 0xDA:                                  # entropy data
                while True:
                    p = data.find(b"\xff", p)
                    if p < 0 or p + 1 >= n:
                        p = n
                        break
                    if data[p + 1] in (0x00, 0xFF) or 0xD0 <= data[p + 1] <= 0xD7:
                        p += 1 if data[p + 1] == 0xFF else 2
                        continue
                    break
        end = p + 2 if p + 2 <= n and data[p:p + 2] == b"\xff\xd9" else min(max(p, a + 2), n)
        out.append((data[a:end], size))
        i = end


class JpegDecoder:
    """Baseline JPEG decoding on the device (adas_jpegdec_*): compressed camera frames in -- from the host, or where a JpegEncoder left them --
    BGR u8 frames out in HBM, where AdasPipeline.step_frames reads them.  Grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0, the stream's own tables, any
    restart interval (restart segments decode in parallel; a stream without restart markers on one lane).  The rules D1-D9 are
    csrc/jpegdec_core.h.  Stream content never raises: flags(n) holds one word per frame, and a frame flagged UNSUPPORTED, FORMAT or SIZE is
    black; CORRUPT marks an error in the entropy data, after which the rest of that restart segment is flat.
    capacity: the most bytes per stream (None: JpegEncoder.bound(width, height))."""
    UNSUPPORTED, FORMAT, SIZE, CORRUPT = L.JPEGDEC_UNSUPPORTED, L.JPEGDEC_FORMAT, L.JPEGDEC_SIZE, L.JPEGDEC_CORRUPT

    def __init__(self, width, height, max_batch=1, capacity=None):
        self.p = L.JpegDecParams(int(width), int(height), (C.c_int32 * 2)(0, 0), int(capacity or 0))
        self.width, self.height, self.max_batch = int(width), int(height), int(max_batch)
        h = C.c_void_p()
        L.check(L.lib().adas_jpegdec_create(C.byref(self.p), self.max_batch, C.byref(h)))
        self.h = h.value
        self.capacity = int(capacity) if capacity else JpegEncoder.bound(width, height)

    def run_host(self, streams, d_dst=None, stream=None):
        """streams: a list of bytes, one JPEG stream per frame.  Asynchronous on `stream`; the bytes are free again on return.  d_dst: device
        pointer of [len(streams)][height][width][3] u8 (None: the handle's own frames)."""
        ptrs, lengths, keep = host_streams(streams)
        L.check(L.lib().adas_jpegdec_run_host(self.h, ptrs, L.ptr(lengths), len(streams), d_dst, stream))

    def run_device(self, d_ptr, d_lengths_ptr, stride, n, d_dst=None, stream=None):
        """Streams on the device: frame f at d_ptr + f * stride (any byte), its int64 length at d_lengths_ptr[f]: JpegEncoder.device_view()."""
        L.check(L.lib().adas_jpegdec_run(self.h, d_ptr, d_lengths_ptr, int(stride), int(n), d_dst, stream))

    def image(self, frame=0):
        """Frame `frame` of the last run into the handle's own frames: (height, width, 3) uint8 BGR.  Waits for that run."""
        out = np.empty((self.height, self.width, 3), np.uint8)
        L.check(L.lib().adas_jpegdec_fetch(self.h, int(frame), L.ptr(out)))
        return out

    def flags(self, n=1):
        """The flag words of the last run's first n frames (int32).  Waits for that run."""
        f = np.zeros(int(n), np.int32)
        L.check(L.lib().adas_jpegdec_fetch_flags(self.h, int(n), L.ptr(f)))
        return f

    def device_view(self):
        """(device pointer of the handle's frames [max_batch][height][width][3], device pointer of the int32 flags)."""
        d, f = C.c_void_p(), C.c_void_p()
        L.check(L.lib().adas_jpegdec_device_view(self.h, C.byref(d), C.byref(f)))
        return d.value, f.value

    def close(self):
        if getattr(self, "h", None):
            L.lib().adas_jpegdec_destroy(self.h)
            self.h = None

    __del__ = close


class YuvConverter:
    """Uncompressed camera formats into BGR on the device (adas_yuv_*): "nv12", "nv21", "i420", "yuyv" or "uyvy" frames in -- from the host, or
    where a decoder left them -- BGR u8 frames out in HBM, where AdasPipeline.step_frames reads them.  What a caller's
    cv2.cvtColor(frame, cv2.COLOR_YUV2BGR_NV12 / _I420 / _YUY2 / _UYVY) does on host cores.  The rules C1-C7 are csrc/yuv_core.h.
    matrix: "video" (BT.601 limited range, cv2's) or "full" (JFIF, the JPEG decoder's).  layout: None for tightly packed frames, or a dict
    out of frame_stride, y_offset, y_pitch, u_offset, u_pitch, v_offset, v_pitch (bytes) over the tight values -- what a decoder or V4L2
    reports for padded rows and planes; YV12 is "i420" with u_offset and v_offset exchanged.  frame_bytes: the bytes of a frame that are
    read; a batch of n frames is (n - 1) * params.frame_stride + frame_bytes bytes."""

    def __init__(self, format, width, height, matrix="video", layout=None, max_batch=1):
        if format not in L.YUV_FORMATS:
            raise ValueError("format %r is none of %s" % (format, sorted(L.YUV_FORMATS)))
        if matrix not in L.YUV_MATRICES:
            raise ValueError("matrix %r is neither \"video\" nor \"full\"" % (matrix,))
        unknown = set(layout or {}) - set(L.YUV_LAYOUT_FIELDS)
        if unknown:
            raise ValueError("layout= holds unknown keys %s (%s)" % (sorted(unknown), ", ".join(L.YUV_LAYOUT_FIELDS)))
        self.p = L.YuvParams()
        L.check(L.lib().adas_yuv_default_params(C.byref(self.p), L.YUV_FORMATS[format], int(width), int(height)))
        self.p.matrix = L.YUV_MATRICES[matrix]
        for k, v in (layout or {}).items():
            setattr(self.p, k, int(v))
        self.format, self.matrix, self.width, self.height, self.max_batch = format, matrix, int(width), int(height), int(max_batch)
        h = C.c_void_p()
        L.check(L.lib().adas_yuv_create(C.byref(self.p), self.max_batch, C.byref(h)))
        self.h = h.value
        self.frame_bytes = int(L.lib().adas_yuv_frame_bytes(C.byref(self.p)))

    def batch_bytes(self, n):
        return (int(n) - 1) * int(self.p.frame_stride) + self.frame_bytes

    def run_device(self, d_ptr, n, d_dst=None, stream=None):
        """n frames on the device, frame f at d_ptr + f * frame_stride (any byte).  Asynchronous on `stream`.  d_dst: device pointer of
        [n][height][width][3] u8 (None: the handle's own frames)."""
        L.check(L.lib().adas_yuv_run(self.h, d_ptr, int(n), d_dst, stream))

    def run_host(self, frames, n, d_dst=None, stream=None):
        """n frames on the host: a uint8 array (or a host pointer) of batch_bytes(n) bytes; pinned memory (_lib.PinnedBuffer) makes the copy
        asynchronous, and the bytes must then stay as they are until `stream` has passed it."""
        if isinstance(frames, np.ndarray):
            if frames.dtype != np.uint8 or not frames.flags.c_contiguous or frames.nbytes < self.batch_bytes(n):
                raise ValueError("run_host needs a contiguous uint8 array of at least %d bytes" % self.batch_bytes(n))
            frames = L.ptr(frames)
        L.check(L.lib().adas_yuv_run_host(self.h, frames, int(n), d_dst, stream))

    def image(self, frame=0):
        """Frame `frame` of the last run into the handle's own frames: (height, width, 3) uint8 BGR.  Waits for that run."""
        out = np.empty((self.height, self.width, 3), np.uint8)
        L.check(L.lib().adas_yuv_fetch(self.h, int(frame), L.ptr(out)))
        return out

    def device_view(self):
        """Device pointer of the handle's frames [max_batch][height][width][3]."""
        d = C.c_void_p()
        L.check(L.lib().adas_yuv_device_view(self.h, C.byref(d)))
        return d.value

    def close(self):
        if getattr(self, "h", None):
            L.lib().adas_yuv_destroy(self.h)
            self.h = None

    __del__ = close


def yuv_output_args(format="i420", matrix="video", chroma="mean", layout=None, what=""):
    """YuvWriter's argument checks without a handle (so without a GPU): ValueError naming the key."""
    if format not in L.YUV_FORMATS:
        raise ValueError("%sformat %r is none of %s" % (what, format, sorted(L.YUV_FORMATS)))
    if matrix not in L.YUV_MATRICES:
        raise ValueError("%smatrix %r is neither \"video\" nor \"full\"" % (what, matrix))
    if chroma not in L.YUVOUT_CHROMA:
        raise ValueError("%schroma %r is neither \"mean\" nor \"first\"" % (what, chroma))
    if layout is not None and not isinstance(layout, dict):
        raise ValueError("%slayout %r is neither None nor a dict out of %s" % (what, layout, ", ".join(L.YUV_LAYOUT_FIELDS)))
    unknown = set(layout or {}) - set(L.YUV_LAYOUT_FIELDS)
    if unknown:
        raise ValueError("%slayout= holds unknown keys %s (%s)" % (what, sorted(unknown), ", ".join(L.YUV_LAYOUT_FIELDS)))


class YuvWriter:
    """BGR frames on the device into uncompressed video formats (adas_yuvout_*), the inverse of YuvConverter: "nv12", "nv21", "i420", "yuyv" or
    "uyvy" frames out, 1.5 or 2 bytes per pixel in place of 3, for any encoder that is not MJPEG (x264, `ffmpeg -f rawvideo -pix_fmt
    yuv420p`, a V4L2 loopback): what cv2.VideoWriter.write or a caller's cv2.cvtColor(frame, cv2.COLOR_BGR2YUV_I420) does on host cores.  The
    rules E1-E7 are csrc/yuvout_core.h.  matrix: "video" (BT.601 limited range) or "full" (JFIF, the JPEG encoder's).  chroma: "mean" (a
    chroma sample is the rounded mean of its cell, what encoders' scalers do) or "first" (its first pixel's).  layout: as YuvConverter's, now
    the destination's -- bytes no plane row owns are never written; YV12 is "i420" with u_offset and v_offset exchanged.  frame_bytes: the
    bytes of a frame up to the end of its last plane; n frames are (n - 1) * params.frame_stride + frame_bytes bytes."""

    def __init__(self, format, width, height, matrix="video", chroma="mean", layout=None, max_batch=1):
        yuv_output_args(format, matrix, chroma, layout)
        self.p = L.YuvOutParams()
        L.check(L.lib().adas_yuvout_default_params(C.byref(self.p), L.YUV_FORMATS[format], int(width), int(height)))
        self.p.matrix = L.YUV_MATRICES[matrix]
        self.p.chroma = L.YUVOUT_CHROMA[chroma]
        for k, v in (layout or {}).items():
            setattr(self.p, k, int(v))
        self.format, self.matrix, self.chroma, self.width, self.height, self.max_batch = format, matrix, chroma, int(width), int(height), int(max_batch)
        h = C.c_void_p()
        L.check(L.lib().adas_yuvout_create(C.byref(self.p), self.max_batch, C.byref(h)))
        self.h = h.value
        self.frame_bytes = int(L.lib().adas_yuvout_frame_bytes(C.byref(self.p)))

    def batch_bytes(self, n):
        return (int(n) - 1) * int(self.p.frame_stride) + self.frame_bytes

    def run_device(self, d_bgr, n, d_dst=None, stream=None):
        """n BGR frames [n][height][width][3] u8 on the device (any byte).  Asynchronous on `stream`.  d_dst: device pointer of batch_bytes(n)
        bytes, frame f at d_dst + f * frame_stride (None: the handle's own buffer)."""
        L.check(L.lib().adas_yuvout_run(self.h, d_bgr, int(n), d_dst, stream))

    def frame(self, i=0):
        """Frame i of the last run into the handle's own buffer: uint8 [frame_bytes].  Waits for that run."""
        out = np.empty(self.frame_bytes, np.uint8)
        L.check(L.lib().adas_yuvout_fetch(self.h, int(i), L.ptr(out)))
        return out

    def planes_of(self, buf):
        """Views of a frame's bytes: (Y [h][w], U [h/2][w/2], V [h/2][w/2]) for "i420", (Y, UV [h/2][w/2][2]) for "nv12" (VU for "nv21")."""
        if self.format in ("yuyv", "uyvy"):
            raise ValueError("format %r is packed: it has no planes" % (self.format,))
        as_strided = np.lib.stride_tricks.as_strided
        w, h, p = self.width, self.height, self.p
        y = as_strided(buf[p.y_offset:], (h, w), (p.y_pitch, 1), writeable=False)
        if self.format == "i420":
            return (y, as_strided(buf[p.u_offset:], (h // 2, w // 2), (p.u_pitch, 1), writeable=False),
                    as_strided(buf[p.v_offset:], (h // 2, w // 2), (p.v_pitch, 1), writeable=False))
        return y, as_strided(buf[p.u_offset:], (h // 2, w // 2, 2), (p.u_pitch, 2, 1), writeable=False)

    def planes(self, i=0):
        """planes_of(frame(i))"""
        if self.format in ("yuyv", "uyvy"):
            raise ValueError("format %r is packed: it has no planes" % (self.format,))
        return self.planes_of(self.frame(i))

    def fetch_all(self, n, out=None):
        """The first n frames of the last run in ONE copy: uint8 [batch_bytes(n)], frame f at f * frame_stride.  out: a uint8 array of at least
        that size to fill (_lib.PinnedBuffer(...).array for the fastest copy); the filled part is returned."""
        need = self.batch_bytes(n)
        if out is None:
            out = np.empty(need, np.uint8)
        elif not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < need:
            raise ValueError("fetch_all needs a contiguous uint8 array of at least %d bytes" % need)
        L.check(L.lib().adas_yuvout_fetch_all(self.h, int(n), L.ptr(out)))
        return out.reshape(-1)[:need]

    def device_view(self):
        """Device pointer of the handle's own frames, frame f at f * frame_stride."""
        d = C.c_void_p()
        L.check(L.lib().adas_yuvout_device_view(self.h, C.byref(d)))
        return d.value

    def close(self):
        if getattr(self, "h", None):
            L.lib().adas_yuvout_destroy(self.h)
            self.h = None

    __del__ = close


SCALE_DEFAULT_BORDER_COLORS = ((0, 255, 255), (0, 255, 0), (0, 102, 255), (0, 0, 255))   # demo.py's ControlPanel.CollisionDict, BGR


def _bgr(v, what):
    try:
        c = tuple(int(x) for x in v)
    except (TypeError, ValueError):
        c = ()
    if len(c) != 3 or any(x < 0 or x > 255 for x in c) or any(int(x) != x for x in v):
        raise ValueError("%s %r is no (B, G, R) of integers in 0..255" % (what, v))
    return c


def _pair(v, what, lo=1):
    try:
        a, b = v
        ok = int(a) == a and int(b) == b and a >= lo and b >= lo
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s %r is no pair of integers >= %d" % (what, v, lo))
    return int(a), int(b)


def scale_args(src_wh, size, mode="area", mosaic=(1, 1), border=0, background=(0, 0, 0), border_colors=None, what=""):
    """FrameScaler's argument checks without a handle (so without a GPU): ValueError naming the key.  Returns the checked values as a dict."""
    if mode not in L.SCALE_MODES:
        raise ValueError("%smode %r is neither \"area\" nor \"linear\"" % (what, mode))
    sw, sh = _pair(src_wh, what + "src_wh")
    dw, dh = _pair(size, what + "size")
    cols, rows = _pair(mosaic, what + "mosaic")
    if max(sw, sh, dw, dh, cols, rows) > 16383:
        raise ValueError("%ssides and mosaic counts must stay within 16383 (src_wh %r, size %r, mosaic %r)" % (what, src_wh, size, mosaic))
    if mode == "area" and (dw > sw or dh > sh):
        raise ValueError("%smode \"area\" does not enlarge: size %r from %r" % (what, (dw, dh), (sw, sh)))
    if mode == "area" and sw * sh > 1 << 23:
        raise ValueError("%smode \"area\" needs src_w * src_h <= 8388608, got %r" % (what, (sw, sh)))
    if isinstance(border, bool) or not isinstance(border, int) or border < 0 or 2 * border >= min(dw, dh):
        raise ValueError("%sborder %r must be an integer >= 0 with 2 * border < min(size)" % (what, border))
    if cols * dw * 3 * rows * dh > 0x7fffffff:
        raise ValueError("%sa canvas of %dx%d tiles of %r must stay below 2^31 bytes" % (what, cols, rows, (dw, dh)))
    colors = SCALE_DEFAULT_BORDER_COLORS if border_colors is None else border_colors
    try:
        n = len(colors)
    except TypeError:
        n = -1
    if n != 4:
        raise ValueError("%sborder_colors %r is no list of four (B, G, R): UNKNOWN, NORMAL, PROMPT, WARNING" % (what, border_colors))
    return dict(src_wh=(sw, sh), size=(dw, dh), mode=mode, mosaic=(cols, rows), border=border, background=_bgr(background, what + "background"),
                border_colors=tuple(_bgr(c, what + "border_colors[%d]" % i) for i, c in enumerate(colors)))


class FrameScaler:
    """Finished BGR frames on the device reduced to previews or a mosaic (adas_scale_*): every frame becomes a tile of `size` (w, h), a canvas
    is mosaic = (cols, rows) tiles, frame f goes to canvas f // (cols * rows) and cell f % (cols * rows) in row-major order; (1, 1) is one
    reduced frame per frame.  What a caller's cv2.resize per frame and NumPy slice assignments do on host cores after fetching every full
    frame.  The rules S1-S8 are csrc/scale_core.h.  mode: "area" (an exact integer box filter, reduction only) or "linear" (8-bit
    INTER_LINEAR, the bird panel's rule).  border: pixel rings of a tile that take border_colors[state] when a run is given states
    (ANA_COLLISION_*: UNKNOWN, NORMAL, PROMPT, WARNING).  background: the (B, G, R) of a cell without a frame.  canvas_hw: (rows * h,
    cols * w)."""

    def __init__(self, src_wh, size, mode="area", mosaic=(1, 1), border=0, background=(0, 0, 0), border_colors=None, max_batch=1):
        a = scale_args(src_wh, size, mode, mosaic, border, background, border_colors)
        self.p = L.ScaleParams()
        L.check(L.lib().adas_scale_default_params(C.byref(self.p), a["src_wh"][0], a["src_wh"][1], a["size"][0], a["size"][1]))
        self.p.mode = L.SCALE_MODES[mode]
        self.p.cols, self.p.rows = a["mosaic"]
        self.p.border = a["border"]
        for c in range(3):
            self.p.background[c] = a["background"][c]
            for k in range(4):
                self.p.border_bgr[k][c] = a["border_colors"][k][c]
        self.src_wh, self.size, self.mode, self.mosaic, self.border, self.max_batch = a["src_wh"], a["size"], mode, a["mosaic"], a["border"], int(max_batch)
        self.canvas_hw = (self.mosaic[1] * self.size[1], self.mosaic[0] * self.size[0])
        h = C.c_void_p()
        L.check(L.lib().adas_scale_create(C.byref(self.p), self.max_batch, C.byref(h)))
        self.h = h.value
        self.canvas_bytes = int(L.lib().adas_scale_canvas_bytes(C.byref(self.p)))

    def canvases(self, n):
        """Canvases a run of n frames writes."""
        return -(-int(n) // (self.mosaic[0] * self.mosaic[1]))

    def run_device(self, d_ptr, n, d_state=None, state_stride=4, d_dst=None, stream=None):
        """n BGR frames [n][src_h][src_w][3] u8 on the device (any byte).  d_state: frame f's int32 state at d_state + f * state_stride bytes
        (None: no border is drawn).  d_dst: device pointer of canvases(n) * canvas_bytes bytes (None: the handle's own buffer).  Asynchronous
        on `stream`."""
        L.check(L.lib().adas_scale_run(self.h, d_ptr, int(n), d_state, int(state_stride), d_dst, stream))

    def canvas(self, i=0):
        """Canvas i of the last run into the handle's own buffer: uint8 [rows * h][cols * w][3].  Waits for that run."""
        out = np.empty(self.canvas_hw + (3,), np.uint8)
        L.check(L.lib().adas_scale_fetch(self.h, int(i), L.ptr(out)))
        return out

    def fetch_all(self, n, out=None):
        """The canvases of the last run's first n frames in ONE copy: uint8 [canvases(n)][rows * h][cols * w][3].  out: a uint8 array of at
        least that size to fill (_lib.PinnedBuffer(...).array for the fastest copy); the filled part is returned."""
        k = self.canvases(n)
        need = k * self.canvas_bytes
        if out is None:
            out = np.empty(need, np.uint8)
        elif not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < need:
            raise ValueError("fetch_all needs a contiguous uint8 array of at least %d bytes" % need)
        L.check(L.lib().adas_scale_fetch_all(self.h, k, L.ptr(out)))
        return out.reshape(-1)[:need].reshape((k,) + self.canvas_hw + (3,))

    def device_view(self):
        """Device pointer of the handle's own canvases, canvas k at k * canvas_bytes."""
        d = C.c_void_p()
        L.check(L.lib().adas_scale_device_view(self.h, C.byref(d)))
        return d.value

    def close(self):
        if getattr(self, "h", None):
            L.lib().adas_scale_destroy(self.h)
            self.h = None

    __del__ = close


def remap_camera(cam, what=""):
    """A lens model as FrameRemapper takes it, checked without a handle: dict(K=, D=, new_K=None, R=None).  K and new_K: (fx, fy, cx, cy) or
    cv2's 3x3 camera matrix; D: 4, 5 or 8 of cv2's (k1, k2, p1, p2, k3, k4, k5, k6), zero-padded; new_K defaults to K (cv2.undistort's
    default), R to the identity.  Returns dict(K, D, new_K, R) of float tuples; ValueError naming the key."""
    if not isinstance(cam, dict):
        raise ValueError("%scamera %r is no dict (K, D, new_K, R)" % (what, cam))
    unknown = set(cam) - {"K", "D", "new_K", "R"}
    if unknown:
        raise ValueError("%scamera holds unknown keys %s (K, D, new_K, R)" % (what, sorted(unknown)))
    if cam.get("K") is None:
        raise ValueError("%scamera needs K: (fx, fy, cx, cy) or the 3x3 camera matrix" % what)

    def numbers(key, v, sizes, camera_matrix=False):
        try:
            a = np.asarray(v, np.float64)
        except (TypeError, ValueError):
            a = np.zeros((2, 0))
        if camera_matrix and a.shape == (3, 3):
            a = np.array([a[0, 0], a[1, 1], a[0, 2], a[1, 2]])
        a = a.reshape(-1)
        if a.size not in sizes:
            raise ValueError("%scamera %s %r has the wrong shape (%s numbers%s)" % (what, key, v, " or ".join(str(s) for s in sizes),
                                                                                  " or a 3x3 matrix" if camera_matrix else ""))
        if not np.isfinite(a).all():
            raise ValueError("%scamera %s %r holds a non-finite parameter" % (what, key, v))
        return a

    K = numbers("K", cam["K"], (4,), True)
    D = numbers("D", () if cam.get("D") is None else cam["D"], (0, 4, 5, 8))
    new_K = K if cam.get("new_K") is None else numbers("new_K", cam["new_K"], (4,), True)
    R = np.eye(3).reshape(9) if cam.get("R") is None else numbers("R", cam["R"], (9,))
    return dict(K=tuple(map(float, K)), D=tuple(map(float, np.concatenate([D, np.zeros(8 - D.size)]))), new_K=tuple(map(float, new_K)),
                R=tuple(map(float, R)))


def remap_maps(maps, dst_hw, what=""):
    """Caller maps as FrameRemapper takes them: a list of (xy, frac), xy (h, w, 2) int16 and frac (h, w) uint16 -- what
    cv2.initUndistortRectifyMap(..., cv2.CV_16SC2) and cv2.convertMaps return.  ValueError naming the entry."""
    try:
        pairs = [tuple(m) for m in maps]
    except TypeError:
        pairs = None
    if not pairs or any(len(m) != 2 for m in pairs):
        raise ValueError("%smaps %r is no list of (xy, frac) pairs" % (what, type(maps).__name__))
    h, w = int(dst_hw[0]), int(dst_hw[1])
    out = []
    for i, (xy, frac) in enumerate(pairs):
        xy, frac = np.asarray(xy), np.asarray(frac)
        if xy.dtype != np.int16 or xy.shape != (h, w, 2):
            raise ValueError("%smaps[%d] xy is %s %s, not int16 (%d, %d, 2)" % (what, i, xy.dtype, xy.shape, h, w))
        if frac.dtype != np.uint16 or frac.shape != (h, w):
            raise ValueError("%smaps[%d] frac is %s %s, not uint16 (%d, %d)" % (what, i, frac.dtype, frac.shape, h, w))
        out.append((np.ascontiguousarray(xy), np.ascontiguousarray(frac)))
    return out


def remap_stream_map(stream_map, n_streams, n_maps, what=""):
    """The map of every stream: None is stream s -> map min(s, n_maps - 1).  ValueError naming the entry."""
    if stream_map is None:
        return [min(s, n_maps - 1) for s in range(n_streams)]
    try:
        sm = [int(v) for v in stream_map]
        ok = all(int(v) == v for v in stream_map)
    except (TypeError, ValueError):
        sm, ok = [], False
    if not ok or len(sm) != n_streams:
        raise ValueError("%sstream_map %r is no list of %d map indices, one per stream" % (what, stream_map, n_streams))
    for s, m in enumerate(sm):
        if not 0 <= m < n_maps:
            raise ValueError("%sstream_map[%d] = %d is outside the %d maps" % (what, s, m, n_maps))
    return sm


def undistort_args(undistort, n_streams, src_hw):
    """AdasPipeline(undistort=)'s checks without a handle (so without a GPU): ValueError naming the key.  Returns dict(cameras= | maps=,
    stream_map=) as FrameRemapper takes them; identical cameras share one map."""
    keys = "camera, cameras, maps, stream_map"
    if not isinstance(undistort, dict):
        raise ValueError("undistort= %r is neither None nor a dict (%s)" % (undistort, keys))
    unknown = set(undistort) - {"camera", "cameras", "maps", "stream_map"}
    if unknown:
        raise ValueError("undistort= holds unknown keys %s (%s)" % (sorted(unknown), keys))
    given = [k for k in ("camera", "cameras", "maps") if undistort.get(k) is not None]
    if len(given) != 1:
        raise ValueError("undistort= needs exactly one of camera=, cameras= and maps= (got %s)" % (given or "none"))
    if given[0] == "maps":
        maps = remap_maps(undistort["maps"], src_hw, what="undistort= ")
        return dict(maps=maps, stream_map=remap_stream_map(undistort.get("stream_map"), n_streams, len(maps), what="undistort= "))
    if undistort.get("stream_map") is not None:
        raise ValueError("undistort= stream_map goes with maps=; cameras= holds one camera per stream")
    if given[0] == "camera":
        return dict(cameras=[remap_camera(undistort["camera"], what="undistort= ")], stream_map=[0] * n_streams)
    try:
        cams = list(undistort["cameras"])
    except TypeError:
        cams = []
    if len(cams) != n_streams:
        raise ValueError("undistort= cameras holds %d cameras, the pipeline has %d streams (one per stream)" % (len(cams), n_streams))
    cams = [remap_camera(c, what="undistort= cameras[%d] " % i) for i, c in enumerate(cams)]
    distinct, stream_map = [], []
    for c in cams:
        key = (c["K"], c["D"], c["new_K"], c["R"])
        if key not in [(d["K"], d["D"], d["new_K"], d["R"]) for d in distinct]:
            distinct.append(c)
        stream_map.append([(d["K"], d["D"], d["new_K"], d["R"]) for d in distinct].index(key))
    return dict(cameras=distinct, stream_map=stream_map)


class FrameRemapper:
    """Camera frames rectified on the device (adas_remap_*): cv2.remap(frame, map1, map2, INTER_LINEAR, BORDER_CONSTANT 0) of BGR u8 frames in
    HBM through one fixed-point map per stream -- cv2.undistort when the map comes from a lens model.  cameras: a list of lens models
    (remap_camera's dict), one map each, built on the device as cv2.initUndistortRectifyMap writes it; or maps: a list of (xy int16 (h, w, 2),
    frac uint16 (h, w)), cv2's CV_16SC2 + CV_16UC1 pair.  stream_map[s] is the map stream s reads (None: min(s, maps - 1)); frame f of a batch
    belongs to stream f % n_streams.  dst_hw: the rectified size (None: src_hw).  The rules U1-U6 are csrc/remap_core.h; parity with a real
    cv2 build unpinned."""

    def __init__(self, src_hw, n_streams, cameras=None, maps=None, stream_map=None, dst_hw=None, max_batch=None):
        if (cameras is None) == (maps is None):
            raise ValueError("FrameRemapper needs cameras= or maps=, not both")
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        self.dst_hw = self.src_hw if dst_hw is None else (int(dst_hw[0]), int(dst_hw[1]))
        self.n_streams = int(n_streams)
        cams = None if cameras is None else [remap_camera(c, what="cameras[%d] " % i) for i, c in enumerate(cameras)]
        tables = None if maps is None else remap_maps(maps, self.dst_hw)
        self.n_maps = len(cams if cams is not None else tables)
        if self.n_maps < 1:
            raise ValueError("FrameRemapper needs at least one camera or map")
        sm = remap_stream_map(stream_map, self.n_streams, self.n_maps)
        self.max_batch = self.n_streams if max_batch is None else int(max_batch)
        self.h = None
        p = L.RemapParams(self.src_hw[0], self.src_hw[1], self.dst_hw[0], self.dst_hw[1], self.n_streams, self.n_maps)
        h = C.c_void_p()
        L.check(L.lib().adas_remap_create(C.byref(p), self.max_batch, C.byref(h)))
        self.h = h.value
        for s, m in enumerate(sm):
            if m != min(s, self.n_maps - 1):
                L.check(L.lib().adas_remap_assign(self.h, s, m))
        self.stream_map = sm
        for i in range(self.n_maps):
            if cams is not None:
                self.set_camera(i, **cams[i])
            else:
                self.set_map(i, *tables[i])

    def set_camera(self, map, K, D=(), new_K=None, R=None):
        """Map `map` (-1: every map) from a lens model; finished on return."""
        c = remap_camera(dict(K=K, D=D, new_K=new_K, R=R))
        cam = L.RemapCamera()
        for key in ("K", "D", "new_K", "R"):
            for i, v in enumerate(c[key]):
                getattr(cam, key)[i] = v
        L.check(L.lib().adas_remap_set_camera(self.h, int(map), C.byref(cam)))

    def set_map(self, map, xy, frac):
        """Map `map` from the caller's tables."""
        (xy, frac), = remap_maps([(xy, frac)], self.dst_hw)
        L.check(L.lib().adas_remap_set_map(self.h, int(map), L.ptr(xy), L.ptr(frac)))

    def fetch_map(self, map=0):
        """(xy int16 (h, w, 2), frac uint16 (h, w)) of map `map` as the runs read it."""
        xy, frac = np.empty(self.dst_hw + (2,), np.int16), np.empty(self.dst_hw, np.uint16)
        L.check(L.lib().adas_remap_fetch_map(self.h, int(map), L.ptr(xy), L.ptr(frac)))
        return xy, frac

    def run(self, src_ptr, batch=None, dst_ptr=None, stream=None):
        """src_ptr: device pointer of [batch][src_h][src_w][3] u8.  dst_ptr=None writes the handle's own buffer (fetch / device_view).
        Asynchronous on `stream`."""
        L.check(L.lib().adas_remap_run(self.h, src_ptr, int(self.max_batch if batch is None else batch), dst_ptr, stream))

    def fetch(self, frame=0):
        """Frame `frame` of the handle's own buffer: uint8 (dst_h, dst_w, 3).  Waits for the last run."""
        out = np.empty(self.dst_hw + (3,), np.uint8)
        L.check(L.lib().adas_remap_fetch(self.h, int(frame), L.ptr(out)))
        return out

    def device_view(self):
        p = C.c_void_p()
        L.check(L.lib().adas_remap_device_view(self.h, C.byref(p)))
        return p.value

    def close(self):
        if getattr(self, "h", None):
            L.lib().adas_remap_destroy(self.h)
            self.h = None

    __del__ = close


class OverlayPainter:
    """What the drop-in Draw* methods share (detectors.UltrafastLaneDetectorV2.DrawDetectedOnFrame / .DrawAreaOnFrame,
    analysis.PerspectiveTransformation.DrawDetectedOnBirdView): one LaneOverlay per image size, one stage per call on the caller's image.
    An ndarray is uploaded, drawn in place on the device and copied back into image[:]; a StagedFrame is drawn where it sits."""
    OFFSETS = {"UNKNOWN": 0, "RIGHT": 1, "LEFT": 2, "CENTER": 3}

    def __init__(self):
        self.ov = None
        self.key = None
        self.buf = None
        self._set = {}
        self.tov, self.tkey, self._tset, self._tcls = None, None, {}, {}     # the text's own handle (text())

    def _target(self, image):
        staged = hasattr(image, "ptr") and not isinstance(image, np.ndarray)
        if staged:
            hw = (int(image.height), int(image.width))
        else:
            if not (isinstance(image, np.ndarray) and image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3):
                raise Exception("image must be an HxWx3 uint8 BGR ndarray (or a StagedFrame), got %r" % (getattr(image, "shape", image),))
            hw = (int(image.shape[0]), int(image.shape[1]))
        if self.key != hw:
            if self.ov is not None:
                self.ov.close()
            self.ov = LaneOverlay(hw, hw, 1)
            self.key = hw
            self._set = {}                  # what the handle was last given: the colour table of each stage, the object style
        if staged:
            return image.ptr, None
        n = hw[0] * hw[1] * 3
        if self.buf is None or self.buf.nbytes < n:
            if self.buf is not None:
                self.buf.free()
            self.buf = L.DeviceBuffer(n)
        self.buf.upload(image)
        return self.buf.ptr, image

    def _finish(self, ptr, image):
        if image is not None:
            image[:] = self.buf.download(image.shape, np.uint8)
        else:
            L.check(L.lib().adas_synchronize())     # the caller's staged frame is drawn when the method returns

    @classmethod
    def _offset(cls, type):
        return cls.OFFSETS.get(getattr(type, "name", type), 0) if not isinstance(type, int) else int(type)

    @staticmethod
    def _lane_table(lanes_points):
        pts, cnt = np.zeros((4, L.UFLD_MAX_POINTS, 2), np.int32), np.zeros(4, np.int32)
        for l, lane in enumerate(list(lanes_points)[:4]):
            a = np.asarray(lane if lane is not None else [], np.float64).reshape(-1, 2)[:L.UFLD_MAX_POINTS]
            pts[l, :len(a)], cnt[l] = a.astype(np.int64).astype(np.int32), len(a)     # int(x), int(y)
        return pts, cnt

    def lanes(self, image, lanes_points, type=None, alpha=0.3, bird=False):
        ptr, host = self._target(image)
        pts, cnt = self._lane_table(lanes_points)
        d_pts, d_cnt = L.DeviceBuffer.from_array(pts), L.DeviceBuffer.from_array(cnt)
        d_off = L.DeviceBuffer.from_array(np.array([self._offset(type)], np.int32))
        try:
            if bird:
                self.ov.run_arrays(None, 1, offset_type=d_off.ptr, bird_points=d_pts.ptr, bird_counts=d_cnt.ptr, bird_ptr=ptr, stages=L.OVERLAY_BIRD)
            else:
                self.ov.set_style(lane_alpha=float(alpha))
                self.ov.run_arrays(ptr, 1, lane_points=d_pts.ptr, lane_counts=d_cnt.ptr, offset_type=d_off.ptr, stages=L.OVERLAY_LANES, dst_ptr=ptr)
            self._finish(ptr, host)
        finally:
            for b in (d_pts, d_cnt, d_off):
                b.free()

    def area(self, image, area_points, color=(255, 191, 0), alpha=0.85):
        ptr, host = self._target(image)
        poly = np.ascontiguousarray(np.asarray(area_points, np.float64).reshape(-1, 2).astype(np.int64).astype(np.int32))
        if len(poly) == 0:
            return
        d_poly = L.DeviceBuffer.from_array(poly)
        d_meta = L.DeviceBuffer.from_array(np.array([len(poly), 1], np.int32))
        try:
            self.ov.set_style(area_alpha=float(alpha), area_color=tuple(int(c) for c in color))
            self.ov.run_arrays(ptr, 1, poly=d_poly.ptr, poly_cap=len(poly), poly_counts=d_meta.ptr, area_status=d_meta.ptr + 4, stages=L.OVERLAY_AREA,
                               dst_ptr=ptr)
            self._finish(ptr, host)
        finally:
            d_poly.free()
            d_meta.free()

    def _boxes(self, image, stage, table, boxes, classes, dtype, **style):
        ptr, host = self._target(image)
        b = np.ascontiguousarray(np.asarray(boxes, dtype).reshape(-1, 4))
        if len(b) == 0:
            return
        c = np.ascontiguousarray(np.asarray(classes, np.int64).reshape(-1).astype(np.int32))
        if len(c) != len(b):
            raise Exception("%d boxes, %d classes" % (len(b), len(c)))
        d_b, d_c, d_n = L.DeviceBuffer.from_array(b), L.DeviceBuffer.from_array(c), L.DeviceBuffer.from_array(np.array([len(b)], np.int32))
        try:
            # both setters wait for the device and make a captured step of this process re-capture: only when something changed
            tab = tuple(tuple(int(v) for v in c) for c in table)
            if self._set.get(stage) != tab:
                self.ov.set_class_colors(stage, tab)
                self._set[stage] = tab
            new = {k: v for k, v in style.items() if getattr(self.ov.os, k) != v}
            if new:
                self.ov.set_object_style(**new)
            if stage == L.OVERLAY_DETECTIONS:
                self.ov.run_arrays(ptr, 1, det_xyxy=d_b.ptr, det_cap=len(b), det_cls=d_c.ptr, det_counts=d_n.ptr, stages=stage, dst_ptr=ptr)
            else:
                self.ov.run_arrays(ptr, 1, trk_tlwh=d_b.ptr, trk_cap=len(b), trk_cls=d_c.ptr, trk_counts=d_n.ptr, stages=stage, dst_ptr=ptr)
            self._finish(ptr, host)
        finally:
            for x in (d_b, d_c, d_n):
                x.free()

    def distance(self, image, points):
        """SingleCamDistanceMeasure.DrawDetectedOnFrame's discs (distanceMeasure.py:98): a filled white disc of radius 4 at every (x, y)."""
        pts = np.ascontiguousarray(np.asarray([p[:2] for p in points], np.int64).reshape(-1, 2).astype(np.int32))
        if len(pts) == 0:
            return
        ptr, host = self._target(image)
        d_p, d_n = L.DeviceBuffer.from_array(pts), L.DeviceBuffer.from_array(np.array([len(pts)], np.int32))
        try:
            self.ov.run_arrays(ptr, 1, dist_points=d_p.ptr, dist_cap=len(pts), dist_counts=d_n.ptr, stages=L.OVERLAY_DISTANCE, dst_ptr=ptr)
            self._finish(ptr, host)
        finally:
            d_p.free()
            d_n.free()

    def readouts(self, image, direction, veh_pos, curvature, offset, font, zoom=2, **style):
        """calcCurveAndOffset's drawing on the bird-view image it is handed (LaneOverlay's "readouts" stage; rules R0-R6 of
        csrc/overlay_readout_core.h): the arrow at veh_pos, the arrow at the centre, 'Offset: %.1f m' and 'R : %.1f m' in `font` (an
        atlas rendered at fontScale 3 / zoom) magnified by `zoom`.  direction 0 (no curve) draws nothing."""
        ptr, host = self._target(image)
        if self._set.get("readout_font") is not font:      # the setters wait for the device: only when something changed
            self.ov.set_fonts({10: font})
            self._set["readout_font"] = font
        st = tuple(sorted(dict(style, slot=10, zoom=int(zoom)).items()))
        if self._set.get("readout_style") != st:
            self.ov.set_readout_style(**dict(st))
            self._set["readout_style"] = st
        d_dir = L.DeviceBuffer.from_array(np.array([int(direction)], np.int32))
        d_val = L.DeviceBuffer.from_array(np.array([veh_pos, curvature, offset], np.float64))
        try:
            self.ov.run_arrays(None, 1, bird_ptr=ptr, stages=L.OVERLAY_READOUTS, readouts=(d_dir.ptr, d_val.ptr, d_val.ptr + 8, d_val.ptr + 16))
            self._finish(ptr, host)
        finally:
            d_dir.free()
            d_val.free()

    def text(self, image, kinds, fonts, style=None, det_boxes=(), det_names=(), det_colors=(), tlwhs=(), trk_names=(), trk_colors=(), trk_ids=(),
             trajectories=(), points=(), types=(0, 0, 0)):
        """The reference's putText lines of one Draw* call on the caller's image (LaneOverlay.run_text_arrays; rules T1-T7 of
        csrc/overlay_text_core.h) from `fonts` = {slot: atlas}: kinds out of "detections" (per box its name -- 'unknown' prints black -- and
        colour), "tracks" / "track_ids" (per row of activated tracked tracks its tlwh, name, colour, id and trajectory), "distance" (points
        [x, y, metres]), "panels" (types: the offset, curvature and collision messages as ADAS_* ints).  Names are cut to 31 bytes."""
        mask = LaneOverlay.text_mask(kinds)
        ptr, host = self._target(image)
        # the text has a handle of its own: its class tables are (name, colour) pairs, not the box stages' colours, and every setter waits
        # for the device and makes a captured step of this process re-capture -- so each is called only when what it sets has changed
        if self.tkey != self.key:
            if self.tov is not None:
                self.tov.close()
            self.tov, self.tkey, self._tset = LaneOverlay(self.key, None, 1), self.key, {}
            self._tcls = {"detections": [], "tracks": []}
        if self._tset.get("fonts") is not fonts:
            self.tov.set_fonts(fonts)
            self._tset["fonts"] = fonts
        st = tuple(sorted((style or {}).items(), key=lambda kv: kv[0]))
        if self._tset.get("text_style", ()) != st:
            self.tov.set_text_style(**dict(st))
            self._tset["text_style"] = st
        cut = lambda n: str(n).encode("latin-1", "replace")[:31]

        def classes(which, names, colors, unknown):
            """rows -> their indices into the handle's growing table of (name, colour) classes; -1: 'unknown', black"""
            table, out, grew = self._tcls[which], [], False
            for n, c in zip(names, colors):
                if n == unknown:
                    out.append(-1)
                    continue
                key = (cut(n if n is not None else "unknown"), tuple(int(v) for v in c))
                if key not in table:
                    table.append(key)
                    grew = True
                out.append(table.index(key))
            if grew:
                self.tov.set_class_colors(which, [k[1] for k in table])
                self.tov.set_text_labels(which, [k[0] for k in table])
            return out
        d_cls = classes("detections", det_names, det_colors, "unknown") if mask & L.TEXT["detections"] else []
        t_cls = classes("tracks", trk_names, trk_colors, object()) if mask & (L.TEXT["tracks"] | L.TEXT["track_ids"]) else []
        nd, nt, npt = len(det_boxes), len(tlwhs), len(points)
        arrays = dict(det_xyxy=np.asarray(det_boxes, np.int64).reshape(-1, 4).astype(np.int32), det_cls=np.asarray(d_cls, np.int32),
                      det_counts=np.array([nd], np.int32), trk_tlwh=np.asarray(tlwhs, np.float64).reshape(-1, 4), trk_cls=np.asarray(t_cls, np.int32),
                      trk_ids=np.asarray(trk_ids, np.int64).astype(np.int32), trk_counts=np.array([nt], np.int32),
                      trk_last_tlbr=np.array([np.asarray(t[-1], np.float64) if len(t) else np.zeros(4) for t in trajectories], np.float64).reshape(-1, 4),
                      traj_len=np.array([len(t) for t in trajectories], np.int32), dist_points=np.asarray([p[:2] for p in points], np.int64).reshape(-1, 2).astype(np.int32),
                      dist_d=np.asarray([p[2] for p in points], np.float64), dist_counts=np.array([npt], np.int32),
                      offset_type=np.array([types[0]], np.int32), curvature_type=np.array([types[1]], np.int32), collision_type=np.array([types[2]], np.int32))
        bufs = {k: L.DeviceBuffer.from_array(v if v.size else np.zeros(4, v.dtype)) for k, v in arrays.items()}
        try:
            self.tov.run_text_arrays(ptr, mask, 1, 1, None, max(nd, 1), max(nt, 1), max(npt, 1), **{k: b.ptr for k, b in bufs.items()})
            self._finish(ptr, host)
        finally:
            for b in bufs.values():
                b.free()

    def detections(self, image, boxes, classes, colors=(), arm_thickness=5, rect_thickness=1):
        """DrawDetectedOnFrame's boxes: cornerRect on every (xmin, ymin, xmax, ymax) in order, in colors[class] (outside the table: black).
        No label, no label background, no key points."""
        self._boxes(image, L.OVERLAY_DETECTIONS, colors, boxes, classes, np.int32, det_arm_thickness=int(arm_thickness),
                    det_rect_thickness=int(rect_thickness))

    def tracks(self, image, tlwhs, classes, colors=(), min_box_area=10, thickness=2):
        """DrawTrackedOnFrame's boxes: plot_bbox's rectangle and tint on every tlwh (rows of activated tracked tracks, in list order) whose
        area passes the gate, in colors[class].  No text, trajectories or arrows."""
        self._boxes(image, L.OVERLAY_TRACKS, colors, tlwhs, classes, np.float64, min_box_area=float(min_box_area), track_thickness=int(thickness))

    def _track_style(self, table, min_box_area, thickness):
        # both setters wait for the device and make a captured step of this process re-capture: only when something changed
        if self._set.get(L.OVERLAY_TRACKS) != table:
            self.ov.set_class_colors(L.OVERLAY_TRACKS, table)
            self._set[L.OVERLAY_TRACKS] = table
        new = {k: v for k, v in dict(min_box_area=float(min_box_area), track_thickness=int(thickness)).items() if getattr(self.ov.os, k) != v}
        if new:
            self.ov.set_object_style(**new)

    def trajectories(self, image, tlwhs, trajectories, classes, colors=(), min_box_area=10, boxes=False, thickness=2):
        """DrawTrackedOnFrame(frame, show_box=boxes, show_traject=True) without its text, from host arrays: per tlwh (rows of activated
        tracked tracks, in list order) whose area passes the gate, plot_bbox's rectangle and tint when boxes=True, then plot_trajectories'
        circles over trajectories[row] (tlbr boxes, oldest first; the last 30 count) and plot_directions' lock-on rectangle or shadowed
        arrow, in colors[class] (outside the table: black)."""
        ptr, host = self._target(image)
        b = np.ascontiguousarray(np.asarray(tlwhs, np.float64).reshape(-1, 4))
        if len(b) == 0:
            return
        c = np.ascontiguousarray(np.asarray(classes, np.int64).reshape(-1).astype(np.int32))
        if len(c) != len(b) or len(trajectories) != len(b):
            raise Exception("%d boxes, %d classes, %d trajectories" % (len(b), len(c), len(trajectories)))
        tr, ln = np.zeros((len(b), L.TRAJECTORY_LEN, 4), np.float64), np.zeros(len(b), np.int32)
        for k, t in enumerate(trajectories):
            t = np.asarray(t, np.float64).reshape(-1, 4)[-L.TRAJECTORY_LEN:]
            tr[k, :len(t)], ln[k] = t, len(t)
        bufs = [L.DeviceBuffer.from_array(a) for a in (b, c, np.array([len(b)], np.int32), tr, ln)]
        try:
            self._track_style(tuple(tuple(int(v) for v in col) for col in colors), min_box_area, thickness)
            self.ov.run_arrays(ptr, 1, trk_tlwh=bufs[0].ptr, trk_cap=len(b), trk_cls=bufs[1].ptr, trk_counts=bufs[2].ptr,
                               trajectories=(bufs[3].ptr, bufs[4].ptr), stages=L.OVERLAY_TRAJECTORIES | (L.OVERLAY_TRACKS if boxes else 0), dst_ptr=ptr)
            self._finish(ptr, host)
        finally:
            for x in bufs:
                x.free()

    def live_tracks(self, image, tracker, colors=(), min_box_area=10, boxes=True, trajectories=True, thickness=2):
        """The same from a DeviceTracker's live state (stream 0), with no host copy of it: the rows, their class, tlwh and is_activated and
        each row's trajectory ring are read where they lie in HBM (adas_overlay_run_trajectories).  colors: BGR by the tracker's class id,
        a sequence (a tuple is compared with the last one given, an ndarray [n][3] u8 goes to the device as it is)."""
        stages = (L.OVERLAY_TRACKS if boxes else 0) | (L.OVERLAY_TRAJECTORIES if trajectories else 0)
        if not stages:
            return
        ptr, host = self._target(image)
        if isinstance(colors, np.ndarray):                  # a large table (class ids that are not small): straight to the setter
            key = ("array", colors.shape[0], hash(colors.tobytes()))
            if self._set.get(L.OVERLAY_TRACKS) != key:
                tab = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
                L.check(L.lib().adas_overlay_set_class_colors(self.ov.h, L.OVERLAY_TRACKS, L.ptr(tab) if len(tab) else None, len(tab)))
                self._set[L.OVERLAY_TRACKS] = key
            self._track_style(key, min_box_area, thickness)
        else:
            self._track_style(tuple(tuple(int(v) for v in col) for col in colors), min_box_area, thickness)
        self.ov.run(ptr, tracker=tracker, stages=stages, dst_ptr=ptr)
        self._finish(ptr, host)

    def close(self):
        if self.ov is not None:
            self.ov.close()
        if self.tov is not None:
            self.tov.close()
        if self.buf is not None:
            self.buf.free()
        self.ov = self.key = self.buf = self.tov = self.tkey = None


class DeviceTracker:
    """n_streams independent ByteTrack instances living on the GPU."""

    def __init__(self, n_streams=1, track_thresh=0.5, track_buffer=30, match_thresh=0.8, frame_rate=30,
                 max_tracks=256, max_dets=256):
        p = L.BytetrackParams(track_thresh, match_thresh, float(frame_rate), track_buffer, max_tracks, max_dets, 0)
        self.n_streams, self.max_tracks = n_streams, max_tracks
        h = C.c_void_p()
        L.check(L.lib().adas_bytetrack_create(C.byref(p), n_streams, C.byref(h)))
        self.h = h.value

    def reset(self, stream=-1):
        L.check(L.lib().adas_bytetrack_reset(self.h, stream))

    def update_host(self, stream, boxes, scores, cls):
        b = np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1, 4))
        s = np.ascontiguousarray(np.asarray(scores, np.float64).reshape(-1))
        c = np.ascontiguousarray(np.asarray(cls, np.int32).reshape(-1))
        L.check(L.lib().adas_bytetrack_update_host(self.h, stream, L.ptr(b), L.ptr(s), L.ptr(c), len(s)))

    def update_device(self, views, det_stride, n_streams=None, stream=None, count_stride=4, count_index=2):
        L.check(L.lib().adas_bytetrack_update_device(self.h, views["xyxy"], views["score"], views["cls"],
                                                     views["counts"], det_stride, count_stride, count_index,
                                                     n_streams or self.n_streams, stream))

    def update_device_frames(self, views, det_stride, n_frames, n_streams=None, stream=None, count_stride=4, count_index=2):
        """One launch over n_frames consecutive frames of every stream: frame f of stream s reads detection slab f * n_streams + s.
        Every frame's message stays fetchable with fetch_frame()."""
        L.check(L.lib().adas_bytetrack_update_device_frames(self.h, views["xyxy"], views["score"], views["cls"],
                                                            views["counts"], det_stride, count_stride, count_index,
                                                            n_streams or self.n_streams, n_frames, stream))

    def fetch(self, stream=0):
        hdr = L.TrackHeader()
        recs = np.zeros(2 * self.max_tracks, L.TRACK_DTYPE)
        L.check(L.lib().adas_bytetrack_fetch(self.h, stream, C.byref(hdr), L.ptr(recs), len(recs)))
        return hdr, recs[:hdr.n_tracked], recs[hdr.n_tracked:hdr.n_tracked + hdr.n_lost]

    def fetch_trajectories(self, stream=0):
        """STrack.trajectories (strack.py:53,115) of the live tracks in fetch() order (tracked, then lost): a list of (len, 4) tlbr
        arrays, oldest box first."""
        lens = np.zeros(self.max_tracks, np.int32)
        boxes = np.zeros((self.max_tracks, L.TRAJECTORY_LEN, 4), np.float64)
        n = C.c_int32()
        L.check(L.lib().adas_bytetrack_fetch_trajectories(self.h, stream, L.ptr(lens), L.ptr(boxes), self.max_tracks, C.byref(n)))
        return [boxes[k, :lens[k]].copy() for k in range(n.value)]

    def fetch_frame(self, stream, frame):
        """The tracker message of frame `frame` of the last micro-batched step (what BYTETracker.update returned for that frame)."""
        hdr = L.TrackHeader()
        recs = np.zeros(2 * self.max_tracks, L.TRACK_DTYPE)
        L.check(L.lib().adas_bytetrack_fetch_frame(self.h, stream, frame, C.byref(hdr), L.ptr(recs), len(recs)))
        return hdr, recs[:hdr.n_tracked], recs[hdr.n_tracked:hdr.n_tracked + hdr.n_lost]

    def close(self):
        if getattr(self, "h", None):
            L.lib().adas_bytetrack_destroy(self.h)
            self.h = None

    __del__ = close
