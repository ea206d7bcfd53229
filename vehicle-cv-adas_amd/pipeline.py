"""Fused per-frame ADAS step for S independent video streams on one GPU (C ABI: adas_pipeline_*).

What demo.py:261-281 drives per frame -- detector forward + decode/NMS, tracker update, lane forward +
decode -- runs back to back on one HIP stream (optionally replayed from a hipGraph) with every
intermediate resident in HBM.  Inputs are the engine-seam tensors (NCHW fp32) already on the device.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .coreEngine import HipEngine
from .postproc import YoloPost, UfldDecode, Ufld1Decode, LaneGeometry, DeviceTracker, BirdView, PerspectiveWarp, Analysis, LaneOverlay, JpegEncoder, JpegDecoder, YuvConverter, YuvWriter, yuv_output_args, FrameScaler, scale_args, FrameRemapper, undistort_args, host_streams, letterbox
from . import sharding

CULANE = dict(grid_row=200, cls_row=72, grid_col=100, cls_col=81,
              row_anchor=np.linspace(0.42, 1, 72), col_anchor=np.linspace(0, 1, 81))   # ultrafastLaneDetectorV2.py:49-55


class AdasPipeline:
    def __init__(self, det_model=None, lane_model=None, n_streams=1, precision=None, src_hw=(720, 1280),
                 box_score=0.4, nms_iou=0.45, head_layout=L.HEAD_V8, num_classes=None, use_graph=True,
                 max_candidates=512, track=True, lane_cfg=None, nms_mode=L.NMS_REFERENCE, overlap=True, geometry=None, micro_batch=1,
                 birdview=None, analysis=None, overlay=None, jpeg=None, jpeg_input=None, yuv_input=None, yuv_output=None, scale=None, undistort=None):
        """geometry: None, or dict(bird_wh=(w, h), M=3x3, adjust_lanes=True) to run the lane-geometry kernel behind the decode.
        micro_batch B > 1: temporal micro-batching (adas_pipeline_desc.micro_batch) -- a step takes B consecutive frames of every
        stream, frame b of stream s at index b * n_streams + s of the input and of every per-frame fetch; the tracker consumes
        them in order.  Throughput mode for few streams per GPU.
        birdview: None, or dict(image=bool): one adaptive bird-view trapezoid per stream on the device (postproc.BirdView with
        img_size = geometry["bird_wh"]); the geometry then reads every frame's own matrix, request_transform(stream, mode) re-anchors a
        stream on its next step, and with image=True step_frames also warps every frame into the bird view (birdview_image).
        Needs geometry=; geometry["M"] is then only the handle's stand-alone matrix.
        analysis: None, or dict(class_names=[...], object_list=...): distance points, the collision point and the FCWS / LDWS / LKAS state
        machine per stream as the step's last stage (postproc.Analysis; `.analysis.fetch_stream(s)` / `.fetch_frame(f)` after sync()).
        class_names are the detector's labels by class id, object_list the measured ones (default: the reference's six); further keys go
        to Analysis (ref_height=: the per-class table of inches itself, in place of the two label lists).  Needs det_model=, lane_model= and geometry=.  With birdview= the device then owns the
        re-anchoring requests (request_transform raises) and micro_batch must be 1.
        overlay: None, or dict(stages=("lanes", "area", "distance", "bird") or a subset / mask, plus LaneOverlay's style keys): the lane
        overlay as the step's very last stage, drawn from step_frames' frames into a buffer of its own (overlay_image(frame) after sync()):
        lane-point discs and the ego-lane polygon alpha-blended, distance-point discs, and the discs on the bird-view image -- no text or
        panels.  Needs lane_model= and geometry=; the distance stage needs analysis=, the bird stage
        birdview=dict(image=True).  stages=None: every one of those four stages the pipeline has the handles for.  Only by name: "detections"
        (cornerRect boxes of the step's survivors; needs det_model=) and "tracks" (the tracked tracks' rectangles and tints after this step's
        update; needs track=True and micro_batch 1), drawn between the area and the distance discs in the class colours of
        overlay["detection_colors"] / overlay["track_colors"] (BGR by class id; none: black).  Also only by name: "trajectories" -- what
        the demo's DrawTrackedOnFrame(frame_show, False) draws per tracked track, behind its box: plot_trajectories' circles over its last 30
        boxes and plot_directions' lock-on rectangle or shadowed arrow, in overlay["track_colors"]; read from the tracker's live state on the
        device (needs det_model=, track=True and micro_batch 1 like "tracks").  No labels, key points or other text.
        overlay["panels"]: names out of "bird", "signs", "collision" (or a mask) -- the demo's three UI panels (ControlPanel.Display*Panel
        without their text), painted in place behind the overlay's stages from the step's analysis rows and bird-view image, with
        overlay["panel_sprites"] = {name: (h, w, 4) uint8 BGRA} (LaneOverlay.set_panels) and optionally overlay["panel_params"] = dict(...).
        "bird" needs birdview=dict(image=True), "signs" and "collision" need analysis=.  overlay_image(frame) then holds the panels;
        self.overlay.panel_record(frame) what was chosen.  The curve_status latch of every stream lives on the device.
        overlay["text"]: names out of "detections", "track_ids", "tracks", "distance", "panels", "lines" (or a mask) -- the reference's putText
        lines and the label's filled background, drawn on the device from overlay["fonts"] = {slot: atlas} (LaneOverlay.set_fonts; the
        atlases are the caller's data, tools/make_font_atlas.py writes them), with overlay["text_style"] = dict(...) (slots, ladders,
        offsets), overlay["detection_names"] / ["track_names"] (class names by id; colours are detection_colors / track_colors) and
        overlay["text_lines"] = [(x, y, slot, colour, text)] (at most 8: FPS and the like).  The scene's text lies over every stage and
        under the panels, the panel strings and the lines over the panels.  self.overlay.text_items(frame) is what was placed.
        Also only by name: the stage "readouts" -- what calcCurveAndOffset draws on the bird-view image (the white arrow at the vehicle's
        position, the grey arrow at the centre, 'Offset: %.1f m' and 'R : %.1f m'), under the "bird" stage's discs, with
        overlay["readout"] = dict(slot=10, zoom=2, ...) (LaneOverlay.set_readout_style) and a font in that slot of overlay["fonts"] rendered
        at fontScale 3 / zoom.  It needs birdview=dict(image=True); birdview_image(frame) and the bird panel then show the readouts, and
        self.overlay.readout_record(frame) is what was laid out.  A frame without a curve (direction None) is not drawn on.
        jpeg: None, or dict(quality=90, source="overlay" | "frames", capacity=None): every frame of the step as a baseline JPEG stream
        (postproc.JpegEncoder), the step's last launch group -- what the demo's vout.write(frame_show) gets, without the uncompressed frame
        leaving the device: jpeg(frame) -> bytes after sync(), jpeg_lengths() -> (lengths, flags).  source="overlay" (the default) encodes
        the drawn frames, behind the overlay's stages and panels, and needs overlay=; source="frames" encodes the camera frames the step was
        given.  Either needs step_frames / step_frames_host.  capacity: bytes per frame (None: height * width * 3); a frame that would not
        fit comes back as b"" with JpegEncoder.OVERFLOW in its flag.  Any micro_batch: frames are independent.
        jpeg_input: None, True or dict(capacity=None): a decoder in FRONT of the step (postproc.JpegDecoder for src_hw frames) for cameras and
        files that deliver MJPEG: step_jpeg_host(list_of_bytes) uploads the compressed streams (a few hundred KB per frame in place of
        height * width * 3 bytes), decodes them on the device and runs the step on the decoded frames; input_flags() -> one flag word per
        frame after sync() (a rejected frame is a black frame to the step).  capacity: the most bytes per stream (None:
        JpegEncoder.bound(width, height)).  Nothing inside the captured step changes.
        yuv_input: None, or dict(format="nv12" | "nv21" | "i420" | "yuyv" | "uyvy", matrix="video" | "full", layout=None): a colour conversion
        in FRONT of the step (postproc.YuvConverter for src_hw frames) for sources that deliver what cameras and decoders really deliver --
        a UVC camera's YUYV, an ISP's, a hardware decoder's or ffmpeg's NV12 / I420 -- in place of the cv2.cvtColor a caller's host code
        would run: step_yuv_host(array_or_ptr) uploads the raw frames (1.5 or 2 bytes per pixel in place of 3) on the copy stream,
        converts them on the device and runs the step on the result; step_yuv(d_ptr) takes frames already on the device, such as a
        decoder's surface.  matrix: "video" (BT.601 limited range, cv2's; the default) or "full" (JFIF).  layout: None for tightly packed
        frames, or YuvConverter's dict of byte strides and plane offsets.  Not together with jpeg_input=.  Nothing inside the captured step
        changes.
        yuv_output: None, or dict(format="i420", matrix="video" | "full", chroma="mean" | "first", source="overlay" | "frames", layout=None):
        every frame of the step as raw video (postproc.YuvWriter) for an encoder that is not MJPEG -- x264, `ffmpeg -f rawvideo -pix_fmt
        yuv420p`, a V4L2 loopback -- behind the overlay's stages, text and panels, one more launch inside the captured step: yuv(frame) ->
        uint8 [frame_bytes] after sync(), yuv_all() -> all of the step's frames in one copy.  source="overlay" (the default) converts the
        drawn frames and needs overlay=; source="frames" converts the camera frames the step was given.  Either needs step_frames /
        step_frames_host.  Independent of jpeg=: both may be on.  Any micro_batch: frames are independent.
        scale: None, or dict(size=(w, h), mode="area" | "linear", mosaic=(cols, rows), source="overlay" | "frames", border=0,
        background=(0, 0, 0), border_colors=None, jpeg=None | dict(quality, capacity), yuv=None | dict(format, matrix, chroma, layout)): every
        frame of the step reduced to a tile of `size`, mosaic tiles to a canvas (postproc.FrameScaler) -- a preview per stream with
        mosaic=(1, 1), a video wall of the whole step otherwise -- behind the overlay's stages, text and panels, one more launch inside the
        captured step: scaled_image(canvas) -> uint8 [rows * h][cols * w][3] after sync().  Frame f (index b * n_streams + s) is cell
        f % (cols * rows) of canvas f // (cols * rows), so any micro_batch works.  border > 0 draws each tile's collision state as a frame of
        border_colors[state] and needs analysis=.  jpeg= and yuv= add a second JpegEncoder and a second YuvWriter at the canvas size that
        consume the canvases inside the same step: scaled_jpeg(canvas), scaled_jpeg_lengths(), scaled_yuv(canvas), scaled_yuv_all().
        source="overlay" (the default) needs overlay=.  Independent of jpeg= and yuv_output=, which keep encoding the full frames.
        undistort: None, or dict(camera=dict(K=, D=, new_K=None, R=None)) | dict(cameras=[one such dict per stream]) | dict(maps=[(xy, frac),
        ...], stream_map=[map of stream s, ...]): a rectification stage in FRONT of the step (postproc.FrameRemapper at src_hw) for cameras
        whose frames are not pinhole images -- in place of the cv2.undistort / cv2.remap a caller's host code would run before the upload.
        Every way in (step_frames, step_frames_host, step_jpeg_host, step_yuv, step_yuv_host) then resamples its frames on the device
        through the stream's map, and the whole step -- both nets, the bird view, the overlay, source="frames" -- reads the rectified
        frames: undistorted_image(frame) after sync().  camera / cameras: a Brown-Conrady / rational lens model as
        cv2.initUndistortRectifyMap takes it (K and new_K as (fx, fy, cx, cy) or 3x3, D of 4, 5 or 8 coefficients); identical cameras share
        one map.  maps: cv2's CV_16SC2 + CV_16UC1 pairs (int16 (h, w, 2), uint16 (h, w)), which covers fisheye lenses and stereo
        rectification.  Composes with jpeg_input= and yuv_input=.  Nothing inside the captured step changes."""
        self.S = n_streams
        self.stream_ids = list(range(n_streams))      # job-wide ids of the local streams (for_rank overrides)
        self.B = max(1, int(micro_batch))
        n_tracks = n_streams
        n_streams = n_streams * self.B          # frames per step through the engines / post / decode handles
        self.det = self.lane = self.post = self.decode = self.tracker = self.geometry = self.birdview = self.warp = self.analysis = None
        self.overlay = self.jpeg_encoder = self.jpeg_decoder = self.yuv_converter = self.yuv_writer = None
        self.scaler = self.scaled_jpeg_encoder = self.scaled_yuv_writer = self.remapper = None
        if undistort is not None:
            undistort_checked = undistort_args(undistort, n_tracks, src_hw)
        if jpeg_input is not None and jpeg_input is not False:
            jpeg_input = {} if jpeg_input is True else dict(jpeg_input)
            unknown = set(jpeg_input) - {"capacity"}
            if unknown:
                raise ValueError("jpeg_input= holds unknown keys %s (capacity)" % sorted(unknown))
        else:
            jpeg_input = None
        if yuv_input is not None:
            yuv_input = dict(yuv_input)
            unknown = set(yuv_input) - {"format", "matrix", "layout"}
            if unknown:
                raise ValueError("yuv_input= holds unknown keys %s (format, matrix, layout)" % sorted(unknown))
            if jpeg_input is not None:
                raise ValueError("yuv_input= and jpeg_input= are two decoders in front of one step: choose the one the source delivers")
            if yuv_input.get("format", "nv12") not in L.YUV_FORMATS:
                raise ValueError("yuv_input= format %r is none of %s" % (yuv_input.get("format"), sorted(L.YUV_FORMATS)))
            if yuv_input.get("matrix", "video") not in L.YUV_MATRICES:
                raise ValueError("yuv_input= matrix %r is neither \"video\" nor \"full\"" % (yuv_input.get("matrix"),))
        if jpeg is not None:
            unknown = set(dict(jpeg)) - {"quality", "source", "capacity"}
            if unknown:
                raise ValueError("jpeg= holds unknown keys %s (quality, source, capacity)" % sorted(unknown))
            jpeg_source = dict(jpeg).get("source", "overlay")
            if jpeg_source not in L.JPEG_SOURCES:
                raise ValueError("jpeg= source %r is neither \"overlay\" nor \"frames\"" % (jpeg_source,))
            if jpeg_source == "overlay" and overlay is None:
                raise ValueError("jpeg= with source=\"overlay\" needs overlay= (the drawn frames it encodes); source=\"frames\" encodes the camera frames")
            if not 1 <= int(dict(jpeg).get("quality", 90)) <= 100:
                raise ValueError("jpeg= quality %r is outside 1..100" % (dict(jpeg).get("quality"),))
        if yuv_output is not None:
            if not isinstance(yuv_output, dict):
                raise ValueError("yuv_output= %r is neither None nor a dict (format, matrix, chroma, source, layout)" % (yuv_output,))
            yuv_output = dict(yuv_output)
            unknown = set(yuv_output) - {"format", "matrix", "chroma", "source", "layout"}
            if unknown:
                raise ValueError("yuv_output= holds unknown keys %s (format, matrix, chroma, source, layout)" % sorted(unknown))
            yuv_output_args(yuv_output.get("format", "i420"), yuv_output.get("matrix", "video"), yuv_output.get("chroma", "mean"),
                            yuv_output.get("layout"), what="yuv_output= ")
            if yuv_output.get("source", "overlay") not in L.YUVOUT_SOURCES:
                raise ValueError("yuv_output= source %r is neither \"overlay\" nor \"frames\"" % (yuv_output.get("source"),))
            if yuv_output.get("source", "overlay") == "overlay" and overlay is None:
                raise ValueError("yuv_output= with source=\"overlay\" needs overlay= (the drawn frames it converts); source=\"frames\" converts the "
                                 "camera frames")
        if scale is not None:
            if not isinstance(scale, dict):
                raise ValueError("scale= %r is neither None nor a dict (size, mode, mosaic, source, border, background, border_colors, jpeg, yuv)" % (scale,))
            scale = dict(scale)
            unknown = set(scale) - {"size", "mode", "mosaic", "source", "border", "background", "border_colors", "jpeg", "yuv"}
            if unknown:
                raise ValueError("scale= holds unknown keys %s (size, mode, mosaic, source, border, background, border_colors, jpeg, yuv)" % sorted(unknown))
            if "size" not in scale:
                raise ValueError("scale= needs size=(w, h), the tile every frame is reduced to")
            scale_checked = scale_args((src_hw[1], src_hw[0]), scale["size"], scale.get("mode", "area"), scale.get("mosaic", (1, 1)), scale.get("border", 0),
                                       scale.get("background", (0, 0, 0)), scale.get("border_colors"), what="scale= ")
            if scale.get("source", "overlay") not in L.SCALE_SOURCES:
                raise ValueError("scale= source %r is neither \"overlay\" nor \"frames\"" % (scale.get("source"),))
            if scale.get("source", "overlay") == "overlay" and overlay is None:
                raise ValueError("scale= with source=\"overlay\" needs overlay= (the drawn frames it reduces); source=\"frames\" reduces the camera frames")
            if scale_checked["border"] > 0 and analysis is None:
                raise ValueError("scale= with border > 0 needs analysis= (the collision state a tile's border shows)")
            if scale.get("jpeg") is not None:
                if not isinstance(scale["jpeg"], dict):
                    raise ValueError("scale= jpeg %r is neither None nor a dict (quality, capacity)" % (scale["jpeg"],))
                unknown = set(scale["jpeg"]) - {"quality", "capacity"}
                if unknown:
                    raise ValueError("scale= jpeg holds unknown keys %s (quality, capacity)" % sorted(unknown))
                if not 1 <= int(scale["jpeg"].get("quality", 90)) <= 100:
                    raise ValueError("scale= jpeg quality %r is outside 1..100" % (scale["jpeg"].get("quality"),))
            if scale.get("yuv") is not None:
                if not isinstance(scale["yuv"], dict):
                    raise ValueError("scale= yuv %r is neither None nor a dict (format, matrix, chroma, layout)" % (scale["yuv"],))
                unknown = set(scale["yuv"]) - {"format", "matrix", "chroma", "layout"}
                if unknown:
                    raise ValueError("scale= yuv holds unknown keys %s (format, matrix, chroma, layout)" % sorted(unknown))
                yuv_output_args(scale["yuv"].get("format", "i420"), scale["yuv"].get("matrix", "video"), scale["yuv"].get("chroma", "mean"),
                                scale["yuv"].get("layout"), what="scale= yuv ")
        if overlay is not None:
            if geometry is None or not lane_model:
                raise ValueError("overlay= needs lane_model= and geometry= (the lane points and the ego-lane polygon it draws)")
            ov_stages = dict(overlay).get("stages")
            ov_mask = None if ov_stages is None else LaneOverlay.stage_mask(ov_stages)
            ro_on = bool(ov_mask is not None and ov_mask & L.OVERLAY_READOUTS)      # only by name; a switch of its own behind the stage mask
            ro_style = dict(dict(overlay).get("readout") or {})
            ro_slot = int(ro_style.get("slot", 10))
            has_bird = birdview is not None and dict(birdview).get("image", False)
            live = "the tracker's live table holds only the last frame of a step"
            for bits, ok, msg in (      # (stage bits, what they need, the refusal), in the order they are checked
                    (L.OVERLAY_DISTANCE, analysis is not None, "distance stage needs analysis= (the distance points it draws)"),
                    (L.OVERLAY_BIRD, has_bird, "bird stage needs birdview=dict(image=True) (the bird-view image it draws on)"),
                    (L.OVERLAY_READOUTS, has_bird, "readouts stage needs birdview=dict(image=True) (the bird-view image it draws on)"),
                    (L.OVERLAY_READOUTS, ro_slot in dict(dict(overlay).get("fonts") or {}),
                     "readouts stage needs fonts={%d: atlas}: a font in its slot (readout=dict(slot=...))" % ro_slot),
                    (L.OVERLAY_DETECTIONS, det_model, "detections stage needs det_model= (the survivors it draws)"),
                    (L.OVERLAY_TRACKS, det_model and track, "tracks stage needs det_model= and track=True (the tracked tracks it draws)"),
                    (L.OVERLAY_TRACKS, self.B <= 1, "tracks stage needs micro_batch=1: " + live),
                    (L.OVERLAY_TRAJECTORIES, det_model, "trajectories stage needs det_model= (the detector that feeds the tracker it draws from)"),
                    (L.OVERLAY_TRAJECTORIES, track, "trajectories stage needs det_model= and track=True (the tracked tracks it draws)"),
                    (L.OVERLAY_TRAJECTORIES, self.B <= 1, "trajectories stage needs micro_batch=1: " + live)):
                if ov_mask is not None and ov_mask & bits and not ok:
                    raise ValueError("the overlay's " + msg)
            pn_mask = LaneOverlay.panel_mask(dict(overlay).get("panels") or 0)
            for bits, ok, msg in (
                    (L.PANEL_BIRD, has_bird, "bird panel needs birdview=dict(image=True) (the bird-view image it shows)"),
                    (L.PANEL_SIGNS, analysis is not None, "signs panel needs analysis= (the offset and curvature messages it shows)"),
                    (L.PANEL_COLLISION, analysis is not None, "collision panel needs analysis= (the collision message it shows)"),
                    (pn_mask, not (pn_mask & ~7), "panels= holds unknown bits 0x%x" % pn_mask),
                    (pn_mask, dict(overlay).get("panel_sprites") is not None, "panels= needs panel_sprites= (the BGRA arrays ControlPanel loads)")):
                if pn_mask & bits and not ok:
                    raise ValueError("the overlay's " + msg)
            tx_mask = LaneOverlay.text_mask(dict(overlay).get("text") or 0)
            T = L.TEXT
            for bits, ok, msg in (
                    (tx_mask, not (tx_mask & ~63), "text= holds unknown bits 0x%x" % tx_mask),
                    (tx_mask, dict(overlay).get("fonts"), "text= needs fonts= ({slot: atlas}: the glyph atlases are the caller's data)"),
                    (T["detections"], det_model, "detections text needs det_model= (the survivors it labels)"),
                    (T["tracks"] | T["track_ids"], det_model and track, "tracks and track_ids text need det_model= and track=True"),
                    (T["tracks"] | T["track_ids"], self.B <= 1, "tracks and track_ids text need micro_batch=1: " + live),
                    (T["distance"] | T["panels"], analysis is not None, "distance and panels text need analysis= (the distances and messages they print)")):
                if tx_mask & bits and not ok:
                    raise ValueError("the overlay's " + msg)
        if birdview is not None and (geometry is None or not lane_model):
            raise ValueError("birdview= needs lane_model= and geometry= (its bird_wh is the bird view's img_size)")
        if det_model:
            self.det = HipEngine(det_model, precision, n_streams)
            ishape = self.det.get_engine_input_shape()
            oshape = self.det.get_engine_output_shape()[0][0]
            A = oshape[2] if head_layout == L.HEAD_V8 else oshape[1]
            nc_model = oshape[1] - 4 if head_layout == L.HEAD_V8 else oshape[2] - 5     # yoloDetector.py:110-124
            if num_classes is None:
                num_classes = nc_model
            elif num_classes != nc_model:
                raise ValueError("num_classes=%d but the detector head %s carries %d classes" % (num_classes, oshape, nc_model))
            lb = letterbox(src_hw, ishape[2:])
            self.post = YoloPost(head_layout, A, num_classes, box_score, nms_iou, lb, nms_mode, max_candidates, n_streams)
            if track:
                self.tracker = DeviceTracker(n_tracks, max_dets=max_candidates)
        if lane_model:
            self.lane = HipEngine(lane_model, precision, n_streams)
            cfg = dict(CULANE)
            cfg.update(lane_cfg or {})
            if "griding_num" in cfg:          # UFLD v1 (ultrafastLaneDetector.py ModelConfig): one output tensor
                ish = self.lane.get_engine_input_shape()
                self.decode = Ufld1Decode(cfg["griding_num"], cfg["cls_num_per_lane"], cfg["img_w"], cfg["img_h"], ish[3], ish[2],
                                          src_hw[1], src_hw[0], cfg["row_anchor"], n_streams)
            else:
                nl = self.lane.get_engine_output_shape()[0][0][3]
                self.decode = UfldDecode(cfg["grid_row"], cfg["cls_row"], cfg["grid_col"], cfg["cls_col"], src_hw[1], src_hw[0],
                                         cfg["row_anchor"], cfg["col_anchor"], 1, n_streams, num_lanes=nl)
            if geometry is not None:
                self.geometry = LaneGeometry(src_hw[0], geometry["bird_wh"], geometry["M"], geometry.get("adjust_lanes", True), n_streams)
        d = L.PipelineDesc(self.det.handle if self.det else None, self.lane.handle if self.lane else None,
                           self.post.h if self.post else None, self.decode.h if self.decode else None,
                           self.tracker.h if self.tracker else None, n_tracks, (1 if use_graph else 0) | (0 if overlap else 2),
                           self.geometry.h if self.geometry else None, self.B if self.B > 1 else 0, 0)
        h = C.c_void_p()
        L.check(L.lib().adas_pipeline_create(C.byref(d), C.byref(h)))
        self.h = h.value
        if birdview is not None:
            bw, bh = (int(v) for v in geometry["bird_wh"])
            self.birdview = BirdView((bw, bh), n_tracks, n_streams)
            if dict(birdview).get("image", False):
                self.warp = PerspectiveWarp(src_hw, (bh, bw), n_streams)
            L.check(L.lib().adas_pipeline_attach_birdview(self.h, self.birdview.h, self.warp.h if self.warp else None))
        if analysis is not None:
            kw = dict(analysis)
            if "class_names" not in kw and "ref_height" not in kw:
                raise ValueError("analysis= needs class_names: the detector's label of every class id (or ref_height: the per-class table)")
            kw.setdefault("max_points", min(int(max_candidates), 2048))
            kw.setdefault("max_poly", 2 * int(src_hw[0]))
            self.analysis = Analysis(n_streams=n_tracks, max_frames=n_streams, **kw)
            L.check(L.lib().adas_pipeline_attach_analysis(self.h, self.analysis.h))
        if overlay is not None:
            style = {k: v for k, v in dict(overlay).items() if k not in ("stages", "detection_colors", "track_colors", "panels", "panel_sprites",
                                                                         "panel_params", "text", "fonts", "text_style", "text_lines", "detection_names",
                                                                         "track_names", "readout")}
            self.overlay = LaneOverlay(src_hw, self.warp.dst_hw if self.warp else None, n_streams, **style)
            for key, which in (("detection_colors", "detections"), ("track_colors", "tracks")):
                if dict(overlay).get(key) is not None:
                    self.overlay.set_class_colors(which, overlay[key])
            L.check(L.lib().adas_pipeline_attach_overlay(self.h, self.overlay.h))
            if ov_mask is not None:
                L.check(L.lib().adas_pipeline_set_overlay_stages(self.h, ov_mask & ~L.OVERLAY_READOUTS))
            if pn_mask:
                self.overlay.set_panels(overlay["panel_sprites"], **dict(dict(overlay).get("panel_params") or {}))
                L.check(L.lib().adas_pipeline_set_overlay_panels(self.h, pn_mask))
            if dict(overlay).get("fonts"):
                self.overlay.set_fonts(overlay["fonts"])
            if dict(overlay).get("text_style"):
                self.overlay.set_text_style(**dict(overlay["text_style"]))
            for key, which in (("detection_names", "detections"), ("track_names", "tracks")):
                if dict(overlay).get(key) is not None:
                    self.overlay.set_text_labels(which, overlay[key])
            if dict(overlay).get("text_lines") is not None:
                self.overlay.set_text_lines(overlay["text_lines"])
            if tx_mask:
                L.check(L.lib().adas_pipeline_set_overlay_text(self.h, tx_mask))
            if ro_on:
                self.overlay.set_readout_style(**ro_style)
                L.check(L.lib().adas_pipeline_set_overlay_readouts(self.h, 1))
        if jpeg is not None:
            self.jpeg_encoder = JpegEncoder(src_hw[1], src_hw[0], int(dict(jpeg).get("quality", 90)), n_streams, dict(jpeg).get("capacity"))
            L.check(L.lib().adas_pipeline_attach_jpeg(self.h, self.jpeg_encoder.h, L.JPEG_SOURCES[jpeg_source]))
        if jpeg_input is not None:
            self.jpeg_decoder = JpegDecoder(src_hw[1], src_hw[0], n_streams, jpeg_input.get("capacity"))
            L.check(L.lib().adas_pipeline_attach_jpegdec(self.h, self.jpeg_decoder.h))
        if yuv_input is not None:
            self.yuv_converter = YuvConverter(yuv_input.get("format", "nv12"), src_hw[1], src_hw[0], yuv_input.get("matrix", "video"),
                                              yuv_input.get("layout"), n_streams)
            L.check(L.lib().adas_pipeline_attach_yuv(self.h, self.yuv_converter.h))
        if yuv_output is not None:
            self.yuv_writer = YuvWriter(yuv_output.get("format", "i420"), src_hw[1], src_hw[0], yuv_output.get("matrix", "video"),
                                        yuv_output.get("chroma", "mean"), yuv_output.get("layout"), n_streams)
            L.check(L.lib().adas_pipeline_attach_yuvout(self.h, self.yuv_writer.h, L.YUVOUT_SOURCES[yuv_output.get("source", "overlay")]))
        if scale is not None:
            self.scaler = FrameScaler(scale_checked["src_wh"], scale_checked["size"], scale_checked["mode"], scale_checked["mosaic"], scale_checked["border"],
                                      scale_checked["background"], scale_checked["border_colors"], n_streams)
            L.check(L.lib().adas_pipeline_attach_scale(self.h, self.scaler.h, L.SCALE_SOURCES[scale.get("source", "overlay")]))
            ch, cw = self.scaler.canvas_hw
            if scale.get("jpeg") is not None:
                self.scaled_jpeg_encoder = JpegEncoder(cw, ch, int(scale["jpeg"].get("quality", 90)), self.scaler.canvases(n_streams),
                                                       scale["jpeg"].get("capacity"))
                L.check(L.lib().adas_pipeline_attach_scale_jpeg(self.h, self.scaled_jpeg_encoder.h))
            if scale.get("yuv") is not None:
                y = scale["yuv"]
                self.scaled_yuv_writer = YuvWriter(y.get("format", "i420"), cw, ch, y.get("matrix", "video"), y.get("chroma", "mean"), y.get("layout"),
                                                   self.scaler.canvases(n_streams))
                L.check(L.lib().adas_pipeline_attach_scale_yuvout(self.h, self.scaled_yuv_writer.h))
        if undistort is not None:
            self.remapper = FrameRemapper(src_hw, n_tracks, max_batch=n_streams, **undistort_checked)
            L.check(L.lib().adas_pipeline_attach_remap(self.h, self.remapper.h))

    @classmethod
    def for_rank(cls, det_model, lane_model, total_streams, env=None, **kw):
        """The pipeline of ONE rank of a `total_streams`-stream job (one process per GPU): the rank runs the streams
        sharding.streams_of_rank deals it (stream s -> rank s mod world); `.stream_ids[i]` is the job-wide id of local stream i.
        Returns None for a rank that owns no stream (fewer streams than ranks).  undistort= may carry cameras= or stream_map= for the whole
        job (total_streams entries, by job-wide stream id): each rank takes its own streams' entries; a list of the rank's own length is
        taken as it is."""
        env = env or sharding.RankEnv.from_environ()
        ids = sharding.streams_of_rank(int(total_streams), env)
        if not ids:
            return None
        und = kw.get("undistort")
        if isinstance(und, dict) and und.get("cameras") is not None and len(und["cameras"]) == int(total_streams):
            kw["undistort"] = dict(und, cameras=[und["cameras"][s] for s in ids])       # a job-wide list: this rank's streams, in local order
        elif isinstance(und, dict) and und.get("stream_map") is not None and len(und["stream_map"]) == int(total_streams):
            kw["undistort"] = dict(und, stream_map=[und["stream_map"][s] for s in ids])
        p = cls(det_model, lane_model, n_streams=len(ids), **kw)
        p.stream_ids = ids
        return p

    def step(self, d_det_ptr=None, d_lane_ptr=None):
        L.check(L.lib().adas_pipeline_step(self.h, d_det_ptr, d_lane_ptr))

    def step_frames(self, d_frames_ptr, src_hw, lane_crop_ratio=0.6):
        """One step from n_streams BGR u8 frames (H x W x 3, back to back) in HBM: pre-processing runs inside the step."""
        L.check(L.lib().adas_pipeline_step_frames(self.h, d_frames_ptr, int(src_hw[0]), int(src_hw[1]), float(lane_crop_ratio)))

    def step_frames_host(self, h_frames_ptr, src_hw, lane_crop_ratio=0.6):
        """The same step from HOST frames (pinned: _lib.PinnedBuffer): the upload runs on a copy stream into one of two device
        staging buffers, overlapped with the previous step's compute."""
        L.check(L.lib().adas_pipeline_step_frames_host(self.h, h_frames_ptr, int(src_hw[0]), int(src_hw[1]), float(lane_crop_ratio)))

    def step_jpeg_host(self, streams, lane_crop_ratio=0.6):
        """The same step from COMPRESSED host frames: a list of n_streams x micro_batch baseline JPEG streams (bytes).  Their upload runs on
        the copy stream, overlapped with the previous step's compute; they are decoded on the device into the decoder's frames and the
        step runs on those.  The bytes are free again on return.  Needs jpeg_input=."""
        if self.jpeg_decoder is None:
            raise ValueError("the pipeline was created without jpeg_input=")
        if len(streams) != self.S * self.B:
            raise ValueError("step_jpeg_host got %d streams, a step has %d frames" % (len(streams), self.S * self.B))
        ptrs, lengths, keep = host_streams(streams)
        L.check(L.lib().adas_pipeline_step_jpeg_host(self.h, ptrs, L.ptr(lengths), float(lane_crop_ratio)))

    def step_yuv(self, d_ptr, lane_crop_ratio=0.6):
        """The same step from n_streams x micro_batch camera frames in yuv_input's format ALREADY ON THE DEVICE (frame f at d_ptr + f *
        frame_stride): converted into the converter's frames, and the step runs on those.  Needs yuv_input=."""
        if self.yuv_converter is None:
            raise ValueError("the pipeline was created without yuv_input=")
        L.check(L.lib().adas_pipeline_step_yuv(self.h, d_ptr, float(lane_crop_ratio)))

    def step_yuv_host(self, frames, lane_crop_ratio=0.6):
        """The same step from HOST frames in yuv_input's format: a uint8 array of yuv_converter.batch_bytes(frames per step) bytes, or a host
        pointer to as many (pinned: _lib.PinnedBuffer, for the upload to overlap the previous step's compute; wait_upload() before
        refilling it).  Needs yuv_input=."""
        if self.yuv_converter is None:
            raise ValueError("the pipeline was created without yuv_input=")
        if isinstance(frames, np.ndarray):
            need = self.yuv_converter.batch_bytes(self.S * self.B)
            if frames.dtype != np.uint8 or not frames.flags.c_contiguous or frames.nbytes < need:
                raise ValueError("step_yuv_host needs a contiguous uint8 array of at least %d bytes, a step has %d frames" % (need, self.S * self.B))
            frames = L.ptr(frames)
        L.check(L.lib().adas_pipeline_step_yuv_host(self.h, frames, float(lane_crop_ratio)))

    def input_flags(self):
        """The decoder's flag word of every frame of the last step_jpeg_host (after sync()): int32 [frames], 0 for a clean frame
        (JpegDecoder.UNSUPPORTED / FORMAT / SIZE: the step saw a black frame; CORRUPT: damaged entropy data)."""
        if self.jpeg_decoder is None:
            raise ValueError("the pipeline was created without jpeg_input=")
        return self.jpeg_decoder.flags(self.S * self.B)

    def request_transform(self, stream, mode_name):
        """updateTransformParams(..., type=mode_name) for local stream `stream` on its NEXT step ("Default" | "Top" | "Bottom"): applied
        there if that frame's two ego lanes are detected, consumed either way; None or any other name is consumed without effect, as the
        reference ignores it (TaskConditions.transform_status can be None).  No re-capture."""
        if self.birdview is None:
            raise ValueError("the pipeline was created without birdview=")
        m = BirdView.MODES.get(mode_name, -1) if (mode_name is None or isinstance(mode_name, str)) else int(mode_name)
        L.check(L.lib().adas_pipeline_request_transform(self.h, int(stream), m))

    def birdview_image(self, frame=0):
        """The bird-view image of frame `frame` of the last step_frames (after sync()): (bird_h, bird_w, 3) uint8."""
        if self.warp is None:
            raise ValueError("the pipeline was created without birdview=dict(image=True)")
        return self.warp.fetch(frame)

    def overlay_image(self, frame=0):
        """frame_show of frame `frame` of the last step_frames (after sync()): (src_h, src_w, 3) uint8, the frame with the overlay drawn."""
        if self.overlay is None:
            raise ValueError("the pipeline was created without overlay=")
        return self.overlay.fetch(frame)

    def jpeg(self, frame=0):
        """The JPEG stream of frame `frame` of the last step_frames (after sync()) as bytes: write it out, or append it to a raw MJPEG file."""
        if self.jpeg_encoder is None:
            raise ValueError("the pipeline was created without jpeg=")
        return self.jpeg_encoder.fetch(frame)

    def jpeg_lengths(self):
        """(lengths [frames] int64, flags [frames] int32) of the last step's streams (after sync()); flag JpegEncoder.OVERFLOW: length 0."""
        if self.jpeg_encoder is None:
            raise ValueError("the pipeline was created without jpeg=")
        return self.jpeg_encoder.lengths(self.S * self.B)

    def yuv(self, frame=0):
        """Frame `frame` of the last step_frames (after sync()) in yuv_output's format: uint8 [yuv_writer.frame_bytes]."""
        if self.yuv_writer is None:
            raise ValueError("the pipeline was created without yuv_output=")
        return self.yuv_writer.frame(frame)

    def undistorted_image(self, frame=0):
        """Frame `frame` of the last step (after sync()) as the step read it, rectified: uint8 (src_h, src_w, 3)."""
        if self.remapper is None:
            raise ValueError("the pipeline was created without undistort=")
        return self.remapper.fetch(frame)

    def scaled_image(self, canvas=0):
        """Canvas `canvas` of the last step_frames (after sync()): uint8 [rows * h][cols * w][3] BGR, frame f in cell f % (cols * rows) of
        canvas f // (cols * rows)."""
        if self.scaler is None:
            raise ValueError("the pipeline was created without scale=")
        return self.scaler.canvas(canvas)

    def scaled_jpeg(self, canvas=0):
        """Canvas `canvas` of the last step (after sync()) as a baseline JPEG stream: uint8 [length]."""
        if self.scaled_jpeg_encoder is None:
            raise ValueError("the pipeline was created without scale= jpeg")
        return self.scaled_jpeg_encoder.fetch(canvas)

    def scaled_jpeg_lengths(self):
        """The stream lengths of the last step's canvases."""
        if self.scaled_jpeg_encoder is None:
            raise ValueError("the pipeline was created without scale= jpeg")
        return self.scaled_jpeg_encoder.lengths(self.scaler.canvases(self.S * self.B))

    def scaled_yuv(self, canvas=0):
        """Canvas `canvas` of the last step (after sync()) in scale= yuv's format: uint8 [scaled_yuv_writer.frame_bytes]."""
        if self.scaled_yuv_writer is None:
            raise ValueError("the pipeline was created without scale= yuv")
        return self.scaled_yuv_writer.frame(canvas)

    def scaled_yuv_all(self, out=None):
        """All canvases of the last step (after sync()) in one copy, canvas k at k * scaled_yuv_writer.p.frame_stride."""
        if self.scaled_yuv_writer is None:
            raise ValueError("the pipeline was created without scale= yuv")
        return self.scaled_yuv_writer.fetch_all(self.scaler.canvases(self.S * self.B), out)

    def yuv_all(self, out=None):
        """All n_streams x micro_batch frames of the last step (after sync()) in one copy: uint8 [yuv_writer.batch_bytes(frames)], frame f at
        f * yuv_writer.p.frame_stride.  out: a uint8 array to fill (pinned: _lib.PinnedBuffer(...).array)."""
        if self.yuv_writer is None:
            raise ValueError("the pipeline was created without yuv_output=")
        return self.yuv_writer.fetch_all(self.S * self.B, out)

    def graph_kernels(self):
        """Kernel launches of the captured step the last step replayed (use_graph=True)."""
        n = C.c_int32()
        L.check(L.lib().adas_pipeline_graph_kernels(self.h, C.byref(n)))
        return int(n.value)

    def wait_upload(self):
        """Block until the last step_frames_host upload has read its host buffer (then the buffer may be refilled)."""
        L.check(L.lib().adas_pipeline_wait_upload(self.h))

    def sync(self):
        L.check(L.lib().adas_pipeline_sync(self.h))

    def timings(self):
        ms = (C.c_float * 6)()
        L.check(L.lib().adas_pipeline_timings(self.h, ms))
        return dict(zip(("det_net", "det_post", "lane_net", "lane_decode", "tracker", "step"), [float(v) for v in ms]))

    def flops_per_frame(self):
        f = 0.0
        for e in (self.det, self.lane):
            if e:
                f += e.stats()["flops_per_frame"]
        return f

    def close(self):
        if getattr(self, "h", None):
            L.lib().adas_pipeline_destroy(self.h)
            self.h = None
        for o in (getattr(self, "remapper", None), getattr(self, "scaled_yuv_writer", None), getattr(self, "scaled_jpeg_encoder", None), getattr(self, "scaler", None),
                  getattr(self, "yuv_writer", None), getattr(self, "yuv_converter", None), getattr(self, "jpeg_decoder", None), getattr(self, "jpeg_encoder", None), self.overlay, self.analysis, self.birdview, self.warp, self.geometry, self.post, self.decode, self.tracker, self.det, self.lane):
            if o:
                o.close()

    __del__ = close
