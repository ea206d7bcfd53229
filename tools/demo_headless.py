#!/usr/bin/env python3
"""Headless counterpart of the reference's demo.py main loop (demo.py:230-296) on the drop-in classes: per frame
detector -> tracker, lane detector (+ device geometry), distance / collision point, bird-view image (device warp of the frame the
detector staged), FCWS / LDWS / LKAS state machine.
No window, no video codec: frames come from a seeded synthetic 1280x720 clip (moving rectangles on noise) or from a
.npy file of uint8 BGR frames (N, H, W, 3); one summary line per frame.

    python tools/demo_headless.py [--frames 30] [--det yolov8n.onnx|.hipm] [--det-type yolov8|efficientdet] [--lane culane_res18.onnx|.hipm] [--video clip.npy]
                                  [--mjpeg out.mjpeg] [--from-mjpeg in.mjpeg] [--from-yuv in.yuv --yuv-format nv12 --yuv-size 1280x720]
                                  [--yuv-out out.yuv --yuv-out-format i420] [--preview-mjpeg small.mjpeg --preview-size 320x180]
                                  [--readout-font FONT.npz [--readout-zoom 2] [--bird-out bird.npy]]

Without model paths, seeded random-weight models are built (their detections are noise: the point is the data flow)."""
import argparse, importlib, os, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

D = importlib.import_module("vehicle-cv-adas_amd.detectors")
A = importlib.import_module("vehicle-cv-adas_amd.analysis")
M = importlib.import_module("vehicle-cv-adas_amd.models")
PP = importlib.import_module("vehicle-cv-adas_amd.postproc")


def synthetic_clip(n, h=720, w=1280, seed=3):
    """SURVEY 8d C4 recipe: rectangles with constant velocity + jitter + 10 % dropout on grey noise."""
    rng = np.random.default_rng(seed)
    k = int(rng.integers(8, 30))
    pos = rng.uniform([100, 100], [w - 100, h - 100], (k, 2)); vel = rng.normal(0, 5, (k, 2))
    size = rng.uniform(40, 200, (k, 2)); col = rng.integers(0, 255, (k, 3))
    for _ in range(n):
        img = rng.normal(114, 20, (h, w, 3)).clip(0, 255).astype(np.uint8)
        pos += vel + rng.normal(0, 1, (k, 2))
        for i in range(k):
            if rng.uniform() < 0.1:
                continue
            x0, y0 = (pos[i] - size[i] / 2).astype(int); x1, y1 = (pos[i] + size[i] / 2).astype(int)
            img[max(0, y0):max(0, y1), max(0, x0):max(0, x1)] = col[i]
        yield img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--det", default=None); ap.add_argument("--lane", default=None); ap.add_argument("--video", default=None)
    ap.add_argument("--classes", default=None, help="label file, one name per line (default: 80 generic names)")
    ap.add_argument("--det-type", default="yolov8", choices=["yolov8", "efficientdet"],
                    help="demo.py picks EfficientdetDetector for ObjectModelType.EfficientDet and YoloDetector otherwise")
    ap.add_argument("--mjpeg", default=None, metavar="PATH",
                    help="demo.py:314 (vout.write): encode every frame on the device (postproc.JpegEncoder, quality 90) from the staged frame in HBM "
                         "and append its stream to PATH -- concatenated JPEGs are a raw MJPEG file.  This loop draws nothing, so the frames are "
                         "the camera's; the fused pipeline's jpeg= encodes the drawn overlay")
    ap.add_argument("--from-mjpeg", default=None, metavar="PATH",
                    help="demo.py:261 (cap.read) for a camera or file that delivers MJPEG: the inverse of --mjpeg.  PATH is a raw MJPEG file "
                         "(concatenated baseline JPEG streams); every frame is decoded on the device (postproc.JpegDecoder) instead of coming "
                         "from the synthetic clip.  A stream the decoder rejects is reported and shown to the loop as a black frame")
    ap.add_argument("--from-yuv", default=None, metavar="PATH",
                    help="demo.py:261 (cap.read) for a source that delivers raw camera frames: PATH holds tightly packed frames of --yuv-size in "
                         "--yuv-format, back to back (what `ffmpeg -f rawvideo -pix_fmt nv12` writes); every frame is converted to BGR on the "
                         "device (postproc.YuvConverter) instead of coming from the synthetic clip -- the cv2.cvtColor that cap.read() hides")
    ap.add_argument("--fonts", default=None, metavar="DIR",
                    help="demo.py:303-305 with their text: DIR holds glyph atlases slot<k>.npz (tools/make_font_atlas.py; slots as in "
                         "adas_overlay_text_style: 0 / 1 the label's size and text, 2 the tracker's label, 3 / 4 'ID:' and its shadow, 5 / 6 / 7 the "
                         "distance's size, text and shadow).  The three Draw*OnFrame calls then run on the staged frame in HBM -- boxes, "
                         "trajectories, discs and text -- and --mjpeg encodes the drawn frames")
    ap.add_argument("--readout-font", default=None, metavar="FONT.npz",
                    help="demo.py:292 with its drawing: calcCurveAndOffset also paints the arrow at the vehicle's position, the arrow at the "
                         "centre, 'Offset: %%.1f m' and 'R : %%.1f m' on the bird-view image, on the device, in this glyph atlas "
                         "(tools/make_font_atlas.py --scale 3 / zoom, e.g. --scale 1.5 for zoom 2); DrawDetectedOnBirdView's discs (demo.py:299) "
                         "then go on top.  The summary line counts the pixels they changed; --bird-out keeps the last image")
    ap.add_argument("--readout-zoom", type=int, default=2, help="the integer magnification of --readout-font's glyphs, 1 .. 4")
    ap.add_argument("--bird-out", default=None, metavar="PATH.npy", help="save the last frame's bird-view image (H, W, 3) uint8 as drawn")
    ap.add_argument("--yuv-format", default="nv12", choices=["nv12", "nv21", "i420", "yuyv", "uyvy"])
    ap.add_argument("--yuv-size", default="1280x720", metavar="WxH")
    ap.add_argument("--yuv-matrix", default="video", choices=["video", "full"])
    ap.add_argument("--yuv-out", default=None, metavar="PATH",
                    help="demo.py:314 (vout.write) for an encoder that is not MJPEG: convert every frame on the device (postproc.YuvWriter, BT.601 "
                         "limited range, chroma by the mean of a cell) from the staged frame in HBM -- the drawn frame with --fonts -- and append it "
                         "raw to PATH in --yuv-out-format, tightly packed: `ffmpeg -f rawvideo -pix_fmt yuv420p -s WxH -i PATH` reads an i420 file "
                         "(nv12, nv21, yuyv422, uyvy422 for the others)")
    ap.add_argument("--yuv-out-format", default="i420", choices=["nv12", "nv21", "i420", "yuyv", "uyvy"])
    ap.add_argument("--preview-mjpeg", default=None, metavar="PATH",
                    help="a low-rate preview next to the full-size outputs: reduce every frame on the device (postproc.FrameScaler, the exact "
                         "box filter) from the staged frame in HBM -- the drawn frame with --fonts -- to --preview-size, encode the reduced frame "
                         "(postproc.JpegEncoder, quality 90) and append its stream to PATH as raw MJPEG; the border of 2 pixels shows the frame's "
                         "FCWS state")
    ap.add_argument("--preview-size", default="320x180", metavar="WxH")
    ap.add_argument("--undistort", default=None, metavar="CAMERA.json",
                    help="the cv2.undistort a caller with a wide-angle camera runs in front of demo.py's loop: CAMERA.json holds {\"K\": [fx, fy, cx, "
                         "cy] or 3x3, \"D\": [k1, k2, p1, p2, (k3, (k4, k5, k6))], \"new_K\": optional}; the map is built on the device as "
                         "cv2.initUndistortRectifyMap writes it and every frame, whichever way it came in, is resampled through it on the device "
                         "(postproc.FrameRemapper) before the detectors see it")
    a = ap.parse_args()
    work = tempfile.mkdtemp(prefix="adas_demo_")
    effdet = a.det_type == "efficientdet"
    det_path = a.det or (M.build("efficientdet-d0").save(os.path.join(work, "efficientdet-d0.hipm")) if effdet
                         else M.build("yolov8n").save(os.path.join(work, "yolov8n.hipm")))
    lane_path = a.lane or M.build("ufldv2_res18", wsrc=M.SynthWeights(1, gain=M.RELU_RES_GAIN)).save(os.path.join(work, "culane_res18.hipm"))
    classes = a.classes
    if classes is None:
        classes = os.path.join(work, "labels.txt")
        names = ["person", "bicycle", "car", "motorbike", "aeroplane", "bus", "train", "truck"] + ["class%d" % i for i in range(8, 90 if effdet else 80)]
        open(classes, "w").write("\n".join(names) + "\n")

    # demo.py:236-260
    laneDetector = D.UltrafastLaneDetectorV2(lane_path, D.LaneModelType.UFLDV2_CULANE)
    if effdet:     # the EfficientDet-D0 network + its in-graph decode / NMS on the device (coreEngine.EfficientdetEngine)
        objectDetector = D.EfficientdetDetector(model_path=det_path, classes_path=classes, box_score=0.1 if a.det is None else 0.6)
    else:
        objectDetector = D.YoloDetector(model_path=det_path, model_type=D.ObjectModelType.YOLOV8, classes_path=classes, box_score=0.4, box_nms_iou=0.45)
    frames = np.load(a.video) if a.video else None
    decoder = None
    if a.from_mjpeg:
        streams = PP.split_mjpeg(open(a.from_mjpeg, "rb").read())
        if not streams or streams[0][1] is None:
            raise SystemExit("%s holds no JPEG stream with a frame header" % a.from_mjpeg)
        width, height = streams[0][1]
        decoder = PP.JpegDecoder(width, height, capacity=max(len(s) for s, _ in streams))

        def decoded():
            for k, (s, _) in enumerate(streams):
                decoder.run_host([s])
                flag = int(decoder.flags(1)[0])
                if flag:
                    print("stream %d of %s: decoder flags 0x%x" % (k, a.from_mjpeg, flag))
                yield decoder.image(0)
        frames = decoded()
    elif a.from_yuv:
        width, height = (int(v) for v in a.yuv_size.lower().split("x"))
        decoder = PP.YuvConverter(a.yuv_format, width, height, matrix=a.yuv_matrix)
        raw = np.fromfile(a.from_yuv, np.uint8)
        if len(raw) < decoder.frame_bytes:
            raise SystemExit("%s holds %d bytes, a %dx%d %s frame has %d" % (a.from_yuv, len(raw), width, height, a.yuv_format, decoder.frame_bytes))

        def converted():
            for k in range(len(raw) // decoder.frame_bytes):
                decoder.run_host(raw[k * decoder.frame_bytes:(k + 1) * decoder.frame_bytes], 1)
                yield decoder.image(0)
        frames = converted()
    else:
        first = frames[0] if frames is not None else next(synthetic_clip(1))
        height, width = first.shape[:2]
    transformView = A.PerspectiveTransformation((width, height))
    laneDetector.enable_device_geometry(transformView)
    distanceDetector = A.SingleCamDistanceMeasure()
    fonts = None
    if a.fonts:
        import glob, re
        fonts = {int(re.search(r"slot(\d+)\.npz$", f).group(1)): {k: (v if v.ndim else v.item()) for k, v in np.load(f).items()}
                 for f in sorted(glob.glob(os.path.join(a.fonts, "slot*.npz")))}
        if not fonts:
            raise SystemExit("%s holds no slot<k>.npz atlas" % a.fonts)
    objectTracker = D.BYTETracker(names=dict(objectDetector.colors_dict), draw_trajectories=True) if fonts else D.BYTETracker()
    if fonts:
        for task in (objectDetector, objectTracker, distanceDetector):
            task.set_text_fonts(fonts)
    if a.readout_font:
        transformView.set_readout_font({k: (v if v.ndim else v.item()) for k, v in np.load(a.readout_font).items()}, a.readout_zoom)
    analyzeMsg = A.TaskConditions()

    encoder = PP.JpegEncoder(width, height, quality=90, capacity=PP.JpegEncoder.bound(width, height)) if a.mjpeg else None
    vout = open(a.mjpeg, "wb") if a.mjpeg else None
    writer = PP.YuvWriter(a.yuv_out_format, width, height) if a.yuv_out else None
    yout = open(a.yuv_out, "ab") if a.yuv_out else None
    scaler = pv_encoder = pout = d_state = None
    if a.preview_mjpeg:
        pw, ph = (int(v) for v in a.preview_size.lower().split("x"))
        scaler = PP.FrameScaler((width, height), (pw, ph), "area", border=2 if min(pw, ph) > 4 else 0)
        pv_encoder = PP.JpegEncoder(pw, ph, quality=90, capacity=PP.JpegEncoder.bound(pw, ph))
        pout = open(a.preview_mjpeg, "ab")
        d_state = PP.L.DeviceBuffer(4)
    written = raw_written = pv_written = 0
    src = iter(frames) if frames is not None else synthetic_clip(a.frames)
    remapper = None
    if a.undistort:
        import json
        cam = json.load(open(a.undistort))
        unknown = set(cam) - {"K", "D", "new_K"}
        if unknown or "K" not in cam:
            raise SystemExit("%s: a camera file holds K, D and optionally new_K (unknown: %s)" % (a.undistort, sorted(unknown)))
        remapper = PP.FrameRemapper((height, width), 1, cameras=[cam])
        d_cam = PP.L.DeviceBuffer(height * width * 3)

        def rectified(it):
            for f in it:
                d_cam.upload(np.ascontiguousarray(f, np.uint8))
                remapper.run(d_cam.ptr, 1)
                yield remapper.fetch(0)
        src = rectified(src)
    t0 = time.perf_counter()
    n = 0
    for frame in src:
        if n >= a.frames:
            break
        # demo.py:268-281
        objectDetector.DetectFrame(frame)
        box = [obj.tolist(format_type="xyxy") for obj in objectDetector.object_info]
        score = [obj.conf for obj in objectDetector.object_info]
        ids = [obj.label for obj in objectDetector.object_info]
        tracks = objectTracker.update(box, score, ids, frame)
        laneDetector.DetectFrame(frame)
        # demo.py:284-296
        distanceDetector.updateDistance(objectDetector.object_info)
        vehicle_distance = distanceDetector.calcCollisionPoint(laneDetector.lane_info.area_points)
        if analyzeMsg.CheckStatus() and laneDetector.lane_info.area_status:
            transformView.updateTransformParams(*laneDetector.lane_info.lanes_points[1:3], analyzeMsg.transform_status)
        birdview_show = transformView.transformToBirdView(objectDetector.staged_frame)    # demo.py:289, from the frame already in HBM
        bird = laneDetector.birdview_lanes_points                                         # demo.py:291, left by the device geometry
        # demo.py:292 calls calcCurveAndOffset on the warped image, so this loop does too; laneDetector.curve_and_offset holds the same
        # three values from the device geometry (the two agree to 1e-7 relative, test_lane_detector_device_geometry: the same points, an fp64 fit on either side)
        bird_before = birdview_show.copy() if a.readout_font else None
        if min(len(bird[1]), len(bird[2])) >= 3:                                          # a parabola needs three points per ego lane
            (vehicle_direction, vehicle_curvature), vehicle_offset = transformView.calcCurveAndOffset(birdview_show, *bird[1:3])
        else:
            (vehicle_direction, vehicle_curvature), vehicle_offset = (None, None), None
        if a.readout_font:                                                                # demo.py:299, over the readouts
            readout_px = int((birdview_show != bird_before).any(axis=2).sum())
            transformView.DrawDetectedOnBirdView(birdview_show, bird, analyzeMsg.offset_msg)
            print("frame %3d: bird view: readouts changed %d pixels" % (n, readout_px))
        analyzeMsg.UpdateCollisionStatus(vehicle_distance, laneDetector.lane_info.area_status)
        analyzeMsg.UpdateOffsetStatus(vehicle_offset)
        analyzeMsg.UpdateRouteStatus(vehicle_direction, vehicle_curvature)
        print("frame %3d: %2d objects, %2d tracks | lanes %s area %-5s | dir %-4s R %s off %s | FCWS %-8s LDWS %-8s LKAS %s" % (
            n, len(box), len(tracks), "".join("1" if s else "0" for s in laneDetector.lane_info.lanes_status),
            laneDetector.lane_info.area_status, vehicle_direction,
            "%.0f m" % vehicle_curvature if vehicle_curvature is not None else "-",
            "%+.2f m" % vehicle_offset if vehicle_offset is not None else "-",
            analyzeMsg.collision_msg.name, analyzeMsg.offset_msg.name, analyzeMsg.curvature_msg.name))
        if fonts:                                                                         # demo.py:303-305, where the frame sits
            frame_show = objectDetector.staged_frame
            objectDetector.DrawDetectedOnFrame(frame_show)
            objectTracker.DrawTrackedOnFrame(frame_show, False)
            distanceDetector.DrawDetectedOnFrame(frame_show)
        if encoder is not None:                                                           # demo.py:314
            encoder.run(objectDetector.staged_frame.ptr, 1)
            written += vout.write(encoder.fetch(0))
        if writer is not None:                                                            # demo.py:314, for any other encoder
            writer.run_device(objectDetector.staged_frame.ptr, 1)
            raw_written += yout.write(writer.frame(0).tobytes())
        if scaler is not None:                                                            # the reduced frame of the same finished frame
            state = np.array([("UNKNOWN", "NORMAL", "PROMPT", "WARNING").index(analyzeMsg.collision_msg.name)], np.int32)
            PP.L.check(PP.L.lib().adas_memcpy_h2d(d_state.ptr, PP.L.ptr(state), 4))
            scaler.run_device(objectDetector.staged_frame.ptr, 1, d_state=d_state.ptr)
            pv_encoder.run(scaler.device_view(), 1)
            pv_written += pout.write(pv_encoder.fetch(0))
        n += 1
    dt = time.perf_counter() - t0
    if a.bird_out and n:
        np.save(a.bird_out, birdview_show)
    if encoder is not None:
        vout.close(); encoder.close()
        print("%s: %d JPEG streams, %d bytes (%.0f per frame, 1 / %.1f of the raw frames)" % (a.mjpeg, n, written, written / max(n, 1),
                                                                                            n * height * width * 3 / max(written, 1)))
    if writer is not None:
        yout.close(); writer.close()
        print("%s: %d %s frames of %dx%d appended, %d bytes (%d per frame, 1 / %.1f of the BGR frames)"
              % (a.yuv_out, n, a.yuv_out_format, width, height, raw_written, raw_written // max(n, 1), n * height * width * 3 / max(raw_written, 1)))
    if scaler is not None:
        pout.close(); pv_encoder.close(); scaler.close(); d_state.free()
        print("%s: %d JPEG streams of %s appended, %d bytes (%.0f per frame)" % (a.preview_mjpeg, n, a.preview_size, pv_written, pv_written / max(n, 1)))
    print("%d frames in %.2f s (%.1f frames/s, single stream, host frames: upload + 2 nets + post-processing + fetch per frame)" % (n, dt, n / dt))
    transformView.close(); objectDetector.close(); laneDetector.close(); objectTracker.close()
    if decoder is not None:
        decoder.close()
    if remapper is not None:
        remapper.close(); d_cam.free()
    return n


if __name__ == "__main__":
    main()
