#!/usr/bin/env python3
"""Golden TEXT calls of the REFERENCE, run unmodified under the usual import stubs with a cv2 stub that RECORDS putText and
the filled cv2.rectangle with their arguments instead of drawing:

    python tests/golden/make_golden_text.py     # needs the reference checkout (ADAS_REFERENCE); writes text_calls.json.gz

The functions: YoloDetector.DrawDetectedOnFrame (yoloDetector.py:170-191), SingleCamDistanceMeasure.DrawDetectedOnFrame
(distanceMeasure.py:95-115) and ControlPanel.DisplaySignsPanel / DisplayCollisionPanel (demo.py:173-174, 212; the class is lifted from
demo.py's syntax tree as tests/golden/make_golden_panels.py does).  The tracker's putText calls are already held by track_draw.json.gz
(make_golden_trackdraw.py); the test reads them from there.  The stub's getTextSize answers from the tests' synthetic font
(tests/text_scene.py) by rule T2: thickness 3 is the distance's size slot, anything else the label box's.  Per frame the fixture holds the
inputs (boxes with labels, distance points, the three message types) and the recorded calls in call order: ["rectangle", pt1, pt2, colour]
for a filled rectangle, ["putText", text, org, face, scale, colour, thickness].  The FPS and inference-time strings are not restated by the
device (they are caller lines) and are left out.  REQUIRED lists what the recording must contain; asserted here and again by the test."""
import gzip, json, os, sys
from decimal import Decimal
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG
import make_golden_panels as MP
import panel_scene as PS
import text_ref as R
import text_scene as TS

HW = PS.SMALL                        # 368 x 416: the smallest frame the panels fit
NAMES = ["car", "person", "truck", "traffic light"]
COLORS = [(255, 64, 0), (20, 200, 25), (0, 0, 255), (7, 8, 9)]
REQUIRED = ["label_ymin_0", "label_unknown", "d_negative", "d_binary_tie", "inv_d_above_0.4", "inv_d_below_0.4", "inv_d_above_1", "inv_d_below_1",
            "every_offset_string", "every_curvature_string", "every_collision_string"]
SKIPPED_PREFIXES = ("FPS", "object-infer", "lane-infer")


def frames():
    """The inputs: six frames walk the six curvature types (and the four offset and collision types)."""
    H, W = HW
    out = []
    dists = [[-1.0, 2.125, 0.375], [2.4, 2.6], [0.9999, 1.0001, 12.345], [0.5, 2.675, 60.0], [1.0, 0.4, 2.5], [7.005, -0.25]]
    for k in range(6):
        dets = [[3 + k, 0, 40, 30, NAMES[k % 4]], [W // 2 - 5 * k, H // 2 + k, 60, 50, "unknown" if k % 2 == 0 else NAMES[(k + 1) % 4]],
                [W - 12, H - 3 - k, 30, 20, NAMES[(k + 2) % 4]], [-6, 14 + k, 25, 25, NAMES[(k + 3) % 4]]]
        pts = [[(37 * (i + 1) * (k + 2)) % W, (53 * (i + 2) * (k + 1)) % H, d] for i, d in enumerate(dists[k])]
        out.append(dict(dets=dets, points=pts, offset=k % 4, curvature=k, collision=(k + 1) % 4))
    return out


def coverage(fr):
    """Which of REQUIRED the recording holds, from the recorded inputs and calls alone (the test runs it too)."""
    got, strings = set(), set()
    for f in fr:
        for x, y, w, h, label in f["dets"]:
            if y == 0:
                got.add("label_ymin_0")
            if label == "unknown":
                got.add("label_unknown")
        for x, y, d in f["points"]:
            if d < 0:
                got.add("d_negative")
                continue
            if Decimal(d) == Decimal("%.3f" % d) and ("%.3f" % d).endswith("5"):     # x.xx5 exactly: '%.2f' of it is a binary tie
                got.add("d_binary_tie")
            r = 1 / d
            if r > 1:
                got.add("inv_d_above_1")
            elif 0.4 < r < 1:
                got |= {"inv_d_below_1", "inv_d_above_0.4"}
            elif r < 0.4:
                got.add("inv_d_below_0.4")
        strings |= {c[1] for c in f["calls"] if c[0] == "putText"}
    if {"LDWS : " + s for s in R.OFFSET} <= strings:
        got.add("every_offset_string")
    if {"LKAS : " + s for s in R.CURVATURE} <= strings:
        got.add("every_curvature_string")
    if {"FCWS : " + s for s in R.COLLISION} <= strings:
        got.add("every_collision_string")
    return got


def install_recorder(cv2, log, fonts):
    def ints(v):
        return [int(x) for x in v]

    def putText(img, text, org, fontFace=0, fontScale=1.0, color=(0, 0, 0), thickness=1, lineType=8, bottomLeftOrigin=False):
        assert all(isinstance(c, (int, np.integer)) for c in org), org
        if not str(text).startswith(SKIPPED_PREFIXES):
            log.append(["putText", str(text), ints(org), int(fontFace), float(fontScale), ints(color), int(thickness)])
        return img

    def rectangle(img, pt1, pt2, color, thickness=1, lineType=8, shift=0):
        if thickness == -1:           # the label's background; cornerRect's outline is the object layer's
            assert all(isinstance(c, (int, np.integer)) for c in tuple(pt1) + tuple(pt2))
            log.append(["rectangle", ints(pt1), ints(pt2), ints(color)])
        return img

    def getTextSize(text, fontFace, fontScale, thickness):
        assert fontFace == 0
        w, h = R.text_size(fonts[5 if thickness == 3 else 0], text)
        return (w, h), 0

    def nothing(img, *a, **k):
        return img
    for f in (putText, rectangle, getTextSize):
        setattr(cv2, f.__name__, f)
    cv2.circle = cv2.line = nothing


def main():
    MG.install_stubs()
    log = []
    fonts = TS.fonts()
    sprites = PS.sprites()
    cv2 = MP.install_cv2(log, sprites)
    install_recorder(cv2, log, fonts)
    from ObjectDetector.utils import CollisionType
    from ObjectDetector.core import RectInfo
    from ObjectDetector.yoloDetector import YoloDetector
    from ObjectDetector.distanceMeasure import SingleCamDistanceMeasure
    from TrafficLaneDetector.ufldDetector.utils import OffsetType, CurvatureType
    ControlPanel = MP.lift_control_panel(cv2, dict(CollisionType=CollisionType, OffsetType=OffsetType, CurvatureType=CurvatureType))
    OFF = [getattr(OffsetType, n) for n in PS.OFFSETS]
    CUR = [getattr(CurvatureType, n) for n in PS.CURVATURES]
    COL = [getattr(CollisionType, n) for n in PS.COLLISIONS]
    det = object.__new__(YoloDetector)
    det.colors_dict = dict(zip(NAMES, COLORS))
    dist = SingleCamDistanceMeasure()
    cp = ControlPanel()
    out = []
    for f in frames():
        img = PS.collision_frame(HW)
        del log[:]
        det._object_info = [RectInfo(float(x), float(y), float(w), float(h), 0.9, label) for x, y, w, h, label in f["dets"]]
        det.DrawDetectedOnFrame(img)
        dist.distance_points = [list(p) for p in f["points"]]
        dist.DrawDetectedOnFrame(img)
        cp.DisplaySignsPanel(img, OFF[f["offset"]], CUR[f["curvature"]])
        cp.DisplayCollisionPanel(img, COL[f["collision"]], 0.02, 0.0125)
        out.append(dict(f, calls=[list(c) for c in log]))
    missing = [r for r in REQUIRED if r not in coverage(out)]
    assert not missing, "the scenario lacks %s: change the scenario, not the list" % missing
    res = dict(H=HW[0], W=HW[1], names=NAMES, colors=[list(c) for c in COLORS], required=REQUIRED, frames=out)
    path = os.path.join(HERE, "text_calls.json.gz")
    with open(path, "wb") as raw:       # mtime 0, no file name: the same bytes on every run
        with gzip.GzipFile(filename="", fileobj=raw, mode="wb", mtime=0) as g:
            g.write(json.dumps(res).encode())
    print("frames", len(out), "calls", sum(len(f["calls"]) for f in out), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
