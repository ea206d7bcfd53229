"""GPU: the text of the drop-in Draw*OnFrame classes (detectors.YoloDetector / EfficientdetDetector through their shared mixin,
detectors.BYTETracker, analysis.SingleCamDistanceMeasure) and tools/demo_headless.py --fonts.  Without fonts a call draws what it drew
before; with set_text_fonts the image is the NumPy restatement's (tests/text_ref.py) painted over that."""
import importlib
import os
import runpy
import sys

import numpy as np
import pytest

from conftest import load_pkg
import text_ref as R
import text_scene as TS

pytestmark = pytest.mark.gpu
load_pkg()
D = importlib.import_module("adas_amd.detectors")
A = importlib.import_module("adas_amd.analysis")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 240, 320
COLORS = {"car": (0, 0, 255), "person": (0, 255, 0), "truck": (255, 5, 0)}


@pytest.fixture(scope="module")
def fonts():
    return TS.fonts()


def frame(seed=3):
    return TS.background(1, H, W, seed)[0]


class Boxes(D._DrawsBoxes):          # DrawDetectedOnFrame as the two detector classes inherit it, without a network
    def __init__(self, infos, style=None):
        self._object_info, self.colors_dict = infos, COLORS
        if style is not None:
            self.TEXT_STYLE = style


@pytest.mark.parametrize("style", ({}, D.EfficientdetDetector.TEXT_STYLE), ids=("yolo", "efficientdet"))
def test_detector_labels(fonts, style):
    infos = [D.RectInfo(5.0, 0.0, 60.0, 40.0, 0.9, "car"), D.RectInfo(100.5, 80.2, 70.0, 50.0, 0.8, "unknown"), D.RectInfo(280.0, 200.0, 60.0, 60.0, 0.7, "truck"),
             D.RectInfo(-10.0, 120.0, 40.0, 30.0, 0.7, "person")]
    plain, text = Boxes(infos, style), Boxes(infos, style)
    before, got = frame(), frame()
    plain.DrawDetectedOnFrame(before)                       # no fonts: the boxes only, as before
    assert not np.array_equal(before, frame())
    text.set_text_fonts(fonts)
    assert text.text_style == dict(style)
    text.DrawDetectedOnFrame(got)
    names = [i.label for i in infos]
    known = [n for n in names if n != "unknown"]
    scene = dict(det_xyxy=[i.tolist() for i in infos], det_cls=[known.index(n) if n != "unknown" else -1 for n in names], det_names=known,
                 det_colors=[COLORS[n] for n in known])
    items, _ = R.layout(scene, fonts, W, H, R.DETECTIONS, style)
    assert [i["text"] for i in items if i["kind"] == R.RUN] == names
    assert np.array_equal(got, R.paint(before.copy(), items, fonts))
    assert (got != before).any()
    # the same labels again: no table, font or style is set a second time (each setter waits for the device and makes a captured step of
    # the process re-capture), and the frame is the same
    calls = []
    tov = text._painter.tov
    for name in ("set_fonts", "set_text_style", "set_class_colors", "set_text_labels"):
        setattr(tov, name, lambda *a, _n=name, **k: calls.append(_n))
    again = frame()
    text.DrawDetectedOnFrame(again)
    assert calls == [] and np.array_equal(again, got)
    for name in ("set_fonts", "set_text_style", "set_class_colors", "set_text_labels"):
        delattr(tov, name)
    for o in (plain, text):
        o._close_painter()


def test_distance_discs_and_text(fonts):
    plain, text = A.SingleCamDistanceMeasure(), A.SingleCamDistanceMeasure()
    pts = [[40, 50, 2.125], [200, 120, -1.0], [310, 230, 0.375], [150, 30, 12.5]]
    plain.distance_points = text.distance_points = pts
    before, got = frame(), frame()
    plain.DrawDetectedOnFrame(before)
    assert (before[50, 40] == 255).all() and not np.array_equal(before, frame())       # the disc
    text.set_text_fonts(fonts, **TS.STYLE)
    text.DrawDetectedOnFrame(got)
    items, _ = R.layout(dict(dist_points=[p[:2] for p in pts], dist_d=[p[2] for p in pts]), fonts, W, H, R.DISTANCE, TS.STYLE)
    assert [i["text"] for i in items[1::2]] == [" 2.12 m", " unknown m", " 0.38 m", " 12.50 m"]
    assert np.array_equal(got, R.paint(before.copy(), items, fonts))
    empty = A.SingleCamDistanceMeasure()
    empty.set_text_fonts(fonts)
    untouched = frame()
    empty.DrawDetectedOnFrame(untouched)
    assert np.array_equal(untouched, frame())


def test_tracker_labels_and_ids(fonts):
    plain = D.BYTETracker(names=dict(COLORS), draw_trajectories=True)
    text = D.BYTETracker(names=dict(COLORS), draw_trajectories=True)
    text.set_text_fonts(fonts, **TS.STYLE)
    labels = ["car", "person", "truck"]
    for f in range(5):
        boxes = [[20.0 + 4 * f, 100.0, 60.0 + 4 * f, 130.0], [150.0, 60.0 + f, 180.0, 100.0 + f], [200.0 - 3 * f, 150.0, 250.0 - 3 * f, 194.0], [260.0, 20.0, 263.0, 23.0]]
        for t in (plain, text):
            t.update(boxes, [0.9, 0.88, 0.86, 0.84], labels + ["car"], None)
    for args in ((True, True), (False, True), (True, False)):
        before, got = frame(), frame()
        plain.DrawTrackedOnFrame(before, *args)
        text.DrawTrackedOnFrame(got, *args)
        online = [t for t in text.tracked_stracks if t["is_activated"]]
        traj = text.trajectories()
        scene = dict(trk_tlwh=[t["tlwh"] for t in online], trk_cls=list(range(len(online))), trk_ids=[t["track_id"] for t in online],
                     trk_names=[t["class_id"] for t in online], trk_colors=[COLORS[t["class_id"]] for t in online],
                     trk_last=[traj[int(t["track_id"])][-1] for t in online], traj_len=[len(traj[int(t["track_id"])]) for t in online])
        mask = (R.TRACKS if args[0] else 0) | (R.TRACK_IDS if args[1] else 0)
        items, _ = R.layout(scene, fonts, W, H, mask, TS.STYLE)
        assert len(items) >= (3 if args[0] else 0) + (6 if args[1] else 0), args      # the 3 x 3 box fails the area gate
        assert np.array_equal(got, R.paint(before.copy(), items, fonts)), args
    for t in (plain, text):
        t.close()


def test_headless_demo_with_fonts(fonts, tmp_path, capsys):
    for slot in range(10):
        np.savez(str(tmp_path / ("slot%d.npz" % slot)), **fonts[slot])
    out = str(tmp_path / "drawn.mjpeg")
    argv = sys.argv
    sys.argv = ["demo_headless.py", "--frames", "3", "--fonts", str(tmp_path), "--mjpeg", out]
    try:
        mod = runpy.run_path(os.path.join(ROOT, "tools", "demo_headless.py"), run_name="demo_headless")
        assert mod["main"]() == 3
    finally:
        sys.argv = argv
    assert capsys.readouterr().out.count("frame ") == 3 and os.path.getsize(out) > 0
