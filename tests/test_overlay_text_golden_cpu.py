"""CPU: the item lists of the host build of csrc/overlay_text_core.h against the calls the REFERENCE's own functions made under a recording
cv2 -- tests/golden/text_calls.json.gz (YoloDetector.DrawDetectedOnFrame, SingleCamDistanceMeasure.DrawDetectedOnFrame, ControlPanel's two
text-bearing panels; tests/golden/make_golden_text.py) and the putText calls of tests/golden/track_draw.json.gz (BYTETracker.
DrawTrackedOnFrame): strings, origins, colours, rectangle corners and call order, field for field, for every recorded frame.  What the
fixture cannot hold is the font: the ladder's slot is checked against the fontScale the reference passed."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

import emu_overlay_text_api as emu
import text_ref as R
import text_scene as TS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
STYLE = dict(TS.STYLE, id_shadow_first=TS.LADDER[0], id_shadow_count=TS.LADDER[1])       # three ladders of three slots, the rest of one


@pytest.fixture(scope="module")
def fonts():
    return TS.fonts()


def load(name):
    with gzip.open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def clamp(colour):
    return tuple(max(0, min(255, int(c))) for c in colour)     # a cv2 scalar saturates


def check_run(item, call, fonts, ladder):
    kind, text, org, face, scale, colour, thickness = call
    assert kind == "putText" and item["kind"] == R.RUN
    assert (item["text"], [item["x"], item["y"]], tuple(item["color"])) == (text, org, clamp(colour)), (item, call)
    assert item["slot"] == R.ladder(fonts, ladder[0], ladder[1], scale), (item, call)


def test_fixture_holds_the_cases():
    import make_golden_text as MT
    fx = load("text_calls.json.gz")
    assert fx["required"] == MT.REQUIRED
    assert set(MT.REQUIRED) <= MT.coverage(fx["frames"])
    assert [[f[k] for k in ("dets", "points", "offset", "curvature", "collision")] for f in fx["frames"]] == \
        [[f[k] for k in ("dets", "points", "offset", "curvature", "collision")] for f in MT.frames()]


def test_items_equal_the_reference_calls(fonts):
    fx = load("text_calls.json.gz")
    H, W, names = fx["H"], fx["W"], fx["names"]
    st = dict(R.default_style(), **STYLE)
    scenes = []
    for f in fx["frames"]:
        s = TS.empty_scene()
        s.update(det_names=names, det_colors=[tuple(c) for c in fx["colors"]], offset=f["offset"], curvature=f["curvature"], collision=f["collision"],
                 det_xyxy=np.array([[x, y, x + w, y + h] for x, y, w, h, _ in f["dets"]], np.int32),
                 det_cls=np.array([names.index(l) if l in names else -1 for *_, l in f["dets"]], np.int32),
                 dist_points=np.array([p[:2] for p in f["points"]], np.int32), dist_d=np.array([p[2] for p in f["points"]]))
        scenes.append(s)
    mask = R.DETECTIONS | R.DISTANCE | R.PANELS
    _, items, flags = emu.run(np.zeros((len(scenes), H, W, 3), np.uint8), scenes, fonts, mask, style=STYLE)
    assert flags == [0] * len(scenes)
    for q, (f, got) in enumerate(zip(fx["frames"], items)):
        calls = f["calls"]
        assert len(got) == len(calls), q
        n_det, n_pts = len(f["dets"]), len(f["points"])
        for i, (it, c) in enumerate(zip(got, calls)):
            if c[0] == "rectangle":
                assert (it["kind"], [it["x"], it["y"]], [it["x1"], it["y1"]], tuple(it["color"])) == (R.RECT, c[1], c[2], tuple(c[3])), (q, i)
                assert it["source"] == R.DETECTIONS
            elif i < 2 * n_det:
                check_run(it, c, fonts, (st["det_label_slot"], 1))
            elif i < 2 * n_det + 2 * n_pts:
                shadow = (i - 2 * n_det) % 2 == 0            # putText_shadow: the shadow first
                assert c[3] == (3 if shadow else 4) and c[6] == (2 if shadow else 1), (q, i, c)
                check_run(it, c, fonts, (st["dist_shadow_first"], st["dist_shadow_count"]) if shadow else (st["dist_first"], st["dist_count"]))
            else:
                check_run(it, c, fonts, ((st["ldws_slot"], 1), (st["lkas_slot"], 1), (st["fcws_slot"], 1))[i - 2 * n_det - 2 * n_pts])
                assert it["source"] == R.PANELS


def test_track_text_equals_the_reference_calls(fonts):
    fx = load("track_draw.json.gz")
    H, W = fx["H"], fx["W"]
    names, colors = [n for n, _ in fx["names"]], [tuple(c) for _, c in fx["names"]]
    st = dict(R.default_style(), **STYLE)
    scenes, want = [], []
    for f in fx["frames"]:
        rows = [t for t in f["tracks"] if t["listed"] == "tracked" and t["is_activated"]]
        s = TS.empty_scene()
        s.update(trk_names=names, trk_colors=colors, trk_tlwh=np.array([t["tlwh"] for t in rows], np.float64).reshape(-1, 4),
                 trk_cls=np.array([t["class_id"] for t in rows], np.int32), trk_ids=np.array([t["track_id"] for t in rows], np.int32),
                 trk_last=np.array([t["trajectory"][-1] if t["trajectory"] else [0.0] * 4 for t in rows], np.float64).reshape(-1, 4),
                 traj_len=np.array([len(t["trajectory"]) for t in rows], np.int32))
        scenes.append(s)
        texts = [c for c in f["calls_both"] if c[0] == "putText"]
        want.append(([c for c in texts if not c[1].startswith("ID: ")], [c for c in texts if c[1].startswith("ID: ")]))
    _, items, flags = emu.run(np.zeros((len(scenes), H, W, 3), np.uint8), scenes, fonts, R.TRACKS | R.TRACK_IDS, style=STYLE)
    n_labels = n_ids = 0
    for q, (got, (labels, ids)) in enumerate(zip(items, want)):
        g_labels, g_ids = [i for i in got if i["source"] == R.TRACKS], [i for i in got if i["source"] == R.TRACK_IDS]
        assert got == g_labels + g_ids and len(g_labels) == len(labels) and len(g_ids) == len(ids), q
        for it, c in zip(g_labels, labels):
            check_run(it, c, fonts, (st["track_slot"], 1))
        for k, (it, c) in enumerate(zip(g_ids, ids)):
            shadow = k % 2 == 0
            assert c[3] == (3 if shadow else 4) and c[6] == (2 if shadow else 1), (q, k, c)
            check_run(it, c, fonts, (st["id_shadow_first"], st["id_shadow_count"]) if shadow else (st["id_first"], st["id_count"]))
        n_labels, n_ids = n_labels + len(labels), n_ids + len(ids)
    assert n_labels > 100 and n_ids > 100 and flags == [0] * len(scenes)
