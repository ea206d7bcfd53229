#!/usr/bin/env python3
"""Golden drawing calls of the REFERENCE's BYTETracker.DrawTrackedOnFrame (byteTracker.py:202-215, ObjectTracker/core.py:39-245), run
unmodified under the usual import stubs with a cv2 stub that RECORDS every circle, rectangle, arrowedLine, putText and
addWeighted call with its arguments instead of drawing:

    python tests/golden/make_golden_trackdraw.py     # needs the reference checkout (ADAS_REFERENCE); writes track_draw.json.gz

A scene of moving boxes on a 240 x 320 frame (small, so that filter_trajectories' 10-pixel border bites), 52 frames (rings wrap).  After
every update the calls are recorded twice: DrawTrackedOnFrame(frame, False) -- the demo's call -- and DrawTrackedOnFrame(frame, True, True).
Per frame the fixture holds the detections fed to update(), the live tracks (tracked then lost: id, state, is_activated, class, tlwh,
trajectory) and the two call lists.  REQUIRED lists what the recording must contain; it is asserted here and again by the test."""
import gzip, json, os, sys, types
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG

H, W, N_FRAMES = 240, 320, 52
NAMES = {"car": (0, 0, 255), "person": (0, 255, 0), "truck": (255, 5, 0)}      # a channel under 10: the lock-on colour saturates at 0
REQUIRED = ["lock_n1", "lock_n2", "lock_n3", "lock_n4", "arrow", "wrapped_ring", "border_filtered", "shift_below_2", "area_gate", "not_activated_or_lost"]


def scene():
    """(boxes xyxy fp64, scores, class index) per frame: constant-velocity rectangles with a deterministic sub-pixel wobble."""
    objs = [  # x, y, w, h, vx, vy, class, first frame, last frame
        (20.0, 100.0, 40.0, 30.0, 4.0, 0.5, 0, 0, 51),      # crosses the frame: its ring wraps, an arrow
        (1.0, 30.0, 36.0, 28.0, 3.0, 1.0, 1, 0, 51),        # starts on the left border: its first boxes fail the 10-pixel filter
        (150.0, 60.0, 30.0, 40.0, 0.0, 0.0, 2, 0, 51),      # stands still: every pair has shift < 2
        (260.0, 20.0, 3.0, 3.0, 0.0, 0.0, 0, 0, 51),        # 3 x 3: fails the area gate
        (200.0, 150.0, 50.0, 44.0, -3.0, -1.5, 1, 20, 51),  # appears late: tracked but not activated on its first frame
        (60.0, 170.0, 44.0, 36.0, 2.0, 0.0, 2, 0, 30),      # disappears: lost
        (250.0, 180.0, 60.0, 50.0, 2.5, 1.0, 0, 5, 51),     # runs into the bottom right corner: its last boxes fail the filter
    ]
    frames = []
    for f in range(N_FRAMES):
        boxes, scores, ids = [], [], []
        for k, (x, y, w, h, vx, vy, c, f0, f1) in enumerate(objs):
            if not f0 <= f <= f1:
                continue
            wob = 0.25 * ((f * 7 + k * 3) % 4) - 0.375      # -0.375 .. 0.375, exact in binary
            x1, y1 = x + vx * (f - f0) + wob, y + vy * (f - f0) - wob
            boxes.append([x1, y1, x1 + w, y1 + h])
            scores.append(0.9 - 0.01 * k)
            ids.append(c)
        frames.append(dict(boxes=boxes, scores=scores, ids=ids))
    return frames


def install_cv2_recorder(log):
    cv2 = types.ModuleType("cv2")
    for k, v in dict(INTER_LINEAR=1, FONT_HERSHEY_TRIPLEX=4, FONT_HERSHEY_SIMPLEX=0, LINE_AA=16, LINE_8=8, LINE_4=4, COLOR_BGR2RGB=4, FILLED=-1).items():
        setattr(cv2, k, v)

    def num(v):
        if isinstance(v, (tuple, list, np.ndarray)):
            return [num(x) for x in v]
        if isinstance(v, (bool, np.bool_)):
            return bool(v)
        if isinstance(v, (int, np.integer)):
            return int(v)
        return float(v)

    def circle(img, center, radius, color, thickness=1, lineType=8, shift=0):
        assert isinstance(radius, int) and isinstance(thickness, int) and all(isinstance(c, int) for c in center)
        log.append(["circle", num(center), radius, num(color), thickness])
        return img

    def rectangle(img, pt1, pt2, color, thickness=1, lineType=8, shift=0):
        assert all(isinstance(c, (int, np.integer)) for c in tuple(pt1) + tuple(pt2))
        log.append(["rectangle", num(pt1), num(pt2), num(color), int(thickness)])
        return img

    def arrowedLine(img, pt1, pt2, color, thickness=1, line_type=8, shift=0, tipLength=0.1):
        assert all(isinstance(c, (int, np.integer)) for c in tuple(pt1) + tuple(pt2))
        log.append(["arrowedLine", num(pt1), num(pt2), num(color), int(thickness), float(tipLength)])
        return img

    def putText(img, text, org, fontFace=0, fontScale=1.0, color=(0, 0, 0), thickness=1, lineType=8, bottomLeftOrigin=False):
        log.append(["putText", str(text), num(org), int(fontFace), float(fontScale), num(color), int(thickness)])
        return img

    def addWeighted(src1, alpha, src2, beta, gamma, dst=None, dtype=-1):
        log.append(["addWeighted", list(src1.shape), float(alpha), num(src2.reshape(-1, src2.shape[-1])[0]) if src2.size else [], float(beta), float(gamma)])
        return src1.copy()

    for f in (circle, rectangle, arrowedLine, putText, addWeighted):
        setattr(cv2, f.__name__, f)
    sys.modules["cv2"] = cv2
    return cv2


def coverage(frames):
    """Which of REQUIRED the recording holds (from the recorded calls and track states alone: the test runs it too)."""
    got = set()
    for fr in frames:
        calls = fr["calls_traject"]
        for c in calls:
            if c[0] == "arrowedLine":
                got.add("arrow")
        for t in fr["tracks"]:
            tr, tl = t["trajectory"], t["tlwh"]
            drawn = t["listed"] == "tracked" and t["is_activated"] and tl[2] * tl[3] > 10
            kept = [b for b in tr if b[0] >= 10 and b[1] >= 10 and b[2] <= W - 10 and b[3] <= H - 10]
            if t["listed"] == "lost" or (t["listed"] == "tracked" and not t["is_activated"]):
                got.add("not_activated_or_lost")
            if t["listed"] == "tracked" and t["is_activated"] and not tl[2] * tl[3] > 10:
                got.add("area_gate")
            if not drawn:
                continue
            if len(kept) < len(tr):
                got.add("border_filtered")
            if t["appended"] > 30 and len(tr) == 30:
                got.add("wrapped_ring")
            n = len(kept) - 1
            if 1 <= n <= 4:
                got.add("lock_n%d" % n)
            for a, b in zip(kept, kept[1:]):
                if abs(min(q - p for p, q in zip(a, b))) < 2:
                    got.add("shift_below_2")
    return got


def main():
    MG.install_stubs()
    log = []
    install_cv2_recorder(log)
    from ObjectTracker.byteTrack.byteTracker import BYTETracker
    from ObjectTracker.byteTrack.dtypes import BaseTrack, STrack
    BaseTrack.reset_counter()
    STrack.update_crops = lambda self, frame: None
    lab = list(NAMES.keys())
    trk = BYTETracker(names=NAMES)
    appended = {}
    out = []
    for k, fr in enumerate(scene()):
        trk.update(np.asarray(fr["boxes"], np.float64).reshape(-1, 4), np.asarray(fr["scores"], np.float64), [lab[i] for i in fr["ids"]], None)
        tracks = []
        for listed, lst in (("tracked", trk.tracked_stracks), ("lost", trk.lost_stracks)):
            for t in lst:
                traj = [[float(v) for v in b] for b in t.trajectories]
                last = appended.get(t.track_id, (0, None))
                if traj and traj[-1] != last[1]:      # one append per matched frame; the wobble makes consecutive boxes differ
                    appended[t.track_id] = (last[0] + 1, traj[-1])
                tracks.append(dict(track_id=int(t.track_id), listed=listed, state=int(t.state), is_activated=bool(t.is_activated),
                                   class_id=lab.index(t.class_id), tlwh=[float(v) for v in t.tlwh], trajectory=traj,
                                   appended=appended.get(t.track_id, (0, None))[0]))
        rec = {}
        for key, args in (("calls_traject", (False,)), ("calls_both", (True, True))):
            del log[:]
            trk.DrawTrackedOnFrame(np.zeros((H, W, 3), np.uint8), *args)
            rec[key] = [list(c) for c in log]
        out.append(dict(boxes=fr["boxes"], scores=fr["scores"], ids=fr["ids"], tracks=tracks, **rec))
    got = coverage(out)
    missing = [r for r in REQUIRED if r not in got]
    assert not missing, "the scenario lacks %s: change the scenario, not the list" % missing
    res = dict(H=H, W=W, names=[[k, list(v)] for k, v in NAMES.items()], required=REQUIRED, frames=out)
    path = os.path.join(HERE, "track_draw.json.gz")
    with open(path, "wb") as raw:       # mtime 0, no file name: the same bytes on every run
        with gzip.GzipFile(filename="", fileobj=raw, mode="wb", mtime=0) as f:
            f.write(json.dumps(res).encode())
    n_calls = sum(len(f["calls_traject"]) for f in out)
    print("frames", len(out), "calls (demo's form)", n_calls, "arrows", sum(c[0] == "arrowedLine" for f in out for c in f["calls_traject"]),
          "rectangles", sum(c[0] == "rectangle" for f in out for c in f["calls_traject"]), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
