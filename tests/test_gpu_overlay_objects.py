"""GPU: the overlay's object layer (boxes of the detector and of the tracker: csrc/overlay_kernels.hip, rules D6-D9 of overlay_core.h)
through the C ABI, postproc.LaneOverlay, the fused step and the drop-in Draw* methods against the NumPy restatement
(tests/overlay_objects_ref.py), every byte."""
import ctypes as C
import importlib

import numpy as np
import pytest

from conftest import load_pkg
import overlay_ref as ref
import overlay_objects_ref as oref
import overlay_scene as OS
from overlay_scene import noise
import synth

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")
CE = importlib.import_module("adas_amd.coreEngine")
PP = importlib.import_module("adas_amd.postproc")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")
A = importlib.import_module("adas_amd.analysis")
D = importlib.import_module("adas_amd.detectors")

INVALID = -1        # ADAS_ERR_INVALID
H, W = 45, 70       # three coverage words per row
DET, TRK = oref.DETECTIONS, oref.TRACKS
POLY = [(10, 5), (8, 12), (8, 12), (3, 20), (2, 30), (40, 30), (35, 21), (30, 12), (28, 5)]
DET_TABLE = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (200, 100, 50), (17, 34, 51)]
TRK_TABLE = [(10, 200, 250), (250, 10, 120), (90, 90, 10)]


class Scene(OS.Scene):
    """Per-frame geometry and boxes of a batch."""

    def __init__(self, n, det_cap=12, trk_cap=8, dist_cap=8, poly_cap=16):
        super().__init__(n, ("boxes",), det_cap, trk_cap, dist_cap, poly_cap)

    def want(self, src, stages, det_table=DET_TABLE, trk_table=TRK_TABLE, **kw):
        out = []
        for f in range(self.n):
            d, t = np.asarray(self.dets[f], np.int64).reshape(-1, 5), np.asarray(self.trks[f], np.float64).reshape(-1, 5)
            o, flags = oref.compose(src[f], self.lanes[f], self.poly[f], True, self.dist[f], stages=stages, dets=d[:, :4], det_cls=d[:, 4],
                                    det_table=det_table, trks=t[:, :4], trk_cls=t[:, 4].astype(np.int64), trk_table=trk_table, **kw)
            assert flags == 0
            out.append(o)
        return np.stack(out)


def make_overlay(n, h=H, w=W, det_table=DET_TABLE, trk_table=TRK_TABLE, **style):
    return OS.make_overlay(n, h, w, None, det_table, trk_table, **style)


def run(scene, src, stages, det_table=DET_TABLE, trk_table=TRK_TABLE, **kw):
    """OS.run with this file's class colours -> frames"""
    return OS.run(scene, src, stages, det_table=det_table, trk_table=trk_table, **kw).frames


def three_frames():
    """Frame 0: boxes over every border and with negative corners, one wholly outside, one narrower than its arms, a zero-size one, boxes
    straddling columns 31 / 32 and 63 / 64.  Frame 1: two overlapping detections of different classes and two overlapping tracks, over a
    polygon, lane discs and distance discs.  Frame 2: the same boxes in the other order, and a class id outside either table."""
    s = Scene(3)
    s.dets[0] = [(-6, -4, 20, 15, 0), (50, 30, W + 9, H + 5, 1), (-40, -40, -20, -20, 2), (W + 20, 3, W + 40, 9, 2), (40, 5, 43, 25, 3), (12, 30, 12, 30, 4),
                 (29, 20, 34, 40, 1), (60, 10, 66, 14, 0), (5, H - 3, 25, H + 10, 3), (W - 4, -8, W + 6, 8, 4)]
    s.trks[0] = [(-5.5, -3.2, 20.9, 15.1, 0), (55.0, 28.0, 40.0, 40.0, 1), (28.4, 8.0, 8.2, 12.0, 2), (60.2, 2.0, 6.9, 9.9, 0), (-60.0, 5.0, 20.0, 9.0, 1),
                 (W + 5.0, 5.0, 9.0, 9.0, 2)]
    s.lanes[1] = [[(20, 18), (40, 30)], [(22, 18)], [(21, 19)], [(21, 18), (60, 40)]]
    s.poly[1] = POLY
    s.dist[1] = [(30, 25), (12, 12), (45, 20)]
    s.dets[1] = [(10, 10, 40, 30, 0), (20, 15, 50, 35, 1)]
    s.trks[1] = [(10.9, 10.2, 30.7, 20.5, 0), (20.1, 15.0, 30.0, 20.0, 2)]
    s.lanes[2], s.poly[2], s.dist[2] = s.lanes[1], POLY, s.dist[1]
    s.dets[2] = [(20, 15, 50, 35, 1), (10, 10, 40, 30, 0), (3, 3, 9, 9, 99), (55, 3, 62, 12, -1)]
    s.trks[2] = [(20.1, 15.0, 30.0, 20.0, 2), (10.9, 10.2, 30.7, 20.5, 0), (50.0, 30.0, 12.0, 9.0, 7)]
    return s


@pytest.mark.parametrize("mode", ["offset16", "offset3", "own", "in_place"])
def test_three_frames_every_byte(mode):
    """210-byte rows: a frame's rows start on every alignment of a 16-byte piece, so a pixel's three bytes fall into two pieces."""
    src = noise(3, H, W, 1)
    s = three_frames()
    want = s.want(src, 7 | DET | TRK)
    got = run(s, src, 7 | DET | TRK, offset=3 if mode == "offset3" else 16, own=mode == "own", in_place=mode == "in_place")
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert tuple(want[1, 15, 40]) != tuple(want[2, 15, 40])                              # the order of the two detections shows where they cross
    assert tuple(want[1, 28, 33]) != tuple(want[2, 28, 33])                              # and the order of the two tints inside both tracks
    assert tuple(want[2, 3, 5]) == (0, 0, 0) and tuple(want[2, 3, 58]) == (0, 0, 0)      # class 99 and class -1: unknown, black
    assert tuple(want[1, 25, 30]) == ref.DIST_COLOR                                      # a distance disc over the boxes
    assert (want != src).any(axis=3).mean() > 0.2


@pytest.mark.parametrize("stages", [DET, TRK, DET | TRK, 1 | DET, 2 | TRK, 4 | DET | TRK, 3 | DET, 7 | TRK, 7 | DET | TRK])
def test_each_stage_alone_and_together(stages):
    src = noise(3, H, W, 2)
    s = three_frames()
    got = run(s, src, stages)
    assert np.array_equal(got, s.want(src, stages))


def test_new_stages_off_is_the_image_without_them():
    """Stages 7 through adas_overlay_run_arrays_objects with boxes given equals stages 7 through adas_overlay_run_arrays without them; the old
    entry point refuses the new bits."""
    src = noise(3, H, W, 3)
    s = three_frames()
    got = run(s, src, 7)
    plain = three_frames()
    plain.dets, plain.trks = [[] for _ in range(3)], [[] for _ in range(3)]
    assert np.array_equal(got, plain.want(src, 7))
    ov = PP.LaneOverlay((H, W), None, 1)
    sbuf = L.DeviceBuffer.from_array(src)
    with pytest.raises(RuntimeError, match="adas_overlay_run_arrays: unknown stage bits") as ei:
        L.check(L.lib().adas_overlay_run_arrays(ov.h, sbuf.ptr, None, None, None, None, 0, None, None, None, None, None, 0, None, None, None, None, DET, 1, None))
    assert ei.value.code == INVALID
    with pytest.raises(RuntimeError, match="adas_overlay_run: unknown stage bits") as ei:
        L.check(L.lib().adas_overlay_run(ov.h, sbuf.ptr, None, None, None, None, None, TRK, 1, 1, None))
    assert ei.value.code == INVALID
    ov.close(); sbuf.free()


@pytest.mark.parametrize("w", [1, 5, 64])
def test_widths(w):
    """Width 1 and 5: a 16-byte piece spans several rows; width 64: 192-byte rows, every row 16-byte aligned, two whole coverage words."""
    h = 23
    src = noise(2, h, w, 4)
    s = Scene(2)
    s.dets[0] = [(0, 2, w - 1, 9, 0), (w // 2, 12, w // 2 + 3, 20, 1)]
    s.trks[0] = [(0.0, 5.0, float(w), 9.5, 1), (w / 2.0, 14.0, 4.0, 6.0, 2)]
    s.dist[0] = [(0, 11)]
    s.dets[1] = [(-3, -3, w + 2, h + 2, 2), (w - 2, 1, w - 1, 4, 3)]
    s.trks[1] = [(-2.0, 10.0, w + 4.0, 8.0, 0)]
    want = s.want(src, 4 | DET | TRK)
    for offset in (16, 3):
        got = run(s, src, 4 | DET | TRK, offset=offset)
        assert np.array_equal(got, want), (w, offset)


def test_empty_lists_full_lists_and_the_area_gate():
    """Frame 0: no boxes at all -- a copy.  Frame 1: counts equal to the capacities.  Frame 2: tracks under, at and over min_box_area (the
    product is taken before the truncation), one whose clamped region is empty, and one with a NaN."""
    src = noise(3, H, W, 5)
    s = Scene(3, det_cap=6, trk_cap=5)
    rng = np.random.default_rng(6)
    s.dets[1] = [(int(x), int(y), int(x + dx), int(y + dy), int(c)) for x, y, dx, dy, c in
                 zip(rng.integers(-5, W, 6), rng.integers(-5, H, 6), rng.integers(0, 30, 6), rng.integers(0, 20, 6), rng.integers(0, 5, 6))]
    s.trks[1] = [(float(x), float(y), float(dx), float(dy), int(c)) for x, y, dx, dy, c in
                 zip(rng.uniform(-5, W, 5), rng.uniform(-5, H, 5), rng.uniform(2, 30, 5), rng.uniform(2, 20, 5), rng.integers(0, 3, 5))]
    s.trks[2] = [(5.0, 5.0, 3.3, 3.0, 0), (15.0, 5.0, 2.0, 5.0, 1), (25.0, 5.0, 3.4, 3.0, 2), (-30.0, 20.0, 29.5, 12.0, 0), (40.0, 20.0, float("nan"), 5.0, 1)]
    want = s.want(src, DET | TRK)
    got = run(s, src, DET | TRK)
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], src[0])
    assert np.array_equal(got[2, 4:10, 4:10], src[2, 4:10, 4:10]) and np.array_equal(got[2, 4:11, 14:18], src[2, 4:11, 14:18])   # 9.9 and 10.0 fail
    assert (got[2, 5:8, 25:28] != src[2, 5:8, 25:28]).any()                                                                    # 10.2 passes
    assert np.array_equal(got[2, 15:40, 35:], src[2, 15:40, 35:])                                                              # the NaN draws nothing
    assert (got[2, 19:33, 0] != src[2, 19:33, 0]).any() and np.array_equal(got[2, 19:33, 2:12], src[2, 19:33, 2:12])           # outline only: no tint


def test_second_run_starts_clean_and_style_changes_between_runs():
    """One handle: a full scene, then fewer boxes (the first run's coverage and records are gone), then other colours, thicknesses and gate."""
    src = noise(3, H, W, 7)
    ov = make_overlay(3)
    s = three_frames()
    assert np.array_equal(run(s, src, 7 | DET | TRK, own=True, ov=ov), s.want(src, 7 | DET | TRK))
    few = Scene(3)
    few.dets[1], few.trks[2] = [(30, 10, 55, 30, 1)], [(5.0, 5.0, 20.0, 20.0, 0)]
    assert np.array_equal(run(few, src, DET | TRK, own=True, ov=ov), few.want(src, DET | TRK))
    none = Scene(3)
    assert np.array_equal(run(none, src, DET | TRK, own=True, ov=ov), src)
    ov.set_class_colors("detections", DET_TABLE[::-1])
    ov.set_class_colors("tracks", [])                                                   # no table: every track is unknown, black
    ov.set_object_style(det_rect_thickness=2, det_arm_thickness=3, track_thickness=5, min_box_area=120.0)
    s2 = three_frames()
    want = s2.want(src, 7 | DET | TRK, det_table=DET_TABLE[::-1], trk_table=None, thickness=(2, 3, 5), min_box_area=120.0)
    assert np.array_equal(run(s2, src, 7 | DET | TRK, own=True, ov=ov), want)
    ov.set_object_style(det_rect_thickness=1, det_arm_thickness=1, track_thickness=1, min_box_area=10.0)     # thin everywhere: D3 lines
    s3 = three_frames()
    assert np.array_equal(run(s3, src, DET | TRK, own=True, ov=ov), s3.want(src, DET | TRK, det_table=DET_TABLE[::-1], trk_table=None, thickness=(1, 1, 1)))
    with pytest.raises(RuntimeError, match="thicknesses") as ei:
        ov.set_object_style(track_thickness=128)
    assert ei.value.code == INVALID
    with pytest.raises(RuntimeError, match="which") as ei:
        L.check(L.lib().adas_overlay_set_class_colors(ov.h, 1, None, 0))
    assert ei.value.code == INVALID
    ov.close()


def test_a_list_longer_than_the_staged_records():
    """500 detections and 40 tracks in one frame: more records than the streaming pass stages in LDS; the rest is walked from HBM, in order."""
    h, w = 40, 96
    src = noise(1, h, w, 8)
    rng = np.random.default_rng(9)
    s = Scene(1, det_cap=500, trk_cap=40)
    s.dets[0] = [(int(x), int(y), int(x + dx), int(y + dy), int(c)) for x, y, dx, dy, c in
                 zip(rng.integers(-4, w, 500), rng.integers(-4, h, 500), rng.integers(0, 9, 500), rng.integers(0, 7, 500), rng.integers(0, 6, 500))]
    s.trks[0] = [(float(x), float(y), float(dx), float(dy), int(c)) for x, y, dx, dy, c in
                 zip(rng.uniform(-4, w, 40), rng.uniform(-4, h, 40), rng.uniform(2, 12, 40), rng.uniform(2, 9, 40), rng.integers(0, 4, 40))]
    want = s.want(src, DET | TRK)
    assert np.array_equal(run(s, src, DET | TRK), want)


def test_all_six_entry_points_are_masks_over_one_path():
    """LaneOverlay goes through the widest entry of each family, so the six are called here as the C ABI has them: the array entries draw
    overlay_ref.compose at stages 7 and, where they take boxes, overlay_objects_ref.compose at 7 | 16 | 32; the handle entries draw a
    decoder's uploaded lanes at stage 1; each refuses the first bit outside its own mask."""
    lib, src, s = L.lib(), noise(3, H, W, 21), three_frames()
    kw = s.upload()
    sbuf = L.DeviceBuffer.from_array(src)
    ov = make_overlay(3)
    dec = PP.UfldDecode(100, 36, 50, 41, W, H, np.linspace(0.4, 1.0, 36), np.linspace(0.0, 1.0, 41), 1, 3)
    for f in range(3):
        dec.upload(s.lanes[f], [True] * 4, f)
    lane = (kw["lane_points"], kw["lane_counts"], kw["poly"], kw["poly_cap"], kw["poly_counts"], kw["area_status"], None, None, kw["dist_points"],
            kw["dist_cap"], kw["dist_counts"], None, None, None)
    boxes = tuple(kw[k] for k in ("det_xyxy", "det_cap", "det_cls", "det_counts", "trk_tlwh", "trk_cap", "trk_cls", "trk_counts"))

    def struct(dst, st):
        return C.byref(L.OverlayArrays(d_src_bgr=sbuf.ptr, d_dst_bgr=dst, stages=st, n_frames=3, **{
            k if k.endswith("_cap") else "d_" + k: v for k, v in kw.items()}))

    arrays = {"adas_overlay_run_arrays": (15, lambda dst, st: lib.adas_overlay_run_arrays(ov.h, sbuf.ptr, dst, *lane, st, 3, None)),
              "adas_overlay_run_arrays_objects": (63, lambda dst, st: lib.adas_overlay_run_arrays_objects(ov.h, sbuf.ptr, dst, *lane, *boxes, st, 3, None)),
              "adas_overlay_run_arrays_trajectories": (63 | 128, lambda dst, st: lib.adas_overlay_run_arrays_trajectories(ov.h, struct(dst, st)))}
    handles = {"adas_overlay_run": (15, lambda dst, st: lib.adas_overlay_run(ov.h, sbuf.ptr, dst, dec.h, None, None, None, st, 3, 1, None)),
               "adas_overlay_run_objects": (63, lambda dst, st: lib.adas_overlay_run_objects(ov.h, sbuf.ptr, dst, dec.h, None, None, None, None, None, st, 3,
                                                                                            1, None)),
               "adas_overlay_run_trajectories": (63 | 128, lambda dst, st: lib.adas_overlay_run_trajectories(ov.h, sbuf.ptr, dst, dec.h, None, None, None, None,
                                                                                                          None, st, 3, 1, None))}

    def draw(call, st):                                                                  # into a fresh destination: a run that did nothing would show
        dbuf = L.DeviceBuffer.from_array(np.full(src.nbytes, 0xA5, np.uint8))
        L.check(call(dbuf.ptr, st))
        L.check(lib.adas_synchronize())
        got = dbuf.download((src.nbytes,), np.uint8).reshape(src.shape)
        dbuf.free()
        return got

    plain = np.stack([ref.compose(src[f], s.lanes[f], s.poly[f], True, s.dist[f], ref.OFFSET_UNKNOWN, ref.AREA_COLOR, 7)[0] for f in range(3)])
    lanes = np.stack([ref.draw_lanes(src[f], s.lanes[f]) for f in range(3)])
    assert (plain != src).any() and (lanes != src).any() and (s.want(src, 7 | DET | TRK) != plain).any()
    for name, (mask, call) in arrays.items():
        assert np.array_equal(draw(call, 7), plain), name
        if mask & DET:
            assert np.array_equal(draw(call, 7 | DET | TRK), s.want(src, 7 | DET | TRK)), name
    for name, (mask, call) in handles.items():
        assert np.array_equal(draw(call, 1), lanes), name
    for name, (mask, call) in list(arrays.items()) + list(handles.items()):
        outside = next(b for b in (16, 32, 64, 128) if not mask & b)
        with pytest.raises(RuntimeError, match=name + ": unknown stage bits") as ei:
            L.check(call(None, 1 | outside))
        assert ei.value.code == INVALID
    ov.close(); dec.close(); s.free(); sbuf.free()


# ------------------------------------------------------------------------------------------------ the handles
def test_run_objects_from_a_real_post_and_a_real_tracker():
    """adas_overlay_run_objects reads a yolo_post handle's survivors (an injected head tensor, the SURVEY 8c recipe at a few candidates, on
    45 x 70 frames) and a bytetrack handle's live table after two updates; the restatement is fed from adas_yolo_post_fetch_dets and
    adas_bytetrack_fetch."""
    S = 3
    lb = PP.letterbox((H, W), (640, 640))
    yp = PP.YoloPost(L.HEAD_V8, 8400, 80, 0.4, 0.45, lb, L.NMS_REFERENCE, 64, S)
    trk = PP.DeviceTracker(S, max_tracks=64, max_dets=64)
    rng = np.random.default_rng(10)
    det_table = rng.integers(0, 256, (80, 3)).tolist()
    trk_table = rng.integers(0, 256, (40, 3)).tolist()                                  # classes 40 .. 79 have no colour: black
    base = [synth.synth_v8_head(500 + s, 14, 4) for s in range(S)]
    for f in range(2):
        heads = np.stack([b.copy() for b in base])
        heads[:, 0] += 6.0 * f
        buf = L.DeviceBuffer.from_array(heads)
        yp.run_device(buf.ptr, S)
        trk.update_device(yp.device_views(), det_stride=64, n_streams=S)
        L.check(L.lib().adas_synchronize())
        buf.free()
    src = noise(S, H, W, 11)
    sbuf = L.DeviceBuffer.from_array(src)
    ov = make_overlay(S, det_table=det_table, trk_table=trk_table)
    n_boxes = 0
    for stages in (DET, TRK, DET | TRK):
        ov.run(sbuf.ptr, post=yp, tracker=trk, stages=stages, n_streams=S, n_frames=1)
        for s in range(S):
            r = yp.fetch_dets(s)
            hdr, tracked, _ = trk.fetch(s)
            act = [t for t in tracked if t["is_activated"]]
            want, _ = oref.compose(src[s], stages=stages, dets=r["xyxy_int"], det_cls=r["class_id"], det_table=det_table,
                                   trks=[t["tlwh"] for t in act], trk_cls=[int(t["class_id"]) for t in act], trk_table=trk_table)
            assert np.array_equal(ov.fetch(s), want), (stages, s)
            n_boxes += len(r["xyxy_int"]) + len(act)
            assert len(r["xyxy_int"]) >= 5 and len(act) >= 3
        via_run = [ov.fetch(s) for s in range(S)]                                         # LaneOverlay.run goes through the widest entry:
        L.check(L.lib().adas_overlay_run_objects(ov.h, sbuf.ptr, None, None, None, None, yp.h, trk.h, None, stages, S, 1, None))
        assert all(np.array_equal(ov.fetch(s), via_run[s]) for s in range(S)), stages     # the entry the docstring names draws the same bytes
    print("boxes drawn:", n_boxes)
    with pytest.raises(RuntimeError, match="yolo_post handle") as ei:                    # the refusals, by name
        ov.run(sbuf.ptr, tracker=trk, stages=DET | TRK, n_streams=S)
    assert ei.value.code == INVALID
    with pytest.raises(RuntimeError, match="bytetrack handle") as ei:
        ov.run(sbuf.ptr, post=yp, stages=DET | TRK, n_streams=S)
    assert ei.value.code == INVALID
    with pytest.raises(RuntimeError, match="n_frames must be 1") as ei:
        ov.run(sbuf.ptr, post=yp, tracker=trk, stages=TRK, n_streams=1, n_frames=2)
    assert ei.value.code == INVALID
    with pytest.raises(RuntimeError, match="boxes, classes and counts") as ei:
        ov.run_arrays(sbuf.ptr, 1, stages=DET)
    assert ei.value.code == INVALID
    for o in (ov, yp, trk):
        o.close()
    sbuf.free()


def test_a_tracked_row_that_is_not_activated_is_not_drawn():
    """A track born after the first frame sits in tracked_stracks with is_activated False until it is matched again (byteTracker.py:161-168):
    the device reads the flag from the live table and draws nothing for that row."""
    trk = PP.DeviceTracker(1, max_tracks=16, max_dets=16)
    old = np.array([[5.0, 5.0, 30.0, 25.0], [40.0, 12.0, 65.0, 40.0]])
    trk.update_host(0, old, [0.9, 0.8], [0, 1])
    trk.update_host(0, np.concatenate([old, [[20.0, 28.0, 38.0, 42.0]]]), [0.9, 0.8, 0.95], [0, 1, 2])
    _, tracked, _ = trk.fetch(0)
    flags = [int(t["is_activated"]) for t in tracked]
    assert len(tracked) == 3 and sorted(flags) == [0, 1, 1]
    act = [t for t in tracked if t["is_activated"]]
    src = noise(1, H, W, 14)
    sbuf = L.DeviceBuffer.from_array(src)
    ov = make_overlay(1)
    ov.run(sbuf.ptr, tracker=trk, stages=TRK)
    want = oref.draw_tracks(src[0], [t["tlwh"] for t in act], [int(t["class_id"]) for t in act], TRK_TABLE)
    assert np.array_equal(ov.fetch(0), want)
    assert np.array_equal(want[30:41, 22:37], src[0, 30:41, 22:37])                      # inside the newborn's box: untouched
    trk.update_host(0, np.concatenate([old, [[20.0, 28.0, 38.0, 42.0]]]), [0.9, 0.8, 0.95], [0, 1, 2])     # matched again: activated, drawn
    _, tracked, _ = trk.fetch(0)
    assert all(int(t["is_activated"]) for t in tracked) and len(tracked) == 3
    ov.run(sbuf.ptr, tracker=trk, stages=TRK)
    again = oref.draw_tracks(src[0], [t["tlwh"] for t in tracked], [int(t["class_id"]) for t in tracked], TRK_TABLE)
    assert np.array_equal(ov.fetch(0), again) and (again[30:41, 22:37] != src[0, 30:41, 22:37]).any()
    for o in (ov, trk):
        o.close()
    sbuf.free()


# ------------------------------------------------------------------------------------------------ the fused step
SRC = (180, 320)    # camera frames of the fused step here
LANE_KW = dict(in_h=160, in_w=800, num_grid_row=100, num_cls_row=36, num_grid_col=50, num_cls_col=41)      # the reduced lane net of
LANE_CFG = dict(grid_row=100, cls_row=36, grid_col=50, cls_col=41, row_anchor=np.linspace(0.42, 1, 36),     # test_gpu_pipeline.py
                col_anchor=np.linspace(0, 1, 41))
MAXC = 256
BOX_SCORE = 0.1


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    import bench
    import netutil
    from test_gpu_overlay import PrescribedLanes
    d = tmp_path_factory.mktemp("ovobj")
    lane = str(d / "lanes.hipm")
    M.build("ufldv2_res18", wsrc=PrescribedLanes(0), **LANE_KW).save(lane)
    seam = np.concatenate([netutil.coco_like_frames(2, seed=60 + i) for i in range(2)])
    det, _, _ = bench.build_detector(M, CE, "yolov8n", seam, str(d), "a", target_per_frame=25.0, capacity=MAXC)
    cam = [bench.cam_frames(2, 400 + i, SRC[0], SRC[1]) for i in range(2)]
    return det, lane, cam


def pipeline_kw():
    Mh = A.PerspectiveTransformation((SRC[1], SRC[0])).M
    car = A.SingleCamDistanceMeasure.RefSizeDict["car"][0]
    return dict(n_streams=2, precision="bf16", src_hw=SRC, lane_cfg=LANE_CFG, track=True, box_score=BOX_SCORE, max_candidates=MAXC,
                geometry=dict(bird_wh=(SRC[1], SRC[0]), M=Mh), analysis=dict(ref_height=[car] * 80))


def restate(p, frame, s, stages, det_table, trk_table):
    lanes, _ = p.decode.fetch(s)
    geo = p.geometry.fetch(s)
    fr = p.analysis.fetch_frame(s)
    pts = [(x, y) for x, y, _ in p.analysis.fetch_points(s)]
    colour = ref.COLLISION_COLORS[{"UNKNOWN": 0, "NORMAL": 1, "PROMPT": 2, "WARNING": 3}[fr["collision_msg"].name]]
    off = {"UNKNOWN": ref.OFFSET_UNKNOWN, "RIGHT": ref.OFFSET_RIGHT, "LEFT": ref.OFFSET_LEFT, "CENTER": ref.OFFSET_CENTER}[fr["offset_msg"].name]
    r = p.post.fetch_dets(s)
    _, tracked, _ = p.tracker.fetch(s)
    act = [t for t in tracked if t["is_activated"]]
    want, flags = oref.compose(frame, lanes, geo["area_points"], geo["area_status"], pts, off, colour, stages, dets=r["xyxy_int"], det_cls=r["class_id"],
                               det_table=det_table, trks=[t["tlwh"] for t in act], trk_cls=[int(t["class_id"]) for t in act], trk_table=trk_table)
    assert flags == 0
    return want, len(r["xyxy_int"]), len(act)


def test_pipeline_graph_eager_and_restatement(models):
    """The fused step with the two new stages on: graph and eager give the same frame_show, both equal the restatement applied to what the
    pipeline fetches (lanes, polygon, analysis row, distance points, survivors, tracked tracks after this step's update).  A third pipeline
    without the new stages gives the image the restatement gives without them."""
    det_model, lane_model, cam = models
    rng = np.random.default_rng(12)
    det_table, trk_table = rng.integers(0, 256, (80, 3)).tolist(), rng.integers(0, 256, (80, 3)).tolist()
    names = ("lanes", "area", "distance", "detections", "tracks")
    ovl = dict(stages=names, detection_colors=det_table, track_colors=trk_table)
    pg = PL.AdasPipeline(det_model, lane_model, use_graph=True, overlay=ovl, **pipeline_kw())
    pe = PL.AdasPipeline(det_model, lane_model, use_graph=False, overlay=ovl, **pipeline_kw())
    po = PL.AdasPipeline(det_model, lane_model, use_graph=True, overlay=dict(), **pipeline_kw())          # the default stage set: no boxes
    dev = [L.DeviceBuffer.from_array(c) for c in cam]
    nd = nt = 0
    for k in range(4):
        for p in (pg, pe, po):
            p.step_frames(dev[k % 2].ptr, SRC, 0.6)
            p.sync()
        for s in range(2):
            want, a, b = restate(pg, cam[k % 2][s], s, 7 | DET | TRK, det_table, trk_table)
            nd, nt = nd + a, nt + b
            ig, ie = pg.overlay_image(s), pe.overlay_image(s)
            assert np.array_equal(ig, ie), (k, s)
            assert np.array_equal(ig, want), (k, s, np.argwhere(ig != want)[:5])
            plain, _, _ = restate(po, cam[k % 2][s], s, 7, None, None)
            assert np.array_equal(po.overlay_image(s), plain), (k, s)
            assert np.array_equal(dev[k % 2].download(cam[k % 2].shape, np.uint8), cam[k % 2])
    print("survivors drawn", nd, "tracks drawn", nt)
    assert nd > 0 and nt > 0
    for o in (pg, pe, po):
        o.close()
    for b in dev:
        b.free()


def test_pipeline_refusals(models):
    det_model, lane_model, cam = models
    kw = pipeline_kw()
    with pytest.raises(ValueError, match="micro_batch"):
        PL.AdasPipeline(det_model, lane_model, micro_batch=2, overlay=dict(stages=("lanes", "tracks")), **kw)
    with pytest.raises(ValueError, match="track=True"):
        PL.AdasPipeline(det_model, lane_model, overlay=dict(stages=("tracks",)), **dict(kw, track=False))
    with pytest.raises(ValueError, match="det_model"):
        PL.AdasPipeline(None, lane_model, overlay=dict(stages=("detections",)), **dict(kw, analysis=None))
    d = L.DeviceBuffer.from_array(np.concatenate([cam[0], cam[1]]))
    kw2 = dict(kw, analysis=None)
    p = PL.AdasPipeline(det_model, lane_model, micro_batch=2, overlay=dict(stages=("lanes", "detections")), **kw2)   # detections: any micro_batch
    p.step_frames(d.ptr, SRC, 0.6)
    p.sync()
    frames4 = np.concatenate([cam[0], cam[1]])
    n_drawn = 0
    for f in range(4):                                                                                         # frame b of stream s: b * 2 + s
        lanes, _ = p.decode.fetch(f)
        r = p.post.fetch_dets(f)
        want, flags = oref.compose(frames4[f], lanes, stages=1 | DET, dets=r["xyxy_int"], det_cls=r["class_id"], det_table=None)
        assert flags == 0 and np.array_equal(p.overlay_image(f), want), f
        n_drawn += len(r["xyxy_int"])
    assert n_drawn > 0
    L.check(L.lib().adas_pipeline_set_overlay_stages(p.h, 1 | TRK))                                            # refused at the step, by name
    with pytest.raises(RuntimeError, match="micro_batch <= 1") as ei:
        p.step_frames(d.ptr, SRC, 0.6)
    assert ei.value.code == INVALID
    with pytest.raises(RuntimeError, match="unknown stage bits") as ei:
        L.check(L.lib().adas_pipeline_set_overlay_stages(p.h, 64))
    assert ei.value.code == INVALID
    p.close()
    q = PL.AdasPipeline(det_model, lane_model, overlay=dict(stages=("lanes",)), **dict(kw2, track=False))
    L.check(L.lib().adas_pipeline_set_overlay_stages(q.h, 1 | TRK))
    with pytest.raises(RuntimeError, match="needs a tracker") as ei:
        q.step_frames(d.ptr, SRC, 0.6)
    assert ei.value.code == INVALID
    q.close()
    d.free()


# ------------------------------------------------------------------------------------------------ the drop-in methods
def test_drop_in_methods(models, tmp_path):
    det_model, _, _ = models
    img = noise(1, H, W, 13)[0]
    names = tmp_path / "labels.txt"
    names.write_text("\n".join("class%d" % i for i in range(80)) + "\n")
    yd = D.YoloDetector(model_path=det_model, model_type=D.ObjectModelType.YOLOV8, classes_path=str(names), precision="bf16")
    assert sorted(yd.colors_dict) == sorted(yd.class_names) and all(len(c) == 3 and all(0 <= v <= 255 for v in c) for c in yd.colors_dict.values())
    boxes = [(10.2, 10.9, 30.5, 20.1, "class3"), (20.0, 15.0, 30.0, 20.0, "class7"), (-4.5, 30.0, 12.0, 20.0, "unknown"), (60.0, 5.0, 3.0, 30.0, "class3")]
    yd._object_info = [D.RectInfo(np.float64(x), np.float64(y), np.float64(w), np.float64(h), conf=0.9, label=lab, kpss=[]) for x, y, w, h, lab in boxes]
    cols = [yd.colors_dict[lab] if lab != "unknown" else (0, 0, 0) for *_, lab in boxes]
    xyxy = [info.tolist() for info in yd._object_info]
    want = oref.draw_detections(img, xyxy, range(4), cols)
    a = img.copy()
    yd.DrawDetectedOnFrame(a)
    assert np.array_equal(a, want) and (a != img).any()
    dbuf = L.DeviceBuffer.from_array(img)                                               # a StagedFrame is drawn where it sits
    yd.DrawDetectedOnFrame(D.StagedFrame(dbuf.ptr, H, W, 0))
    assert np.array_equal(dbuf.download(img.shape, np.uint8), want)
    yd._object_info = []
    b = img.copy()
    yd.DrawDetectedOnFrame(b)
    assert np.array_equal(b, img)
    assert D.EfficientdetDetector.DrawDetectedOnFrame is D.YoloDetector.DrawDetectedOnFrame

    class Graph:                                                                        # the EngineBase surface EfficientdetDetector(engine=) takes
        engine_dtype = np.float32

        def get_engine_input_shape(self):
            return (1, 3, 512, 512)

        def get_engine_output_shape(self):
            return [(1, 100, 4), (1, 100), (1, 100)], ["boxes", "ids", "scores"]

    ed = D.EfficientdetDetector(engine=Graph(), classes_path=str(names))
    assert sorted(ed.colors_dict) == sorted(ed.class_names)
    ed._object_info = [D.RectInfo(np.float32(x), np.float32(y), np.float32(w), np.float32(h), conf=np.float32(0.9), label=lab) for x, y, w, h, lab in boxes]
    ecols = [ed.colors_dict[lab] if lab != "unknown" else (0, 0, 0) for *_, lab in boxes]
    f = img.copy()
    ed.DrawDetectedOnFrame(f)
    assert np.array_equal(f, oref.draw_detections(img, [info.tolist() for info in ed._object_info], range(4), ecols)) and (f != img).any()
    ed.close()
    yd.close()
    colours = {"car": (10, 200, 250), "person": (250, 10, 120)}
    bt = D.BYTETracker(names=colours)
    assert bt.class_colors is colours and bt.names == {"car": "car", "person": "person"}
    dets = np.array([[5.0, 5.0, 30.0, 25.0], [20.0, 12.0, 55.0, 40.0], [40.0, 2.0, 44.0, 4.0]])
    for _ in range(2):
        bt.update(dets, [0.9, 0.8, 0.95], ["car", "person", "bus"])
    online = [t for t in bt.tracked_stracks if t["is_activated"]]
    assert len(online) == 3
    tcols = [colours.get(t["class_id"], (0, 0, 0)) for t in online]
    want = oref.draw_tracks(img, [t["tlwh"] for t in online], range(len(online)), tcols)
    c = img.copy()
    bt.DrawTrackedOnFrame(c)
    assert np.array_equal(c, want) and (c != img).any()
    dbuf.upload(img)
    bt.DrawTrackedOnFrame(D.StagedFrame(dbuf.ptr, H, W, 0), show_traject=False)
    assert np.array_equal(dbuf.download(img.shape, np.uint8), want)
    e = img.copy()
    bt.DrawTrackedOnFrame(e, show_box=False)
    assert np.array_equal(e, img)
    listed = D.BYTETracker(names=["car", "person"])
    assert len(listed.class_colors) == 2 and all(len(c) == 3 for c in listed.class_colors)
    listed.close(); bt.close(); dbuf.free()
