"""GPU: the overlay's trajectories stage (plot_trajectories' circles, plot_directions' lock-on rectangle or shadowed arrow:
csrc/overlay_kernels.hip, rules D10-D12 of overlay_track_core.h) through the C ABI, postproc.LaneOverlay, a real DeviceTracker fed the
golden's detections, the fused step and the drop-in DrawTrackedOnFrame, against the NumPy restatement (tests/overlay_tracks_ref.py),
every byte and every record, and against the calls the reference's own DrawTrackedOnFrame made (tests/golden/track_draw.json.gz)."""
import gzip, importlib, json, os

import numpy as np
import pytest

from conftest import load_pkg
import overlay_ref as ref
import overlay_objects_ref as oref
import overlay_tracks_ref as tref
import overlay_scene as OS
from overlay_scene import noise

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")
CE = importlib.import_module("adas_amd.coreEngine")
PP = importlib.import_module("adas_amd.postproc")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")
A = importlib.import_module("adas_amd.analysis")
D = importlib.import_module("adas_amd.detectors")

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID = -1        # ADAS_ERR_INVALID
H, W = 45, 70       # three coverage words per row, six bands of eight rows
DET, TRK, TRAJ = oref.DETECTIONS, oref.TRACKS, tref.TRAJECTORIES
POLY = [(10, 5), (8, 12), (8, 12), (3, 20), (2, 30), (40, 30), (35, 21), (30, 12), (28, 5)]
DET_TABLE = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (200, 100, 50), (17, 34, 51)]
TRK_TABLE = [(10, 200, 250), (250, 10, 120), (90, 5, 10)]


def path(x, y, w, h, vx, vy, n):
    """n boxes (tlbr) of a w x h rectangle that starts at (x, y) and moves by (vx, vy) a box."""
    return [[x + vx * i, y + vy * i, x + vx * i + w, y + vy * i + h] for i in range(n)]


class Scene(OS.Scene):
    """Per-frame geometry, boxes and trajectories of a batch."""

    def __init__(self, n, det_cap=6, trk_cap=8, dist_cap=8, poly_cap=16):
        super().__init__(n, ("boxes", "trajectories"), det_cap, trk_cap, dist_cap, poly_cap)

    def want(self, src, stages, det_table=DET_TABLE, trk_table=TRK_TABLE, **kw):
        """(frames, flags per frame, marks per frame)"""
        out, flags, marks = [], [], []
        for f in range(self.n):
            d, t = np.asarray(self.dets[f], np.int64).reshape(-1, 5), np.asarray(self.trks[f], np.float64).reshape(-1, 5)
            o, fl, mk = tref.compose(src[f], self.lanes[f], self.poly[f], True, self.dist[f], stages=stages, dets=d[:, :4], det_cls=d[:, 4],
                                     det_table=det_table, trks=t[:, :4], trk_cls=t[:, 4].astype(np.int64), trk_table=trk_table,
                                     trajectories=self.trajs[f], **kw)
            out.append(o); flags.append(fl); marks.append(mk)
        return np.stack(out), flags, marks


def make_overlay(n, h=H, w=W, det_table=DET_TABLE, trk_table=TRK_TABLE, **style):
    return OS.make_overlay(n, h, w, None, det_table, trk_table, **style)


def run(scene, src, stages, det_table=DET_TABLE, trk_table=TRK_TABLE, **kw):
    """OS.run with this file's class colours -> (frames, flags, marks)"""
    return OS.run(scene, src, stages, det_table=det_table, trk_table=trk_table, **kw)[:3]


def check(scene, src, stages, **kw):
    want, wflags, wmarks = scene.want(src, stages)
    got, flags, marks = run(scene, src, stages, **kw)
    for f in range(scene.n):
        assert np.array_equal(got[f], want[f]), (stages, f, np.argwhere(got[f] != want[f])[:5])
        assert flags[f] == wflags[f], (stages, f)
        if stages & TRAJ:
            assert tref.device_marks_table(marks[f]) == tref.marks_table(wmarks[f]), (stages, f)
    return want, wmarks


def three_frames():
    """Frame 0: an arrow that leaves the image through the bottom right (over columns 31 / 32 and 63 / 64 and every band boundary), one that
    leaves it through the top left with negative end coordinates, a lock-on rectangle that hangs over the top left corner, circles on
    boxes that lie beyond every edge.  Frame 1: over lane discs, a polygon and distance discs -- two tracks whose circles cross, a third
    whose box (tint with TRACKS) covers the first one's circles, a distance disc on a circle.  Frame 2: the same tracks in the other order, a
    class outside the table, a track that fails the area gate, rings of length 0, 1, 2."""
    s = Scene(3)
    s.trks[0] = [(20.0, 12.0, 30.0, 22.0, 0), (30.0, 20.0, 24.0, 18.0, 1), (-8.0, -6.0, 30.0, 24.0, 2), (50.0, 30.0, 30.0, 30.0, 0)]
    s.trajs[0] = [path(10, 10, 8, 8, 5.0, 2.5, 8), path(50, 26, 8, 8, -5.5, -2.25, 8), path(12, 12, 9, 7, 3.0, 1.0, 3),
                  path(-12, -14, 10, 8, 9.0, 7.0, 12)]
    s.dets[0] = [(25, 5, 60, 40, 1), (-6, -4, 20, 15, 0)]
    s.lanes[1] = [[(20, 18), (40, 30)], [(22, 18)], [(21, 19)], [(21, 18), (60, 40)]]
    s.poly[1] = POLY
    s.dist[1] = [(33, 24), (5, 5), (69, 44)]
    s.trks[1] = [(24.0, 14.0, 20.0, 16.0, 0), (26.0, 12.0, 18.0, 20.0, 1), (18.0, 10.0, 34.0, 24.0, 2)]
    s.trajs[1] = [path(14, 12, 10, 10, 2.5, 1.5, 9), path(40, 11, 10, 12, -2.5, 1.25, 9), path(11, 11, 12, 9, 1.0, 0.5, 4)]
    s.dets[1] = [(22, 10, 50, 36, 2), (30, 16, 44, 30, 3)]
    s.poly[2] = POLY
    s.dist[2] = [(30, 22)]
    s.trks[2] = [s.trks[1][2], s.trks[1][1], s.trks[1][0][:4] + (7,), (10.0, 30.0, 3.0, 3.0, 0), (40.0, 5.0, 9.0, 9.0, 1), (50.0, 5.0, 9.0, 9.0, 1),
                 (60.0, 5.0, 9.0, 9.0, 2)]
    s.trajs[2] = [s.trajs[1][2], s.trajs[1][1], s.trajs[1][0], path(10, 30, 3, 3, 1.0, 0.0, 10), [], path(50, 5, 9, 9, 0, 0, 1), path(58, 14, 9, 9, 1.0, 1.0, 2)]
    return s


@pytest.mark.parametrize("mode", ["offset16", "offset3", "own", "in_place"])
@pytest.mark.parametrize("stages", [TRAJ, TRK | TRAJ, DET | TRK | TRAJ, 7 | TRAJ, 7 | DET | TRK | TRAJ])
def test_three_frames_every_byte(mode, stages):
    s = three_frames()
    src = noise(3, H, W, 3)
    kw = dict(offset16=dict(offset=16), offset3=dict(offset=3), own=dict(own=True), in_place=dict(offset=16, in_place=True))[mode]
    want, marks = check(s, src, stages, **kw)
    if mode == "own" and stages == 7 | DET | TRK | TRAJ:                                  # the scenes do what their docstring says
        kinds = [[m["kind"] for m in mk] for mk in marks]
        assert kinds[0].count(tref.ARROW) == 6 and kinds[0].count(tref.RECT) == 2 and kinds[0].count(tref.CIRCLE) == 8 + 8 + 3 + 12
        arrows = [m for m in marks[0] if m["kind"] == tref.ARROW]
        assert max(m["x2"] for m in arrows) >= W and max(m["y2"] for m in arrows) >= H and min(m["x2"] for m in arrows) < 0 and min(m["y2"] for m in arrows) < 0
        assert any(m["x1"] < 0 and m["y1"] < 0 for m in marks[0] if m["kind"] == tref.RECT)
        only, _, _ = s.want(src, TRAJ)
        plain = src
        changed = (only[0] != plain[0]).any(axis=2)
        assert changed[:, 31].any() and changed[:, 32].any() and changed[:, 63].any() and changed[:, 64].any()
        assert all(changed[r].any() for r in (7, 8, 15, 16, 23, 24, 31, 32, 39, 40)) and changed[0].any() and changed[H - 1].any()
        assert changed[:, 0].any() and changed[:, W - 1].any()
        both, _, _ = s.want(src, TRK | TRAJ)
        circ = (only[1] != plain[1]).any(axis=2)
        assert (both[1][circ] != only[1][circ]).any(), "a later track's tint lies on an earlier track's circles"
        dist_on, _, _ = s.want(src, 4 | TRAJ)
        assert ((dist_on[1] != only[1]).any(axis=2) & circ).any(), "a distance disc lies on a primitive"


def test_stage_off_is_the_image_without_it_and_the_old_entries_refuse_it():
    s = three_frames()
    src = noise(3, H, W, 4)
    ov = make_overlay(3)
    for stages in (7, 7 | DET | TRK):
        with_it, _, _ = run(s, src, stages | TRAJ, own=True, ov=ov)
        without, _, _ = run(s, src, stages, own=True, ov=ov)                               # the same handle, the stage off after on
        ow, _ = oref_compose_batch(s, src, stages)
        assert np.array_equal(without, ow) and (with_it != without).any()
    kw = s.upload()
    sbuf = L.DeviceBuffer.from_array(src)
    traj = kw.pop("trajectories")
    for call in (lambda: L.lib().adas_overlay_run_objects(ov.h, sbuf.ptr, None, None, None, None, None, None, None, TRK | TRAJ, 3, 1, None),
                 lambda: L.lib().adas_overlay_run(ov.h, sbuf.ptr, None, None, None, None, None, 1 | TRAJ, 3, 1, None),
                 lambda: L.lib().adas_overlay_run_arrays_objects(ov.h, sbuf.ptr, None, None, None, None, 0, None, None, None, None, None, 0, None, None, None,
                                                                 None, None, 0, None, None, kw["trk_tlwh"], kw["trk_cap"], kw["trk_cls"], kw["trk_counts"],
                                                                 TRK | TRAJ, 3, None)):
        with pytest.raises(RuntimeError, match="unknown stage bits") as ei:                # 128 is the new entries' only: the old ones keep their masks
            L.check(call())
        assert ei.value.code == INVALID
    with pytest.raises(RuntimeError, match="unknown stage bits") as ei:                    # and 64 is nobody's
        ov.run_arrays(sbuf.ptr, 3, stages=64 | TRAJ, trajectories=traj, **kw)
    assert ei.value.code == INVALID
    with pytest.raises(RuntimeError, match="trajectories stage needs") as ei:
        ov.run_arrays(sbuf.ptr, 3, stages=TRAJ, trajectories=(None, None), **kw)
    assert ei.value.code == INVALID
    with pytest.raises(RuntimeError, match="unknown stage bits") as ei:
        ov.run(sbuf.ptr, stages=64, n_streams=3)
    assert ei.value.code == INVALID
    assert PP.LaneOverlay.stage_mask(("tracks", "trajectories")) == TRK | TRAJ == 160
    s.free(); sbuf.free(); ov.close()


def oref_compose_batch(s, src, stages):
    out = []
    for f in range(s.n):
        d, t = np.asarray(s.dets[f], np.int64).reshape(-1, 5), np.asarray(s.trks[f], np.float64).reshape(-1, 5)
        o, fl = oref.compose(src[f], s.lanes[f], s.poly[f], True, s.dist[f], stages=stages, dets=d[:, :4], det_cls=d[:, 4], det_table=DET_TABLE,
                             trks=t[:, :4], trk_cls=t[:, 4].astype(np.int64), trk_table=TRK_TABLE)
        out.append(o)
    return np.stack(out), 0


@pytest.mark.parametrize("w", [1, 5, 64])
def test_widths(w):
    s = Scene(2)
    s.trks[0] = [(w / 2 - 4.0, 12.0, 8.0, 20.0, 0), (-2.0, 2.0, 6.0, 9.0, 1)]
    s.trajs[0] = [path(w / 2 - 3, 10, 2, 6, 0.25, 3.0, 9), path(-1, 12, 3, 5, 0.5, 2.0, 4)]
    s.trks[1] = [(0.0, 0.0, float(w), float(H), 2)]
    s.trajs[1] = [path(0, 10, min(w, 4), 4, 0.0, 2.5, 10)]
    src = noise(2, H, w, 5 + w)
    for stages in (TRAJ, TRK | TRAJ):
        check(s, src, stages, offset=5)


def test_record_lists_empty_full_and_short_rings():
    """No tracks at all; a full trk_cap of 70 rows (more than one workgroup of the primitive kernel) with 30-box rings, 33 primitives each;
    rings of length 0, 1 (nothing: circles need two boxes, a direction too), 2 (two circles and the n = 1 lock-on rectangle)."""
    rng = np.random.default_rng(6)
    s = Scene(3, trk_cap=70)
    for k in range(70):
        x, y = float(rng.uniform(0, 50)), float(rng.uniform(0, 25))
        s.trks[1].append((x, y, float(rng.uniform(4, 20)), float(rng.uniform(4, 20)), int(rng.integers(0, 3))))
        s.trajs[1].append(path(float(rng.uniform(10, 14)), float(rng.uniform(10, 13)), 6, 5, float(rng.uniform(0.5, 1.3)), float(rng.uniform(0.1, 0.5)), 30))
    s.trks[2] = [(10.0, 10.0, 12.0, 12.0, 0), (30.0, 10.0, 12.0, 12.0, 1), (50.0, 10.0, 12.0, 12.0, 2)]
    s.trajs[2] = [[], path(30, 10, 12, 12, 0, 0, 1), path(44, 12, 10, 10, 3.0, 2.0, 2)]
    src = noise(3, H, W, 7)
    for stages in (TRAJ, TRK | TRAJ):
        want, marks = check(s, src, stages, own=True)
        assert np.array_equal(want[0], src[0]) and marks[0] == []
        assert len(marks[1]) == 70 * 33 and [m["kind"] for m in marks[1][:33]] == [tref.CIRCLE] * 30 + [tref.ARROW] * 3
        assert [m["kind"] for m in marks[2]] == [tref.CIRCLE] * 2 + [tref.RECT]


def test_second_run_starts_clean_and_the_range_flag():
    """The planes are zero again and the flags reset: a run on an empty scene after a full one is the source; TRACK_RANGE is raised by a
    track whose centre lies beyond +-32767 (its arrows are skipped, its circles drawn) and gone on the next run."""
    src = noise(3, H, W, 8)
    ov = make_overlay(3)
    s = three_frames()
    far = three_frames()
    far.trks[0][0] = (40000.0, 12.0, 30.0, 22.0, 0)
    far.poly[0] = [(0, 0), (40000, 5), (20, 30)]                                           # and POLY_RANGE beside it
    want, wflags, wmarks = far.want(src, 7 | TRK | TRAJ)
    got, flags, marks = run(far, src, 7 | TRK | TRAJ, own=True, ov=ov)
    assert np.array_equal(got, want) and flags == wflags == [L.OVERLAY_TRACK_RANGE | L.OVERLAY_POLY_RANGE, 0, 0]
    assert tref.device_marks_table(marks[0]) == tref.marks_table(wmarks[0])
    assert [int(m["skipped"]) for m in marks[0] if m["kind"] == tref.ARROW and m["track"] == 0] == [7, 7, 7]
    want, wflags, _ = s.want(src, 7 | TRK | TRAJ)
    got, flags, _ = run(s, src, 7 | TRK | TRAJ, own=True, ov=ov)
    assert np.array_equal(got, want) and flags == wflags == [0, 0, 0]
    empty = Scene(3)
    got, flags, marks = run(empty, src, 7 | DET | TRK | TRAJ, own=True, ov=ov)
    assert np.array_equal(got, src) and flags == [0, 0, 0] and all(len(m) == 0 for m in marks)
    ov.close()


# ------------------------------------------------------------------------------------------------ a real tracker, the golden's detections
@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(HERE, "golden", "track_draw.json.gz"), "rt") as f:
        return json.load(f)


def golden_calls(fr):
    """DrawTrackedOnFrame(frame, False)'s recorded calls as mark tuples without the track row and the tips (the recording has neither)."""
    out = []
    for c in fr["calls_traject"]:
        if c[0] == "circle":
            out.append((tref.CIRCLE, c[1][0], c[1][1], c[1][0], c[1][1], c[2], c[4], tuple(c[3])))
        elif c[0] == "rectangle":
            out.append((tref.RECT, c[1][0], c[1][1], c[2][0], c[2][1], 0, c[4], tuple(max(0, v) for v in c[3])))
        elif c[0] == "arrowedLine":
            out.append((tref.ARROW, c[1][0], c[1][1], c[2][0], c[2][1], 0, c[4], tuple(c[3])))
    return out


def test_a_real_tracker_draws_the_reference_s_calls(golden):
    """A DeviceTracker is fed the golden's detections frame by frame and drawn after every update through adas_overlay_run_trajectories:
    the marks the device built from its own rings are the calls the reference's DrawTrackedOnFrame(frame, False) made, frame by frame
    (from the reference to the device, no host arithmetic in between); the image is the restatement's on what the tracker fetches."""
    gh, gw = golden["H"], golden["W"]
    table = [tuple(c) for _, c in golden["names"]]
    trk = PP.DeviceTracker(1, max_tracks=16, max_dets=16)
    ov = make_overlay(1, gh, gw, trk_table=table)
    src = noise(1, gh, gw, 9)
    sbuf = L.DeviceBuffer.from_array(src)
    n = dict(circle=0, rect=0, arrow=0)
    for k, fr in enumerate(golden["frames"]):
        trk.update_host(0, np.asarray(fr["boxes"], np.float64).reshape(-1, 4), fr["scores"], fr["ids"])
        stages = TRK | TRAJ if k % 6 == 5 else TRAJ
        ov.run(sbuf.ptr, tracker=trk, stages=stages)
        marks = ov.track_marks(0)
        got = [t[:1] + t[2:9] for t in tref.device_marks_table(marks)]
        assert got == golden_calls(fr), k
        for m in marks:
            n[{1: "circle", 2: "rect", 3: "arrow"}[int(m["kind"])]] += 1
        if k % 6 == 5 or k == len(golden["frames"]) - 1:
            _, tracked, _ = trk.fetch(0)
            trajs = trk.fetch_trajectories(0)
            act = [i for i, t in enumerate(tracked) if t["is_activated"]]
            want, flags, _ = tref.compose(src[0], stages=stages, trks=[tracked[i]["tlwh"] for i in act], trk_cls=[int(tracked[i]["class_id"]) for i in act],
                                          trk_table=table, trajectories=[trajs[i] for i in act])
            assert flags == 0 and np.array_equal(ov.fetch(0), want), k
    print("marks drawn:", n)
    assert n["circle"] > 1000 and n["rect"] >= 8 and n["arrow"] >= 30
    with pytest.raises(RuntimeError, match="trajectories stage needs a bytetrack handle") as ei:      # the refusals, by name
        ov.run(sbuf.ptr, stages=TRAJ)
    assert ei.value.code == INVALID
    two = make_overlay(2, gh, gw, trk_table=table)                                         # a handle that holds two frames: refused for the stage's sake
    with pytest.raises(RuntimeError, match="trajectories stage draws the tracker's live table.*n_frames must be 1") as ei:
        two.run(sbuf.ptr, tracker=trk, stages=TRAJ, n_streams=1, n_frames=2)
    assert ei.value.code == INVALID
    for o in (ov, two, trk):
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
    d = tmp_path_factory.mktemp("ovtrk")
    lane = str(d / "lanes.hipm")
    M.build("ufldv2_res18", wsrc=PrescribedLanes(0), **LANE_KW).save(lane)
    seam = np.concatenate([netutil.coco_like_frames(2, seed=60 + i) for i in range(2)])
    det, _, _ = bench.build_detector(M, CE, "yolov8n", seam, str(d), "a", target_per_frame=25.0, capacity=MAXC)
    cam = bench.cam_frames(2, 400, SRC[0], SRC[1])
    return det, lane, cam


def pipeline_kw():
    Mh = A.PerspectiveTransformation((SRC[1], SRC[0])).M
    car = A.SingleCamDistanceMeasure.RefSizeDict["car"][0]
    return dict(n_streams=2, precision="bf16", src_hw=SRC, lane_cfg=LANE_CFG, track=True, box_score=BOX_SCORE, max_candidates=MAXC,
                geometry=dict(bird_wh=(SRC[1], SRC[0]), M=Mh), analysis=dict(ref_height=[car] * 80))


def restate(p, frame, s, stages, trk_table):
    lanes, _ = p.decode.fetch(s)
    geo = p.geometry.fetch(s)
    fr = p.analysis.fetch_frame(s)
    pts = [(x, y) for x, y, _ in p.analysis.fetch_points(s)]
    colour = ref.COLLISION_COLORS[{"UNKNOWN": 0, "NORMAL": 1, "PROMPT": 2, "WARNING": 3}[fr["collision_msg"].name]]
    off = {"UNKNOWN": ref.OFFSET_UNKNOWN, "RIGHT": ref.OFFSET_RIGHT, "LEFT": ref.OFFSET_LEFT, "CENTER": ref.OFFSET_CENTER}[fr["offset_msg"].name]
    _, tracked, _ = p.tracker.fetch(s)
    trajs = p.tracker.fetch_trajectories(s)
    act = [i for i, t in enumerate(tracked) if t["is_activated"]]
    want, flags, marks = tref.compose(frame, lanes, geo["area_points"], geo["area_status"], pts, off, colour, stages, trks=[tracked[i]["tlwh"] for i in act],
                                      trk_cls=[int(tracked[i]["class_id"]) for i in act], trk_table=trk_table, trajectories=[trajs[i] for i in act])
    assert flags == 0
    return want, marks


def test_pipeline_graph_eager_and_restatement(models):
    """The fused step with stages=("lanes", "area", "trajectories", "distance"): graph and eager give the same frame_show, both equal the
    restatement applied to what the pipeline fetches (lanes, polygon, analysis row, distance points, the tracker's rows and trajectories
    after this step's update), and the device's marks are the restatement's, over enough steps for rectangles (2 .. 5 boxes in a ring) and
    arrows (7 and more)."""
    det_model, lane_model, cam = models
    rng = np.random.default_rng(12)
    trk_table = rng.integers(0, 256, (80, 3)).tolist()
    ovl = dict(stages=("lanes", "area", "trajectories", "distance"), track_colors=trk_table)
    pg = PL.AdasPipeline(det_model, lane_model, use_graph=True, overlay=ovl, **pipeline_kw())
    pe = PL.AdasPipeline(det_model, lane_model, use_graph=False, overlay=ovl, **pipeline_kw())
    dev = L.DeviceBuffer.from_array(cam)
    n = {tref.CIRCLE: 0, tref.RECT: 0, tref.ARROW: 0}
    for k in range(8):
        for p in (pg, pe):
            p.step_frames(dev.ptr, SRC, 0.6)
            p.sync()
        if k in (0, 2, 7):
            for s in range(2):
                want, marks = restate(pg, cam[s], s, 7 | TRAJ, trk_table)
                ig, ie = pg.overlay_image(s), pe.overlay_image(s)
                assert np.array_equal(ig, ie), (k, s)
                assert np.array_equal(ig, want), (k, s, np.argwhere(ig != want)[:5])
                assert tref.device_marks_table(pg.overlay.track_marks(s)) == tref.marks_table(marks), (k, s)
                for m in marks:
                    n[m["kind"]] += 1
    print("marks drawn", n)
    assert n[tref.CIRCLE] > 0 and n[tref.RECT] > 0 and n[tref.ARROW] > 0
    assert np.array_equal(dev.download(cam.shape, np.uint8), cam)
    for o in (pg, pe):
        o.close()
    dev.free()


def test_pipeline_refusals(models):
    det_model, lane_model, cam = models
    kw = pipeline_kw()
    with pytest.raises(ValueError, match="trajectories stage needs micro_batch"):
        PL.AdasPipeline(det_model, lane_model, micro_batch=2, overlay=dict(stages=("lanes", "trajectories")), **kw)
    with pytest.raises(ValueError, match="trajectories stage needs det_model= and track=True"):
        PL.AdasPipeline(det_model, lane_model, overlay=dict(stages=("trajectories",)), **dict(kw, track=False))
    with pytest.raises(ValueError, match="trajectories stage needs det_model"):
        PL.AdasPipeline(None, lane_model, overlay=dict(stages=("trajectories",)), **dict(kw, analysis=None))
    d = L.DeviceBuffer.from_array(cam)
    q = PL.AdasPipeline(det_model, lane_model, overlay=dict(stages=("lanes",)), **dict(kw, analysis=None, track=False))
    L.check(L.lib().adas_pipeline_set_overlay_stages(q.h, 63 | TRAJ))                       # 128 is accepted beside the other six
    L.check(L.lib().adas_pipeline_set_overlay_stages(q.h, 1 | TRAJ))
    with pytest.raises(RuntimeError, match="trajectories stage needs a tracker") as ei:      # and refused at the step, by name
        q.step_frames(d.ptr, SRC, 0.6)
    assert ei.value.code == INVALID
    for bad in (64, 64 | TRAJ, 256):
        with pytest.raises(RuntimeError, match="unknown stage bits") as ei:
            L.check(L.lib().adas_pipeline_set_overlay_stages(q.h, bad))
        assert ei.value.code == INVALID
    q.close()
    d.free()


# ------------------------------------------------------------------------------------------------ the drop-in method
def test_drop_in_draw_trajectories():
    """BYTETracker(draw_trajectories=True).DrawTrackedOnFrame(frame, False) is the demo's call: circles and direction marks, from the device
    tracker's live state, on an ndarray and on a StagedFrame; with both flags the boxes too.  The default instance draws what it drew."""
    colours = {"car": (10, 200, 250), "person": (250, 5, 120)}
    img = noise(1, H, W, 13)[0]
    bt = D.BYTETracker(names=colours, draw_trajectories=True)
    plain = D.BYTETracker(names=colours)
    assert plain.draw_trajectories is False
    labels = ["car", "person", "bus"]
    for k in range(8):
        dets = np.array([[12.0 + 3 * k, 11.0 + k, 30.0 + 3 * k, 24.0 + k], [40.0 - 2 * k, 12.0, 58.0 - 2 * k, 30.0], [20.0, 26.0 + (k % 2), 32.0, 34.0 + (k % 2)]])
        for t in (bt, plain):
            t.update(dets, [0.9, 0.8, 0.95], labels)
        if k not in (2, 7):
            continue
        online = [t for t in bt.tracked_stracks if t["is_activated"]]
        assert len(online) == 3
        trajs = bt.trajectories()
        tcols = [colours.get(t["class_id"], (0, 0, 0)) for t in online]
        args = dict(trks=[t["tlwh"] for t in online], trk_cls=list(range(len(online))), trk_table=tcols, trajectories=[trajs[t["track_id"]] for t in online])
        demo, f1, m1 = tref.compose(img, stages=TRAJ, **args)
        both, f2, _ = tref.compose(img, stages=TRK | TRAJ, **args)
        boxes, _ = oref.compose(img, stages=TRK, trks=args["trks"], trk_cls=args["trk_cls"], trk_table=tcols)
        assert f1 == f2 == 0 and {m["kind"] for m in m1} == {tref.CIRCLE, tref.RECT if k == 2 else tref.ARROW}
        a = img.copy()
        bt.DrawTrackedOnFrame(a, False)
        assert np.array_equal(a, demo) and (a != img).any()
        b = img.copy()
        bt.DrawTrackedOnFrame(b)
        assert np.array_equal(b, both)
        c = img.copy()
        bt.DrawTrackedOnFrame(c, True, False)
        assert np.array_equal(c, boxes)
        e = img.copy()
        bt.DrawTrackedOnFrame(e, False, False)
        assert np.array_equal(e, img)
        dbuf = L.DeviceBuffer.from_array(img)                                             # a StagedFrame is drawn where it sits
        bt.DrawTrackedOnFrame(D.StagedFrame(dbuf.ptr, H, W, 0), False)
        assert np.array_equal(dbuf.download(img.shape, np.uint8), demo)
        dbuf.upload(img)
        bt.DrawTrackedOnFrame(D.StagedFrame(dbuf.ptr, H, W, 0), True, True)
        assert np.array_equal(dbuf.download(img.shape, np.uint8), both)
        dbuf.free()
        g = img.copy()                                                                      # the default instance: today's bytes
        plain.DrawTrackedOnFrame(g)
        assert np.array_equal(g, boxes)
        g2 = img.copy()
        plain.DrawTrackedOnFrame(g2, show_box=False)
        assert np.array_equal(g2, img)
        plain.draw_trajectories = True                                                      # a plain settable attribute
        g3 = img.copy()
        plain.DrawTrackedOnFrame(g3, False)
        assert np.array_equal(g3, demo)
        plain.draw_trajectories = False
        painter = PP.OverlayPainter()                                                       # the host-array form
        h = img.copy()
        painter.trajectories(h, args["trks"], args["trajectories"], args["trk_cls"], tcols)
        assert np.array_equal(h, demo)
        painter.close()
    bt.close(); plain.close()
