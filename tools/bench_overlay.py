#!/usr/bin/env python3
"""Cost of the lane overlay (csrc/overlay_kernels.hip), stand-alone and as the last stage of the fused step, against a copy and against
drawing on the host:
    python tools/bench_overlay.py [--streams 64] [--steps 30] [--rounds 5] [--iters 50] [--host-steps 2]
(a) stand-alone: LaneOverlay.run_arrays with every stage on --streams frames of 1280x720 (per frame 4 x 72 lane points, an ego-lane
    polygon of 840 vertices, 16 distance points, 4 x 72 bird points), timed with the library's events on the null stream against
    hipMemcpyAsync device-to-device of the same frames between the same events, in alternation.  The copy is the yardstick: the
    streaming pass moves the same bytes plus the coverage words.  The frame stages alone (no bird view) and an empty scene (the pass as a
    pure copy plus the preparation and clean-up launches) are timed the same way to show where the time goes.  So is the object layer:
    the frame stages plus --detections cornerRect boxes per frame, plus --tracks tracked boxes (rectangle and tint), and all six stages;
    and the trajectories stage: the frame stages plus the --tracks tracks' circles over full 30-box rings and their direction marks (every
    other track an arrow, the others a lock-on rectangle), and all seven stages.
(b) fused step: two pipelines of the same two networks, bird-view image and analysis in ONE process, stepped from the same camera frames
    in alternation: `off` as it was, `on` with overlay= (all four stages), `obj` with the detections and tracks stages as well, `trj` with
    the four stages and the trajectories stage.  A window is
    --steps steps between two host clock readings with
    the pipeline drained at both ends; median window of --rounds, with the fastest and the slowest.
(c) the host loop the stage replaces, on the `off` pipeline: sync, fetch every frame's lanes, polygon, analysis row, distance points and
    bird view, and draw with the NumPy restatement (tests/overlay_ref.py) -- --host-steps steps, per step.
Writes profiles/r07/overlay_ab.txt (or --out)."""
import argparse, ctypes as C, importlib, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from conftest import load_pkg
load_pkg()
L = importlib.import_module("adas_amd._lib")
CE = importlib.import_module("adas_amd.coreEngine")
PP = importlib.import_module("adas_amd.postproc")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")
A = importlib.import_module("adas_amd.analysis")
import bench, netutil
import overlay_ref as ref

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--host-steps", type=int, default=2)
ap.add_argument("--precision", default=None)
ap.add_argument("--box-score", type=float, default=0.1)
ap.add_argument("--detections", type=int, default=24, help="boxes per frame of the detections stage in (a)")
ap.add_argument("--tracks", type=int, default=16, help="boxes per frame of the tracks stage in (a)")
ap.add_argument("--no-objects", action="store_true", help="leave the object layer's and the trajectories stage's variants out of (a)'s alternation and (b)")
ap.add_argument("--standalone-only", action="store_true", help="(a) alone, e.g. under a kernel trace")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "overlay_ab.txt"))
a = ap.parse_args()
if L.lib().adas_device_count() <= 0:
    raise SystemExit("bench_overlay.py needs an MI355X: there is no CPU fallback and no CPU timing")
S, H, W, IMG = a.streams, 720, 1280, (1280, 720)
hip = C.CDLL("libamdhip64.so")      # already in the process: libadas_hip.so links it
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
D2D = 3                             # hipMemcpyDeviceToDevice


def median(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


# ------------------------------------------------------------------------------------------------ (a) stand-alone
cams = [bench.cam_frames(S, 900 + i) for i in range(2)]
cam = [L.DeviceBuffer.from_array(c) for c in cams]
nbytes = cams[0].nbytes
rows = np.arange(300, 720)
left = np.stack([0.44 * W - 0.32 * (rows - 300), rows], 1).astype(np.int32)
right = np.stack([0.55 * W + 0.36 * (rows - 300), rows], 1).astype(np.int32)
poly1 = np.concatenate([left, right[::-1]])
lane1 = np.zeros((4, 128, 2), np.int32)
for l, (x0, k) in enumerate(((0.2, -0.5), (0.44, -0.32), (0.55, 0.36), (0.8, 0.5))):
    yy = np.linspace(302, 718, 72)
    lane1[l, :72] = np.stack([x0 * W + k * (yy - 300), yy], 1).astype(np.int32)
rng = np.random.default_rng(0)
arrays = dict(lane_points=np.broadcast_to(lane1, (S, 4, 128, 2)), lane_counts=np.full((S, 4), 72, np.int32),
              poly=np.broadcast_to(poly1, (S,) + poly1.shape), poly_counts=np.full(S, len(poly1), np.int32), area_status=np.ones(S, np.int32),
              offset_type=(np.arange(S) % 4).astype(np.int32), area_bgr=np.array([ref.COLLISION_COLORS[s % 4] for s in range(S)], np.uint8),
              dist_points=np.stack([rng.integers(0, W, (S, 16)), rng.integers(300, H, (S, 16))], 2).astype(np.int32),
              dist_counts=np.full(S, 16, np.int32), bird_points=np.broadcast_to(lane1, (S, 4, 128, 2)), bird_counts=np.full((S, 4), 72, np.int32))
bufs = {k: L.DeviceBuffer.from_array(np.ascontiguousarray(v)) for k, v in arrays.items()}
kw = {k: b.ptr for k, b in bufs.items()}
kw.update(poly_cap=len(poly1), dist_cap=16)
zero = L.DeviceBuffer.from_array(np.zeros(4 * S, np.int32))
kw_empty = dict(kw, lane_counts=zero.ptr, poly_counts=zero.ptr, dist_counts=zero.ptr, bird_counts=zero.ptr)
ND, NT = a.detections, a.tracks            # the object layer's boxes: vehicle-sized, in the lower two thirds of the frame
bx, by = rng.integers(-40, W - 60, (S, ND + NT)), rng.integers(220, H - 60, (S, ND + NT))
bw, bh = rng.integers(60, 300, (S, ND + NT)), rng.integers(50, 220, (S, ND + NT))
obj = dict(det_xyxy=np.stack([bx, by, bx + bw, by + bh], 2)[:, :ND].astype(np.int32), det_cls=rng.integers(0, 80, (S, ND)).astype(np.int32),
           det_counts=np.full(S, ND, np.int32), trk_tlwh=np.stack([bx, by, bw, bh], 2)[:, ND:].astype(np.float64) + 0.5,
           trk_cls=rng.integers(0, 80, (S, NT)).astype(np.int32), trk_counts=np.full(S, NT, np.int32))
# the tracks' trajectories: full rings that end on the track's box, a step of a few pixels a frame; every other track's first 26 boxes hang
# over the bottom border (filter_trajectories drops them): 4 boxes left, a lock-on rectangle -- the others get the shadowed arrow
tl = obj["trk_tlwh"]
vel = np.stack([rng.uniform(-5, 5, (S, NT)), rng.uniform(-2, 2, (S, NT))], 2)
age = np.arange(29, -1, -1, dtype=np.float64)[None, None, :, None]
xy = np.clip(tl[:, :, None, :2] - vel[:, :, None, :] * age, 12.0, None)
ring = np.concatenate([xy, xy + np.minimum(tl[:, :, None, 2:], 200.0)], 3)
ring[:, :, :, 2] = np.minimum(ring[:, :, :, 2], W - 12.0)
ring[:, :, :, 3] = np.minimum(ring[:, :, :, 3], H - 12.0)
ring[:, 1::2, :26, 3] = H - 4.0
obj["traj"] = np.ascontiguousarray(ring)
obj["traj_len"] = np.full((S, NT), 30, np.int32)
obufs = {k: L.DeviceBuffer.from_array(np.ascontiguousarray(v)) for k, v in obj.items()}
okw = dict(kw, det_cap=ND, trk_cap=NT, **{k: b.ptr for k, b in obufs.items() if k not in ("traj", "traj_len")})
tkw = dict(okw, trajectories=(obufs["traj"].ptr, obufs["traj_len"].ptr))
CLASS_COLORS = rng.integers(0, 256, (80, 3)).tolist()
ov = PP.LaneOverlay((H, W), (H, W), S)
ov.set_class_colors("detections", CLASS_COLORS)
ov.set_class_colors("tracks", CLASS_COLORS)
dst = ov.device_view()
bird = L.DeviceBuffer.from_array(cams[1])
timer = L.StreamTimer()


def timed(fn):
    with timer:
        for _ in range(a.iters):
            fn()
    return timer.ms / a.iters * 1e3      # us per call


variants = [("copy", lambda: hip.hipMemcpyAsync(dst, cam[0].ptr, nbytes, D2D, None)),
            ("overlay, all stages", lambda: ov.run_arrays(cam[0].ptr, S, bird_ptr=bird.ptr, stages=15, **kw)),
            ("overlay, frame stages", lambda: ov.run_arrays(cam[0].ptr, S, stages=7, **kw)),
            ("overlay, empty scene", lambda: ov.run_arrays(cam[0].ptr, S, stages=7, **kw_empty)),
            ("frame stages + detections", lambda: ov.run_arrays(cam[0].ptr, S, stages=7 | 16, **okw)),
            ("frame stages + tracks", lambda: ov.run_arrays(cam[0].ptr, S, stages=7 | 32, **okw)),
            ("all six stages", lambda: ov.run_arrays(cam[0].ptr, S, bird_ptr=bird.ptr, stages=63, **okw)),
            ("frame stages + trajectories", lambda: ov.run_arrays(cam[0].ptr, S, stages=7 | 128, **tkw)),
            ("all seven stages", lambda: ov.run_arrays(cam[0].ptr, S, bird_ptr=bird.ptr, stages=63 | 128, **tkw))]
OBJECT_LINES = ("frame stages + detections", "frame stages + tracks", "all six stages", "frame stages + trajectories", "all seven stages")
if a.no_objects:
    variants = [v for v in variants if v[0] not in OBJECT_LINES]
    OBJECT_LINES = ()
for _, fn in variants:                     # warm-up
    fn()
L.check(L.lib().adas_synchronize())
us = {n: [] for n, _ in variants}
for _ in range(a.rounds):
    for n, fn in variants:
        us[n].append(timed(fn))
ov.run_arrays(cam[0].ptr, S, stages=7, **kw)
drawn = float((ov.fetch(0) != cams[0][0]).any(axis=2).mean())
lines = ["tools/bench_overlay.py on one MI355X (gfx950).", "",
         "(a) stand-alone, %d frames of 1280x720 (%.1f MB read + %.1f MB written), %d rounds of %d calls between two events on the null stream,"
         % (S, nbytes / 1e6, nbytes / 1e6, a.rounds, a.iters),
         "    alternated in one process; us per call, median round (fastest, slowest); %.1f %% of a frame's pixels are drawn on." % (100 * drawn), ""]
share = {}
for name, st in (("detections", 16), ("tracks", 32), ("trajectories", 128)):
    ov.run_arrays(cam[0].ptr, S, stages=st, **tkw)
    share[name] = float((ov.fetch(0) != cams[0][0]).any(axis=2).mean())
marks = ov.track_marks(0)
n_marks = {k: int((marks["kind"] == k).sum()) for k in (1, 2, 3)}
cm = median(us["copy"])[0]
for n, _ in variants:
    if n in OBJECT_LINES:
        continue
    m, lo, hi = median(us[n])
    lines.append("    %-22s %9.1f us  (%.1f, %.1f)  %5.2f TB/s of frame bytes  %.2f x the copy" % (n, m, lo, hi, 2 * nbytes / m / 1e6, m / cm))
allm, frm, emp = (median(us[n])[0] for n in ("overlay, all stages", "overlay, frame stages", "overlay, empty scene"))
lines += ["", "    ratio to the copy: %.2f (expected within 1.5).  The empty scene (a mark launch with nothing to mark, the streaming pass as a pure"
          % (allm / cm), "    copy + its ANY-plane reads, the clean-up pass over the ANY plane) costs %.1f us = %.2f x the copy; having something to draw adds"
          % (emp, emp / cm), "    %.1f us to the three frame launches; the bird view's two launches add %.1f us." % (frm - emp, allm - frm)]
if OBJECT_LINES:
    lines += ["", "    the object layer: %d detections per frame (cornerRect: outline and eight arms, %.1f %% of a frame's pixels) and %d tracked boxes per frame"
              % (ND, 100 * share["detections"], NT), "    (thickness-2 rectangle and the tinted region, %.1f %% of a frame's pixels), one record-building launch more:"
              % (100 * share["tracks"]),
              "    the trajectories stage: per frame the same %d tracks' full rings -- %d circles, %d lock-on rectangles, %d arrows (three to a track) in frame 0,"
              % (NT, n_marks[1], n_marks[2], n_marks[3]), "    %.2f %% of a frame's pixels; two launches more (the primitives, one pass per band of rows that draws them):"
              % (100 * share["trajectories"]), ""]
for n in OBJECT_LINES:
    m, lo, hi = median(us[n])
    lines.append("    %-26s %9.1f us  (%.1f, %.1f)  %5.2f x the copy  %+8.1f us on this run's frame stages" % (n, m, lo, hi, m / cm, m - frm))
for b in list(bufs.values()) + list(obufs.values()) + [zero, bird]:
    b.free()
ov.close(); timer.close()

if a.standalone_only:
    for b in cam:
        b.free()
    print("\n".join(lines))
    raise SystemExit(0)

# ------------------------------------------------------------------------------------------------ (b) fused step, (c) host loop


class PrescribedLanes:
    """Zero weights and a last-layer bias that puts both ego lanes on every row anchor (CULane head: 200 x 72 rows, 100 x 81 columns)."""

    def __init__(self, gr=200, r=72, gc=100, c=81):
        loc_row = np.zeros((gr, r, 4), np.float32)
        exist_row = np.zeros((2, r, 4), np.float32)
        for k in range(r):
            loc_row[int(round(0.44 * gr - 0.2 * gr / 100 * k)), k, 1] = 10.0
            loc_row[int(round(0.55 * gr + 0.22 * gr / 100 * k)), k, 2] = 10.0
        exist_row[1, :, 1:3] = 5.0
        self.bias = np.concatenate([loc_row.reshape(-1), np.zeros(gc * c * 4, np.float32), exist_row.reshape(-1), np.zeros(2 * c * 4, np.float32)])

    def __call__(self, name, shape, kind, fill=None):
        return self.bias if name == "cls.3.bias" else np.zeros(shape, np.float32)


work = tempfile.mkdtemp(prefix="ovl_bench_")
base = netutil.coco_like_frames(8, seed=40)
det_path, _, _ = bench.build_detector(M, CE, "yolov8n", base, work, "ovl", target_per_frame=25.0, capacity=512)
lane_path = M.build("ufldv2_res18", wsrc=PrescribedLanes()).save(os.path.join(work, "lane.hipm"))
Mh = A.PerspectiveTransformation(IMG).M
car = A.SingleCamDistanceMeasure.RefSizeDict["car"][0]
pkw = dict(n_streams=S, precision=a.precision, src_hw=(H, W), use_graph=True, track=True, box_score=a.box_score, max_candidates=512,
           geometry=dict(bird_wh=IMG, M=Mh), birdview=dict(image=True), analysis=dict(ref_height=[car] * 80))
pipes = [("off", PL.AdasPipeline(det_path, lane_path, **pkw)), ("on", PL.AdasPipeline(det_path, lane_path, overlay=dict(), **pkw)),
         ("obj", PL.AdasPipeline(det_path, lane_path, overlay=dict(stages=("lanes", "area", "distance", "bird", "detections", "tracks"),
                                                                    detection_colors=CLASS_COLORS, track_colors=CLASS_COLORS), **pkw))]
pipes.append(("trj", PL.AdasPipeline(det_path, lane_path, overlay=dict(stages=("lanes", "area", "distance", "bird", "trajectories"),
                                                                        track_colors=CLASS_COLORS), **pkw)))
if a.no_objects:
    pipes.pop()[1].close()
    pipes.pop()[1].close()
count = {n: 0 for n, _ in pipes}
OFF = {"UNKNOWN": 0, "RIGHT": 1, "LEFT": 2, "CENTER": 3}
COL = {"UNKNOWN": 0, "NORMAL": 1, "PROMPT": 2, "WARNING": 3}


def window(name, p, n):
    p.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        i = count[name]
        count[name] += 1
        p.step_frames(cam[i % 2].ptr, (H, W), 0.6)
    p.sync()
    return (time.perf_counter() - t0) / n * 1e3


def host_loop(p, frames):
    """What a user of the `off` pipeline does to get frame_show and the bird view with its discs for every stream."""
    p.sync()
    t0 = time.perf_counter()
    shown = []
    for s in range(S):
        lanes, _ = p.decode.fetch(s)
        geo = p.geometry.fetch(s)
        fr = p.analysis.fetch_frame(s)
        pts = [(x, y) for x, y, _ in p.analysis.fetch_points(s)]
        off = OFF[fr["offset_msg"].name]
        show, _ = ref.compose(frames[s], lanes, geo["area_points"], geo["area_status"], pts, off, ref.COLLISION_COLORS[COL[fr["collision_msg"].name]], 7)
        birdv = ref.draw_lanes(p.birdview_image(s), geo["bird_points"], off, radius=10, direct=True)
        shown.append((show, birdv))
    return (time.perf_counter() - t0) * 1e3, shown


for name, p in pipes:                      # warm-up: capture, first-launch costs
    window(name, p, 5)
ms = {n: [] for n, _ in pipes}
for _ in range(a.rounds):
    for name, p in pipes:
        ms[name].append(window(name, p, a.steps))
host = []
same = True
for k in range(a.host_steps):
    for name, p in pipes[:2]:
        p.step_frames(cam[k % 2].ptr, (H, W), 0.6)
    t, shown = host_loop(pipes[0][1], cams[k % 2])
    host.append(t)
    pipes[1][1].sync()
    same = same and all(np.array_equal(pipes[1][1].overlay_image(s), shown[s][0]) and np.array_equal(pipes[1][1].birdview_image(s), shown[s][1])
                        for s in range(0, S, max(1, S // 4)))
lines += ["", "(b) fused step (yolov8n + ufldv2_res18, %s, hipGraph, two branches, tracker, bird-view image, analysis), %d streams of 1280x720 from"
          % (pipes[0][1].lane.precision, S),
          "    camera frames, %d windows of %d steps per variant, alternated in one process; ms per step, median window (fastest, slowest)."
          % (a.rounds, a.steps), ""]
med = {}
for name, _ in pipes:
    med[name], lo, hi = median(ms[name])
    lines.append("    %-4s %8.3f ms per step  (%.3f, %.3f)" % (name, med[name], lo, hi))
hm, hlo, hhi = median(host)
lines += ["", "    on - off = %+8.1f us per step (five plain launches behind the analysis stage, inside the capture); the stand-alone run takes %.1f us"
          % ((med["on"] - med["off"]) * 1e3, allm),
          ] + (["    obj - on  = %+8.1f us per step (the detections and tracks stages: the step's survivors and its tracked tracks, one launch more)"
                % ((med["obj"] - med["on"]) * 1e3)] if "obj" in med else []) + (
          ["    trj - on  = %+8.1f us per step (the trajectories stage: the tracker's live rows and rings after this step's update, two launches more)"
           % ((med["trj"] - med["on"]) * 1e3)] if "trj" in med else []) + [
          "", "(c) the host loop the stage replaces, on the `off` pipeline after a sync: per stream 5 fetches (lanes, geometry, analysis row, distance",
          "    points, bird view) and the NumPy restatement's drawing of both images: %.1f ms per step of %d streams (fastest %.1f, slowest %.1f; %d steps),"
          % (hm, S, hlo, hhi, a.host_steps),
          "    during which the device idles; its images equal the `on` pipeline's on the streams compared: %s" % same]
for _, p in pipes:
    p.close()
for b in cam:
    b.free()
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, "w").write(text)
print(text)
