#!/usr/bin/env python3
"""Cost of distance, collision and warning state as the last stage of the fused step, against doing it on the host:
    python tools/bench_analysis.py [--streams 64] [--steps 30] [--rounds 5]
Three pipelines of the same two networks and the points-only bird view in ONE process, stepped from the same seam tensors in alternation
(off, on, host, off, ...) so that clock and thermal drift hit all three alike:
  off   the fused step as it was: nobody asks for a re-anchoring;
  on    analysis= attached: adas_analysis_run behind the join, its request words feed the next step's bird view on the device;
  host  the alternative the stage replaces: after every step sync, fetch every stream's survivors and geometry, run
        analysis.SingleCamDistanceMeasure / TaskConditions, queue request_transform where CheckStatus() says so -- the next step waits.
A window is `--steps` steps between two host clock readings with the pipeline drained at both ends; the median window of `--rounds` is
reported with the fastest and the slowest.  The detector is the calibrated synthetic one of bench.py on eight grey-noise frames dealt
round-robin to the streams, every class given the car's reference height; the lane network carries a prescribed last-layer bias (both
ego lanes on every row anchor), so area_status holds and every frame's polygon has its full length.
Writes profiles/r07/analysis_ab.txt (or --out)."""
import argparse, importlib, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from conftest import load_pkg
load_pkg()
L = importlib.import_module("adas_amd._lib")
CE = importlib.import_module("adas_amd.coreEngine")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")
A = importlib.import_module("adas_amd.analysis")
import bench, netutil

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--precision", default=None)
ap.add_argument("--box-score", type=float, default=0.1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "analysis_ab.txt"))
a = ap.parse_args()
if L.lib().adas_device_count() <= 0:
    raise SystemExit("bench_analysis.py needs an MI355X: there is no CPU fallback and no CPU timing")
S, IMG = a.streams, (1280, 720)


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


class CarBox:
    label = "car"

    def __init__(self, xyxy):
        self.xyxy = [int(v) for v in xyxy]

    def tolist(self):
        return list(self.xyxy)


work = tempfile.mkdtemp(prefix="ana_bench_")
base = netutil.coco_like_frames(8, seed=40)
det_path, _, _ = bench.build_detector(M, CE, "yolov8n", base, work, "ana", target_per_frame=25.0, capacity=512)
lane_path = M.build("ufldv2_res18", wsrc=PrescribedLanes()).save(os.path.join(work, "lane.hipm"))
seam = [L.DeviceBuffer.from_array(np.ascontiguousarray(np.roll(base, i, axis=0)[np.arange(S) % 8])) for i in range(2)]
lane_in = L.DeviceBuffer.from_array(np.zeros((S, 3, 320, 1600), np.float32))
Mh = A.PerspectiveTransformation(IMG).M
kw = dict(n_streams=S, precision=a.precision, src_hw=(720, 1280), use_graph=True, track=True, box_score=a.box_score, max_candidates=512,
          geometry=dict(bird_wh=IMG, M=Mh), birdview=dict(image=False))
car = A.SingleCamDistanceMeasure.RefSizeDict["car"][0]
pipes = [("off", PL.AdasPipeline(det_path, lane_path, **kw)),
         ("on", PL.AdasPipeline(det_path, lane_path, analysis=dict(ref_height=[car] * 80), **kw)),
         ("host", PL.AdasPipeline(det_path, lane_path, **kw))]
tcs = [A.TaskConditions() for _ in range(S)]
dms = [A.SingleCamDistanceMeasure(object_list=["car"]) for _ in range(S)]
count = {n: 0 for n, _ in pipes}
host_ms = []


def host_loop(p):
    """demo.py:284-296 for every stream on what the step left on the device; the request lands on the next step."""
    p.sync()
    t0 = time.perf_counter()
    for s in range(S):
        dets = p.post.fetch_dets(s)
        geo = p.geometry.fetch(s)
        dms[s].updateDistance([CarBox(b) for b in dets["xyxy_int"]])
        point = dms[s].calcCollisionPoint(geo["area_points"])
        tcs[s].UpdateCollisionStatus(point, geo["area_status"])
        tcs[s].UpdateOffsetStatus(geo["offset"])
        tcs[s].UpdateRouteStatus(geo["direction"], geo["curvature"])
        if tcs[s].CheckStatus():
            p.request_transform(s, tcs[s].transform_status)
    host_ms.append((time.perf_counter() - t0) * 1e3)


def window(name, p, n):
    p.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        i = count[name]
        count[name] += 1
        p.step(seam[i % 2].ptr, lane_in.ptr)
        if name == "host":
            host_loop(p)
    p.sync()
    return (time.perf_counter() - t0) / n * 1e3


for s in range(S):                          # the host twin's first CheckStatus(): "Default" on every stream, as attach queues it for "on"
    if tcs[s].CheckStatus():
        pipes[2][1].request_transform(s, tcs[s].transform_status)
for name, p in pipes:                       # warm-up: capture, first-launch costs
    window(name, p, 5)
ms = {n: [] for n, _ in pipes}
for _ in range(a.rounds):
    for name, p in pipes:
        ms[name].append(window(name, p, a.steps))
on = pipes[1][1]
frames = [on.analysis.fetch_frame(s) for s in range(S)]
keep = [len(on.post.fetch_dets(s)["keep"]) for s in range(S)]
area = [len(on.geometry.fetch(s)["area_points"]) for s in range(S)]
same = all((f["collision_msg"], f["offset_msg"], f["curvature_msg"]) == (t.collision_msg, t.offset_msg, t.curvature_msg) for f, t in zip(frames, tcs))
lines = ["tools/bench_analysis.py on one MI355X (gfx950): fused step (yolov8n + ufldv2_res18, %s, hipGraph, two branches, tracker, points-only bird view),"
         % pipes[0][1].lane.precision,
         "%d streams of 1280x720 from seam tensors, %d windows of %d steps per variant, alternated in one process; ms per step, median window"
         % (S, a.rounds, a.steps), "(fastest, slowest).", ""]
med = {}
for name, _ in pipes:
    v = sorted(ms[name])
    med[name] = v[len(v) // 2]
    lines.append("%-5s %8.3f ms per step  (%.3f, %.3f)" % (name, med[name], v[0], v[-1]))
hv = sorted(host_ms[5:])
lines += ["", "last step of the `on` variant: %.1f survivors per frame (%d .. %d), %.1f distance points per frame, %d frames with a collision point,"
          % (np.mean(keep), min(keep), max(keep), np.mean([f["n_points"] for f in frames]), sum(f["collision_point"] is not None for f in frames)),
          "polygons of %d .. %d points; its three messages equal the host variant's on every stream: %s" % (min(area), max(area), same),
          "", "on   - off = %+8.1f us per step (one analysis_kernel launch behind the join, %d workgroups)" % ((med["on"] - med["off"]) * 1e3, S),
          "host - off = %+8.1f us per step; the host loop alone (sync excluded: %d fetches of survivors and geometry, analysis.*, requests)"
          % ((med["host"] - med["off"]) * 1e3, 2 * S),
          "             takes %.3f ms per step (median; fastest %.3f, slowest %.3f) during which the device idles" % (hv[len(hv) // 2], hv[0], hv[-1])]
for _, p in pipes:
    p.close()
for b in seam + [lane_in]:
    b.free()
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, "w").write(text)
print(text)
