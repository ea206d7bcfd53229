#!/usr/bin/env python3
"""Cost of the per-stream adaptive bird view inside the fused step: python tools/bench_birdview.py [--streams 64] [--steps 30] [--rounds 5]
Three pipelines of the same two networks in ONE process -- the stage off, points only (adas_birdview_run + per-frame matrices into the
geometry kernel), points + image (the 1280x720 warp of every frame as well) -- stepped from the same camera frames in alternation
(off, points, image, off, ...) so that clock and thermal drift hit all three alike.  A window is `--steps` steps between two host clock
readings with the pipeline drained at both ends; the median window of `--rounds` is reported with the fastest and the slowest.  The
points and image variants get one request_transform per step (a rotating stream and rule), which is more than a host TaskConditions
issues.  The lane network carries a prescribed last-layer bias (both ego lanes on every row anchor), so area_status holds on every
frame: every request is applied and the geometry does its full work.
Then tools/bench_warp.py runs on the same box, and the share of the stand-alone warp that the overlap with the detector branch hides
is worked out: hidden = warp_alone - (image - points).  The solver-error pair of tests/test_birdview_cpu.py is recorded beside it.
Writes profiles/r07/birdview_ab.txt (or --out)."""
import argparse, importlib, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from conftest import load_pkg
load_pkg()
L = importlib.import_module("adas_amd._lib")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")
A = importlib.import_module("adas_amd.analysis")
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--precision", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "birdview_ab.txt"))
a = ap.parse_args()
if L.lib().adas_device_count() <= 0:
    raise SystemExit("bench_birdview.py needs an MI355X: there is no CPU fallback and no CPU timing")
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


work = tempfile.mkdtemp(prefix="bv_bench_")
det_path = M.build("yolov8n").save(os.path.join(work, "det.hipm"))
lane_path = M.build("ufldv2_res18", wsrc=PrescribedLanes()).save(os.path.join(work, "lane.hipm"))
cam = [L.DeviceBuffer.from_array(bench.cam_frames(S, 900 + i)) for i in range(2)]
Mh = A.PerspectiveTransformation(IMG).M
kw = dict(n_streams=S, precision=a.precision, src_hw=(720, 1280), use_graph=True, geometry=dict(bird_wh=IMG, M=Mh))
pipes = [("off", PL.AdasPipeline(det_path, lane_path, **kw)),
         ("points", PL.AdasPipeline(det_path, lane_path, birdview=dict(image=False), **kw)),
         ("image", PL.AdasPipeline(det_path, lane_path, birdview=dict(image=True), **kw))]
MODES = ("Default", "Top", "Bottom")
count = {n: 0 for n, _ in pipes}


def window(name, p, n):
    p.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        i = count[name]
        count[name] += 1
        if p.birdview is not None:
            p.request_transform(i % S, MODES[i % 3])
        p.step_frames(cam[i % 2].ptr, (720, 1280), 0.6)
    p.sync()
    return (time.perf_counter() - t0) / n * 1e3


for name, p in pipes:                      # warm-up: capture, first-launch costs
    window(name, p, 5)
ms = {n: [] for n, _ in pipes}
for _ in range(a.rounds):
    for name, p in pipes:
        ms[name].append(window(name, p, a.steps))
lines = ["tools/bench_birdview.py on one MI355X (gfx950): fused step (yolov8n + ufldv2_res18, %s, hipGraph, two branches), %d streams of 1280x720,"
         % (pipes[0][1].lane.precision, S),
         "%d windows of %d steps per variant, alternated in one process; ms per step, median window (fastest, slowest)." % (a.rounds, a.steps), ""]
med = {}
for name, p in pipes:
    v = sorted(ms[name])
    med[name] = v[len(v) // 2]
    lines.append("%-7s %8.3f ms per step  (%.3f, %.3f)" % (name, med[name], v[0], v[-1]))
applied = sum(pipes[1][1].birdview.fetch_stream(s)["n_updates"] for s in range(S))
rejected = sum(pipes[1][1].birdview.fetch_stream(s)["n_rejected"] for s in range(S))
lines.append("points variant: %d requests issued, %d applied, %d rejected" % (count["points"], applied, rejected))
for _, p in pipes:
    p.close()
for c in cam:
    c.free()
out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_warp.py"), str(S), "200"], capture_output=True, text=True, cwd=ROOT)
warp_us = None
for l in out.stdout.splitlines():
    if l.startswith("batch %2d:" % S):
        warp_us = float(l.split(":")[1].split("us")[0])
lines += ["", "$ python tools/bench_warp.py %d 200" % S] + out.stdout.strip().splitlines()
lines.append("")
d_pts, d_img = (med["points"] - med["off"]) * 1e3, (med["image"] - med["points"]) * 1e3
lines.append("points - off   = %+8.1f us per step (one birdview_kernel launch; the geometry kernel reads its matrix from a table)" % d_pts)
lines.append("image - points = %+8.1f us per step" % d_img)
if warp_us:
    lines.append("stand-alone warp of %d frames = %.1f us: the overlap with the detector branch hides %.1f us of it (%.0f %%)"
                 % (S, warp_us, warp_us - d_img, 100 * (warp_us - d_img) / warp_us))
import test_birdview_cpu as T
acc = T.accuracy()
lines += ["", "solver error over %d trapezoids (tests/test_birdview_cpu.py, err scaled per row against the exact rational solution):" % acc["n"],
          "  analysis.perspective_matrix (np.linalg.solve): %.3e (M)  %.3e (M_inv)" % (acc["ref_fwd"], acc["ref_inv"]),
          "  birdview_core.h (host build of the device text): %.3e (M)  %.3e (M_inv);  bound 4 x reference (M) = %.3e"
          % (acc["emu_fwd"], acc["emu_inv"], 4 * acc["ref_fwd"])]
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, "w").write(text)
print(text)
