#!/usr/bin/env python3
"""Cost of the demo's three UI panels on the device (csrc/overlay_panels.hip), stand-alone and behind the overlay in the fused step:
    python tools/bench_panels.py [--streams 64] [--steps 30] [--rounds 5] [--iters 50]
(a) stand-alone: LaneOverlay.run_panels_arrays on --streams frames of 1280x720, in place, with the reference's sprite sizes (100 x 100,
    200 x 200, 300 x 200; synthetic content, masks half set) and a 1280 x 720 bird-view image per frame, timed with the library's events
    on the null stream against hipMemcpyAsync device-to-device of the same frames between the same events, in alternation: all three
    panels, and each alone.  The copy is the yardstick: the panels cover 29.1 % of a frame's pixels, which the draw pass reads and writes,
    plus two of every four rows of the bird image -- about 1.08 frame sizes of traffic against the copy's 2.0.
(b) fused step: two pipelines of the same two networks in the default (exact) precision, bird-view image, analysis and the four overlay
    stages in ONE process, stepped from the same camera frames in alternation: `off` without panels, `on` with all three.  A window is
    --steps steps between two host clock readings with the pipeline drained at both ends; median window of --rounds, with the fastest
    and the slowest.
Writes profiles/r07/overlay_panels_ab.txt (or --out)."""
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
import panel_scene as PS

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--precision", default=None)
ap.add_argument("--box-score", type=float, default=0.1)
ap.add_argument("--standalone-only", action="store_true", help="(a) alone, e.g. under a kernel trace")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "overlay_panels_ab.txt"))
a = ap.parse_args()
if L.lib().adas_device_count() <= 0:
    raise SystemExit("bench_panels.py needs an MI355X: there is no CPU fallback and no CPU timing")
S, H, W, IMG = a.streams, 720, 1280, (1280, 720)
hip = C.CDLL("libamdhip64.so")      # already in the process: libadas_hip.so links it
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
D2D = 3                             # hipMemcpyDeviceToDevice


def median(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


# ------------------------------------------------------------------------------------------------ (a) stand-alone
sprites = PS.sprites()
cams = [bench.cam_frames(S, 900 + i) for i in range(2)]
cam = [L.DeviceBuffer.from_array(c) for c in cams]
nbytes = cams[0].nbytes
work_buf = L.DeviceBuffer.from_array(cams[0])      # the panels draw in place: on a buffer of their own
copy_dst = L.DeviceBuffer(nbytes)
bird = L.DeviceBuffer.from_array(cams[1])
types = [L.DeviceBuffer.from_array(((np.arange(S) * k + j) % n).astype(np.int32)) for k, j, n in ((1, 0, 4), (5, 1, 6), (3, 2, 4))]
ov = PP.LaneOverlay((H, W), (H, W), S)
ov.set_panels(sprites)
timer = L.StreamTimer()


def timed(fn):
    with timer:
        for _ in range(a.iters):
            fn()
    return timer.ms / a.iters * 1e3      # us per call


def panels(mask):
    return lambda: ov.run_panels_arrays(work_buf.ptr, types[0].ptr, types[1].ptr, types[2].ptr, bird.ptr, mask, S, 1)


variants = [("copy", lambda: hip.hipMemcpyAsync(copy_dst.ptr, cam[0].ptr, nbytes, D2D, None)), ("panels, all three", panels(7)),
            ("bird panel", panels(1)), ("signs panel", panels(2)), ("collision panel", panels(4))]
for _, fn in variants:                     # warm-up
    fn()
L.check(L.lib().adas_synchronize())
us = {n: [] for n, _ in variants}
for _ in range(a.rounds):
    for n, fn in variants:
        us[n].append(timed(fn))
work_buf.upload(cams[0])
ov.reset_panels()
panels(7)()
L.check(L.lib().adas_synchronize())
drawn = float((work_buf.download(cams[0].shape, np.uint8)[0] != cams[0][0]).any(axis=2).mean())
cm = median(us["copy"])[0]
lines = ["tools/bench_panels.py on one MI355X (gfx950).", "",
         "(a) stand-alone, %d frames of 1280x720 (%.1f MB; the copy reads and writes all of it), %d rounds of %d calls between two events on the null"
         % (S, nbytes / 1e6, a.rounds, a.iters),
         "    stream, alternated in one process; us per call, median round (fastest, slowest); the panels change %.1f %% of a frame's pixels" % (100 * drawn),
         "    (their rectangles hold 29.1 %; a dimmed zero stays zero).", ""]
for n, _ in variants:
    m, lo, hi = median(us[n])
    lines.append("    %-18s %9.1f us  (%.1f, %.1f)  %.2f x the copy" % (n, m, lo, hi, m / cm))
allm = median(us["panels, all three"])[0]
lines += ["", "    expectation: all three panels cost no more than the copy (about 1.08 frame sizes of traffic against 2.0): ratio %.2f -- %s."
          % (allm / cm, "met" if allm <= cm else "MISSED")]
for b in [work_buf, copy_dst, bird] + types:
    b.free()
ov.close(); timer.close()

if a.standalone_only:
    for b in cam:
        b.free()
    print("\n".join(lines))
    raise SystemExit(0)

# ------------------------------------------------------------------------------------------------ (b) fused step


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


work = tempfile.mkdtemp(prefix="pnl_bench_")
base = netutil.coco_like_frames(8, seed=40)
det_path, _, _ = bench.build_detector(M, CE, "yolov8n", base, work, "pnl", target_per_frame=25.0, capacity=512)
lane_path = M.build("ufldv2_res18", wsrc=PrescribedLanes()).save(os.path.join(work, "lane.hipm"))
Mh = A.PerspectiveTransformation(IMG).M
car = A.SingleCamDistanceMeasure.RefSizeDict["car"][0]
pkw = dict(n_streams=S, precision=a.precision, src_hw=(H, W), use_graph=True, track=True, box_score=a.box_score, max_candidates=512,
           geometry=dict(bird_wh=IMG, M=Mh), birdview=dict(image=True), analysis=dict(ref_height=[car] * 80))
pipes = [("off", PL.AdasPipeline(det_path, lane_path, overlay=dict(), **pkw)),
         ("on", PL.AdasPipeline(det_path, lane_path, overlay=dict(panels=("bird", "signs", "collision"), panel_sprites=sprites), **pkw))]
count = {n: 0 for n, _ in pipes}


def window(name, p, n):
    p.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        i = count[name]
        count[name] += 1
        p.step_frames(cam[i % 2].ptr, (H, W), 0.6)
    p.sync()
    return (time.perf_counter() - t0) / n * 1e3


for name, p in pipes:                      # warm-up: capture, first-launch costs
    window(name, p, 5)
ms = {n: [] for n, _ in pipes}
for _ in range(a.rounds):
    for name, p in pipes:
        ms[name].append(window(name, p, a.steps))
kernels = {name: p.graph_kernels() for name, p in pipes}
seen = sorted({tuple(pipes[1][1].overlay.panel_record(s)["signs"]) + (pipes[1][1].overlay.panel_record(s)["collision"],) for s in range(0, S, max(1, S // 8))})
lines += ["", "(b) fused step (yolov8n + ufldv2_res18, %s, hipGraph, two branches, tracker, bird-view image, analysis, the four overlay stages), %d streams"
          % (pipes[0][1].lane.precision, S),
          "    of 1280x720 from camera frames, %d windows of %d steps per variant, alternated in one process; ms per step, median window (fastest,"
          % (a.rounds, a.steps), "    slowest).", ""]
med = {}
for name, _ in pipes:
    med[name], lo, hi = median(ms[name])
    lines.append("    %-4s %8.3f ms per step  (%.3f, %.3f)   %d kernels in the captured step" % (name, med[name], lo, hi, kernels[name]))
lines += ["", "    on - off = %+8.1f us per step (two plain launches behind the overlay's run, inside the capture); the stand-alone run takes %.1f us."
          % ((med["on"] - med["off"]) * 1e3, allm), "    sprites on the streams looked at after the last step: %s" % (seen,)]
for _, p in pipes:
    p.close()
for b in cam:
    b.free()
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, "w").write(text)
print(text)
