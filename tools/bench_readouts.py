#!/usr/bin/env python3
"""Cost of the bird view's readouts on the device (csrc/overlay_readout.hip), stand-alone and inside the fused step:
    python tools/bench_readouts.py [--streams 64] [--steps 30] [--rounds 5] [--iters 50]
(a) stand-alone: the bird stage (LaneOverlay.run_arrays, discs of radius 10 on four lanes of 72 points) on --streams bird images of 1280x720,
    in place, with the readouts off and on (a synthetic font of 24 rows per cell at zoom 2: the repository ships no font; every frame passes
    the gate), and the readouts alone -- timed with the library's events on the null stream against hipMemcpyAsync device-to-device of the
    same bytes, in alternation.  `on` is the layout launch and the draw launch ahead of the stage's mark + apply.
(b) fused step: two pipelines of the same two networks in the default (exact) precision, tracker, bird-view image, analysis and the overlay's
    seven stages in ONE process, stepped from the same camera frames in alternation: `off` without the readouts, `on` with them.  A window is
    --steps steps between two host clock readings with the pipeline drained at both ends; median window of --rounds, fastest and slowest.
(c) with --parent-tree DIR (a checkout of the parent commit, its library built): the `off` step of (b) in processes of their own, the parent's
    tree and this one in alternation (tools/bench_text_step.py, which both trees hold) -- whether the stage off stays inside the parent's spread.
Writes profiles/r07/readouts_ab.txt (or --out)."""
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
import bench
import readout_ref as RR

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--precision", default=None)
ap.add_argument("--box-score", type=float, default=0.1)
ap.add_argument("--standalone-only", action="store_true", help="(a) alone, e.g. under a kernel trace")
ap.add_argument("--parent-tree", default=None, metavar="DIR", help="(c): a checkout of the parent commit with its library built")
ap.add_argument("--parent-rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "readouts_ab.txt"))
a = ap.parse_args()
if L.lib().adas_device_count() <= 0:
    raise SystemExit("bench_readouts.py needs an MI355X: there is no CPU fallback and no CPU timing")
S, H, W, IMG = a.streams, 720, 1280, (1280, 720)
SLOT = 10
hip = C.CDLL("libamdhip64.so")      # already in the process: libadas_hip.so links it
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
D2D = 3                             # hipMemcpyDeviceToDevice


def median(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


# ------------------------------------------------------------------------------------------------ (a) stand-alone
font = RR.synthetic_font(seed=5, cell_h=24, baseline_row=18)
birds = bench.cam_frames(S, 900)
nbytes = birds.nbytes
work_buf = L.DeviceBuffer.from_array(birds)        # drawn in place: on a buffer of its own
copy_src, copy_dst = L.DeviceBuffer.from_array(birds), L.DeviceBuffer(nbytes)
timer = L.StreamTimer()
rng = np.random.default_rng(1)
pts, cnt = np.zeros((S, 4, L.UFLD_MAX_POINTS, 2), np.int32), np.full((S, 4), 72, np.int32)
for q in range(S):
    for l in range(4):
        pts[q, l, :72, 1] = np.arange(0, 720, 10)
        pts[q, l, :72, 0] = 200 + 290 * l + rng.integers(-20, 21, 72)
d_pts, d_cnt = L.DeviceBuffer.from_array(pts), L.DeviceBuffer.from_array(cnt)
d_dir = L.DeviceBuffer.from_array(np.full(S, 3, np.int32))
d_veh = L.DeviceBuffer.from_array(rng.uniform(400, 880, S))
d_cur = L.DeviceBuffer.from_array(rng.uniform(100, 5000, S))
d_off = L.DeviceBuffer.from_array(rng.uniform(-1.5, 1.5, S))
ov = PP.LaneOverlay((8, 8), (H, W), S)
ov.set_fonts({SLOT: font})
ov.set_readout_style(slot=SLOT, zoom=2)
ro = (d_dir.ptr, d_veh.ptr, d_cur.ptr, d_off.ptr)
run = lambda stages: ov.run_arrays(None, S, bird_points=d_pts.ptr, bird_counts=d_cnt.ptr, bird_ptr=work_buf.ptr, stages=stages, readouts=ro)


def timed(fn):
    with timer:
        for _ in range(a.iters):
            fn()
    return timer.ms / a.iters * 1e3      # us per call


variants = [("copy", lambda: hip.hipMemcpyAsync(copy_dst.ptr, copy_src.ptr, nbytes, D2D, None)), ("bird stage, readouts off", lambda: run(L.OVERLAY_BIRD)),
            ("bird stage, readouts on", lambda: run(L.OVERLAY_BIRD | L.OVERLAY_READOUTS)), ("readouts alone", lambda: run(L.OVERLAY_READOUTS))]
for _, fn in variants:                     # warm-up
    fn()
L.check(L.lib().adas_synchronize())
us = {n: [] for n, _ in variants}
for _ in range(a.rounds):
    for n, fn in variants:
        us[n].append(timed(fn))
run(L.OVERLAY_READOUTS)
L.check(L.lib().adas_synchronize())
recs = [ov.readout_record(q) for q in range(S)]
box_px = sum(sum((s["box"][2] - s["box"][0]) * (s["box"][3] - s["box"][1]) for s in r["strings"]) for r in recs) / S
cm = median(us["copy"])[0]
lines = ["tools/bench_readouts.py on one MI355X (gfx950).", "",
         "(a) stand-alone, %d bird images of 1280x720 (%.1f MB; the copy reads and writes all of it), %d rounds of %d calls between two events on the"
         % (S, nbytes / 1e6, a.rounds, a.iters),
         "    null stream, alternated in one process; us per call, median round (fastest, slowest).  The bird stage is mark + apply over 4 x 72 discs",
         "    of radius 10; the readouts are a layout launch and a draw launch (two arrows, two strings of %.0f pixels of box per frame, zoom 2)." % box_px, ""]
for n, _ in variants:
    m, lo, hi = median(us[n])
    lines.append("    %-26s %9.1f us  (%.1f, %.1f)  %.3f x the copy" % (n, m, lo, hi, m / cm))
off_m, on_m, alone_m = (median(us[k])[0] for k in ("bird stage, readouts off", "bird stage, readouts on", "readouts alone"))
lines += ["", "    on - off = %+.1f us per call (%.1f us per frame); the readouts alone take %.1f us, %.2f x the bird stage's mark + apply." %
          (on_m - off_m, (on_m - off_m) / S, alone_m, alone_m / off_m)]
for b in (work_buf, copy_src, copy_dst, d_pts, d_cnt, d_dir, d_veh, d_cur, d_off):
    b.free()
ov.close()
timer.close()

if a.standalone_only:
    print("\n".join(lines))
    raise SystemExit(0)

# ------------------------------------------------------------------------------------------------ (b) fused step
import bench_text_step as BS    # noqa: E402  (the step's configuration, shared with the parent-tree alternation)

P = dict(_lib=L, coreEngine=CE, pipeline=PL, models=M, analysis=A)
det_path, lane_path = BS.models(P, tempfile.mkdtemp(prefix="ro_bench_"))
pkw = BS.pipeline_kw(P, S, a.precision, a.box_score)
ovl = BS.OVERLAY
on = dict(ovl, stages=tuple(ovl["stages"]) + ("readouts",), fonts={SLOT: font}, readout=dict(slot=SLOT, zoom=2))
cam = [L.DeviceBuffer.from_array(bench.cam_frames(S, 900 + i)) for i in range(2)]
pipes = [("off", PL.AdasPipeline(det_path, lane_path, overlay=dict(ovl), **pkw)), ("on", PL.AdasPipeline(det_path, lane_path, overlay=on, **pkw))]
counts = {n: [0] for n, _ in pipes}
for name, p in pipes:                      # warm-up: capture, first-launch costs
    BS.window(p, cam, counts[name], 5)
ms = {n: [] for n, _ in pipes}
for _ in range(a.rounds):
    for name, p in pipes:
        ms[name].append(BS.window(p, cam, counts[name], a.steps))
kernels = {name: p.graph_kernels() for name, p in pipes}
drawn = sum(pipes[1][1].overlay.readout_record(s)["drawn"] for s in range(S))
lines += ["", "(b) fused step (yolov8n + ufldv2_res18, %s, hipGraph, two branches, tracker, bird-view image, analysis, seven overlay stages), %d streams"
          % (pipes[0][1].lane.precision, S),
          "    of 1280x720 from camera frames, %d windows of %d steps per variant, alternated in one process; ms per step, median window (fastest,"
          % (a.rounds, a.steps), "    slowest).  `on` drew the readouts on %d of %d bird images in its last step." % (drawn, S), ""]
med = {}
for name, _ in pipes:
    med[name], lo, hi = median(ms[name])
    lines.append("    %-4s %8.3f ms per step  (%.3f, %.3f)   %d kernels in the captured step" % (name, med[name], lo, hi, kernels[name]))
lines += ["", "    on - off = %+8.1f us per step (two plain launches inside the capture: the layout and the draw)." % ((med["on"] - med["off"]) * 1e3)]
for _, p in pipes:
    p.close()
for b in cam:
    b.free()

# ------------------------------------------------------------------------------------------------ (c) the parent commit, the stage off
if a.parent_tree:
    import json, subprocess
    a.parent_tree = os.path.abspath(a.parent_tree)
    trees = [("parent", a.parent_tree), ("this", ROOT)]
    got = {n: [] for n, _ in trees}
    kern = {}
    for _ in range(a.parent_rounds):
        for n, tree in trees:             # a process each, in alternation
            r = subprocess.run([sys.executable, os.path.join(tree, "tools", "bench_text_step.py"), "--streams", str(S), "--steps", str(a.steps)],
                               capture_output=True, text=True, cwd=tree, env={k: v for k, v in os.environ.items() if k != "ADAS_LIB"})
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode or not line:
                raise SystemExit("%s: bench_text_step.py failed (rc %d): %s" % (n, r.returncode, r.stderr.strip().splitlines()[-3:]))
            d = json.loads(line[-1])
            got[n] += d["ms_per_step"]
            kern[n] = d["kernels"]
    lines += ["", "(c) the same step with the readouts off, the parent commit against this one: %d processes of each tree in alternation in this job, 3"
              % a.parent_rounds, "    windows of %d steps per process; ms per step, median window (fastest, slowest)." % a.steps, ""]
    for n, _ in trees:
        m, lo, hi = median(got[n])
        lines.append("    %-6s %8.3f ms per step  (%.3f, %.3f)   %d kernels in the captured step" % (n, m, lo, hi, kern[n]))
    pm, plo, phi = median(got["parent"])
    tm = median(got["this"])[0]
    inside = plo <= tm <= phi
    lines += ["", "    this - parent = %+.1f us per step; the parent's own windows span %.1f us (%.3f .. %.3f ms): this tree's median lies %s that span."
              % ((tm - pm) * 1e3, (phi - plo) * 1e3, plo, phi, "inside" if inside else "OUTSIDE")]
out = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, "w").write(out)
print(out)
