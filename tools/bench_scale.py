#!/usr/bin/env python3
"""Cost of the scaling stage on the device (csrc/scale_kernels.hip) and of the stage inside the fused step:
    python tools/bench_scale.py [--streams 64] [--rounds 5] [--iters 50] [--sections scale,step] [--parent-tree DIR]
--streams frames of 1280x720 (8 distinct synthetic camera frames, repeated) as BGR on the device.
(a) scale    device to device: FrameScaler.run_device in both modes for a 640x360 reduction per frame and for an 8x8 mosaic of 160x90 tiles,
             timed with the library's events on the null stream against hipMemcpyAsync device-to-device of the same BGR frames between the
             same events, in alternation.  The copy is the yardstick: it reads the bytes a run reads and writes four times as many as the
             largest of these runs writes.
(b) step     the fused step of tools/bench_text_step.py (both networks in the default precision, tracker, bird-view image, analysis, seven
             overlay stages) with scale off and on (the 8x8 mosaic of the drawn frames with a border of 2, its JPEG and its I420), two
             pipelines stepped in alternation in ONE process.  With --parent-tree DIR (a checkout of the parent commit, its library
             built): the `off` step in processes of their own, the parent's tree and this one in alternation (tools/bench_text_step.py in
             each) -- whether the stage unset stays inside the parent's spread.
us per call, median round (fastest, slowest).  Writes profiles/r08/scale.txt (or --out)."""
import argparse, ctypes as C, importlib, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from conftest import load_pkg
load_pkg()
L = importlib.import_module("adas_amd._lib")
PP = importlib.import_module("adas_amd.postproc")
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--sections", default="scale,step")
ap.add_argument("--precision", default=None)
ap.add_argument("--box-score", type=float, default=0.1)
ap.add_argument("--parent-tree", default=None, metavar="DIR", help="(b): a checkout of the parent commit with its library built")
ap.add_argument("--parent-rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "scale.txt"))
a = ap.parse_args()
if L.lib().adas_device_count() <= 0:
    raise SystemExit("bench_scale.py needs an MI355X: there is no CPU fallback and no CPU timing")
S, H, W = a.streams, 720, 1280
sections = a.sections.split(",")
hip = C.CDLL("libamdhip64.so")      # already in the process: libadas_hip.so links it
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
D2D = 3
CASES = (("640x360 per frame", (640, 360), (1, 1)), ("8x8 mosaic of 160x90", (160, 90), (8, 8)))
MODES = ("area", "linear")


def median(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


distinct = min(S, 8)
cams = bench.cam_frames(distinct, 900)
bgr = np.stack([cams[f % distinct] for f in range(S)])
nbytes = bgr.nbytes
d_bgr = L.DeviceBuffer.from_array(bgr)
copy_dst = L.DeviceBuffer(nbytes)
sc = {(name, mode): PP.FrameScaler((W, H), size, mode, mosaic, max_batch=S) for name, size, mosaic in CASES for mode in MODES}
timer = L.StreamTimer()


def timed(fn):
    with timer:
        for _ in range(a.iters):
            fn()
    return timer.ms / a.iters * 1e3


lines = ["tools/bench_scale.py on one MI355X (gfx950).", "",
         "%d frames of 1280x720 (%d distinct synthetic camera frames, repeated): %.1f MB as BGR; %s."
         % (S, distinct, nbytes / 1e6, ", ".join("%s: %.1f MB of canvases" % (n, sc[n, "area"].canvases(S) * sc[n, "area"].canvas_bytes / 1e6) for n, _, _ in CASES)),
         "%d rounds of %d calls, alternated in one process; us per call, median round (fastest, slowest)." % (a.rounds, a.iters)]

if "scale" in sections:
    fns = {"copy d2d": lambda: hip.hipMemcpyAsync(copy_dst.ptr, d_bgr.ptr, nbytes, D2D, None)}
    for key in sc:
        fns["%s, %s" % key] = (lambda k: lambda: sc[k].run_device(d_bgr.ptr, S))(key)
    us = {n: [] for n in fns}
    for fn in fns.values():
        fn()
    for _ in range(a.rounds):
        for n, fn in fns.items():
            us[n].append(timed(fn))
    bm, _, chi = median(us["copy d2d"])
    lines += ["", "(a) device to device, between two events on the null stream (the copy reads and writes %.1f MB):" % (nbytes / 1e6)]
    for n, v in us.items():
        m, lo, hi = median(v)
        lines.append("    %-32s %10.1f us  (%.1f, %.1f)  %5.2f x copy d2d   %.0f frames/s" % (n, m, lo, hi, m / bm, S / m * 1e6))
    lines.append("    expectation: each case no slower than the copy (median %.1f us, slowest round %.1f us)." % (bm, chi))
    for key in sc:
        m = median(us["%s, %s" % key])[0]
        lines.append("    %s, %s: %s" % (key + ("met (%.2f x)" % (m / bm) if m <= bm else "MISSED by %.1f us (%.2f x)" % (m - bm, m / bm),)))

for o in list(sc.values()) + [timer]:
    o.close()
for b in (d_bgr, copy_dst):
    b.free()

if "step" in sections:
    import bench_text_step as BS
    PL = importlib.import_module("adas_amd.pipeline")
    P = {n: importlib.import_module("adas_amd." + n) for n in ("_lib", "coreEngine", "pipeline", "models", "analysis")}
    cam = [L.DeviceBuffer.from_array(bench.cam_frames(S, 900 + i)) for i in range(2)]
    det_path, lane_path = BS.models(P, tempfile.mkdtemp(prefix="scale_bench_"))
    pkw = BS.pipeline_kw(P, S, a.precision, a.box_score)
    wall = dict(size=(160, 90), mosaic=(8, 8), border=2, jpeg=dict(quality=80), yuv=dict(format="i420"))
    pipes = [("off", PL.AdasPipeline(det_path, lane_path, overlay=dict(BS.OVERLAY), **pkw)),
             ("on", PL.AdasPipeline(det_path, lane_path, overlay=dict(BS.OVERLAY), scale=wall, **pkw))]
    counts = {n: [0] for n, _ in pipes}
    for name, p in pipes:                      # warm-up: capture, first-launch costs
        BS.window(p, cam, counts[name], 5)
    ms = {n: [] for n, _ in pipes}
    for _ in range(a.rounds):
        for name, p in pipes:
            ms[name].append(BS.window(p, cam, counts[name], a.steps))
    kernels = {name: p.graph_kernels() for name, p in pipes}
    lines += ["", "(b) fused step (yolov8n + ufldv2_res18, %s, hipGraph, two branches, tracker, bird-view image, analysis, seven overlay stages), %d streams"
              % (pipes[0][1].lane.precision, S),
              "    of 1280x720 from camera frames, %d windows of %d steps per variant, alternated in one process; ms per step, median window (fastest,"
              % (a.rounds, a.steps), "    slowest).  `on`: scale=dict(size=(160, 90), mosaic=(8, 8), border=2, jpeg=dict(quality=80), yuv=dict(format=\"i420\")).", ""]
    med = {}
    for name, _ in pipes:
        med[name], lo, hi = median(ms[name])
        lines.append("    %-4s %8.3f ms per step  (%.3f, %.3f)   %d kernels in the captured step" % (name, med[name], lo, hi, kernels[name]))
    lines += ["", "    on - off = %+8.1f us per step (the stage's launch, three of its JPEG encoder, one of its YUV writer)." % ((med["on"] - med["off"]) * 1e3)]
    for _, p in pipes:
        p.close()
    for b in cam:
        b.free()
    if a.parent_tree:
        import json, subprocess
        trees = [("parent", os.path.abspath(a.parent_tree)), ("this", ROOT)]
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
        lines += ["", "(b') the same step with the stage off, the parent commit against this one: %d processes of each tree in alternation in this job, 3"
                  % a.parent_rounds, "    windows of %d steps per process; ms per step, median window (fastest, slowest)." % a.steps, ""]
        for n, _ in trees:
            m, lo, hi = median(got[n])
            lines.append("    %-6s %8.3f ms per step  (%.3f, %.3f)   %d kernels in the captured step" % (n, m, lo, hi, kern[n]))
        pm, plo, phi = median(got["parent"])
        tm = median(got["this"])[0]
        lines += ["", "    this - parent = %+.1f us per step; the parent's own windows span %.1f us (%s the parent's spread)."
                  % ((tm - pm) * 1e3, (phi - plo) * 1e3, "inside" if plo <= tm <= phi else "OUTSIDE")]

text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, "w").write(text)
print(text)
