#!/usr/bin/env python3
"""Cost of the overlay's text on the device (csrc/overlay_text.hip), stand-alone and inside the fused step:
    python tools/bench_text.py [--streams 64] [--steps 30] [--rounds 5] [--iters 50]
(a) stand-alone: LaneOverlay.run_text_arrays on --streams frames of 1280x720, in place, with synthetic fonts of about 20 rows per cell
    (tests/text_scene.py: the repository ships no font): 24 detections, 16 tracks with ids, 8 distance texts, the three panel strings and 2
    caller lines per frame -- and the same scene with a quarter of the items -- timed with the library's events on the null stream against
    hipMemcpyAsync device-to-device of the same frames, in alternation.  A call is the layout launch and the draw launch together: the tool
    does not time them apart; `rocprofv3 --kernel-trace --stats -- python tools/bench_text.py --standalone-only` does (profiles/r07).  The call is also given per megapixel
    of item box.
(b) fused step: two pipelines of the same two networks in the default (exact) precision, tracker, bird-view image, analysis and the overlay's
    stages in ONE process, stepped from the same camera frames in alternation: `off` without text, `on` with every kind.  A window is
    --steps steps between two host clock readings with the pipeline drained at both ends; median window of --rounds, fastest and slowest.
(c) with --parent-tree DIR (a checkout of the parent commit, its library built): the `off` step of (b) in processes of their own, the parent's
    tree and this one in alternation (tools/bench_text_step.py, copied into DIR/tools) -- whether text off stays inside the parent's spread.
Writes profiles/r07/overlay_text_ab.txt (or --out)."""
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
import text_scene as TS

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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "overlay_text_ab.txt"))
a = ap.parse_args()
if L.lib().adas_device_count() <= 0:
    raise SystemExit("bench_text.py needs an MI355X: there is no CPU fallback and no CPU timing")
S, H, W, IMG = a.streams, 720, 1280, (1280, 720)
hip = C.CDLL("libamdhip64.so")      # already in the process: libadas_hip.so links it
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
D2D = 3                             # hipMemcpyDeviceToDevice


def median(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def bench_fonts():
    """The slots of the default style and two for the lines, cells of 18 .. 22 rows."""
    f = {k: TS.make_font(k, k % 2 == 0, cell_h=18 + k % 5, scale=(1.0, 0.75, 6e-4, 1.0, 1.0, 1.0, 1.0, 1.0, 0.7, 0.6)[k]) for k in range(10)}
    f[TS.LINE_SLOT], f[TS.LINE_SLOT_BINARY] = TS.make_font(31, False, cell_h=20), TS.make_font(32, True, cell_h=20)
    return f


# ------------------------------------------------------------------------------------------------ (a) stand-alone
fonts = bench_fonts()
cams = [bench.cam_frames(S, 900 + i) for i in range(2)]
cam = [L.DeviceBuffer.from_array(c) for c in cams]
nbytes = cams[0].nbytes
work_buf = L.DeviceBuffer.from_array(cams[0])      # the text draws in place: on a buffer of its own
copy_dst = L.DeviceBuffer(nbytes)
timer = L.StreamTimer()


def scene(q, n_det, n_trk, n_dist):
    s = TS.scene_full(W, H, seed=q, n_det=n_det, n_trk=n_trk, n_dist=n_dist)[0]
    s["dist_d"] = np.random.default_rng(q).uniform(0.3, 60, n_dist)      # every distance prints a number
    s["traj_len"][:] = 5                                                 # every track over the area gate prints its id
    return s


def setup(n_det, n_trk, n_dist, lines):
    scenes = [scene(q, n_det, n_trk, n_dist) for q in range(S)]
    arrays, caps = TS.pack_scenes(scenes)
    bufs = {k: L.DeviceBuffer.from_array(v) for k, v in arrays.items()}
    ov = PP.LaneOverlay((H, W), None, S)
    ov.set_fonts(fonts)
    ov.set_class_colors("detections", TS.COLORS); ov.set_class_colors("tracks", TS.COLORS)
    ov.set_text_labels("detections", TS.NAMES); ov.set_text_labels("tracks", TS.NAMES)
    ov.set_text_lines(scenes[0]["lines"][:lines])
    run = lambda mask=63: ov.run_text_arrays(work_buf.ptr, mask, S, 1, None, caps[0], caps[1], caps[2], **{k: b.ptr for k, b in bufs.items()})
    return ov, bufs, run


def timed(fn):
    with timer:
        for _ in range(a.iters):
            fn()
    return timer.ms / a.iters * 1e3      # us per call


full = setup(24, 16, 8, 2)
quarter = setup(6, 4, 2, 1)
variants = [("copy", lambda: hip.hipMemcpyAsync(copy_dst.ptr, cam[0].ptr, nbytes, D2D, None)), ("text, full scene", full[2]), ("text, quarter scene", quarter[2])]
for _, fn in variants:                     # warm-up
    fn()
L.check(L.lib().adas_synchronize())
us = {n: [] for n, _ in variants}
for _ in range(a.rounds):
    for n, fn in variants:
        us[n].append(timed(fn))
area, count = {}, {}
for name, (ov, bufs, run) in (("full", full), ("quarter", quarter)):
    run()
    L.check(L.lib().adas_synchronize())
    items = [ov.text_items(q) for q in range(S)]
    count[name] = sum(len(i) for i in items) / S
    area[name] = sum(int((i["box"][:, 2] - i["box"][:, 0]).astype(np.int64) @ (i["box"][:, 3] - i["box"][:, 1]).astype(np.int64)) for i in items) / 1e6
cm = median(us["copy"])[0]
lines = ["tools/bench_text.py on one MI355X (gfx950).", "",
         "(a) stand-alone, %d frames of 1280x720 (%.1f MB; the copy reads and writes all of it), %d rounds of %d calls between two events on the null"
         % (S, nbytes / 1e6, a.rounds, a.iters),
         "    stream, alternated in one process; us per call (layout launch + draw launch), median round (fastest, slowest).",
         "    full scene: %.1f items per frame, %.2f megapixels of item box over the %d frames; quarter scene: %.1f items, %.2f megapixels." %
         (count["full"], area["full"], S, count["quarter"], area["quarter"]), ""]
for n, _ in variants:
    m, lo, hi = median(us[n])
    lines.append("    %-20s %9.1f us  (%.1f, %.1f)  %.2f x the copy" % (n, m, lo, hi, m / cm))
fm, qm = median(us["text, full scene"])[0], median(us["text, quarter scene"])[0]
lines += ["", "    full / quarter = %.2f in time, %.2f in box area, %.2f in items (were the time to follow the box area alone the first two would be equal);"
          % (fm / qm, area["full"] / area["quarter"], count["full"] / count["quarter"]),
          "    full scene: %.1f us per megapixel of item box, both launches." % (fm / area["full"])]
for ov, bufs, _ in (full, quarter):
    for b in bufs.values():
        b.free()
    ov.close()
for b in (work_buf, copy_dst):
    b.free()
timer.close()

if a.standalone_only:
    for b in cam:
        b.free()
    print("\n".join(lines))
    raise SystemExit(0)

# ------------------------------------------------------------------------------------------------ (b) fused step

import bench_text_step as BS    # noqa: E402  (the step's configuration, shared with the parent-tree alternation)

P = dict(_lib=L, coreEngine=CE, pipeline=PL, models=M, analysis=A)
det_path, lane_path = BS.models(P, tempfile.mkdtemp(prefix="txt_bench_"))
pkw = BS.pipeline_kw(P, S, a.precision, a.box_score)
names, colors, ovl = BS.NAMES, BS.COLORS, BS.OVERLAY
text = dict(text=("detections", "tracks", "track_ids", "distance", "panels", "lines"), fonts=fonts, detection_names=names, track_names=names,
            text_lines=[(10, 345, TS.LINE_SLOT, (255, 255, 255), "FPS  : 31.42"), (900, 300, TS.LINE_SLOT_BINARY, (230, 230, 230), "object-infer : 0.01 s")])
pipes = [("off", PL.AdasPipeline(det_path, lane_path, overlay=dict(ovl), **pkw)), ("on", PL.AdasPipeline(det_path, lane_path, overlay=dict(ovl, **text), **pkw))]
steps = {n: 0 for n, _ in pipes}


def window(name, p, n):
    p.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        i = steps[name]
        steps[name] += 1
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
on_items = sum(len(pipes[1][1].overlay.text_items(s)) for s in range(S)) / S
lines += ["", "(b) fused step (yolov8n + ufldv2_res18, %s, hipGraph, two branches, tracker, bird-view image, analysis, seven overlay stages), %d streams"
          % (pipes[0][1].lane.precision, S),
          "    of 1280x720 from camera frames, %d windows of %d steps per variant, alternated in one process; ms per step, median window (fastest,"
          % (a.rounds, a.steps), "    slowest).  `on` placed %.1f items per frame in its last step." % on_items, ""]
med = {}
for name, _ in pipes:
    med[name], lo, hi = median(ms[name])
    lines.append("    %-4s %8.3f ms per step  (%.3f, %.3f)   %d kernels in the captured step" % (name, med[name], lo, hi, kernels[name]))
lines += ["", "    on - off = %+8.1f us per step (three plain launches inside the capture: the layout and two draws)." % ((med["on"] - med["off"]) * 1e3)]
for _, p in pipes:
    p.close()
for b in cam:
    b.free()

# ------------------------------------------------------------------------------------------------ (c) the parent commit, text off
if a.parent_tree:
    import json, shutil, subprocess
    a.parent_tree = os.path.abspath(a.parent_tree)
    shutil.copy(os.path.join(ROOT, "tools", "bench_text_step.py"), os.path.join(a.parent_tree, "tools", "bench_text_step.py"))
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
    lines += ["", "(c) the same step with text off, the parent commit against this one: %d processes of each tree in alternation in this job, 3 windows"
              % a.parent_rounds, "    of %d steps per process; ms per step, median window (fastest, slowest)." % a.steps, ""]
    for n, _ in trees:
        m, lo, hi = median(got[n])
        lines.append("    %-6s %8.3f ms per step  (%.3f, %.3f)   %d kernels in the captured step" % (n, m, lo, hi, kern[n]))
    pm, plo, phi = median(got["parent"])
    tm = median(got["this"])[0]
    lines += ["", "    this - parent = %+.1f us per step; the parent's own windows span %.1f us." % ((tm - pm) * 1e3, (phi - plo) * 1e3)]
out = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, "w").write(out)
print(out)
