#!/usr/bin/env python3
"""Cost of the rectification stage on the device (csrc/remap_kernels.hip) and of the stage in front of the fused step:
    python tools/bench_remap.py [--streams 64] [--rounds 5] [--iters 300] [--sections stage,step] [--parent-tree DIR]
--streams frames of 1280x720 (8 distinct synthetic camera frames, repeated) as BGR on the device.
(a) stage    device to device: FrameRemapper.run with one map shared by every stream and with a map per stream, each with the identity map
             and with a real lens, each in both forms of the remap kernel -- `direct` (gathers through L1 / L2, what a run takes) and
             `staged` (a workgroup's source box through LDS, ADAS_REMAP_STAGED=1) -- timed with the library's events on the null stream against hipMemcpyAsync device-to-device of the same
             BGR frames between the same events, in alternation.  The copy is the yardstick: its rate applied to each case's bytes -- twice
             the copy's with a map per stream (3 B read, 3 B written and 6 B of map per pixel), the copy's plus one 5.5 MB map with a
             shared one.  Also the build kernel: set_camera of one map, launch and wait included.
(b) step     the fused step of tools/bench_text_step.py (both networks in the default precision, tracker, bird-view image, analysis, seven
             overlay stages) with undistort off and on (a map per stream), two pipelines stepped in alternation in ONE process, between
             host clock readings so that the stage in front of the captured step counts.  With --parent-tree DIR (a checkout of the parent
             commit, its library built): the `off` step in processes of their own, the parent's tree and this one in alternation
             (tools/bench_text_step.py in each) -- whether the stage unset stays inside the parent's spread.
us per call, median round (fastest, slowest).  Writes profiles/r08/remap.txt (or --out)."""
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
ap.add_argument("--iters", type=int, default=300)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--sections", default="stage,step")
ap.add_argument("--precision", default=None)
ap.add_argument("--box-score", type=float, default=0.1)
ap.add_argument("--parent-tree", default=None, metavar="DIR", help="(b): a checkout of the parent commit with its library built")
ap.add_argument("--parent-rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "remap.txt"))
a = ap.parse_args()
if L.lib().adas_device_count() <= 0:
    raise SystemExit("bench_remap.py needs an MI355X: there is no CPU fallback and no CPU timing")
S, H, W = a.streams, 720, 1280
sections = a.sections.split(",")
hip = C.CDLL("libamdhip64.so")      # already in the process: libadas_hip.so links it
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
D2D = 3
K = (900.0, 900.0, 639.5, 359.5)
LENS = (-0.25, 0.08, 0.0005, -0.0005)       # a wide-angle barrel: the corners move by up to 85 pixels


def camera(s, lens):
    """stream s's camera: its own centre, so that no two maps are equal"""
    return dict(K=K[:2] + (K[2] + 0.25 * s, K[3]), D=lens)


def median(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def note(msg):
    print("bench_remap: " + msg, file=sys.stderr, flush=True)


MAP_BYTES = H * W * 6
lines = []

if "stage" in sections:
    distinct = min(S, 8)
    cams = bench.cam_frames(distinct, 900)
    bgr = np.stack([cams[f % distinct] for f in range(S)])
    nbytes = bgr.nbytes
    d_bgr = L.DeviceBuffer.from_array(bgr)
    copy_dst = L.DeviceBuffer(nbytes)
    timer = L.StreamTimer()

    def timed(fn, iters=a.iters):
        with timer:
            for _ in range(iters):
                fn()
        return timer.ms / iters * 1e3

    rm = {}
    for maps, n_maps in (("one shared map", 1), ("a map per stream", S)):
        for lens_name, lens in (("identity", ()), ("lens", LENS)):
            rm[maps, lens_name] = PP.FrameRemapper((H, W), S, cameras=[camera(s if lens else 0, lens) for s in range(n_maps)])
    moved = np.abs(rm["one shared map", "lens"].fetch_map(0)[0].astype(int) - np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1)).max()
    fns = {"copy d2d": lambda: hip.hipMemcpyAsync(copy_dst.ptr, d_bgr.ptr, nbytes, D2D, None)}
    FORMS = ("staged", "direct")

    def form(name):
        os.environ["ADAS_REMAP_STAGED"] = "1" if name == "staged" else "0"      # read by the library at every run

    for key in rm:
        for fm in FORMS:
            fns["%s, %s, %s" % (key + (fm,))] = (lambda k, m: lambda: rm[k].run(d_bgr.ptr, S))(key, fm)
    us = {n: [] for n in fns}
    for n, fn in fns.items():
        form(n.rsplit(", ", 1)[-1])
        fn()
    for r in range(a.rounds):
        for n, fn in fns.items():
            form(n.rsplit(", ", 1)[-1])
            us[n].append(timed(fn))
        note("stage: round %d of %d" % (r + 1, a.rounds))
    form("direct")
    build_us = [timed(lambda: rm["one shared map", "lens"].set_camera(0, **camera(0, LENS)), 10) for _ in range(a.rounds)]
    bm, blo, bhi = median(us["copy d2d"])
    lines += ["tools/bench_remap.py on one MI355X (gfx950).", "",
              "%d frames of 1280x720 (%d distinct synthetic camera frames, repeated): %.1f MB as BGR; a map is %.1f MB.  The lens is K = %s," % (
                  S, distinct, nbytes / 1e6, MAP_BYTES / 1e6, K), "D = %s: an entry moves by up to %d pixels.  With a map per stream every stream has its own centre." % (LENS, moved),
              "%d rounds of %d calls, alternated in one process; us per call, median round (fastest, slowest)." % (a.rounds, a.iters), "",
              "(a) device to device, between two events on the null stream (the copy reads and writes %.1f MB):" % (nbytes / 1e6)]
    for n, v in us.items():
        m, lo, hi = median(v)
        lines.append("    %-44s %10.1f us  (%.1f, %.1f)  %5.2f x copy d2d   %.0f frames/s" % (n, m, lo, hi, m / bm, S / m * 1e6))
    lines.append("    expectation: the copy's rate (median %.1f us for %.1f MB moved) applied to each case's bytes." % (bm, 2 * nbytes / 1e6))
    for key in rm:
        n_maps = 1 if key[0] == "one shared map" else S
        want = bm * (2 * nbytes + n_maps * MAP_BYTES) / (2 * nbytes)
        for fm in FORMS:
            m = median(us["%s, %s, %s" % (key + (fm,))])[0]
            lines.append("    %s, %s, %s: expected %.1f us; %s" % (key + (fm, want, "met (%.2f x)" % (m / want) if m <= want else "MISSED by %.2f x" % (m / want))))
    m, lo, hi = median(build_us)
    lines.append("    build kernel, one 1280x720 map (set_camera: launch and wait included): %.1f us  (%.1f, %.1f)" % (m, lo, hi))
    for o in list(rm.values()) + [timer]:
        o.close()
    for b in (d_bgr, copy_dst):
        b.free()

if "step" in sections:
    import bench_text_step as BS
    PL = importlib.import_module("adas_amd.pipeline")
    P = {n: importlib.import_module("adas_amd." + n) for n in ("_lib", "coreEngine", "pipeline", "models", "analysis")}
    cam = [L.DeviceBuffer.from_array(bench.cam_frames(S, 900 + i)) for i in range(2)]
    det_path, lane_path = BS.models(P, tempfile.mkdtemp(prefix="remap_bench_"))
    pkw = BS.pipeline_kw(P, S, a.precision, a.box_score)
    pipes = [("off", PL.AdasPipeline(det_path, lane_path, overlay=dict(BS.OVERLAY), **pkw)),
             ("on", PL.AdasPipeline(det_path, lane_path, overlay=dict(BS.OVERLAY), undistort=dict(cameras=[camera(s, LENS) for s in range(S)]), **pkw))]
    counts = {n: [0] for n, _ in pipes}
    for name, p in pipes:                      # warm-up: capture, first-launch costs
        BS.window(p, cam, counts[name], 5)
    ms = {n: [] for n, _ in pipes}
    note("step: both pipelines built")
    for r in range(a.rounds):
        for name, p in pipes:
            ms[name].append(BS.window(p, cam, counts[name], a.steps))
        note("step: round %d of %d" % (r + 1, a.rounds))
    kernels = {name: p.graph_kernels() for name, p in pipes}
    lines += ["", "(b) fused step (yolov8n + ufldv2_res18, %s, hipGraph, two branches, tracker, bird-view image, analysis, seven overlay stages), %d streams"
              % (pipes[0][1].lane.precision, S),
              "    of 1280x720 from camera frames, %d windows of %d steps per variant, alternated in one process; ms per step, median window (fastest,"
              % (a.rounds, a.steps), "    slowest).  `on`: undistort=dict(cameras=[a lens per stream]), %d maps." % pipes[1][1].remapper.n_maps, ""]
    med = {}
    for name, _ in pipes:
        med[name], lo, hi = median(ms[name])
        lines.append("    %-4s %8.3f ms per step  (%.3f, %.3f)   %d kernels in the captured step" % (name, med[name], lo, hi, kernels[name]))
    lines += ["", "    on - off = %+8.1f us per step (one launch in front of the captured step)." % ((med["on"] - med["off"]) * 1e3)]
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
                note("parent alternation: %s done" % n)
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
