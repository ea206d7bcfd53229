#!/usr/bin/env python3
"""Cost of the baseline JPEG encoder on the device (csrc/jpeg_kernels.hip), stand-alone and as the last stage of the fused step:
    python tools/bench_jpeg.py [--streams 64] [--steps 30] [--rounds 5] [--iters 50]
(a) stand-alone: JpegEncoder.run on --streams synthetic camera frames of 1280x720 at quality 75 and 90, timed with the library's events on
    the null stream against hipMemcpyAsync device-to-device of the same frames between the same events, in alternation.  The copy is the
    yardstick: it reads and writes every frame byte once; the encoder reads them once, writes and reads the int16 level arena (1.5 levels
    per pixel: as many bytes as the frame, each way) and writes the streams -- about 1.6 x the copy's bytes.
(b) fused step: two pipelines of the same two networks in the default (exact) precision with the lane overlay in ONE process, stepped from
    the same camera frames in alternation: `off` without the stage, `on` with jpeg=dict(quality=90) on the overlay's frames.  A window is
    --steps steps between two host clock readings with the pipeline drained at both ends; median window of --rounds, with the fastest and
    the slowest.  Then the host's wall time to fetch every frame of a step: --streams jpeg(f) calls against --streams overlay_image(f).
Writes profiles/r07/jpeg_ab.txt (or --out)."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--precision", default=None)
ap.add_argument("--standalone-only", action="store_true", help="(a) alone, e.g. under a kernel trace")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "jpeg_ab.txt"))
a = ap.parse_args()
if L.lib().adas_device_count() <= 0:
    raise SystemExit("bench_jpeg.py needs an MI355X: there is no CPU fallback and no CPU timing")
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
copy_dst = L.DeviceBuffer(nbytes)
enc = PP.JpegEncoder(W, H, quality=90, max_batch=S)
timer = L.StreamTimer()


def timed(fn):
    with timer:
        for _ in range(a.iters):
            fn()
    return timer.ms / a.iters * 1e3      # us per call


copy = lambda: hip.hipMemcpyAsync(copy_dst.ptr, cam[0].ptr, nbytes, D2D, None)
encode = lambda: enc.run(cam[0].ptr, S)
us, size = {"copy": []}, {}
for q in (75, 90):
    enc.set_quality(q)
    encode(); copy()                       # warm-up
    L.check(L.lib().adas_synchronize())
    us["jpeg q%d" % q] = []
    for _ in range(a.rounds):
        us["copy"].append(timed(copy))
        us["jpeg q%d" % q].append(timed(encode))
    lens, flags = enc.lengths(S)
    assert not flags.any()
    size[q] = (float(lens.mean()), int(lens.min()), int(lens.max()))
cm = median(us["copy"])[0]
lines = ["tools/bench_jpeg.py on one MI355X (gfx950).", "",
         "(a) stand-alone, %d synthetic camera frames of 1280x720 (%.1f MB; the copy reads and writes all of it), %d rounds of %d calls between two"
         % (S, nbytes / 1e6, a.rounds, a.iters),
         "    events on the null stream, alternated in one process; us per call, median round (fastest, slowest).", ""]
for n in us:
    m, lo, hi = median(us[n])
    extra = ""
    if n != "copy":
        mean, lo_b, hi_b = size[int(n[6:])]
        extra = "   %.0f bytes per frame (%d .. %d): 1 / %.1f of the raw frame" % (mean, lo_b, hi_b, H * W * 3 / mean)
    lines.append("    %-10s %9.1f us  (%.1f, %.1f)  %5.2f x the copy%s" % (n, m, lo, hi, m / cm, extra))
jm = median(us["jpeg q90"])[0]
enc.close(); timer.close(); copy_dst.free()
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


work = tempfile.mkdtemp(prefix="jpg_bench_")
base = netutil.coco_like_frames(8, seed=40)
det_path, _, _ = bench.build_detector(M, CE, "yolov8n", base, work, "jpg", target_per_frame=25.0, capacity=512)
lane_path = M.build("ufldv2_res18", wsrc=PrescribedLanes()).save(os.path.join(work, "lane.hipm"))
pkw = dict(n_streams=S, precision=a.precision, src_hw=(H, W), use_graph=True, track=True, box_score=0.1, max_candidates=512,
           geometry=dict(bird_wh=IMG, M=A.PerspectiveTransformation(IMG).M), overlay=dict())
pipes = [("off", PL.AdasPipeline(det_path, lane_path, **pkw)), ("on", PL.AdasPipeline(det_path, lane_path, jpeg=dict(quality=90), **pkw))]
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
on = pipes[1][1]
fetch = {"jpeg(f)": [], "overlay_image(f)": []}
got = 0
for _ in range(a.rounds):
    t0 = time.perf_counter()
    got = sum(len(on.jpeg(f)) for f in range(S))
    fetch["jpeg(f)"].append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    for f in range(S):
        on.overlay_image(f)
    fetch["overlay_image(f)"].append((time.perf_counter() - t0) * 1e3)
lines += ["", "(b) fused step (yolov8n + ufldv2_res18, %s, hipGraph, two branches, tracker, lane overlay), %d streams of 1280x720 from camera frames,"
          % (on.lane.precision, S),
          "    %d windows of %d steps per variant, alternated in one process; ms per step, median window (fastest, slowest)." % (a.rounds, a.steps), ""]
med = {}
for name, _ in pipes:
    med[name], lo, hi = median(ms[name])
    lines.append("    %-4s %8.3f ms per step  (%.3f, %.3f)   %d kernels in the captured step" % (name, med[name], lo, hi, kernels[name]))
lines += ["", "    on - off = %+8.1f us per step (three plain launches behind the overlay's run, inside the capture); the stand-alone run takes %.1f us."
          % ((med["on"] - med["off"]) * 1e3, jm), "",
          "    the host fetching every frame of a step, %d calls each, ms of wall time, median of %d (fastest, slowest):" % (S, a.rounds)]
for n in fetch:
    m, lo, hi = median(fetch[n])
    mb = got / 1e6 if n.startswith("jpeg") else S * H * W * 3 / 1e6
    lines.append("    %-18s %8.2f ms  (%.2f, %.2f)   %.1f MB" % (n, m, lo, hi, mb))
for _, p in pipes:
    p.close()
for b in cam:
    b.free()
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, "w").write(text)
print(text)
