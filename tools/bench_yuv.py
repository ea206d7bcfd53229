#!/usr/bin/env python3
"""Cost of the YUV conversion on the device (csrc/yuv_kernels.hip) and of feeding the fused step with raw camera formats:
    python tools/bench_yuv.py [--streams 64] [--rounds 5] [--iters 50] [--sections convert,upload,step] [--precisions fp16,fp16x3]
--streams frames of 1280x720 (8 distinct synthetic camera frames, repeated) in NV12, NV21, I420, YUYV and UYVY, tight layout, and as BGR.
(a) convert  device to device: YuvConverter.run_device per format, timed with the library's events on the null stream against
             hipMemcpyAsync device-to-device of the BGR frames between the same events, in alternation.  The copy is the yardstick: it moves
             6 bytes per pixel (3 read, 3 written); a 4:2:0 conversion moves 4.5, a 4:2:2 conversion 5.
(b) upload   one hipMemcpyAsync from pinned host memory of the step's frames as BGR, NV12 and YUYV: host wall time, device drained at
             both ends.
(c) step     the host-fed fused step (YOLOv8n + UFLDv2-R18 + NMS + ByteTrack, --streams streams, graph mode): step_frames_host on the BGR
             frames against step_yuv_host per format on their raw form, per precision, in alternation on ONE pipeline per format (pipelines
             of one process differ among themselves by more than the two ways in do; a pair on one pipeline does not).  The
             detector's seeded random weights are not calibrated as bench.py calibrates them, so the absolute rate is not bench.py's; the
             comparison between the ways in is the point.
us per call, median round (fastest, slowest).  Writes profiles/r08/yuv.txt (or --out)."""
import argparse, ctypes as C, importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from conftest import load_pkg
load_pkg()
L = importlib.import_module("adas_amd._lib")
PP = importlib.import_module("adas_amd.postproc")
import bench
import yuv_ref

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--sections", default="convert,upload,step")
ap.add_argument("--precisions", default="fp16,fp16x3")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "yuv.txt"))
a = ap.parse_args()
if L.lib().adas_device_count() <= 0:
    raise SystemExit("bench_yuv.py needs an MI355X: there is no CPU fallback and no CPU timing")
S, H, W = a.streams, 720, 1280
sections = a.sections.split(",")
hip = C.CDLL("libamdhip64.so")      # already in the process: libadas_hip.so links it
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
H2D, D2D = 1, 3
FORMATS = yuv_ref.FORMATS


def median(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def repack(i420, fmt):
    """a tight I420 frame's bytes in another format (4:2:2: every chroma row twice)"""
    Y = i420[:H * W].reshape(H, W)
    U = i420[H * W:H * W * 5 // 4].reshape(H // 2, W // 2)
    V = i420[H * W * 5 // 4:].reshape(H // 2, W // 2)
    if fmt == "i420":
        return i420
    if fmt in ("nv12", "nv21"):
        pair = np.stack((U, V) if fmt == "nv12" else (V, U), -1)
        return np.concatenate([Y.ravel(), pair.ravel()])
    U2, V2 = np.repeat(U, 2, 0), np.repeat(V, 2, 0)
    out = np.empty((H, W // 2, 4), np.uint8)
    if fmt == "yuyv":
        out[..., 0], out[..., 1], out[..., 2], out[..., 3] = Y[:, 0::2], U2, Y[:, 1::2], V2
    else:
        out[..., 0], out[..., 1], out[..., 2], out[..., 3] = U2, Y[:, 0::2], V2, Y[:, 1::2]
    return out.ravel()


distinct = min(S, 8)
cams = bench.cam_frames(distinct, 900)
i420 = [yuv_ref.from_bgr(cams[f], "i420") for f in range(distinct)]
raw = {fmt: np.concatenate([repack(i420[f % distinct], fmt) for f in range(S)]) for fmt in FORMATS}
conv = {fmt: PP.YuvConverter(fmt, W, H, max_batch=S) for fmt in FORMATS}
d_raw = {fmt: L.DeviceBuffer.from_array(raw[fmt]) for fmt in FORMATS}
# the BGR frames of the comparison are the conversion's own output: both ways in then hand the step the same pixels
conv["nv12"].run_device(d_raw["nv12"].ptr, S)
bgr = np.stack([conv["nv12"].image(f) for f in range(S)])
for fmt in FORMATS:                 # every format carries the same picture (4:2:2 with doubled chroma rows), so the same BGR
    conv[fmt].run_device(d_raw[fmt].ptr, S)
    assert np.array_equal(conv[fmt].image(S - 1), bgr[S - 1]), fmt
nbytes = bgr.nbytes
d_bgr = L.DeviceBuffer.from_array(bgr)
copy_dst = L.DeviceBuffer(nbytes)
timer = L.StreamTimer()


def timed(fn):
    with timer:
        for _ in range(a.iters):
            fn()
    return timer.ms / a.iters * 1e3


def walled(fn, sync=None):
    sync = sync or (lambda: L.check(L.lib().adas_synchronize()))
    sync()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        fn()
    sync()
    return (time.perf_counter() - t0) / a.iters * 1e6


def table(us, base):
    bm = median(us[base])[0]
    out = []
    for n, v in us.items():
        m, lo, hi = median(v)
        out.append("    %-22s %10.1f us  (%.1f, %.1f)  %5.2f x %s   %.0f frames/s" % (n, m, lo, hi, m / bm, base, S / m * 1e6))
    return out


lines = ["tools/bench_yuv.py on one MI355X (gfx950).", "",
         "%d frames of 1280x720 (%d distinct synthetic camera frames, repeated): %.1f MB as BGR, %.1f MB as NV12 / NV21 / I420, %.1f MB as YUYV / UYVY."
         % (S, distinct, nbytes / 1e6, raw["nv12"].nbytes / 1e6, raw["yuyv"].nbytes / 1e6),
         "%d rounds of %d calls, alternated in one process; us per call, median round (fastest, slowest)." % (a.rounds, a.iters)]

if "convert" in sections:
    fns = {"copy d2d": lambda: hip.hipMemcpyAsync(copy_dst.ptr, d_bgr.ptr, nbytes, D2D, None)}
    for fmt in FORMATS:
        fns["convert d2d " + fmt] = (lambda f: lambda: conv[f].run_device(d_raw[f].ptr, S))(fmt)
    us = {n: [] for n in fns}
    for fn in fns.values():
        fn()
    for _ in range(a.rounds):
        for n, fn in fns.items():
            us[n].append(timed(fn))
    lines += ["", "(a) device to device, between two events on the null stream (the copy moves 6 B per pixel, 4:2:0 4.5, 4:2:2 5):"] + table(us, "copy d2d")
    chi = median(us["copy d2d"])[2]
    for fmt in FORMATS:
        m = median(us["convert d2d " + fmt])[0]
        lines.append("    %s: %s the copy's slowest round (%.1f us)" % (fmt, "within" if m <= chi else "%.1f us (%.0f %%) over" % (m - chi, 100 * (m - chi) / chi), chi))

if "upload" in sections:
    pins = {"upload raw bgr": bgr, "upload nv12": raw["nv12"], "upload yuyv": raw["yuyv"]}
    us, fns, keep = {}, {}, []
    for n, arr in pins.items():
        pb = L.PinnedBuffer((arr.nbytes,))
        pb.array[:] = arr.ravel()
        keep.append(pb)
        fns[n] = (lambda p, nb: lambda: hip.hipMemcpyAsync(copy_dst.ptr, p, nb, H2D, None))(pb.ptr, arr.nbytes)
        us[n] = []
    for fn in fns.values():
        fn()
    for _ in range(a.rounds):
        for n, fn in fns.items():
            us[n].append(walled(fn))
    lines += ["", "(b) host to device from pinned memory, host wall time with the device drained at both ends:"] + table(us, "upload raw bgr")
    for n, arr in pins.items():
        lines.append("    %s: %.1f MB, %.1f GB/s" % (n, arr.nbytes / 1e6, arr.nbytes / median(us[n])[0] / 1e3))
    for pb in keep:
        pb.free()

if "step" in sections:
    import netutil
    PL = importlib.import_module("adas_amd.pipeline")
    det_path = netutil.model("yolov8n")[0]
    lane_path = netutil.model("ufldv2_res18")[0]
    pin_bgr = L.PinnedBuffer((nbytes,))
    pin_bgr.array[:] = bgr.ravel()
    pin_raw = {}
    for fmt in FORMATS:
        pin_raw[fmt] = L.PinnedBuffer((raw[fmt].nbytes,))
        pin_raw[fmt].array[:] = raw[fmt]
    for precision in a.precisions.split(","):
        kw = dict(n_streams=S, precision=precision, src_hw=(H, W), use_graph=True, max_candidates=512)
        lines += ["", "(c) the host-fed fused step, %s, %d streams, graph mode; host wall time over %d back-to-back steps; each pair on ONE pipeline:"
                  % (precision, S, a.iters)]
        for fmt in FORMATS:
            p = PL.AdasPipeline(det_path, lane_path, yuv_input=dict(format=fmt), **kw)
            fns = {"step_frames_host bgr": lambda: p.step_frames_host(pin_bgr.ptr, (H, W), 0.6),
                   "step_yuv_host " + fmt: lambda: p.step_yuv_host(pin_raw[fmt].ptr)}
            us = {n: [] for n in fns}
            for fn in fns.values():
                for _ in range(3):
                    fn()
                p.sync()
            for _ in range(a.rounds):
                for n, fn in fns.items():
                    us[n].append(walled(fn, p.sync))
            lines += table(us, "step_frames_host bgr")
            p.close()
    pin_bgr.free()
    for pb in pin_raw.values():
        pb.free()

for o in list(conv.values()) + [timer]:
    o.close()
for b in list(d_raw.values()) + [d_bgr, copy_dst]:
    b.free()
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, "w").write(text)
print(text)
