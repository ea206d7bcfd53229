#!/usr/bin/env python3
"""Cost of the baseline JPEG decoder on the device (csrc/jpegdec_kernels.hip):
    python tools/bench_jpegdec.py [--streams 64] [--rounds 5] [--iters 20] [--quality 90]
--streams synthetic camera frames of 1280x720 are encoded once on the device (JpegEncoder: 4:2:0, one restart interval per MCU row, so 45
segments per frame) and then
(a) device to device: JpegDecoder.run_device on the encoder's streams where they lie, timed with the library's events on the null stream
    against hipMemcpyAsync device-to-device of the raw frames between the same events, in alternation.  The copy is the yardstick: it
    reads and writes every frame byte once; the decoder reads the streams, writes and reads the int16 coefficient arena and the u8 planes
    (3 and 1.5 bytes per pixel) and writes the frames.
(b) host to device: JpegDecoder.run_host of the same streams from host memory against one hipMemcpy of the raw frames from pinned host
    memory -- what adas_pipeline_step_frames_host moves per step.  Host wall time with the device drained at both ends, so (b) holds the
    packing of the streams into the pinned staging buffer as well.
us per call, median round (fastest, slowest).  Writes profiles/r08/jpegdec.txt (or --out)."""
import argparse, ctypes as C, importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from conftest import load_pkg
load_pkg()
L = importlib.import_module("adas_amd._lib")
PP = importlib.import_module("adas_amd.postproc")
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--quality", type=int, default=90)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "jpegdec.txt"))
a = ap.parse_args()
if L.lib().adas_device_count() <= 0:
    raise SystemExit("bench_jpegdec.py needs an MI355X: there is no CPU fallback and no CPU timing")
S, H, W = a.streams, 720, 1280
hip = C.CDLL("libamdhip64.so")      # already in the process: libadas_hip.so links it
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
H2D, D2D = 1, 3


def median(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


cams = bench.cam_frames(S, 900)
cam = L.DeviceBuffer.from_array(cams)
nbytes = cams.nbytes
enc = PP.JpegEncoder(W, H, quality=a.quality, max_batch=S)
enc.run(cam.ptr, S)
lens, flags = enc.lengths(S)
assert not flags.any()
cap = int(lens.max())
dec = PP.JpegDecoder(W, H, max_batch=S, capacity=cap)
d_streams, d_lens, stride = enc.device_view()
copy_dst = L.DeviceBuffer(nbytes)
timer = L.StreamTimer()


def timed(fn):
    with timer:
        for _ in range(a.iters):
            fn()
    return timer.ms / a.iters * 1e3


def walled(fn):
    L.check(L.lib().adas_synchronize())
    t0 = time.perf_counter()
    for _ in range(a.iters):
        fn()
    L.check(L.lib().adas_synchronize())
    return (time.perf_counter() - t0) / a.iters * 1e6


copy = lambda: hip.hipMemcpyAsync(copy_dst.ptr, cam.ptr, nbytes, D2D, None)
decode = lambda: dec.run_device(d_streams, d_lens, stride, S)
decode(); copy()
assert not dec.flags(S).any()
psnr = []
for f in (0, S - 1):                 # the decoded frames are the camera's, to the encoder's quality
    err = dec.image(f).astype(np.float64) - cams[f]
    psnr.append(10 * np.log10(255.0 ** 2 / max((err ** 2).mean(), 1e-9)))
us = {"copy d2d": [], "decode d2d": [], "upload raw": [], "decode host": []}
for _ in range(a.rounds):
    us["copy d2d"].append(timed(copy))
    us["decode d2d"].append(timed(decode))
host_streams = [enc.fetch(f) for f in range(S)]
pinned = L.PinnedBuffer(cams.shape)
pinned.array[...] = cams
upload = lambda: hip.hipMemcpyAsync(copy_dst.ptr, pinned.ptr, nbytes, H2D, None)
decode_host = lambda: dec.run_host(host_streams)
upload(); decode_host()
for _ in range(a.rounds):
    us["upload raw"].append(walled(upload))
    us["decode host"].append(walled(decode_host))
assert not dec.flags(S).any()
lines = ["tools/bench_jpegdec.py on one MI355X (gfx950).", "",
         "%d synthetic camera frames of 1280x720 (%.1f MB raw), encoded on the device at quality %d: %.0f bytes per frame (%d .. %d), %.1f MB in all,"
         % (S, nbytes / 1e6, a.quality, lens.mean(), lens.min(), lens.max(), lens.sum() / 1e6),
         "1 / %.1f of the raw frames; 45 restart segments per frame.  PSNR of the decoded against the camera frame: %.1f dB, %.1f dB." % (
             nbytes / lens.sum(), psnr[0], psnr[1]),
         "%d rounds of %d calls, alternated in one process; us per call, median round (fastest, slowest)." % (a.rounds, a.iters), "",
         "(a) device to device, between two events on the null stream:"]
for group, base in ((("copy d2d", "decode d2d"), "copy d2d"), (("upload raw", "decode host"), "upload raw")):
    if base == "upload raw":
        lines += ["", "(b) host to device, host wall time with the device drained at both ends:"]
    bm = median(us[base])[0]
    for n in group:
        m, lo, hi = median(us[n])
        lines.append("    %-12s %10.1f us  (%.1f, %.1f)  %5.2f x %s   %.0f frames/s" % (n, m, lo, hi, m / bm, base, S / m * 1e6))
for o in (enc, dec, timer):
    o.close()
for b in (cam, copy_dst):
    b.free()
pinned.free()
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, "w").write(text)
print(text)
