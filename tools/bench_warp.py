#!/usr/bin/env python3
"""Device time of warp_perspective_kernel at S frames of 1280x720 resident in HBM: python tools/bench_warp.py [S] [launches]
One launch warps all S frames (bird-view matrix on even frames, frontal on odd ones when --mixed; bird-view on all otherwise);
after a warm-up, 5 windows of back-to-back launches between hipEvents (adas_timer), each window at least `launches` launches and long
enough to last about half a second (sized from a 20-launch probe); the median window is reported with the fastest and the slowest
beside it.  Then the same for batch 1.  GB/s is against the
algorithmic 5.53 MB per frame (2.76 MB read + 2.76 MB written), whatever the gathers really fetch.
ADAS_WARP_ROWS=<destination rows per workgroup> is read by the library at first launch (one process per value)."""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from conftest import load_pkg
load_pkg()
L = importlib.import_module("adas_amd._lib")
PP = importlib.import_module("adas_amd.postproc")
A = importlib.import_module("adas_amd.analysis")
import bench, warp_ref

args = [a for a in sys.argv[1:] if not a.startswith("--")]
S = int(args[0]) if len(args) > 0 else 64
N = int(args[1]) if len(args) > 1 else 200
H, W = 720, 1280
FRAME_BYTES = 2 * H * W * 3
WINDOW_MS = 500.0
if L.lib().adas_device_count() <= 0:
    raise SystemExit("bench_warp.py needs an MI355X: there is no CPU fallback and no CPU timing")
cam = bench.cam_frames(S, 3)
src = L.DeviceBuffer.from_array(cam)
dst = L.DeviceBuffer(S * H * W * 3)
pt = A.PerspectiveTransformation((W, H))
w = PP.PerspectiveWarp((H, W), (H, W), S)
w.set_matrix(pt.M)
if "--mixed" in sys.argv:
    for f in range(1, S, 2):
        w.set_matrix(pt.M_inv, f)
out = []
for batch in (S, 1):
    for _ in range(5):
        w.run(src.ptr, batch, dst.ptr)
    L.check(L.lib().adas_synchronize())
    def window(n):
        with L.StreamTimer(None) as t:
            for _ in range(n):
                w.run(src.ptr, batch, dst.ptr)
        ms = t.ms
        t.close()
        return ms / n * 1e3
    n = max(N, int(WINDOW_MS * 1e3 / window(20)) + 1)
    reps = sorted(window(n) for _ in range(5))
    us = reps[2]
    out.append("batch %2d: %8.1f us per launch (median of 5 windows of %d launches, %.0f ms each; fastest %.1f, slowest %.1f), "
               "%6.2f us per frame, %7.1f GB/s algorithmic" % (
        batch, us, n, us * n * 1e-3, reps[0], reps[-1], us / batch, batch * FRAME_BYTES / us * 1e-3))
got = dst.download((S, H, W, 3), np.uint8)
ok = np.array_equal(got[0], warp_ref.warp_perspective(cam[0], pt.M, (W, H)))
print("ADAS_WARP_ROWS=%s  S=%d  %s  frame 0 equals the restatement: %s  checksum %d" % (
    os.environ.get("ADAS_WARP_ROWS", "default"), S, "mixed" if "--mixed" in sys.argv else "bird-view", ok, int(got.astype(np.uint64).sum())))
for line in out:
    print(line)
w.close(); src.free(); dst.free()
