"""ctypes wrapper over tests/_build/libemu_overlay.so (host build of csrc/overlay_core.h, tests/hostemu/emu_overlay.cpp).
Test scaffolding: lets the CPU suite run the device kernels' pixel rules and compare them with tests/overlay_ref.py."""
import ctypes as C, os, subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "emu_overlay.cpp")
OUT = os.path.join(ROOT, "tests", "_build", "libemu_overlay.so")
INC = os.path.join(ROOT, "vehicle-cv-adas_amd", "csrc")


def build():
    deps = [SRC, os.path.join(INC, "overlay_core.h")]
    if os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I", INC, SRC, "-o", OUT])
    return OUT


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_overlay_blend.argtypes = [C.c_int, C.c_double, C.c_int]
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def blend(a, alpha, b):
    return int(lib().emu_overlay_blend(int(a), float(alpha), int(b)))


def disc_halfwidths(r):
    hw = np.zeros(r + 1, np.int32)
    lib().emu_overlay_disc_halfwidths(int(r), _p(hw))
    return [int(v) for v in hw]


def disc_mask(cx, cy, r, H, W):
    m = np.zeros((H, W), np.uint8)
    lib().emu_overlay_disc(C.c_int(int(cx)), C.c_int(int(cy)), int(r), H, W, _p(m))
    return m.astype(bool)


def line_mask(ax, ay, bx, by, H, W):
    m = np.zeros((H, W), np.uint8)
    lib().emu_overlay_line(int(ax), int(ay), int(bx), int(by), H, W, _p(m))
    return m.astype(bool)


def poly_mask(pts, H, W):
    pts = np.ascontiguousarray(np.asarray(pts, np.int32).reshape(-1, 2))
    m = np.zeros((H, W), np.uint8)
    flags = lib().emu_overlay_poly(_p(pts), len(pts), H, W, _p(m))
    return m.astype(bool), int(flags)


def compose(img, lanes=None, poly=None, area_status=False, dist=None, lane_bgr=None, area_color=(255, 191, 0), stages=7, lane_alpha=0.3,
            area_alpha=0.85, radii=(3, 4), direct=False, dist_color=(255, 255, 255)):
    """One frame through the core's D5; lane_bgr: the four lane colours after the offset rule.  (frame_show, flags)."""
    out = np.ascontiguousarray(img, np.uint8).copy()
    H, W = out.shape[:2]
    lp, lc = np.zeros((4, 128, 2), np.int32), np.zeros(4, np.int32)
    for l in range(4 if lanes is not None else 0):
        a = np.asarray(lanes[l], np.int32).reshape(-1, 2)
        lp[l, :len(a)], lc[l] = a, len(a)
    pl = np.ascontiguousarray(np.asarray(poly if poly is not None else [], np.int32).reshape(-1, 2))
    ds = np.ascontiguousarray(np.asarray(dist if dist is not None else [], np.int32).reshape(-1, 2))
    lb = np.ascontiguousarray(lane_bgr if lane_bgr is not None else [(255, 0, 0), (46, 139, 87), (50, 205, 50), (0, 255, 255)], np.uint8)
    ab, db = np.array(area_color, np.uint8), np.array(dist_color, np.uint8)
    fn = lib().emu_overlay_compose
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                   C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    flags = fn(_p(out), H, W, _p(lp), _p(lc), int(radii[0]), _p(lb), float(lane_alpha), _p(pl), len(pl), 1 if area_status else 0, _p(ab),
               float(area_alpha), _p(ds), len(ds), int(radii[1]), _p(db), int(stages), 1 if direct else 0)
    return out, int(flags)
