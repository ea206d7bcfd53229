"""ctypes wrapper over tests/_build/libemu_overlay_objects.so (host build of the object layer of csrc/overlay_core.h,
tests/hostemu/emu_overlay_objects.cpp).  Test scaffolding: lets the CPU suite run the device kernels' closed forms of rules D6-D9 and
compare them with tests/overlay_objects_ref.py."""
import ctypes as C, os, subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "emu_overlay_objects.cpp")
OUT = os.path.join(ROOT, "tests", "_build", "libemu_overlay_objects.so")
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
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def tint(a, b):
    return int(lib().emu_overlay_tint(int(a), int(b)))


def thick_segment_mask(ax, ay, bx, by, t, H, W):
    m = np.zeros((H, W), np.uint8)
    lib().emu_overlay_segment(int(ax), int(ay), int(bx), int(by), int(t), H, W, _p(m))
    return m.astype(bool)


def rect_mask(x1, y1, x2, y2, t, H, W):
    m = np.zeros((H, W), np.uint8)
    lib().emu_overlay_rect(int(x1), int(y1), int(x2), int(y2), int(t), H, W, _p(m))
    return m.astype(bool)


def corner_rect_mask(xmin, ymin, xmax, ymax, H, W, t=5, rt=1):
    m = np.zeros((H, W), np.uint8)
    box = np.array([xmin, ymin, xmax, ymax], np.int32)
    lib().emu_overlay_corner_rect(_p(box), int(t), int(rt), H, W, _p(m))
    return m.astype(bool)


def objects(img, dets=None, det_cls=None, det_table=None, trks=None, trk_cls=None, trk_table=None, min_box_area=10.0, thickness=(1, 5, 2),
            stages=48):
    """D9 on one frame that has been through AREA: the core's fold over the records, every pixel."""
    out = np.ascontiguousarray(img, np.uint8).copy()
    H, W = out.shape[:2]
    d = np.ascontiguousarray(np.asarray(dets if dets is not None else [], np.int32).reshape(-1, 4))
    dc = np.ascontiguousarray(np.asarray(det_cls if det_cls is not None else [], np.int32).reshape(-1))
    t = np.ascontiguousarray(np.asarray(trks if trks is not None else [], np.float64).reshape(-1, 4))
    tc = np.ascontiguousarray(np.asarray(trk_cls if trk_cls is not None else [], np.int32).reshape(-1))
    dt = np.ascontiguousarray(np.asarray(det_table if det_table is not None else [], np.uint8).reshape(-1, 3))
    tt = np.ascontiguousarray(np.asarray(trk_table if trk_table is not None else [], np.uint8).reshape(-1, 3))
    fn = lib().emu_overlay_objects
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                   C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int]
    fn(_p(out), H, W, _p(d), _p(dc), len(d), _p(dt), len(dt), _p(t), _p(tc), len(t), _p(tt), len(tt), float(min_box_area), int(thickness[0]),
       int(thickness[1]), int(thickness[2]), int(stages))
    return out
