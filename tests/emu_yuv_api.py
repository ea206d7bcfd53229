"""ctypes wrapper over tests/_build/libemu_yuv.so (host build of csrc/yuv_core.h, tests/hostemu/emu_yuv.cpp).
Test scaffolding: lets the CPU suite walk the device kernel's work items of rules C1-C7 with every load and store audited, and compare the
frames with tests/yuv_ref.py; the GPU suite compares the device's frames with these.  Builds itself on first use."""
import ctypes as C, os, subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "emu_yuv.cpp")
BOUNDS_SRC = os.path.join(ROOT, "tests", "hostemu", "yuv_bounds_main.cpp")
OUT = os.path.join(ROOT, "tests", "_build", "libemu_yuv.so")
BOUNDS_OUT = os.path.join(ROOT, "tests", "_build", "yuv_bounds")
INC = os.path.join(ROOT, "vehicle-cv-adas_amd", "csrc")
FORMATS = {"nv12": 0, "nv21": 1, "i420": 2, "yuyv": 3, "uyvy": 4}
MATRICES = {"video": 0, "full": 1}
FIELDS = ("frame_stride", "y_offset", "y_pitch", "u_offset", "u_pitch", "v_offset", "v_pitch")
WHY = {0: None, 1: "format", 2: "matrix", 3: "size", 4: "odd width", 5: "odd height", 6: "short pitch", 7: "outside", 8: "overlap"}


class Params(C.Structure):          # YuvGeom as this file believes it to be (test_yuv_cpu.py compares it with the header's and _lib's)
    _fields_ = [("format", C.c_int32), ("matrix", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)] + [(f, C.c_int64) for f in FIELDS]


def _fresh(out, deps):
    return os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)


def _deps(src):
    return [src] + [os.path.join(INC, h) for h in ("yuv_core.h", "jpegdec_core.h", "jpeg_core.h")]


def build():
    if _fresh(OUT, _deps(SRC)):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", INC, SRC, "-o", OUT])
    return OUT


def build_bounds():
    """The stand-alone bounds program (tests/hostemu/yuv_bounds_main.cpp), plain g++ -O1."""
    if _fresh(BOUNDS_OUT, _deps(BOUNDS_SRC)):
        return BOUNDS_OUT
    os.makedirs(os.path.dirname(BOUNDS_OUT), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", INC, BOUNDS_SRC, "-o", BOUNDS_OUT])
    return BOUNDS_OUT


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_yuv_default.argtypes = [C.POINTER(Params), C.c_int, C.c_int, C.c_int]
        _lib.emu_yuv_check.argtypes = [C.POINTER(Params)]
        _lib.emu_yuv_frame_bytes.restype = C.c_longlong
        _lib.emu_yuv_frame_bytes.argtypes = [C.POINTER(Params)]
        _lib.emu_yuv_colour.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
        _lib.emu_yuv_run.argtypes = [C.POINTER(Params), C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p]
    return _lib


def params_layout():
    """(sizeof, {field: offset}) of the header's struct as g++ lays it out"""
    v = (C.c_int * 12)()
    lib().emu_yuv_params_layout(v)
    names = ("format", "matrix", "width", "height") + FIELDS
    return int(v[0]), dict(zip(names, (int(x) for x in v[1:])))


def params(fmt, w, h, matrix="video", layout=None):
    """The header's own tight layout (yuv_default), or `layout` (a dict of FIELDS)."""
    p = Params()
    lib().emu_yuv_default(C.byref(p), FORMATS[fmt], int(w), int(h))
    p.matrix = MATRICES[matrix]
    for k, v in (layout or {}).items():
        setattr(p, k, int(v))
    return p


def layout_of(p):
    return {k: int(getattr(p, k)) for k in FIELDS}


def check(p):
    """None, or yuv_check's refusal by name"""
    return WHY[int(lib().emu_yuv_check(C.byref(p)))]


def frame_bytes(p):
    return int(lib().emu_yuv_frame_bytes(C.byref(p)))


def colour(Y, U, V, matrix="video"):
    Y, U, V = (np.ascontiguousarray(a, np.uint8).ravel() for a in (Y, U, V))
    out = np.empty((len(Y), 3), np.uint8)
    lib().emu_yuv_colour(MATRICES[matrix], Y.ctypes.data, U.ctypes.data, V.ctypes.data, len(Y), out.ctypes.data)
    return out


def aligned(n, offset=0, fill=0, guard=0):
    """(whole, view): a uint8 view of n bytes whose address is `offset` mod 64, with `guard` bytes of `fill` on either side inside whole."""
    whole = np.full(n + 2 * guard + 128, fill, np.uint8)
    a = (-(whole.ctypes.data + guard) + offset) % 64
    return whole, whole[guard + a:guard + a + n]


class Run:
    """bgr [batch][h][w][3]; vector (the path taken); outside, misaligned, loads, stores, wide: the audit's counts; guard_ok"""


def run(buf, p, batch=1, path=-1, src_offset=0, dst_offset=0, guard=64):
    """`batch` frames of bytes `buf` (exactly the bytes the parameters imply, or more) through the work items.  The source and the destination
    are placed `*_offset` bytes off a multiple of 64 and handed over with their exact sizes; guard bytes around the destination are checked."""
    buf = np.asarray(buf, np.uint8)
    w, h = p.width, p.height
    need = (batch - 1) * p.frame_stride + frame_bytes(p)
    assert check(p) is None and len(buf) >= need, (check(p), len(buf), need)
    _, src = aligned(need, src_offset)
    src[:] = buf[:need]
    nd = batch * h * w * 3
    whole, dst = aligned(nd, dst_offset, fill=0xA5, guard=guard)
    info = np.zeros(6, np.int64)
    rc = lib().emu_yuv_run(C.byref(p), src.ctypes.data, need, dst.ctypes.data, nd, batch, path, info.ctypes.data)
    assert rc == 0, rc
    r = Run()
    r.vector, r.outside, r.misaligned, r.loads, r.stores, r.wide = (int(v) for v in info)
    r.bgr = dst.reshape(batch, h, w, 3).copy()
    lo = dst.ctypes.data - whole.ctypes.data
    r.guard_ok = bool((whole[:lo] == 0xA5).all() and (whole[lo + nd:] == 0xA5).all())
    return r


def convert(buf, p, batch=1):
    """What the device's run must give: [batch][h][w][3]."""
    r = run(buf, p, batch)
    assert r.outside == 0 and r.misaligned == 0 and r.guard_ok
    return r.bgr
