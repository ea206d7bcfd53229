"""ctypes wrapper over tests/_build/libemu_scale.so (host build of csrc/scale_core.h, tests/hostemu/emu_scale.cpp).
Test scaffolding: lets the CPU suite walk the device kernel's work items of rules S1-S8 with every load and store audited, and compare the
bytes with tests/scale_ref.py; the GPU suite compares the device's bytes with these.  Builds itself on first use."""
import ctypes as C, os, subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "emu_scale.cpp")
OUT = os.path.join(ROOT, "tests", "_build", "libemu_scale.so")
INC = os.path.join(ROOT, "vehicle-cv-adas_amd", "csrc")
MODES = {"area": 0, "linear": 1}
WHY = {0: None, 1: "mode", 2: "size", 3: "mosaic", 4: "enlarge", 5: "big D", 6: "border", 7: "big canvas"}
DEFAULT_COLORS = ((0, 255, 255), (0, 255, 0), (0, 102, 255), (0, 0, 255))
SENTINEL = 0xA5
FIELDS = ("src_w", "src_h", "dst_w", "dst_h", "mode", "cols", "rows", "border", "background", "border_bgr")


class Params(C.Structure):          # ScaleParams as this file believes it to be (test_scale_cpu.py compares it with the header's and _lib's)
    _fields_ = [(f, C.c_int32) for f in FIELDS[:8]] + [("background", C.c_uint8 * 4), ("border_bgr", (C.c_uint8 * 4) * 4)]


def _fresh(out, deps):
    return os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)


def build():
    deps = [SRC] + [os.path.join(INC, h) for h in ("scale_core.h", "overlay_panel_core.h")]
    if _fresh(OUT, deps):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", INC, SRC, "-o", OUT])
    return OUT


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_scale_check.argtypes = [C.POINTER(Params)]
        _lib.emu_scale_canvas_bytes.restype = C.c_longlong
        _lib.emu_scale_canvas_bytes.argtypes = [C.POINTER(Params)]
        _lib.emu_scale_canvases.argtypes = [C.POINTER(Params), C.c_int]
        _lib.emu_scale_vector_ok.argtypes = [C.POINTER(Params), C.c_void_p, C.c_void_p]
        _lib.emu_scale_area_weights.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.emu_scale_run.argtypes = [C.POINTER(Params), C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_longlong,
                                       C.c_int, C.c_int, C.c_void_p]
    return _lib


def params_layout():
    """(sizeof, {field: offset}) of the header's struct as g++ lays it out"""
    v = (C.c_int * 11)()
    lib().emu_scale_params_layout(v)
    return int(v[0]), dict(zip(FIELDS, (int(x) for x in v[1:])))


def params(src_wh, size, mode="area", mosaic=(1, 1), border=0, background=(0, 0, 0), border_colors=DEFAULT_COLORS):
    p = Params()
    p.src_w, p.src_h = (int(v) for v in src_wh)
    p.dst_w, p.dst_h = (int(v) for v in size)
    p.mode = MODES[mode] if isinstance(mode, str) else int(mode)
    p.cols, p.rows = (int(v) for v in mosaic)
    p.border = int(border)
    for c in range(3):
        p.background[c] = int(background[c])
        for k in range(4):
            p.border_bgr[k][c] = int(border_colors[k][c])
    return p


def check(p):
    """None, or the refusal by name"""
    return WHY[int(lib().emu_scale_check(C.byref(p)))]


def canvas_bytes(p):
    return int(lib().emu_scale_canvas_bytes(C.byref(p)))


def canvases(p, batch):
    return int(lib().emu_scale_canvases(C.byref(p), int(batch)))


def area_weights(d, dn, sn):
    """(lo, [weights of lo .. hi - 1]) of destination index d, as the header computes them"""
    lo, hi, w = C.c_int(), C.c_int(), np.zeros(sn + 1, np.int32)
    lib().emu_scale_area_weights(int(d), int(dn), int(sn), C.byref(lo), C.byref(hi), w.ctypes.data)
    return lo.value, [int(v) for v in w[:hi.value - lo.value]]


def aligned(n, offset=0, fill=0, guard=0):
    """(whole, view): a uint8 view of n bytes whose address is `offset` mod 64, with `guard` bytes of `fill` on either side inside whole."""
    whole = np.full(n + 2 * guard + 128, fill, np.uint8)
    a = (-(whole.ctypes.data + guard) + offset) % 64
    return whole, whole[guard + a:guard + a + n]


class Run:
    """out: uint8 [canvases][rows * dst_h][cols * dst_w][3], pre-filled with SENTINEL; vector (the path taken: 0 generic items, 1 vector
    items, 2 staged blocks); outside, misaligned, loads,
    stores, wide, state_loads, not_once: the audit's counts; guard_ok"""


def run(bgr, p, states=None, path=-1, src_offset=0, dst_offset=0, guard=64):
    """bgr [batch][src_h][src_w][3] through the work items.  states: None or int32 [batch].  The source and the destination are placed
    `*_offset` bytes off a multiple of 64 and handed over with their exact sizes; the destination is pre-filled with SENTINEL and the guard
    bytes around it are checked."""
    bgr = np.ascontiguousarray(bgr, np.uint8)
    batch, h, w, _ = bgr.shape
    assert check(p) is None and (w, h) == (p.src_w, p.src_h), (check(p), w, h)
    _, src = aligned(bgr.size, src_offset)
    src[:] = bgr.ravel()
    k = canvases(p, batch)
    nd = k * canvas_bytes(p)
    whole, dst = aligned(nd, dst_offset, fill=SENTINEL, guard=guard)
    st = None if states is None else np.ascontiguousarray(states, np.int32)
    assert st is None or st.shape == (batch,)
    info = np.zeros(8, np.int64)
    rc = lib().emu_scale_run(C.byref(p), src.ctypes.data, src.size, None if st is None else st.ctypes.data, 0 if st is None else st.nbytes, 4,
                             dst.ctypes.data, nd, batch, path, info.ctypes.data)
    assert rc == 0, rc
    r = Run()
    r.vector, r.outside, r.misaligned, r.loads, r.stores, r.wide, r.state_loads, r.not_once = (int(v) for v in info)
    r.out = dst.copy().reshape(k, p.rows * p.dst_h, p.cols * p.dst_w, 3)
    lo = dst.ctypes.data - whole.ctypes.data
    r.guard_ok = bool((whole[:lo] == SENTINEL).all() and (whole[lo + nd:] == SENTINEL).all())
    return r


def scale(bgr, p, states=None):
    """What the device's run must write: uint8 [canvases][rows * dst_h][cols * dst_w][3]."""
    r = run(bgr, p, states)
    assert (r.outside, r.misaligned, r.not_once) == (0, 0, 0) and r.guard_ok
    return r.out
